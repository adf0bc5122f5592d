"""Timing of gem_costmap_inflate against the only path there was before it: the window read over the link and written back, with a
host wait (gem_costmap_read + gem_costmap_write), WITHOUT counting any host inflation in between.  Needs a GPU; prints a table and,
with --out, writes it to a file as well.

Workloads: a local costmap of 400 x 400 at 0.05 m with R = 11 cells (inflation radius 0.55 m) and a global one of 4000 x 4000 at
0.05 m with R = 20 (1.0 m), both marked by gem_costmap_mark_points from a seeded noise cloud (--density points per cell, uniform
over the map, travers uniform around the threshold, so about half of them lethal), default value FREE_SPACE.  Each is timed for the
whole map and for a 100 x 100 window in its middle.
Rows, host clock (time.perf_counter) between two gem_synchronize:
  inflate_fresh    one call on the marked grid (restored on the device before every round, outside the clock): computes and stores
  inflate_again    one call on the grid the call before left: computes, stores nothing
  inflate_x20      twenty calls enqueued back to back, one synchronize, divided by twenty: what a call costs without the wait
  read_write       the baseline: gem_costmap_read of the window, then gem_costmap_write of the same bytes
The rows are alternated round by round (--rounds) after --warmup rounds; each reports its median and the min .. max of its rounds.
Before timing, the local map's result is compared with tests/inflate_ref.py's inflate_exact byte for byte (the global one: twice
equals once, and no 254 appears or disappears), and the numpy brushfire of the same file is timed once on the local map, for
information.  The bytes a call must move are computed from the result: the widened window read once by the seed pass, its bit words
written and read, the old byte of every cell within R of a seed, and a store for every cell that changes."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from gem_amd import POINT_DTYPE, ElevationMap, _lib  # noqa: E402
import inflate_ref as ref  # noqa: E402

RES, THRESH = 0.05, 0.5
WORKLOADS = {"local": (400, 11, 0.55), "global": (4000, 20, 1.0)}        # size, R, inflation radius
INSCRIBED, FACTOR = 0.3, 10.0


def noise_cloud(rng, size, density):
    n = int(size * size * density)
    pts = np.zeros(n, POINT_DTYPE)
    pts["x"] = rng.uniform(0.0, size * RES, n).astype(np.float32)
    pts["y"] = rng.uniform(0.0, size * RES, n).astype(np.float32)
    pts["travers"] = rng.uniform(THRESH - 0.3, THRESH + 0.3, n).astype(np.float32)
    return pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS))
    ap.add_argument("--density", type=float, default=0.02)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_inflate.py needs a GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"bench_inflate: {args.density} points per cell, inscribed radius {INSCRIBED} m, scaling factor {FACTOR}, rounds {args.rounds} "
        f"(alternated), warmup {args.warmup}")
    for name in args.workloads:
        size, R, radius = WORKLOADS[name]
        p = ref.Params(radius, INSCRIBED, FACTOR, False)
        assert ref.cells(p, RES) == R
        rng = np.random.default_rng(size)
        m = ElevationMap(32, 0.1)
        marked, cm = m.costmap(size, size, RES, 0.0, 0.0, _lib.COST_FREE_SPACE), m.costmap(size, size, RES, 0.0, 0.0, _lib.COST_FREE_SPACE)
        marked.mark_points(noise_cloud(rng, size, args.density), THRESH, None)
        before = marked.read()
        lethal = int((before == 254).sum())
        mid = size // 2
        for wname, window in (("whole map", (0, 0, size, size)), ("100 x 100 window", (mid - 50, mid - 50, mid + 50, mid + 50))):
            def restore():
                marked.merge(cm, None, _lib.COSTMAP_OVERWRITE)

            def inflate():
                cm.inflate(p.inflation_radius, p.inscribed_radius, p.cost_scaling_factor, p.inflate_unknown, window)

            restore(); inflate()
            after = cm.read()
            inflate()
            assert cm.read().tobytes() == after.tobytes(), "twice is not once"
            assert ((after == 254) == (before == 254)).all(), "a 254 appeared or disappeared"
            checked = "twice equals once, the 254 cells are the same"
            if name == "local":
                assert after.tobytes() == ref.inflate_exact(before, p, RES, window).tobytes(), "the device differs from inflate_exact"
                checked = "equal to inflate_exact byte for byte"
            w = ref.widened(before.shape, window, R)
            seed_bytes = (w[2] - w[0]) * (w[3] - w[1])
            bits = ((w[2] - 1) // 64 - w[0] // 64 + 1) * (w[3] - w[1]) * 8
            seeds = int((before[w[1]:w[3], w[0]:w[2]] == 254).sum())
            changed = int((after != before).sum())
            if name == "local":
                reach = int((ref.nearest_d2(before.shape, ref.seeds(before, window, R), R) != ref.NONE).sum())
            else:
                reach = changed                                          # a lower bound: the cells within R that did not change are not counted
            moved = seed_bytes + 2 * bits + reach + changed
            win_bytes = (window[2] - window[0]) * (window[3] - window[1])
            say()
            say(f"{name} {size} x {size} at {RES} m, R = {R}, {wname}: {lethal} lethal cells on the map, {seeds} seeds in the widened window, "
                f"{changed} cells change; {checked}")
            say(f"  bytes a call must move: {moved} (widened window {seed_bytes} + bit words 2 x {bits} + old bytes "
                f"{'' if name == 'local' else '>= '}{reach} + stores {changed}) against {win_bytes} in the window, "
                f"{2 * win_bytes} over the link for read_write")
            rows = ("inflate_fresh", "inflate_again", "inflate_x20", "read_write")
            times = {r: [] for r in rows}

            def run(row):
                if row == "inflate_fresh":
                    restore()
                m.synchronize()
                t = time.perf_counter()
                if row == "read_write":
                    cm.write(cm.read(window), window)
                else:
                    for _ in range(20 if row == "inflate_x20" else 1):
                        inflate()
                m.synchronize()
                dt = time.perf_counter() - t
                return dt / 20 if row == "inflate_x20" else dt

            for r in range(args.warmup + args.rounds):
                for row in rows:
                    dt = run(row)
                    if r >= args.warmup:
                        times[row].append(dt * 1e6)
            say(f"  {'row':<16} {'median us':>10} {'min us':>10} {'max us':>10}   rounds")
            for row, v in times.items():
                v = np.array(v)
                say(f"  {row:<16} {np.median(v):>10.1f} {v.min():>10.1f} {v.max():>10.1f}   {v.size}")
            ok = np.median(times["inflate_fresh"]) < np.median(times["read_write"])
            say(f"  the device call costs {'less' if ok else 'NOT less'} than the round trip")
            if name == "local" and wname == "whole map":
                t = time.perf_counter()
                brush = ref.inflate_brushfire(before, p, RES, window)
                say(f"  for information: the numpy brushfire of tests/inflate_ref.py takes {time.perf_counter() - t:.2f} s here and differs from the "
                    f"exact result in {int((brush != after).sum())} of {size * size} cells")
        marked.close(); cm.close()
        m.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
