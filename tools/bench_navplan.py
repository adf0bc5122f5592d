"""Timing of gem_costmap_navplan against what a user does without it: gem_costmap_read of the whole grid plus the host twin
gem_navplan_host (a binary-heap Dijkstra and the same getPath, C++ inside libgem_hip.so, called through ctypes).  Needs a GPU; prints
a table and, with --out, writes it to a file as well.

Workloads, all at 0.2 m with the default weight table and the outline on, start and goal near opposite corners:
  1000x1000 noise   the reference's global costmap; 20 % of the cells a random byte 0 .. 255
  1000x1000 maze    walls of 254 every 40 rows, each with a gap of 10 cells, alternating between the right and the left end: a plan
                    of about 25 map widths
  200x200 noise     a small map, 20 % noise
Rows, host clock (time.perf_counter) around calls that end in a wait, alternated round by round (--rounds) after --warmup rounds; each
reports its median and the min .. max of its rounds:
  navplan           Costmap.nav_plan(start, goal): init, the rounds of the tiled potential in chunks, the walk, the path's download
  potential_only    the same call with goal = start: the walk is one cell, so this is init + rounds + round trips
  path (derived)    navplan - potential_only, medians: the walk of n_path dependent steps and the download of its cells
  host_baseline     read of the grid + gem_navplan_host
rounds and chunks are the status words of the navplan row's last call.  Before timing, the device's potential and path are compared
with the host twin's byte for byte."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import gem_amd  # noqa: E402
from gem_amd import ElevationMap  # noqa: E402

RES = 0.2


def noise(rng, n):
    g = np.zeros((n, n), np.uint8)
    hit = rng.random(g.shape) < 0.2
    g[hit] = rng.integers(0, 256, int(hit.sum()), dtype=np.uint8)
    return g


def maze(n, every=40, gap=10):
    g = np.zeros((n, n), np.uint8)
    for k, y in enumerate(range(every, n - 1, every)):
        g[y, :] = 254
        if k % 2 == 0:
            g[y, n - 1 - gap:n - 1] = 0
        else:
            g[y, 1:1 + gap] = 0
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_navplan.py needs a GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(1000)
    cases = [("1000x1000 noise", noise(rng, 1000)), ("1000x1000 maze", maze(1000)), ("200x200 noise", noise(rng, 200))]
    m = ElevationMap(32, 0.1)
    say(f"bench_navplan: resolution {RES} m, default weights, outline on; rounds {args.rounds} (alternated), warmup {args.warmup}")
    for name, g in cases:
        n = g.shape[0]
        start, goal = (3, 4), (n - 5, n - 10)
        g[start[1], start[0]] = 0
        g[goal[1], goal[0]] = 0
        cm = m.costmap(n, n, RES, 0.0, 0.0, 0)
        cm.write(g)
        ws, wg = ((start[0] + 0.5) * RES, (start[1] + 0.5) * RES), ((goal[0] + 0.5) * RES, (goal[1] + 0.5) * RES)
        pot_h, cells_h, st_h = gem_amd.nav_plan_host(g, start, goal)
        path, st = cm.nav_plan(ws, wg)
        pot_d, cells_d = cm.read_potential()
        assert pot_d.tobytes() == pot_h.tobytes() and cells_d.tolist() == cells_h.tolist() and st["found"] == st_h["found"] == 1, name
        rows = ("navplan", "potential_only", "host_baseline")
        times = {r: [] for r in rows}
        last = st

        def run(row):
            nonlocal last
            m.synchronize()
            t = time.perf_counter()
            if row == "navplan":
                _, last = cm.nav_plan(ws, wg)
            elif row == "potential_only":
                cm.nav_plan(ws, ws)
            else:
                gem_amd.nav_plan_host(cm.read(), start, goal)
            return time.perf_counter() - t

        for r in range(args.warmup + args.rounds):
            for row in rows:
                dt = run(row)
                if r >= args.warmup:
                    times[row].append(dt * 1e6)
        say(f"{name}: {int((pot_h != gem_amd._lib.NAV_UNREACHED).sum())} cells reached, a plan of {st['n_path']} cells; "
            f"rounds {last['rounds']}, chunks {last['chunks']}; potential and path equal to the host twin byte for byte")
        say(f"  {'row':<22} {'median us':>11} {'min us':>11} {'max us':>11}   rounds")
        med = {}
        for row, v in times.items():
            v = np.array(v)
            med[row] = float(np.median(v))
            say(f"  {row:<22} {np.median(v):>11.1f} {v.min():>11.1f} {v.max():>11.1f}   {v.size}")
        say(f"  {'path (derived)':<22} {med['navplan'] - med['potential_only']:>11.1f}")
        ok = med["navplan"] < med["host_baseline"]
        say(f"  the device call costs {'less' if ok else 'NOT less'} than the read plus the host twin ({med['navplan']:.1f} us against "
            f"{med['host_baseline']:.1f} us); the {'path' if med['navplan'] - med['potential_only'] > med['potential_only'] else 'potential'} "
            f"is the larger part of it")
        cm.close()
    m.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
