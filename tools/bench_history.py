"""Timing of gem_costmap_mark_history (the history cloud marked where it lies, blocks off the costmap culled) against the paths it
replaces.  Needs a GPU; prints a table and, with --out, writes it to a file as well.

Input: a history of about N records (--records, default 2e6 and 8e6) laid by appends along a meandering trajectory several times the
costmap's 200 m window -- one append of --per-frame random-noise records per 0.2 m step, scattered over the 20 m x 20 m around the
robot, travers uniform in [0, 1] -- and a 1000 x 1000 costmap at 0.2 m rolled to the trajectory's end.
Rows, all with bounds NULL and a gem_synchronize behind the call (host clock around both):
  history_cull_on    gem_costmap_mark_history, "history_cull" 1
  history_cull_off   gem_costmap_mark_history, "history_cull" 0
  points_device      gem_costmap_mark_points_device over the same records in a caller's buffer: the parent's path, the baseline
  points_host        gem_costmap_mark_points from a host array: the upload the history replaces
The rows are alternated round by round (--rounds), after --warmup rounds; each row reports its median and the min .. max of its
rounds.  Before timing, all four rows are run once into fresh costmaps and their grids compared byte for byte."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from gem_amd import ElevationMap  # noqa: E402
from gem_amd.api import POINT_DTYPE  # noqa: E402

THRESH = 0.5


def trajectory_point(s):
    """arc-length-ish parameter s (metres along x) -> position: a meander 120 m wide"""
    return np.array([s, 60.0 * np.sin(s / 150.0)])


def build_history(m, n_records, per_frame, seed):
    """appends along the trajectory; returns (records appended, last position, path length in x)"""
    rng = np.random.default_rng(seed)
    frames = max(1, n_records // per_frame)
    chunk = 256                                              # frames generated per host batch (each frame is still one append)
    pos = trajectory_point(0.0)
    total = 0
    for f0 in range(0, frames, chunk):
        k = min(chunk, frames - f0)
        rec = np.zeros((k, per_frame), POINT_DTYPE)
        centres = np.stack([trajectory_point(0.2 * (f0 + i)) for i in range(k)])
        rec["x"] = (centres[:, :1] + rng.uniform(-10.0, 10.0, (k, per_frame))).astype(np.float32)
        rec["y"] = (centres[:, 1:] + rng.uniform(-10.0, 10.0, (k, per_frame))).astype(np.float32)
        rec["z"] = rng.normal(0.0, 0.3, (k, per_frame)).astype(np.float32)
        rec["travers"] = rng.uniform(0.0, 1.0, (k, per_frame)).astype(np.float32)
        rec["intensity"] = rng.uniform(0.0, 100.0, (k, per_frame)).astype(np.float32)
        for i in range(k):
            m.history_append(rec[i])
        total += k * per_frame
        pos = centres[-1]
    return total, pos, 0.2 * frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, nargs="+", default=[2_000_000, 8_000_000])
    ap.add_argument("--per-frame", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_history.py needs a GPU")

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"bench_history: rounds {args.rounds} (alternated), warmup {args.warmup}, costmap 1000 x 1000 at 0.2 m, {args.per_frame} records per append")
    for n_records in args.records:
        m = ElevationMap(32, 0.1)
        m.history_enable(1 << 20)
        t0 = time.perf_counter()
        n, pos, length = build_history(m, n_records, args.per_frame, seed=n_records)
        m.synchronize()
        build_s = time.perf_counter() - t0
        host = m.history_export()
        assert host.shape[0] == n == m.history_size()
        dev_copy = torch.from_numpy(host.view(np.uint8).reshape(-1, 32)).to("cuda:0")
        maps = {name: m.costmap(1000, 1000, 0.2) for name in ("history_cull_on", "history_cull_off", "points_device", "points_host")}
        for c in maps.values():
            c.roll_to(float(pos[0]), float(pos[1]))

        def run(name):
            c = maps[name]
            if name.startswith("history"):
                m.debug_set("history_cull", 1 if name.endswith("on") else 0)
                c.mark_history(THRESH, None)
            elif name == "points_device":
                c.mark_points(dev_copy, THRESH, None)
            else:
                c.mark_points(host, THRESH, None)
            m.synchronize()

        # the same grid from all four, once
        grids = {}
        culled = {}
        for name in maps:
            run(name)
            if name.startswith("history"):
                culled[name] = m.debug_get("history_blocks_culled")
            grids[name] = maps[name].read().tobytes()
        first = grids["points_device"]
        assert all(g == first for g in grids.values()), "the four paths disagree"
        marked = int((np.frombuffer(first, np.uint8) != 255).sum())
        blocks = m.debug_get("history_blocks")
        say()
        say(f"history of {n} records ({n * 32 / 1e6:.0f} MB) along {length:.0f} m of trajectory, built by {n // args.per_frame} appends in {build_s:.2f} s; "
            f"{blocks} blocks, {culled['history_cull_on']} culled with cull on, {culled['history_cull_off']} with cull off; "
            f"{marked} of 1000000 cells marked; the four grids are byte-identical")
        times = {name: [] for name in maps}
        for r in range(args.warmup + args.rounds):
            for name in maps:                                    # alternated: one call of each row per round
                t = time.perf_counter()
                run(name)
                dt = time.perf_counter() - t
                if r >= args.warmup:
                    times[name].append(dt * 1e6)
        say(f"  {'row':<18} {'median us':>10} {'min us':>10} {'max us':>10}   rounds")
        for name, v in times.items():
            v = np.array(v)
            say(f"  {name:<18} {np.median(v):>10.1f} {v.min():>10.1f} {v.max():>10.1f}   {v.size}")
        for c in maps.values():
            c.close()
        del dev_copy
        m.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
