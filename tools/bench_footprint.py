"""Timing of gem_costmap_score_trajectories (a planning cycle's trajectories scored against the grid where it lies) against what a
caller does today.  Needs a GPU; prints a table and, with --out, writes it to a file as well.

Input: --trajectories (default 2000) trajectories of --poses (default 30) poses of the reference node's rectangular footprint
(layers/params/costmap_common_params_local.yaml:8): a trajectory starts at a random pose inside the map and advances 0.1 m per pose
along a heading that turns by a random constant rate, the way a local planner's samples do.  The grids are random noise, bytes uniform
in 0 .. 252 with --lethal (default 0.1 %) of the cells 254 and as many 255: 75 x 75 at 0.2 m (the local window) and 1000 x 1000 at
0.2 m.
Rows, host clock around the call and, where the call only enqueues, a gem_synchronize:
  score_device       gem_costmap_score_trajectories_device: poses and results in device memory
  score_host         gem_costmap_score_trajectories: poses up, results down
  read_and_host_loop the baseline: gem_costmap_read of the whole grid, then a single-thread C++ restatement of the same loop
                     (tools/footprint_host.cpp, compiled by this tool with -O2 -ffp-contract=off)
  host_loop_only     that loop alone, the grid already on the host
The rows are alternated round by round (--rounds), after --warmup rounds; each row reports its median and the min .. max of its
rounds.  Before timing, the rows' trajectory costs are compared with each other, integer for integer."""
import argparse
import ctypes as C
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from gem_amd import ElevationMap  # noqa: E402

RECTANGLE = np.array([[-0.64, -0.40], [-0.64, 0.40], [0.64, 0.40], [0.64, -0.40]], np.float64)


def build_host_loop(td):
    lib = Path(td) / "libfootprint_host.so"
    subprocess.run(["c++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", str(ROOT / "tools" / "footprint_host.cpp"), "-o", str(lib)],
                   check=True)
    fn = C.CDLL(str(lib)).host_score_trajectories
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_int,
                   C.c_int, C.c_void_p]
    return fn


def trajectories(rng, n_traj, T, size, res):
    x = rng.uniform(0.1 * size * res, 0.9 * size * res, n_traj)
    y = rng.uniform(0.1 * size * res, 0.9 * size * res, n_traj)
    th = rng.uniform(-np.pi, np.pi, n_traj)
    rate = rng.uniform(-0.1, 0.1, n_traj)
    out = np.empty((n_traj, T, 4), np.float64)
    for k in range(T):
        out[:, k, 0], out[:, k, 1], out[:, k, 2], out[:, k, 3] = x, y, np.cos(th), np.sin(th)
        x, y, th = x + 0.1 * np.cos(th), y + 0.1 * np.sin(th), th + rate
    return out.reshape(-1, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trajectories", type=int, default=2000)
    ap.add_argument("--poses", type=int, default=30)
    ap.add_argument("--sizes", type=int, nargs="+", default=[75, 1000])
    ap.add_argument("--lethal", type=float, default=0.001)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_footprint.py needs a GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    nt, T, res = args.trajectories, args.poses, 0.2
    say(f"bench_footprint: {nt} trajectories x {T} poses, the 1.28 m x 0.80 m rectangle, rounds {args.rounds} (alternated), warmup {args.warmup}")
    with tempfile.TemporaryDirectory() as td:
        host_loop = build_host_loop(td)
        for size in args.sizes:
            rng = np.random.default_rng(size)
            grid = rng.integers(0, 253, (size, size), dtype=np.uint8)
            u = rng.random((size, size))
            grid[u < args.lethal] = 254
            grid[(u >= args.lethal) & (u < 2 * args.lethal)] = 255
            poses = trajectories(rng, nt, T, size, res)
            m = ElevationMap(32, 0.1)
            cm = m.costmap(size, size, res)
            cm.write(grid)
            d_poses = torch.from_numpy(poses).to("cuda:0")
            host_grid = grid.copy()
            out = {}

            def run(name):
                if name == "score_device":
                    out[name] = cm.score_trajectories(d_poses, T, RECTANGLE)
                    m.synchronize()
                elif name == "score_host":
                    out[name] = cm.score_trajectories(poses, T, RECTANGLE)
                else:
                    g = cm.read() if name == "read_and_host_loop" else host_grid
                    t = np.zeros(nt, np.int32)
                    host_loop(g.ctypes.data, size, size, res, 0.0, 0.0, poses.ctypes.data, nt, T, RECTANGLE.ctypes.data, 4, 0, t.ctypes.data)
                    out[name] = t

            rows = ("score_device", "score_host", "read_and_host_loop", "host_loop_only")
            for name in rows:
                run(name)
            first = out["score_device"].cpu().numpy()
            assert all(np.array_equal(first, out[name]) for name in rows[1:]), "the rows disagree"
            say()
            say(f"{size} x {size} at {res} m ({size * size / 1e3:.1f} KB): {int((first < 0).sum())} of {nt} trajectories end negative, "
                f"the others' mean cost is {float(first[first >= 0].mean()) if (first >= 0).any() else 0.0:.1f}; the four rows' costs are identical")
            times = {name: [] for name in rows}
            for r in range(args.warmup + args.rounds):
                for name in rows:                                    # alternated: one call of each row per round
                    t = time.perf_counter()
                    run(name)
                    dt = time.perf_counter() - t
                    if r >= args.warmup:
                        times[name].append(dt * 1e6)
            say(f"  {'row':<20} {'median us':>10} {'min us':>10} {'max us':>10}   rounds")
            for name, v in times.items():
                v = np.array(v)
                say(f"  {name:<20} {np.median(v):>10.1f} {v.min():>10.1f} {v.max():>10.1f}   {v.size}")
            cm.close()
            del d_poses
            m.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
