"""Timing of gem_costmap_best_trajectory_device against the way a DWA cycle ended before it: five scoring launches, five result arrays
across the link and the combination on the host.  Needs a GPU; prints a table and, with --out, writes it to a file as well.

Workload: tools/bench_mapgrid.py's local costmap of 400 x 400 at 0.05 m (marked from a seeded noise cloud, inflated with R = 11), its
plan across the diagonal, 2 000 trajectories of 30 device poses, the robot's rectangle, and DWA's obstacle and four grid critics
(goal_front, alignment, path, goal).  The table is made once per --density: at that tool's 0.02 points per cell two thirds of the
cells are blocked and the rectangle fits nowhere, so every trajectory is rejected by the first critic (row B then skips the grids,
row A cannot); at 0.001 some trajectories survive every critic.  Both are reported, with the valid count.
Rows, host clock (time.perf_counter) between two gem_synchronize, every call through ctypes on buffers made before the clock starts:
  A five_calls       gem_costmap_score_trajectories_device, gem_costmap_mapgrid_score_device four times (the front critic on the GOAL grid,
                     for want of a third at those entry points), gem_synchronize, five downloads into pinned host arrays, and
                     gem_critics_select over the five arrays converted to double
  B best_trajectory  gem_costmap_best_trajectory_device with the FRONT critic on the GOAL grid too, so that both rows time equal work,
                     gem_synchronize, and the 32-byte download
  A x20, B x20       twenty enqueued back to back, one synchronize, divided by twenty (no download, no combination): what the
                     enqueued work costs without the wait
The rows are alternated round by round (--rounds) after --warmup rounds; each reports its median and the min .. max of its rounds.
Before timing, both ways are compared: the same winner, cost and valid count."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from gem_amd import Costmap, ElevationMap, _lib, external_critic, map_grid_critic, obstacle_critic  # noqa: E402
from bench_mapgrid import FACTOR, INSCRIBED, N_TRAJ, RADIUS, RES, SIZE, T, THRESH, noise_cloud  # noqa: E402

RECTANGLE = [[-0.64, -0.40], [-0.64, 0.40], [0.64, 0.40], [0.64, -0.40]]
FORWARD = 0.325
SCALES = (0.01, 24.0, 32.0, 32.0, 24.0)                                  # obstacle, goal_front, alignment, path, goal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--density", type=float, nargs="+", default=[0.02, 0.001])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_critics.py needs a GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    for density in args.density:
        table(args, density, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


def table(args, density, say):
    import torch
    rng = np.random.default_rng(SIZE)
    m = ElevationMap(32, 0.1)
    lib, h = m._lib, m._h
    cm = m.costmap(SIZE, SIZE, RES, 0.0, 0.0, _lib.COST_FREE_SPACE)
    cm.mark_points(noise_cloud(rng, SIZE, density), THRESH, None)
    cm.inflate(RADIUS, INSCRIBED, FACTOR, False, None)
    plan = np.stack([np.linspace(0.5 * RES, (SIZE - 0.5) * RES, 60)] * 2, axis=1)
    cm.prepare_map_grid(plan)
    rs = np.random.default_rng(1)
    xy = rs.uniform(0.0, SIZE * RES, (N_TRAJ, 1, 2)) + rs.uniform(-2 * RES, 2 * RES, (N_TRAJ, T, 2)).cumsum(axis=1)
    poses = Costmap.poses_from_yaw(np.concatenate([xy.reshape(-1, 2), rs.uniform(-np.pi, np.pi, (N_TRAJ * T, 1))], axis=1))
    d_poses = torch.from_numpy(poses).to("cuda:0")
    spec = np.ascontiguousarray(RECTANGLE, np.float64)
    ps = spec.ctypes.data_as(C.POINTER(C.c_double))
    PATH, GOAL, STOP = _lib.MAPGRID_PATH, _lib.MAPGRID_GOAL, _lib.MAPGRID_STOP_ON_FAILURE
    grid_calls = ((GOAL, FORWARD, 0), (PATH, FORWARD, 0), (PATH, 0.0, STOP), (GOAL, 0.0, STOP))       # goal_front on GOAL | alignment | path | goal
    critics = [obstacle_critic(SCALES[0])] + [map_grid_critic(SCALES[k + 1], g, x, f) for k, (g, x, f) in enumerate(grid_calls)]
    cs = (_lib.Critic * 5)(*critics)
    # row A's buffers
    d_obst = torch.empty(N_TRAJ, dtype=torch.int32, device="cuda:0")
    d_grid = [torch.empty(N_TRAJ, dtype=torch.int64, device="cuda:0") for _ in range(4)]
    h_obst = torch.empty(N_TRAJ, dtype=torch.int32).pin_memory()
    h_grid = [torch.empty(N_TRAJ, dtype=torch.int64).pin_memory() for _ in range(4)]
    scores = np.zeros((5, N_TRAJ), np.float64)
    totals = np.zeros(N_TRAJ, np.float64)
    ext_cs = (_lib.Critic * 5)(*[external_critic(s, k) for k, s in enumerate(SCALES)])        # gem_critics_select reads the scales alone
    best_a = _lib.BestTrajectory()
    # row B's
    d_best = torch.empty(4, dtype=torch.int64, device="cuda:0")
    h_best = torch.empty(4, dtype=torch.int64).pin_memory()
    pp = C.c_void_p(d_poses.data_ptr())

    def check(rc):
        if rc != _lib.GEM_OK:
            raise SystemExit(f"a call failed ({rc})")

    def enqueue_a():
        check(lib.gem_costmap_score_trajectories_device(h, cm.id, pp, N_TRAJ, T, ps, 4, 0, None, C.c_void_p(d_obst.data_ptr())))
        for k, (g, x, f) in enumerate(grid_calls):
            check(lib.gem_costmap_mapgrid_score_device(h, cm.id, g, pp, N_TRAJ, T, x, f, C.c_void_p(d_grid[k].data_ptr())))

    def enqueue_b():
        check(lib.gem_costmap_best_trajectory_device(h, cm.id, cs, 5, pp, None, N_TRAJ, T, ps, 4, None, 0, None, C.c_void_p(d_best.data_ptr())))

    def row_a():
        enqueue_a()
        m.synchronize()
        h_obst.copy_(d_obst)
        for k in range(4):
            h_grid[k].copy_(d_grid[k])
        scores[0] = h_obst.numpy()
        for k in range(4):
            scores[k + 1] = h_grid[k].numpy()
        check(lib.gem_critics_select(ext_cs, 5, scores.ctypes.data_as(C.POINTER(C.c_double)), N_TRAJ, totals.ctypes.data_as(C.POINTER(C.c_double)),
                                     C.byref(best_a)))
        return best_a.index, best_a.cost, best_a.n_valid

    def row_b():
        enqueue_b()
        m.synchronize()
        h_best.copy_(d_best)
        return int(h_best[0]), float(h_best.view(torch.float64)[2]), int(h_best[1])

    a, b = row_a(), row_b()
    assert a == b, f"the two ways disagree: {a} against {b}"
    blocked = float((cm.read() >= 253).mean())
    say(f"bench_critics: {SIZE} x {SIZE} at {RES} m, {density} points per cell, inflated with R = 11 ({100.0 * blocked:.1f} % blocked); {N_TRAJ} trajectories of {T} device poses, "
        f"a 4-vertex footprint, 5 critics; rounds {args.rounds} (alternated), warmup {args.warmup}")
    say(f"  both ways answer trajectory {a[0]} at {a[1]!r} with {a[2]} valid of {N_TRAJ}")

    rows = ("A five_calls", "B best_trajectory", "A x20", "B x20")
    times = {r: [] for r in rows}

    def run(row):
        m.synchronize()
        t = time.perf_counter()
        if row == "A five_calls":
            row_a()
        elif row == "B best_trajectory":
            row_b()
        else:
            for _ in range(20):
                (enqueue_a if row == "A x20" else enqueue_b)()
            m.synchronize()
        dt = time.perf_counter() - t
        return dt / 20 if row.endswith("x20") else dt

    for r in range(args.warmup + args.rounds):
        for row in rows:
            dt = run(row)
            if r >= args.warmup:
                times[row].append(dt * 1e6)
    say(f"  {'row':<22} {'median us':>10} {'min us':>10} {'max us':>10}   rounds")
    for row, v in times.items():
        v = np.array(v)
        say(f"  {row:<22} {np.median(v):>10.1f} {v.min():>10.1f} {v.max():>10.1f}   {v.size}")
    ma, mb = float(np.median(times["A five_calls"])), float(np.median(times["B best_trajectory"]))
    say(f"  the bar, B below A: {'met' if mb < ma else 'MISSED'} ({mb:.1f} us against {ma:.1f} us)")
    say("  NOT MEASURED: the two kernels' own durations and the pick launch's share (no trace was taken), other batch sizes, other footprints")
    cm.close()
    m.close()


if __name__ == "__main__":
    main()
