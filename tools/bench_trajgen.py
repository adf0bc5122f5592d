"""Timing of gem_costmap_dwa_best_device -- DWA's trajectories generated on the device, then the critics -- against the way a cycle ran
before it: SimpleTrajectoryGenerator on the host, the poses across the link, then gem_costmap_best_trajectory_device.  Needs a GPU;
prints a table and, with --out, writes it to a file as well.

Workload: tools/bench_critics.py's local costmap of 400 x 400 at 0.05 m (marked from a seeded noise cloud, inflated with R = 11), its
plan across the diagonal, the robot's rectangle and its five critics (obstacle, goal_front, alignment, path, goal); 2 000 samples
(10 x 10 x 20 velocities, every list on the positive side so that nothing is inserted) of 30 poses each (by time: sim_time 1.5 s in 30
steps), the robot heading along the plan from the free spot nearest the map's centre (the centre itself where the rectangle fits
nowhere).  Every sample is generated.  The table is made once per --density (65 % and 5 % blocked, as there).
Rows, host clock (time.perf_counter) between two gem_synchronize, every call through ctypes on buffers made before the clock starts:
  A twin+upload+best  gem_trajgen_generate into pinned host arrays (the host twin: the same arithmetic as the kernel, one thread), three
                      asynchronous copies to the device (poses, lengths, external columns) and the wait for them,
                      gem_costmap_best_trajectory_device, gem_synchronize, the 32-byte download
  A1 twin alone       gem_trajgen_generate alone
  A2 upload alone     the three copies and their wait alone
  B dwa_best          gem_costmap_dwa_best_device, gem_synchronize, the 32-byte download
  B x20               twenty enqueued back to back, one synchronize, divided by twenty: what the three launches cost without the wait
The rows are alternated round by round (--rounds) after --warmup rounds; each reports its median and the min .. max of its rounds.
Before timing, both ways are compared: the same winner, cost and valid count.  Bytes across the link per cycle are stated, not
measured: the arrays' sizes."""
import argparse
import ctypes as C
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import gem_amd  # noqa: E402
from gem_amd import ElevationMap, _lib, map_grid_critic, obstacle_critic  # noqa: E402
from bench_critics import FORWARD, RECTANGLE, SCALES  # noqa: E402
from bench_mapgrid import FACTOR, INSCRIBED, N_TRAJ, RADIUS, RES, SIZE, T, THRESH, noise_cloud  # noqa: E402

LIMITS = dict(max_vel_x=0.55, min_vel_x=0.05, max_vel_y=0.1, min_vel_y=0.01, max_vel_theta=1.0, min_vel_theta=0.4, max_vel_trans=-1.0,
              min_vel_trans=-1.0, acc_lim_x=2.5, acc_lim_y=2.5, acc_lim_theta=3.2)
CONFIG = dict(sim_time=1.5, sim_granularity=0.0500001, angular_sim_granularity=0.1, sim_period=0.05, use_dwa=True, discretize_by_time=True,
              continued_acceleration=False, oscillation_flags=0, vsamples=(10, 10, 20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--density", type=float, nargs="+", default=[0.02, 0.001])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_trajgen.py needs a GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    for density in args.density:
        table(args, density, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


def free_start(grid, half=18):
    """the centre of the cell nearest the map's centre whose surrounding box of 2 * half + 1 cells holds no inscribed or lethal cell
    (the rectangle fits there at any heading); the map's centre where there is none"""
    blocked = (grid >= 253).astype(np.int32)
    c = np.pad(blocked.cumsum(axis=0).cumsum(axis=1), ((1, 0), (1, 0)))
    w = 2 * half + 1
    box = c[w:, w:] - c[:-w, w:] - c[w:, :-w] + c[:-w, :-w]
    ys, xs = np.nonzero(box == 0)
    if ys.size == 0:
        return 0.5 * SIZE * RES, 0.5 * SIZE * RES
    mid = (grid.shape[0] - 1) / 2.0
    k = int(np.argmin((ys + half - mid) ** 2 + (xs + half - mid) ** 2))
    return (xs[k] + half + 0.5) * RES, (ys[k] + half + 0.5) * RES


def table(args, density, say):
    import torch
    rng = np.random.default_rng(SIZE)
    m = ElevationMap(32, 0.1)
    lib, h = m._lib, m._h
    cm = m.costmap(SIZE, SIZE, RES, 0.0, 0.0, _lib.COST_FREE_SPACE)
    cm.mark_points(noise_cloud(rng, SIZE, density), THRESH, None)
    cm.inflate(RADIUS, INSCRIBED, FACTOR, False, None)
    line = np.stack([np.linspace(0.5 * RES, (SIZE - 0.5) * RES, 60)] * 2, axis=1)
    cm.prepare_map_grid(line)
    pos, vel = (*free_start(cm.read()), math.pi / 4), (0.3, 0.05, 0.3)
    plan = gem_amd.trajgen_plan(LIMITS, CONFIG, pos, vel)
    assert plan.n_traj == N_TRAJ and plan.max_steps == T, (plan.n_traj, plan.max_steps)
    p3, v3 = (C.c_float * 3)(*pos), (C.c_float * 3)(*vel)
    spec = np.ascontiguousarray(RECTANGLE, np.float64)
    ps = spec.ctypes.data_as(C.POINTER(C.c_double))
    PATH, GOAL, STOP = _lib.MAPGRID_PATH, _lib.MAPGRID_GOAL, _lib.MAPGRID_STOP_ON_FAILURE
    grid_calls = ((GOAL, FORWARD, 0), (PATH, FORWARD, 0), (PATH, 0.0, STOP), (GOAL, 0.0, STOP))       # goal_front on GOAL | alignment | path | goal
    critics = [obstacle_critic(SCALES[0])] + [map_grid_critic(SCALES[k + 1], g, x, f) for k, (g, x, f) in enumerate(grid_calls)]
    cs = (_lib.Critic * 5)(*critics)
    # row A's buffers: pinned host arrays the twin writes, their device copies
    h_poses = torch.zeros((N_TRAJ * T, 4), dtype=torch.float64).pin_memory()
    h_lens = torch.zeros(N_TRAJ, dtype=torch.int32).pin_memory()
    h_ext = torch.zeros((2, N_TRAJ), dtype=torch.float64).pin_memory()
    d_poses, d_lens, d_ext = (torch.empty_like(t, device="cuda:0") for t in (h_poses, h_lens, h_ext))
    link_a = sum(t.numel() * t.element_size() for t in (h_poses, h_lens, h_ext))
    link_b = C.sizeof(_lib.DwaPlan) + 24                                  # the kernel arguments carry the lists, the state and the parameters
    d_best = torch.empty(4, dtype=torch.int64, device="cuda:0")
    h_best = torch.empty(4, dtype=torch.int64).pin_memory()
    P = lambda t: C.c_void_p(t.data_ptr())

    def check(rc):
        if rc != _lib.GEM_OK:
            raise SystemExit(f"a call failed ({rc})")

    def twin():
        check(lib.gem_trajgen_generate(C.byref(plan), p3, v3, P(h_poses), P(h_lens), P(h_ext), None, T))

    def upload():
        d_poses.copy_(h_poses, non_blocking=True)
        d_lens.copy_(h_lens, non_blocking=True)
        d_ext.copy_(h_ext, non_blocking=True)
        torch.cuda.current_stream().synchronize()                        # the handle's stream knows nothing of this one

    def enqueue_b():
        check(lib.gem_costmap_dwa_best_device(h, cm.id, cs, 5, C.byref(plan), p3, v3, T, ps, 4, None, P(d_best)))

    def answer():
        m.synchronize()
        h_best.copy_(d_best)
        return int(h_best[0]), float(h_best.view(torch.float64)[2]), int(h_best[1])

    def row_a():
        twin()
        upload()
        check(lib.gem_costmap_best_trajectory_device(h, cm.id, cs, 5, P(d_poses), P(d_lens), N_TRAJ, T, ps, 4, P(d_ext), 2, None, P(d_best)))
        return answer()

    def row_b():
        enqueue_b()
        return answer()

    a, b = row_a(), row_b()
    assert a == b, f"the two ways disagree: {a} against {b}"
    assert int(h_lens.min()) == T, "every sample is generated"
    blocked = float((cm.read() >= 253).mean())
    say(f"bench_trajgen: {SIZE} x {SIZE} at {RES} m, {density} points per cell, inflated with R = 11 ({100.0 * blocked:.1f} % blocked); {N_TRAJ} samples "
        f"(10 x 10 x 20) of {T} poses, a 4-vertex footprint, 5 critics; rounds {args.rounds} (alternated), warmup {args.warmup}")
    say(f"  the robot starts at ({pos[0]:.3f}, {pos[1]:.3f}) heading pi / 4; both ways answer trajectory {a[0]} at {a[1]!r} with {a[2]} valid of {N_TRAJ}")
    say(f"  bytes across the link per cycle (the arrays' sizes): A {link_a} up + 32 down, B {link_b} in kernel arguments + 32 down")

    rows = ("A twin+upload+best", "A1 twin alone", "A2 upload alone", "B dwa_best", "B x20")
    times = {r: [] for r in rows}

    def run(row):
        m.synchronize()
        t = time.perf_counter()
        if row == "A twin+upload+best":
            row_a()
        elif row == "A1 twin alone":
            twin()
        elif row == "A2 upload alone":
            upload()
        elif row == "B dwa_best":
            row_b()
        else:
            for _ in range(20):
                enqueue_b()
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
    ma, mb = float(np.median(times["A twin+upload+best"])), float(np.median(times["B dwa_best"]))
    say(f"  B against A: {mb:.1f} us against {ma:.1f} us")
    say("  NOT MEASURED: k_trajgen's own duration (no trace was taken), other sample counts and lengths, continued acceleration")
    cm.close()
    m.close()


if __name__ == "__main__":
    main()
