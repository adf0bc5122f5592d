"""Timing of gem_costmap_rollout_best_device -- TrajectoryPlanner::createTrajectories on the device costmap -- against what a caller
without it does: read the local costmap's bytes and both distance grids back, roll out on the CPU, hold the answer.  Needs a GPU;
prints a table and, with --out, writes it to a file as well.

Workload: the reference's local costmap, 75 x 75 at 0.2 m, with seeded costs below 253 everywhere, a sprinkle of lethal blocks outside
a free disc around the robot, a plan across the diagonal, the launch files' rectangle (+-0.64, +-0.40).  The robot stands at the map's
centre heading along the plan.  Two plans:
  defaults   TrajectoryPlannerROS's defaults: 3 x 20 samples, holonomic, four y_vels -- 87 candidates
  20 x 40    vx_samples 20, vtheta_samples 40 -- 847 candidates
Rows, host clock (time.perf_counter) between two gem_synchronize, every call through ctypes on buffers made before the clock starts:
  A read+twin         gem_costmap_read, gem_costmap_mapgrid_read of PATH and of GOAL, gem_rollout_host (the host twin: the same arithmetic
                      as the kernels, one thread): the baseline is never the code under test
  A1 read alone       the three read-backs alone
  A2 twin alone       gem_rollout_host alone
  B rollout_best      gem_costmap_rollout_best_device, gem_synchronize, the 64-byte download
  B x20               twenty enqueued back to back, one synchronize, divided by twenty: what the two launches cost without the wait
  D dwa_best          gem_costmap_dwa_best_device at a like sample count and length (obstacle, path and goal critics), gem_synchronize, its
                      32-byte download: beside the others for scale, another planner's answer
The rows are alternated round by round (--rounds) after --warmup rounds; each reports its median and the min .. max of its rounds.
Before timing the device answer is compared with the twin's byte for byte, the costs and `ahead` too."""
import argparse
import ctypes as C
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import gem_amd  # noqa: E402
from gem_amd import ElevationMap, _lib, map_grid_critic, obstacle_critic  # noqa: E402

SIZE, RES = 75, 0.2
RECTANGLE = [[-0.64, -0.40], [-0.64, 0.40], [0.64, 0.40], [0.64, -0.40]]
DEFAULTS = dict(sim_time=1.0, sim_granularity=0.025, angular_sim_granularity=0.025, sim_period=0.05, pdist_scale=0.6, gdist_scale=0.8,
                occdist_scale=0.01, heading_lookahead=0.325, max_vel_x=0.5, min_vel_x=0.1, max_vel_th=1.0, min_vel_th=-1.0,
                min_in_place_vel_th=0.4, backup_vel=-0.1, acc_lim_x=2.5, acc_lim_y=2.5, acc_lim_theta=3.2, vx_samples=3, vtheta_samples=20,
                dwa=1, holonomic_robot=1, y_vels=(-0.3, -0.1, 0.1, 0.3))
WORKLOADS = {"defaults": DEFAULTS, "20 x 40": dict(DEFAULTS, vx_samples=20, vtheta_samples=40)}
DWA_LIMITS = dict(max_vel_x=0.5, min_vel_x=0.1, max_vel_y=0.0, min_vel_y=0.0, max_vel_theta=1.0, min_vel_theta=0.4, max_vel_trans=-1.0,
                  min_vel_trans=-1.0, acc_lim_x=2.5, acc_lim_y=2.5, acc_lim_theta=3.2)


def local_map():
    rng = np.random.default_rng(SIZE)
    g = rng.integers(0, 253, (SIZE, SIZE), dtype=np.uint8)
    ys, xs = np.mgrid[0:SIZE, 0:SIZE]
    far = (ys - SIZE // 2) ** 2 + (xs - SIZE // 2) ** 2 > 12 ** 2
    for _ in range(40):                                                   # lethal blocks of 2 x 2 outside the disc
        y, x = rng.integers(0, SIZE - 2, 2)
        if far[y, x] and abs(int(y) - int(x)) > 3:                        # (and off the plan's diagonal)
            g[y:y + 2, x:x + 2] = 254
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout.py needs a GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    for name in WORKLOADS:
        table(args, name, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


def table(args, name, say):
    import torch
    m = ElevationMap(32, 0.1)
    lib, h = m._lib, m._h
    cm = m.costmap(SIZE, SIZE, RES, 0.0, 0.0, _lib.COST_FREE_SPACE)
    cm.write(local_map())
    line = np.stack([np.linspace(0.5 * RES, (SIZE - 0.5) * RES, 40)] * 2, axis=1)
    cm.prepare_map_grid(line)
    pos, vel = ((SIZE // 2 + 0.5) * RES, (SIZE // 2 + 0.5) * RES, math.pi / 4), (0.3, 0.0, 0.1)
    plan = gem_amd.rollout_plan(WORKLOADS[name], pos, vel, 0)
    nc = int(plan.n_cand)
    p3, v3 = (C.c_double * 3)(*pos), (C.c_double * 3)(*vel)
    spec = np.ascontiguousarray(RECTANGLE, np.float64)
    ps = spec.ctypes.data_as(C.POINTER(C.c_double))
    geom = _lib.CostmapConfig(SIZE, SIZE, RES, 0.0, 0.0, 0)
    bytes_, path, goal = np.zeros((SIZE, SIZE), np.uint8), np.zeros((SIZE, SIZE), np.int32), np.zeros((SIZE, SIZE), np.int32)
    cost, ahead, steps = np.zeros(nc), np.zeros(nc, np.int32), np.zeros(nc, np.int32)
    twin_best = _lib.RolloutBest()
    d_best = torch.empty(64, dtype=torch.uint8, device="cuda:0")
    d_cost = torch.empty(nc, dtype=torch.float64, device="cuda:0")
    d_ahead = torch.empty(nc, dtype=torch.int32, device="cuda:0")
    h_best = torch.empty(64, dtype=torch.uint8).pin_memory()
    P = lambda t: C.c_void_p(t.data_ptr())
    A = lambda a: a.ctypes.data_as(C.c_void_p)
    # the DWA plan beside them: as many samples, as many poses, three critics
    n_th = max(2, round(nc / int(plan.n_vx)))
    T = int(plan.max_steps)
    dwa_cfg = dict(sim_time=1.0, sim_granularity=1.0 / T * 1.000001, angular_sim_granularity=0.025, sim_period=0.05, use_dwa=True, discretize_by_time=True,
                   continued_acceleration=False, oscillation_flags=0, vsamples=(int(plan.n_vx), 1, n_th))
    dwa = gem_amd.trajgen_plan(DWA_LIMITS, dwa_cfg, pos, vel)
    assert dwa.max_steps == T, (dwa.max_steps, T)
    critics = [obstacle_critic(0.01), map_grid_critic(0.6, _lib.MAPGRID_PATH, 0.0, _lib.MAPGRID_STOP_ON_FAILURE),
               map_grid_critic(0.8, _lib.MAPGRID_GOAL, 0.0, _lib.MAPGRID_STOP_ON_FAILURE)]
    cs = (_lib.Critic * 3)(*critics)
    f3, g3 = (C.c_float * 3)(*pos), (C.c_float * 3)(*vel)
    d_dwa = torch.empty(4, dtype=torch.int64, device="cuda:0")
    h_dwa = torch.empty(4, dtype=torch.int64).pin_memory()

    def check(rc):
        if rc != _lib.GEM_OK:
            raise SystemExit(f"a call failed ({rc})")

    def read_back():
        check(lib.gem_costmap_read(h, cm.id, 0, 0, SIZE, SIZE, A(bytes_), SIZE))
        s, gc = C.c_int(0), (C.c_int * 2)()
        check(lib.gem_costmap_mapgrid_read(h, cm.id, _lib.MAPGRID_PATH, A(path), C.byref(s), gc))
        check(lib.gem_costmap_mapgrid_read(h, cm.id, _lib.MAPGRID_GOAL, A(goal), C.byref(s), gc))

    def twin():
        check(lib.gem_rollout_host(C.byref(plan), p3, v3, C.byref(geom), A(bytes_), A(path), A(goal), ps, 4, 0, A(cost), A(ahead), A(steps), None,
                                   C.byref(twin_best)))

    def enqueue_b(with_costs=False):
        check(lib.gem_costmap_rollout_best_device(h, cm.id, C.byref(plan), p3, v3, 0, ps, 4, 0, P(d_cost) if with_costs else None,
                                                  P(d_ahead) if with_costs else None, P(d_best)))

    def answer_b():
        m.synchronize()
        h_best.copy_(d_best)
        return h_best.numpy().tobytes()

    def row_d():
        check(lib.gem_costmap_dwa_best_device(h, cm.id, cs, 3, C.byref(dwa), f3, g3, T, ps, 4, None, P(d_dwa)))
        m.synchronize()
        h_dwa.copy_(d_dwa)

    read_back()
    twin()
    enqueue_b(with_costs=True)
    got = answer_b()
    assert got == bytes(twin_best), "the device answer is not the twin's"
    assert d_cost.cpu().numpy().tobytes() == cost.tobytes() and d_ahead.cpu().numpy().tobytes() == ahead.tobytes(), "the candidates differ"
    a = gem_amd.rollout_answer(twin_best)
    say(f"bench_rollout [{name}]: {SIZE} x {SIZE} at {RES} m ({100.0 * float((bytes_ >= 253).mean()):.1f} % blocked), the rectangle; {nc} candidates "
        f"({plan.n_vx} x {plan.n_vth}) of at most {T} steps, {int((cost >= 0).sum())} legal; rounds {args.rounds} (alternated), warmup {args.warmup}")
    say(f"  device and twin answer candidate {a['index']} in stage {a['stage']} at {a['cost']!r}, velocity {a['velocity']}; costs and ahead equal byte for byte")
    say(f"  bytes across the link per cycle (the arrays' sizes): A {bytes_.nbytes + path.nbytes + goal.nbytes} down, B {C.sizeof(_lib.RolloutPlan)} in "
        f"kernel arguments + 64 down; D: {int(dwa.n_traj)} samples of {T} poses, 3 critics")

    rows = ("A read+twin", "A1 read alone", "A2 twin alone", "B rollout_best", "B x20", "D dwa_best")
    times = {r: [] for r in rows}

    def run(row):
        m.synchronize()
        t = time.perf_counter()
        if row == "A read+twin":
            read_back()
            twin()
        elif row == "A1 read alone":
            read_back()
        elif row == "A2 twin alone":
            twin()
        elif row == "B rollout_best":
            enqueue_b()
            answer_b()
        elif row == "B x20":
            for _ in range(20):
                enqueue_b()
            m.synchronize()
        else:
            row_d()
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
    ma, mb = float(np.median(times["A read+twin"])), float(np.median(times["B rollout_best"]))
    say(f"  B against A: {mb:.1f} us against {ma:.1f} us")
    say("  NOT MEASURED: the kernels' own durations (no trace was taken), counters, other group widths, other maps and footprints")
    cm.close()
    m.close()


if __name__ == "__main__":
    main()
