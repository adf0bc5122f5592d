"""Timing of gem_costmap_mapgrid_prepare / _score against the path there was before them: gem_costmap_read of the whole map plus
MapGrid::computeTargetDistance's literal queue run twice (path, goal) on the host, in C++ (the `bench` mode of
tests/cpp/mapgrid_check.cpp; not the Python restatement).  Needs a GPU; prints a table and, with --out, writes it to a file as well.

Workload: the local costmap of 400 x 400 at 0.05 m, default value FREE_SPACE, marked by gem_costmap_mark_points from a seeded noise
cloud (--density points per cell, uniform over the map, travers uniform around the threshold, so about half of them lethal: 1 % of
the cells at the default) and inflated with R = 11 cells (inflation radius 0.55 m, inscribed radius 0.3 m).  The plan is 60 points
across the map's diagonal.
Rows, host clock (time.perf_counter) between two gem_synchronize:
  prepare_wait     gem_costmap_mapgrid_prepare(PATH | GOAL) and the wait for it
  prepare_x20      twenty calls enqueued back to back, one synchronize, divided by twenty: what a call costs without the wait
  score_2000x30    gem_costmap_mapgrid_score_device of 2 000 trajectories of 30 device poses against the path grid (Last, xshift 0)
These rows are alternated round by round (--rounds) after --warmup rounds; each reports its median and the min .. max of its rounds.
  host_baseline    the child process: read + adjustPlanResolution + the literal queue twice, its own clock, the same number of rounds
                   after two of warm-up.  It is a process of its own, so it cannot alternate with the rows above: it runs once before
                   and once after them, and both runs are reported.
Before timing, both grids are compared with tests/mapgrid_ref.py's set form byte for byte."""
import argparse
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from gem_amd import POINT_DTYPE, Costmap, ElevationMap, _lib  # noqa: E402
import costmap_ref as cref  # noqa: E402
import mapgrid_ref as ref  # noqa: E402

RES, THRESH, SIZE = 0.05, 0.5, 400
RADIUS, INSCRIBED, FACTOR = 0.55, 0.3, 10.0
N_TRAJ, T = 2000, 30


def noise_cloud(rng, size, density):
    n = int(size * size * density)
    pts = np.zeros(n, POINT_DTYPE)
    pts["x"] = rng.uniform(0.0, size * RES, n).astype(np.float32)
    pts["y"] = rng.uniform(0.0, size * RES, n).astype(np.float32)
    pts["travers"] = rng.uniform(THRESH - 0.3, THRESH + 0.3, n).astype(np.float32)
    return pts


def build_baseline(out: Path) -> Path:
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc", "-std=c++17", "-O2", "-I", str(ROOT / "include"),
           str(ROOT / "tests" / "cpp" / "mapgrid_check.cpp"), "-o", str(out), f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}",
           "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--density", type=float, default=0.02)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-exe", type=str, default="", help="a built tests/cpp/mapgrid_check.cpp (default: built into a temporary directory)")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mapgrid.py needs a GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(SIZE)
    m = ElevationMap(32, 0.1)
    cm = m.costmap(SIZE, SIZE, RES, 0.0, 0.0, _lib.COST_FREE_SPACE)
    cm.mark_points(noise_cloud(rng, SIZE, args.density), THRESH, None)
    lethal = int((cm.read() == 254).sum())
    cm.inflate(RADIUS, INSCRIBED, FACTOR, False, None)
    grid = cm.read()
    plan = np.stack([np.linspace(0.5 * RES, (SIZE - 0.5) * RES, 60)] * 2, axis=1)
    host = cref.Costmap(SIZE, SIZE, RES, 0.0, 0.0, cref.FREE_SPACE)
    host.grid[:] = grid
    want = ref.grids(host, plan)
    cm.prepare_map_grid(plan)
    for bit, name in ((_lib.MAPGRID_PATH, "path"), (_lib.MAPGRID_GOAL, "goal")):
        got, started, goal = cm.read_map_grid(bit)
        assert got.tobytes() == want[name].tobytes() and started == want["started"] and goal == want["goal_cell"], f"the {name} grid differs from the set form"
    OB, UN = ref.constants(grid)
    levels = {k: int(want[k][want[k] < OB].max()) for k in ("path", "goal")}
    reached = {k: int((want[k] < OB).sum()) for k in ("path", "goal")}
    n_adj = ref.adjust_plan(plan, RES).shape[0]
    say(f"bench_mapgrid: {SIZE} x {SIZE} at {RES} m, {args.density} points per cell -> {lethal} lethal cells ({100.0 * lethal / SIZE ** 2:.2f} %), inflated "
        f"with R = 11: {int((grid >= 253).sum())} blocked cells ({100.0 * (grid >= 253).mean():.1f} %); rounds {args.rounds} (alternated), warmup {args.warmup}")
    say(f"  plan: 60 points across the diagonal, {n_adj} after adjustPlanResolution; started = {want['started']}, goal cell {want['goal_cell']}")
    say(f"  path grid: {reached['path']} cells reached in {levels['path']} levels; goal grid: {reached['goal']} cells in {levels['goal']} levels; "
        f"both equal to the set form of tests/mapgrid_ref.py byte for byte")

    with tempfile.TemporaryDirectory() as td:
        exe = Path(args.baseline_exe) if args.baseline_exe else build_baseline(Path(td) / "mapgrid_check")
        gpath, ppath = Path(td) / "grid.bin", Path(td) / "plan.bin"
        gpath.write_bytes(grid.tobytes())
        ppath.write_bytes(np.ascontiguousarray(plan, np.float64).tobytes())

        def baseline():
            res = subprocess.run([str(exe), "bench", str(gpath), str(SIZE), str(SIZE), repr(RES), str(ppath), str(args.rounds)],
                                 capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                raise SystemExit("the baseline child failed:\n" + res.stdout + res.stderr)
            return [float(v) for v in res.stdout.split("\n") if v and not v.startswith("check")]

        base = [baseline()]
        rs = np.random.default_rng(1)
        xy = rs.uniform(0.0, SIZE * RES, (N_TRAJ, 1, 2)) + rs.uniform(-2 * RES, 2 * RES, (N_TRAJ, T, 2)).cumsum(axis=1)
        poses = Costmap.poses_from_yaw(np.concatenate([xy.reshape(-1, 2), rs.uniform(-np.pi, np.pi, (N_TRAJ * T, 1))], axis=1))
        d_poses = torch.from_numpy(poses).to("cuda:0")
        first = cm.score_map_grid(_lib.MAPGRID_PATH, d_poses, T)
        m.synchronize()
        assert first.cpu().numpy().tolist() == cm.score_map_grid(_lib.MAPGRID_PATH, poses, T).tolist(), "device and host poses score differently"
        rows = ("prepare_wait", "prepare_x20", "score_2000x30")
        times = {r: [] for r in rows}

        def run(row):
            m.synchronize()
            t = time.perf_counter()
            if row == "score_2000x30":
                cm.score_map_grid(_lib.MAPGRID_PATH, d_poses, T)
            else:
                for _ in range(20 if row == "prepare_x20" else 1):
                    cm.prepare_map_grid(plan)
            m.synchronize()
            dt = time.perf_counter() - t
            return dt / 20 if row == "prepare_x20" else dt

        for r in range(args.warmup + args.rounds):
            for row in rows:
                dt = run(row)
                if r >= args.warmup:
                    times[row].append(dt * 1e6)
        base.append(baseline())
    say(f"  {'row':<22} {'median us':>10} {'min us':>10} {'max us':>10}   rounds")
    for row, v in times.items():
        v = np.array(v)
        say(f"  {row:<22} {np.median(v):>10.1f} {v.min():>10.1f} {v.max():>10.1f}   {v.size}")
    for k, v in enumerate(base):
        v = np.array(v)
        say(f"  {'host_baseline ' + ('before', 'after')[k]:<22} {np.median(v):>10.1f} {v.min():>10.1f} {v.max():>10.1f}   {v.size}")
    best_base = min(float(np.median(v)) for v in base)
    ok = float(np.median(times["prepare_wait"])) < best_base
    say(f"  prepare(PATH | GOAL) + wait costs {'less' if ok else 'NOT less'} than the read plus the host queue run twice "
        f"({np.median(times['prepare_wait']):.1f} us against {best_base:.1f} us, the lower of the two baseline medians)")
    cm.close()
    m.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
