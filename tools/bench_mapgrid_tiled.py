"""Timing of gem_costmap_mapgrid_prepare_tiled (the distance grids on a costmap of any size, gem_mapgrid_tiled.hip) in tools/bench_mapgrid.py's
manner.  Needs a GPU; prints a table per workload and, with --out, writes them to a file as well.

Workloads, each a costmap with default value FREE_SPACE, marked by gem_costmap_mark_points from bench_mapgrid.py's seeded noise cloud
(--density points per cell, about half of them lethal) and inflated (inflation radius 0.55 m, inscribed radius 0.3 m), or left empty;
the plan is 60 points across the map's diagonal:
  400 x 400 at 0.05      the workload of profiles/mapgrid_c2.txt: the one place where the LDS form, the tiled form and the host baseline
                         exist side by side
  600 x 600 at 0.05      the elevation map's geometry, above the LDS form's cap: noise, and empty
  1000 x 1000 at 0.2     the reference's global costmap, above the cap: noise, and empty
Rows, host clock (time.perf_counter) between two gem_synchronize, alternated round by round (--rounds) after --warmup rounds; each
reports its median and the min .. max of its rounds:
  lds_prepare_wait       gem_costmap_mapgrid_prepare(PATH | GOAL) and the wait for it (400 x 400 only: above the cap it is refused)
  tiled_prepare          gem_costmap_mapgrid_prepare_tiled(PATH | GOAL): the call waits itself; its rounds and chunks are reported
  upload_2_grids         two int32 grids of the map's size from host memory to the device and the wait: what a user above the cap adds
                         to the host baseline today (torch's copy from pageable memory; the library has no call that takes a grid)
  host_baseline          the child process (the `bench` mode of tests/cpp/mapgrid_check.cpp): gem_costmap_read of the whole map +
                         adjustPlanResolution + the literal queue twice, its own clock, the same number of rounds after two of warm-up;
                         a process of its own, so it runs once before and once after the alternated rows and both runs are reported.
Before timing, both grids of the tiled call are compared with tests/mapgrid_ref.py's set form byte for byte (and with the LDS form's
where that runs)."""
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
sys.path.insert(0, str(ROOT / "tools"))

from gem_amd import ElevationMap, _lib  # noqa: E402
import costmap_ref as cref  # noqa: E402
import mapgrid_ref as ref  # noqa: E402
from bench_mapgrid import FACTOR, INSCRIBED, RADIUS, THRESH, build_baseline  # noqa: E402
from gem_amd import POINT_DTYPE  # noqa: E402

WORKLOADS = [("400 x 400 at 0.05, noise", 400, 0.05, True), ("600 x 600 at 0.05, noise", 600, 0.05, True), ("600 x 600 at 0.05, empty", 600, 0.05, False),
             ("1000 x 1000 at 0.2, noise", 1000, 0.2, True), ("1000 x 1000 at 0.2, empty", 1000, 0.2, False)]
BOTH = _lib.MAPGRID_PATH | _lib.MAPGRID_GOAL


def noise_cloud(rng, size, res, density):
    n = int(size * size * density)
    pts = np.zeros(n, POINT_DTYPE)
    pts["x"] = rng.uniform(0.0, size * res, n).astype(np.float32)
    pts["y"] = rng.uniform(0.0, size * res, n).astype(np.float32)
    pts["travers"] = rng.uniform(THRESH - 0.3, THRESH + 0.3, n).astype(np.float32)
    return pts


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
        raise SystemExit("bench_mapgrid_tiled.py needs a GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    m = ElevationMap(32, 0.1)
    say(f"bench_mapgrid_tiled: {args.density} points per cell where a map is marked, inflation radius {RADIUS} m; rounds {args.rounds} (alternated), warmup {args.warmup}")
    with tempfile.TemporaryDirectory() as td:
        exe = Path(args.baseline_exe) if args.baseline_exe else build_baseline(Path(td) / "mapgrid_check")
        for name, size, res, marked in WORKLOADS:
            rng = np.random.default_rng(size)
            cm = m.costmap(size, size, res, 0.0, 0.0, _lib.COST_FREE_SPACE)
            if marked:
                cm.mark_points(noise_cloud(rng, size, res, args.density), THRESH, None)
                cm.inflate(RADIUS, INSCRIBED, FACTOR, False, None)
            grid = cm.read()
            plan = np.stack([np.linspace(0.5 * res, (size - 0.5) * res, 60)] * 2, axis=1)
            host = cref.Costmap(size, size, res, 0.0, 0.0, cref.FREE_SPACE)
            host.grid[:] = grid
            want = ref.grids(host, plan)
            capped = -(-size // 64) * size <= _lib.MAPGRID_MAX_WORDS
            st = cm.prepare_map_grid_tiled(plan)
            tiled = {}
            for bit, key in ((_lib.MAPGRID_PATH, "path"), (_lib.MAPGRID_GOAL, "goal")):
                got, started, goal = cm.read_map_grid(bit)
                assert got.tobytes() == want[key].tobytes() and started == want["started"] and goal == want["goal_cell"], f"{name}: the {key} grid differs from the set form"
                tiled[bit] = got
            if capped:
                cm.prepare_map_grid(plan)
                for bit in tiled:
                    assert cm.read_map_grid(bit)[0].tobytes() == tiled[bit].tobytes(), f"{name}: the LDS form and the tiled form differ"
            OB, _ = ref.constants(grid)
            say()
            say(f"{name}: {int((grid >= 253).sum())} blocked cells ({100.0 * (grid >= 253).mean():.1f} %); plan {ref.adjust_plan(plan, res).shape[0]} points after "
                f"adjustPlanResolution; path grid {int((want['path'] < OB).sum())} cells reached in {int(want['path'][want['path'] < OB].max())} levels, goal grid "
                f"{int((want['goal'] < OB).sum())} cells in {int(want['goal'][want['goal'] < OB].max())} levels; tiles {-(-size // 64)} x {-(-size // 64)}; "
                f"the tiled grids equal the set form of tests/mapgrid_ref.py byte for byte" + (" and the LDS form's" if capped else ""))
            gpath, ppath = Path(td) / "grid.bin", Path(td) / "plan.bin"
            gpath.write_bytes(grid.tobytes())
            ppath.write_bytes(np.ascontiguousarray(plan, np.float64).tobytes())

            def baseline():
                out = subprocess.run([str(exe), "bench", str(gpath), str(size), str(size), repr(res), str(ppath), str(args.rounds)],
                                     capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    raise SystemExit("the baseline child failed:\n" + out.stdout + out.stderr)
                return [float(v) for v in out.stdout.split("\n") if v and not v.startswith("check")]

            base = [baseline()]
            rows = (("lds_prepare_wait",) if capped else ()) + ("tiled_prepare", "upload_2_grids")
            times = {r: [] for r in rows}
            status = []
            h_grids = [np.ascontiguousarray(want["path"]), np.ascontiguousarray(want["goal"])]

            def run(row):
                m.synchronize()
                t = time.perf_counter()
                if row == "lds_prepare_wait":
                    cm.prepare_map_grid(plan)
                elif row == "tiled_prepare":
                    status.append(cm.prepare_map_grid_tiled(plan))
                else:
                    keep = [torch.from_numpy(a).to("cuda:0") for a in h_grids]
                    torch.cuda.synchronize()
                    del keep
                m.synchronize()
                return time.perf_counter() - t

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
            rounds = sorted({s["rounds"] for s in status})
            say(f"  tiled_prepare: protocol rounds {rounds[0]} .. {rounds[-1]} (first call {st['rounds']}), chunks {sorted({s['chunks'] for s in status})}")
            best_base, tiled_med = min(float(np.median(v)) for v in base), float(np.median(times["tiled_prepare"]))
            if capped:
                lds = float(np.median(times["lds_prepare_wait"]))
                say(f"  the tiled form is {'FASTER' if tiled_med < lds else 'SLOWER'} than the LDS form ({tiled_med:.1f} us against {lds:.1f} us) and "
                    f"{'FASTER' if tiled_med < best_base else 'SLOWER'} than the read plus the host queue run twice ({best_base:.1f} us, the lower of the two baseline medians)")
            else:
                today = best_base + float(np.median(times["upload_2_grids"]))
                say(f"  the tiled prepare is {'FASTER' if tiled_med < today else 'SLOWER'} than what a user does above the cap today: read + host queue twice + upload of both grids "
                    f"({tiled_med:.1f} us against {best_base:.1f} + {np.median(times['upload_2_grids']):.1f} = {today:.1f} us)")
            cm.close()
    m.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
