"""Timing of gem_costmap_frontiers against what a caller of the library without it must do: gem_costmap_read of the whole grid plus
gem_costmap_navplan_read of the potential, then a CPU search -- the host twin gem_frontiers_host (a flood fill in C++ inside
libgem_hip.so, called through ctypes) stands for that search.  Needs a GPU; prints a table and, with --out, writes it to a file as well.

Workloads, all at 0.2 m, planned from the robot's cell with allow_unknown = 0 and the outline on; min_frontier_size 1 m,
potential_scale 0.001, gain_scale 1:
  1000x1000 ragged   the reference's global costmap: a known region with a ragged rim, 20 % of its cells a random byte, unknown outside
  1000x1000 thin     the same size with ONE long thin frontier: known below a gently waving line, unknown above it
  200x200 ragged     a small map of the first kind
Rows, host clock (time.perf_counter) around calls that end in a wait, alternated round by round (--rounds) after --warmup rounds; each
reports its median and the min .. max of its rounds:
  frontiers          gem_costmap_frontiers: classification, the label rounds in chunks, the reduction, the pick; the winner is in the status
  reads_only         gem_costmap_read + gem_costmap_navplan_read of the potential: code of the library without frontier search, and a
                     lower bound of the baseline whatever the host search costs
  host_baseline      the two reads + gem_frontiers_host (status only: the winner)
  navplan_goal       Costmap.nav_plan_to(the winner's access cell): one walk on the potential that is there
  navplan_full       Costmap.nav_plan(robot, the same goal): the whole potential again, then the same walk
rounds and chunks are the status words of the frontiers row's last call.  Before timing, the device's labels, kept list and status are
compared with the host twin's byte for byte, and nav_plan_to's path with nav_plan's."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import gem_amd  # noqa: E402
from gem_amd import ElevationMap, _lib  # noqa: E402

RES = 0.2
PARAMS = (1.0, 0.001, 1.0)


def ragged(n, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n, 0:n]
    dx, dy = xx - n / 2, yy - n / 2
    ang = np.arctan2(dy, dx)
    rim = n * (0.33 + 0.07 * np.sin(5 * ang) + 0.03 * np.sin(17 * ang))
    g = np.full((n, n), 255, np.uint8)
    inside = dx * dx + dy * dy < rim * rim
    g[inside] = 0
    hit = inside & (rng.random((n, n)) < 0.2)
    g[hit] = rng.integers(0, 256, int(hit.sum()), dtype=np.uint8)
    g[n // 2, n // 2] = 0
    return g, (n // 2, n // 2)


def thin(n):
    yy, xx = np.mgrid[0:n, 0:n]
    return np.where(yy > n / 2 + 40 * np.sin(xx / 37.0), 255, 0).astype(np.uint8), (n // 2, n // 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_frontier.py needs a GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    cases = [("1000x1000 ragged", *ragged(1000, 1000)), ("1000x1000 thin", *thin(1000)), ("200x200 ragged", *ragged(200, 200))]
    m = ElevationMap(32, 0.1)
    lib, h = m._lib, m._h
    w = gem_amd.nav_weights(allow_unknown=False)
    prm = _lib.FrontierParams(*PARAMS)
    say(f"bench_frontier: resolution {RES} m, allow_unknown 0, outline on, params {PARAMS}; rounds {args.rounds} (alternated), warmup {args.warmup}")
    for name, g, robot in cases:
        n = g.shape[0]
        cm = m.costmap(n, n, RES, 0.0, 0.0, 0)
        cm.write(g)
        wr = ((robot[0] + 0.5) * RES, (robot[1] + 0.5) * RES)
        cm.nav_plan(wr, wr, w)
        pot_d = cm.read_potential()[0]
        kept_h, labels_h, st_h = gem_amd.frontiers_host(g, pot_d, RES, *PARAMS)
        st_d = cm.frontiers(*PARAMS)
        kept_d, labels_d = cm.read_frontiers()
        same = ("n_cells", "n_frontiers", "n_kept", "best", "best_frontier")
        assert labels_d.tobytes() == labels_h.tobytes() and kept_d == kept_h and all(st_d[k] == st_h[k] for k in same), name
        assert st_d["best"] >= 0, name
        ac = st_d["best_frontier"]["access_cell"]
        wg = ((ac % n + 0.5) * RES, (ac // n + 0.5) * RES)
        path_to, st_to = cm.nav_plan_to(wg)
        path_full, st_full = cm.nav_plan(wr, wg, w)
        assert path_to.tobytes() == path_full.tobytes() and st_to["n_path"] == st_full["n_path"] > 0, name
        rows = ("frontiers", "reads_only", "host_baseline", "navplan_goal", "navplan_full")
        times = {r: [] for r in rows}
        st = _lib.FrontierStatus()
        hst = _lib.FrontierStatus()
        pot = np.zeros((n, n), np.int32)

        def reads():
            grid = cm.read()
            cm._call("gem_costmap_navplan_read", pot.ctypes.data_as(C.c_void_p), None, 0)
            return grid

        def run(row):
            m.synchronize()
            t = time.perf_counter()
            if row == "frontiers":
                assert lib.gem_costmap_frontiers(h, cm.id, C.byref(prm), C.byref(st)) == 0
            elif row == "reads_only":
                reads()
            elif row == "host_baseline":
                grid = reads()
                assert lib.gem_frontiers_host(grid.ctypes.data_as(C.c_void_p), pot.ctypes.data_as(C.c_void_p), n, n, RES, C.byref(prm), None, None, 0,
                                              C.byref(hst)) == 0
            elif row == "navplan_goal":
                cm.nav_plan_to(wg)
            else:
                cm.nav_plan(wr, wg, w)
            return time.perf_counter() - t

        for r in range(args.warmup + args.rounds):
            for row in rows:
                dt = run(row)
                if r >= args.warmup:
                    times[row].append(dt * 1e6)
        assert (st.best_frontier.root, st.n_kept) == (hst.best_frontier.root, hst.n_kept) == (st_h["best_frontier"]["root"], st_h["n_kept"]), name
        say(f"{name}: {st.n_cells} frontier cells in {st.n_frontiers} frontiers, {st.n_kept} kept, the winner has {st.best_frontier.size} cells; "
            f"rounds {st.rounds}, chunks {st.chunks}; labels, kept list and status equal to the host twin byte for byte; "
            f"the path to the access cell has {st_to['n_path']} cells")
        say(f"  {'row':<22} {'median us':>11} {'min us':>11} {'max us':>11}   rounds")
        med = {}
        for row, v in times.items():
            v = np.array(v)
            med[row] = float(np.median(v))
            say(f"  {row:<22} {np.median(v):>11.1f} {v.min():>11.1f} {v.max():>11.1f}   {v.size}")
        say(f"  the device search costs {'less' if med['frontiers'] < med['host_baseline'] else 'NOT less'} than the reads plus the host twin "
            f"({med['frontiers']:.1f} us against {med['host_baseline']:.1f} us) and {'less' if med['frontiers'] < med['reads_only'] else 'NOT less'} "
            f"than the two reads alone ({med['reads_only']:.1f} us); nav_plan_to costs {'less' if med['navplan_goal'] < med['navplan_full'] else 'NOT less'} "
            f"than a full plan to the same goal ({med['navplan_goal']:.1f} us against {med['navplan_full']:.1f} us)")
        cm.close()
    m.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
