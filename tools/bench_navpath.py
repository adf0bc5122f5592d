"""Timing of gem_costmap_navplan_paths against the route that exists without it: gem_costmap_navplan_read of the potential followed by
the host twin gem_navpath_host for the same goals, goal by goal on one thread (C++ inside libgem_hip.so, called through ctypes).  Needs a
GPU; prints a table and, with --out, writes it to a file as well.

Workloads, all at 0.2 m with the default weight table and the outline on, planned once from a start near a corner:
  1000x1000 noise, 1000x1000 maze, 200x200 noise   the three cases of tools/bench_navplan.py
  75x75 local                                     the size of the reference's local costmap, 20 % noise
Goals: reached cells drawn at random (the same ones for every row), 1, 16, 256 and 1024 of them; the single goal is the far corner's.
max_points is the longest walk's length plus one, or 2^24 / n_goals where that is smaller (the maze: the longest walks then end in CAP on
both sides alike).  Both forms.  Rows, host clock (time.perf_counter) around calls that end in a wait, alternated round by round
(--rounds) after --warmup rounds, the caller's buffers allocated once outside the clock; each reports its median and min .. max:
  paths            gem_costmap_navplan_paths: goal cells up, one launch, results and points down
  paths_device     gem_costmap_navplan_paths_device into device buffers, then gem_synchronize: the walk without the download
  read+host        gem_costmap_navplan_read of the potential, then gem_navpath_host per goal
Before timing, results and points of the device are compared with the host twin's, bit for bit.  The per-step time of a single wave is
(paths_device with one goal - paths_device with max_points = 2) / the walk's points."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import gem_amd  # noqa: E402
from gem_amd import ElevationMap, _lib  # noqa: E402
from bench_navplan import maze, noise  # noqa: E402

RES = 0.2
COUNTS = (1, 16, 256, 1024)
FORMS = ((_lib.NAVPATH_GRADIENT, "gradient"), (_lib.NAVPATH_GRID, "grid"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_navpath.py needs a GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(1000)
    cases = [("1000x1000 noise", noise(rng, 1000)), ("1000x1000 maze", maze(1000)), ("200x200 noise", noise(rng, 200)),
             ("75x75 local", noise(rng, 75))]
    m = ElevationMap(32, 0.1)
    lib, h = m._lib, m._h
    host = _lib.load().gem_navpath_host
    say(f"bench_navpath: resolution {RES} m, default weights, outline on; rounds {args.rounds} (alternated), warmup {args.warmup}")
    for name, g in cases:
        n = g.shape[0]
        start, far = (3, 4), (n - 5, n - 10)
        g[start[1], start[0]] = 0
        g[far[1], far[0]] = 0
        cm = m.costmap(n, n, RES, 0.0, 0.0, 0)
        cm.write(g)
        ws = ((start[0] + 0.5) * RES, (start[1] + 0.5) * RES)
        _path, st = cm.nav_plan(ws, ws)
        pot = np.zeros((n, n), np.int32)
        assert lib.gem_costmap_navplan_read(h, cm.id, pot.ctypes.data_as(C.c_void_p), None, 0) == 0
        ys, xs = np.nonzero(pot != _lib.NAV_UNREACHED)
        pick = rng.permutation(xs.size)[:1024]
        cells_all = np.stack([xs[pick], ys[pick]], axis=1).astype(np.int32)
        say(f"{name}: {xs.size} cells reached from {start}")
        s_cell = (C.c_int * 2)(*start)
        per_step = {}
        wins = {}
        for form, fname in FORMS:
            for count in COUNTS:
                cells = np.ascontiguousarray(cells_all[:count]) if count > 1 else np.array([far], np.int32)
                world = np.ascontiguousarray((cells.astype(np.float64) + 0.5) * RES)
                # the longest walk, by the twin without points, sizes max_points
                res_h = np.zeros((count, 8), np.int32)

                def twin(cap, pts):
                    for i in range(count):
                        e = (C.c_int * 2)(int(cells[i, 0]), int(cells[i, 1]))
                        rc = host(pot.ctypes.data_as(C.c_void_p), n, n, s_cell, e, form, cap, pts[i].ctypes.data_as(C.c_void_p) if pts is not None else None,
                                  C.cast(res_h[i].ctypes.data_as(C.c_void_p), C.POINTER(_lib.NavpathResult)))
                        assert rc == 0

                limit = min(1 << 20, (1 << 24) // count)
                twin(limit, None)
                cap = min(limit, int(res_h[:, 1].max()) + 1)
                capped = int((res_h[:, 0] == _lib.NAVPATH_CAP).sum())
                pts_h = np.zeros((count, cap, 2), np.float32)
                pts_d = np.zeros((count, cap, 2), np.float32)
                res_d = np.zeros((count, 8), np.int32)
                t_pts = torch.empty((count, cap, 2), dtype=torch.float32, device="cuda")
                t_res = torch.empty((count, 8), dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()

                def paths():
                    assert lib.gem_costmap_navplan_paths(h, cm.id, world.ctypes.data_as(C.c_void_p), count, form, cap, pts_d.ctypes.data_as(C.c_void_p),
                                                         res_d.ctypes.data_as(C.c_void_p)) == 0

                def paths_device(c=None):
                    assert lib.gem_costmap_navplan_paths_device(h, cm.id, world.ctypes.data_as(C.c_void_p), count, form, cap if c is None else c,
                                                                C.c_void_p(t_pts.data_ptr()), C.c_void_p(t_res.data_ptr())) == 0
                    m.synchronize()

                def read_host():
                    assert lib.gem_costmap_navplan_read(h, cm.id, pot.ctypes.data_as(C.c_void_p), None, 0) == 0
                    twin(cap, pts_h)

                read_host(); paths(); paths_device()
                assert res_d.tobytes() == res_h.tobytes() == t_res.cpu().numpy().tobytes(), (name, fname, count)
                dev_pts = t_pts.cpu().numpy()
                for i in range(count):
                    k = int(res_h[i, 1])
                    assert pts_d[i, :k].tobytes() == pts_h[i, :k].tobytes() == dev_pts[i, :k].tobytes(), (name, fname, count, i)
                rows = {"paths": paths, "paths_device": paths_device, "read+host": read_host}
                if count == 1:
                    rows["paths_device cap 2"] = lambda: paths_device(2)
                times = {r: [] for r in rows}
                for r in range(args.warmup + args.rounds):
                    for row, fn in rows.items():
                        m.synchronize()
                        t = time.perf_counter()
                        fn()
                        dt = time.perf_counter() - t
                        if r >= args.warmup:
                            times[row].append(dt * 1e6)
                total = int(res_h[:, 1].sum())
                say(f"  {fname}, {count} goal(s): max_points {cap}, {total} points in all, longest {int(res_h[:, 1].max())}"
                    + (f", {capped} walk(s) end in CAP" if capped else "") + "; equal to the host twin bit for bit")
                say(f"    {'row':<22} {'median us':>11} {'min us':>11} {'max us':>11}   rounds")
                med = {}
                for row, v in times.items():
                    v = np.array(v)
                    med[row] = float(np.median(v))
                    say(f"    {row:<22} {np.median(v):>11.1f} {v.min():>11.1f} {v.max():>11.1f}   {v.size}")
                if count == 1:
                    per_step[fname] = (med["paths_device"] - med["paths_device cap 2"]) / max(int(res_h[0, 1]) - 2, 1)
                    say(f"    one wave: {per_step[fname] * 1000:.0f} ns per point of the walk")
                ok = med["paths"] < med["read+host"]
                say(f"    the device call costs {'less' if ok else 'NOT less'} than the read plus the host walk ({med['paths']:.1f} us against "
                    f"{med['read+host']:.1f} us, x{med['read+host'] / med['paths']:.1f})")
                if ok and fname not in wins:
                    wins[fname] = count
        say("  the device wins from " + ", ".join(f"{wins.get(f, 'more than 1024')} goal(s) ({f})" for _c, f in FORMS)
            + "; one wave takes " + ", ".join(f"{per_step[f] * 1000:.0f} ns per point ({f})" for _c, f in FORMS))
        cm.close()
    m.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
