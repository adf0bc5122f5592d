"""Timing of gem_costmap_navplan_quadratic against (a) gem_costmap_navplan, the linear plan on the same map in the same process, and
(b) what a user does without the call: gem_costmap_read of the whole grid plus the host twin gem_navquad_host (a heap relaxation and the
same getPath, C++ inside libgem_hip.so, called through ctypes).  Needs a GPU; prints a table and, with --out, writes it to a file.

Workloads: those of tools/bench_navpath.py, drawn from the same generator in the same order -- 1000x1000 with 20 % noise, the 1000x1000
maze, 200x200 noise and the 75x75 local costmap -- at 0.2 m with the default weight table and the outline on, start and goal near
opposite corners.
Rows, host clock (time.perf_counter) around calls that end in a wait, alternated round by round (--rounds) after --warmup rounds; each
reports its median and the min .. max of its rounds:
  quadratic         Costmap.nav_plan_quadratic(start, goal): init, the rounds of the tiled potential in chunks, the walk, the download
  linear            Costmap.nav_plan(start, goal), the same with k_nav_round
  host_baseline     read of the grid + gem_navquad_host
rounds and chunks are the status words of each row's last call.  Before timing, the device's quadratic potential and path are compared
with the host twin's byte for byte.
The pass bound: the kernel counts nothing (its one atomic is the protocol's round counter), so the in-tile work is measured from
outside -- the call's median time and its rounds with "navquad_passes" set to 1, 2, 3, 4, 6, 8, 16 and 64 passes a round.  With 64 a
tile practically always ends at its local fixed point, as the linear plan's tiles do; the smallest bound whose round count equals
that one's is the number of passes the hardest tile needs.
The gradient walk: 1024 goals drawn as tools/bench_navpath.py draws them (from the cells the LINEAR plan reaches from the start, which
are the quadratic plan's too), max_points 16384, on each potential; the count of walks that end in CAP."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import gem_amd  # noqa: E402
from gem_amd import ElevationMap, _lib  # noqa: E402

RES = 0.2
PASSES = (1, 2, 3, 4, 6, 8, 16, 64)


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
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sweep-rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_navquad.py needs a GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(1000)
    cases = [("1000x1000 noise", noise(rng, 1000)), ("1000x1000 maze", maze(1000)), ("200x200 noise", noise(rng, 200)),
             ("75x75 local", noise(rng, 75))]
    m = ElevationMap(32, 0.1)
    say(f"bench_navquad: resolution {RES} m, default weights, outline on; rounds {args.rounds} (alternated), warmup {args.warmup}; "
        f"default pass bound {m.debug_get('navquad_passes') or 3}")
    for name, g in cases:
        n = g.shape[0]
        start, goal = (3, 4), (n - 5, n - 10)
        g[start[1], start[0]] = 0
        g[goal[1], goal[0]] = 0
        cm = m.costmap(n, n, RES, 0.0, 0.0, 0)
        cm.write(g)
        ws, wg = ((start[0] + 0.5) * RES, (start[1] + 0.5) * RES), ((goal[0] + 0.5) * RES, (goal[1] + 0.5) * RES)
        pot_h, cells_h, st_h = gem_amd.nav_quad_host(g, start, goal)
        path, st = cm.nav_plan_quadratic(ws, wg)
        pot_d, cells_d = cm.read_potential()
        assert pot_d.tobytes() == pot_h.tobytes() and cells_d.tolist() == cells_h.tolist() and st["found"] == st_h["found"] == 1, name
        rows = ("quadratic", "linear", "host_baseline")
        times = {r: [] for r in rows}
        last = {"quadratic": st, "linear": None}

        def run(row):
            m.synchronize()
            t = time.perf_counter()
            if row == "quadratic":
                _, last[row] = cm.nav_plan_quadratic(ws, wg)
            elif row == "linear":
                _, last[row] = cm.nav_plan(ws, wg)
            else:
                gem_amd.nav_quad_host(cm.read(), start, goal)
            return time.perf_counter() - t

        for r in range(args.warmup + args.rounds):
            for row in rows:
                dt = run(row)
                if r >= args.warmup:
                    times[row].append(dt * 1e6)
        say(f"{name}: {int((pot_h != _lib.NAV_UNREACHED).sum())} cells reached, a quadratic plan of {st['n_path']} cells, goal potential "
            f"{st['goal_potential']} (linear: {last['linear']['n_path']} cells, {last['linear']['goal_potential']}); equal to the host twin byte for byte")
        say(f"  {'row':<22} {'median us':>11} {'min us':>11} {'max us':>11}   n   rounds chunks")
        med = {}
        for row, v in times.items():
            v = np.array(v)
            med[row] = float(np.median(v))
            rc = f"{last[row]['rounds']:>6} {last[row]['chunks']:>6}" if row in last else ""
            say(f"  {row:<22} {np.median(v):>11.1f} {v.min():>11.1f} {v.max():>11.1f}   {v.size:<3} {rc}")
        say(f"  quadratic / linear = {med['quadratic'] / med['linear']:.2f}; the device call costs "
            f"{'less' if med['quadratic'] < med['host_baseline'] else 'NOT less'} than the read plus the host twin "
            f"({med['quadratic']:.1f} us against {med['host_baseline']:.1f} us, {med['host_baseline'] / med['quadratic']:.1f} x)")

        # the pass bound
        say(f"  {'navquad_passes':<22} {'median us':>11} {'rounds':>8} {'chunks':>7}")
        for p in PASSES:
            m.debug_set("navquad_passes", p)
            v = []
            for r in range(1 + args.sweep_rounds):
                m.synchronize()
                t = time.perf_counter()
                _, s = cm.nav_plan_quadratic(ws, wg)
                if r:
                    v.append((time.perf_counter() - t) * 1e6)
            say(f"  {p:<22} {np.median(v):>11.1f} {s['rounds']:>8} {s['chunks']:>7}")
        m.debug_set("navquad_passes", 0)

        # the gradient walk on each potential
        cm.nav_plan(ws, ws)
        pot_l, _ = cm.read_potential()
        ys, xs = np.nonzero(pot_l != _lib.NAV_UNREACHED)
        pick = rng.permutation(xs.size)[:1024]
        world = (np.stack([xs[pick], ys[pick]], axis=1).astype(np.float64) + 0.5) * RES
        counts = {}
        for which in ("linear", "quadratic"):
            (cm.nav_plan if which == "linear" else cm.nav_plan_quadratic)(ws, ws)
            _, res = cm.nav_paths(world, _lib.NAVPATH_GRADIENT, 16384, points=False, raw=True)
            counts[which] = (int((res[:, 0] == _lib.NAVPATH_CAP).sum()), int((res[:, 0] == _lib.NAVPATH_FOUND).sum()))
        say(f"  gradient walks of {len(pick)} goals, max_points 16384: on the linear potential {counts['linear'][0]} end in CAP and "
            f"{counts['linear'][1]} arrive; on the quadratic potential {counts['quadratic'][0]} end in CAP and {counts['quadratic'][1]} arrive")
        cm.close()
    m.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
