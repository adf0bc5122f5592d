"""The quadratic plan on the device costmap (gem_costmap_navplan_quadratic) against tests/navquad_ref.py.  Every comparison is exact:
potentials by tobytes(), paths and status as integers, world points as doubles.  Nothing here is above 200 x 130 cells.

  1. 64 x 64, 65 x 65 (four tiles, three of them slivers) and 130 x 90 with noise, walls and blocked noise: the plans test_navquad_cpu.py
     pins four ways on the CPU;
  2. 1 x 1, the special starts and goals (a start off the map, an unreached goal), an all-blocked map, the corridor across a seam,
     custom weights with w = 1 and w = 462;
  3. 200 x 70 noise; a serpentine that crosses the tile edges in both directions; a start at cell 63 and at cell 64 of a row;
  4. one in-tile pass a round ("navquad_passes" 1: every unfinished tile marks itself) and chunks of two rounds give the same plan;
  5. no allocation in a second identical call;
  6. nav_paths in gradient and grid form, nav_plan_to and frontiers run on the quadratic potential and equal their references fed it;
  7. a linear plan replaces a quadratic one and the other way round;
  8. stale after a roll or an observe, fresh after the next plan; the error list, nothing enqueued, the last plan unchanged;
  9. the C++ facade (tests/cpp/navquad_facade.cpp) as a child process."""
import ctypes as C
import functools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gem_amd import ElevationMap, _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import frontier_ref as fref  # noqa: E402
import navpath_ref as pref  # noqa: E402
import navplan_ref as lin  # noqa: E402
import navquad_ref as ref  # noqa: E402
from test_navplan_cpu import default_weights, scenario  # noqa: E402
from test_navquad_cpu import GEOMS, KINDS, build_navquad_facade, expected, odd_cases  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
RES, ORIGIN = 0.2, (-3.1, 2.7)
INV = _lib.GEM_OK - 1


@pytest.fixture(scope="module")
def emap():
    m = ElevationMap(32, 0.05)
    yield m
    m.close()


def device_copy(m, grid, res=RES, origin=ORIGIN):
    dev = m.costmap(grid.shape[1], grid.shape[0], res, origin[0], origin[1], 0)
    dev.write(grid)
    return dev


def centre(cell, res=RES, origin=ORIGIN):
    """a world point well inside cell (x, y); off the map for a cell that is"""
    return (origin[0] + (cell[0] + 0.5) * res, origin[1] + (cell[1] + 0.5) * res)


def same_plan(dev, want, start, goal, flags, what, weights=None):
    """one nav_plan_quadratic on the device against a reference plan; returns the status"""
    sx = dev.size_x
    path, st = dev.nav_plan_quadratic(centre(start), centre(goal), weights, outline=bool(flags & ref.OUTLINE))
    pot, cells = dev.read_potential()
    assert pot.dtype == np.int32 and pot.tobytes() == want["pot"].tobytes(), f"{what}: {int((pot != want['pot']).sum())} potentials differ"
    assert (st["found"], st["n_path"], st["goal_potential"]) == (want["found"], want["n_path"], want["goal_potential"]), (what, st)
    assert (st["start_cell"], st["goal_cell"]) == (want["start_cell"], want["goal_cell"]), (what, st)
    assert cells.tolist() == np.asarray(want["cells"]).tolist(), what
    assert path.tobytes() == lin.centres(want["cells"], sx, RES, *ORIGIN).tobytes(), what
    assert st["chunks"] >= 1 and st["rounds"] >= (1 if want["start_cell"] != (-1, -1) else 0), (what, st)
    assert dev.nav_status() == st, what
    return st


@functools.lru_cache(maxsize=None)
def wide_noise():
    """200 x 70: four tiles in a row, the last a sliver, two tile rows"""
    rng = np.random.default_rng(20070)
    g = np.zeros((70, 200), np.uint8)
    hit = rng.random(g.shape) < 0.3
    g[hit] = rng.integers(0, 256, int(hit.sum()), dtype=np.uint8)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def both_ways_serpentine():
    """130 x 130: a one-cell corridor that runs along every fourth row of the upper part (each run crosses the seams at x = 64 and
    x = 128), comes down column 129 and then runs along every fourth column of the lower part, rows 62 .. 129 (each run crosses the seams
    at y = 64 and y = 128).  From (0, 0) to (1, 129)."""
    g = np.full((130, 130), 254, np.uint8)
    for k, y in enumerate(range(0, 60, 4)):                              # rows 0, 4, .. 56, joined at alternating ends; row 56 ends at x = 129
        g[y, :] = 0
        g[y:y + 4, 129 if k % 2 == 0 else 0] = 0
    g[60:62, 129] = 0
    for k, x in enumerate(range(129, 0, -4)):                            # columns 129, 125, .. 1, joined at the bottom, then at the top, ...
        g[62:, x] = 0
        if x - 4 > 0:
            g[129 if k % 2 == 0 else 62, x - 4:x] = 0
    g.setflags(write=False)
    return g


# ---- 1. the geometries the CPU tests pin -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_geometries(emap, geom, kind):
    g = scenario(geom, kind)
    dev = device_copy(emap, g)
    try:
        for start, goal, flags, want in expected(geom, kind):
            same_plan(dev, want, start, goal, flags, f"{geom} {kind} {start} -> {goal} flags {flags}")
        assert dev.read().tobytes() == g.tobytes()                        # the outline is not written into the costmap
    finally:
        dev.close()


# ---- 2. the odd cases ------------------------------------------------------------------------------------------------------------------
def test_odd_cases(emap):
    devs = {}
    try:
        for name, g, start, goal, flags, w in odd_cases():
            if g.shape not in devs:
                devs[g.shape] = emap.costmap(g.shape[1], g.shape[0], RES, ORIGIN[0], ORIGIN[1], 0)
            devs[g.shape].write(g)
            want = ref.plan(g, w, flags, start, goal)
            same_plan(devs[g.shape], want, start, goal, flags, name, np.asarray(w))
    finally:
        for dev in devs.values():
            dev.close()


# ---- 3. more tiles, both directions, the tile edge ---------------------------------------------------------------------------------------
def test_200_x_70_noise(emap):
    g = wide_noise()
    dev = device_copy(emap, g)
    try:
        for start, goal, flags in (((2, 3), (197, 66), ref.OUTLINE), ((198, 1), (1, 68), 0)):
            want = ref.plan(g, default_weights(), flags, start, goal)
            assert want["found"] == 1
            st = same_plan(dev, want, start, goal, flags, f"200 x 70 {start}")
            assert st["rounds"] >= 4                                      # four tiles from the start's to the goal's
    finally:
        dev.close()


def test_serpentine_across_the_seams_in_both_directions(emap):
    g = both_ways_serpentine()
    start, goal = (0, 0), (1, 129)
    want = ref.plan(g, default_weights(), 0, start, goal)
    assert want["found"] == 1 and want["n_path"] > 4000
    xs, ys = want["cells"] % 130, want["cells"] // 130
    across_x = int(((xs[:-1] == 63) & (xs[1:] == 64) | (xs[:-1] == 64) & (xs[1:] == 63)).sum())
    across_y = int(((ys[:-1] == 63) & (ys[1:] == 64) | (ys[:-1] == 127) & (ys[1:] == 128) | (ys[:-1] == 128) & (ys[1:] == 127)).sum())
    assert across_x >= 10 and across_y >= 10, (across_x, across_y)
    dev = device_copy(emap, g)
    try:
        st = same_plan(dev, want, start, goal, 0, "serpentine, both directions")
        assert st["rounds"] > 20, st
    finally:
        dev.close()


@pytest.mark.parametrize("x", [63, 64])
def test_start_on_the_tile_edge(emap, x):
    g = scenario("130x90", "noise")
    dev = device_copy(emap, g)
    try:
        for start in ((x, 30), (30, x)):                                  # the edge column, then the edge row: the init marks the neighbour tile
            want = ref.plan(g, default_weights(), 0, start, (120, 80))
            assert want["found"] == 1
            same_plan(dev, want, start, (120, 80), 0, f"start {start}")
    finally:
        dev.close()


# ---- 4. the pass bound and the chunk length do not change the plan -------------------------------------------------------------------------
def test_one_pass_a_round_and_short_chunks_give_the_same_plan(emap):
    g = scenario("130x90", "noise")
    start, goal, flags, want = expected("130x90", "noise")[0]
    dev = device_copy(emap, g)
    try:
        base = same_plan(dev, want, start, goal, flags, "the default pass bound")
        emap.debug_set("navquad_passes", 1)
        emap.debug_set("nav_chunk", 2)
        one = same_plan(dev, want, start, goal, flags, "one pass a round, chunks of two")
        assert one["rounds"] > base["rounds"] and one["chunks"] > 1, (base, one)      # unfinished tiles marked themselves and went on
        emap.debug_set("navquad_passes", 64)
        same_plan(dev, want, start, goal, flags, "64 passes a round")
        assert emap.debug_get("navquad_passes") == 64
    finally:
        emap.debug_set("navquad_passes", 0)
        emap.debug_set("nav_chunk", 0)
        dev.close()


# ---- 5. nothing is allocated the second time ---------------------------------------------------------------------------------------------
def test_second_identical_call_allocates_nothing(emap):
    g = scenario("130x90", "noise")
    start, goal, flags, want = expected("130x90", "noise")[0]
    dev = device_copy(emap, g)
    try:
        same_plan(dev, want, start, goal, flags, "first")
        a1 = emap.debug_get("arena_allocations")
        for k in range(2):
            same_plan(dev, want, start, goal, flags, f"again {k}")
        assert emap.debug_get("arena_allocations") == a1
    finally:
        dev.close()


# ---- 6. what runs on the plan's slots -----------------------------------------------------------------------------------------------------
def test_paths_goal_and_frontiers_run_on_the_quadratic_potential(emap):
    rng = np.random.default_rng(66)
    g = np.array(scenario("130x90", "noise"))
    g[20:40, 100:115] = 255                                              # an unknown patch: frontier cells around it
    g[60:70, 10:30] = 255
    w = lin.weights(allow_unknown=False)
    start = (5, 6)
    want = ref.plan(g, w, 0, start, start)
    pot = want["pot"]
    reached = np.argwhere(pot < ref.UNREACHED)
    goals = [(int(x), int(y)) for y, x in rng.choice(reached, 62, replace=False)] + [(-1, 4), (101, 25)]     # off the map; unknown: unreached
    dev = device_copy(emap, g)
    try:
        same_plan(dev, want, start, start, 0, "start = goal", w)
        world = [centre(c) for c in goals]
        cap = 8 * 130
        for form, walk in ((pref.GRADIENT, pref.walk), (pref.GRID, pref.walk_grid)):
            pts, res = dev.nav_paths(world, form, cap, raw=True)
            found = 0
            for i, goal in enumerate(goals):
                wpts, wres = walk(pot, start, goal, cap)
                assert res[i].tolist() == pref.words(wres), (form, i, goal)
                assert pts[i, :wres["n_points"]].tobytes() == pref.points_array(wpts).tobytes(), (form, i, goal)
                found += wres["status"] == pref.FOUND
            assert found >= 30 and {int(r[0]) for r in res} >= {pref.FOUND, pref.OFF_MAP, pref.UNREACHED_GOAL}
        assert dev.read_potential()[0].tobytes() == pot.tobytes()
        fwant = fref.search(g, pot, RES, 0.0, 1.0, 0.001)
        assert fwant["n_kept"] >= 2 and fwant["best"] >= 0
        fst = dev.frontiers(0.0, 1.0, 0.001)
        assert (fst["n_cells"], fst["n_frontiers"], fst["n_kept"], fst["best"]) == (fwant["n_cells"], fwant["n_frontiers"], fwant["n_kept"], fwant["best"])
        assert fst["best_frontier"]["access_potential"] == fwant["best_frontier"]["access_potential"]
        assert fst["best_frontier"]["centroid"] == fref.centroid(fwant["best_frontier"], RES, *ORIGIN)
        kept, labels = dev.read_frontiers()
        assert labels.tobytes() == fwant["labels"].tobytes() and [k["access_potential"] for k in kept] == [r["access_potential"] for r in fwant["kept"]]
        goal = goals[0]                                                   # another goal on the same potential: one walk, no second search
        path, st = dev.nav_plan_to(centre(goal))
        cells = [y * 130 + x for x, y in lin.get_path(pot, start, goal)]
        assert st["found"] == 1 and st["goal_potential"] == int(pot[goal[1], goal[0]]) and dev.read_potential()[1].tolist() == cells
        assert path.tobytes() == lin.centres(cells, 130, RES, *ORIGIN).tobytes()
        assert dev.read_potential()[0].tobytes() == pot.tobytes()
    finally:
        dev.close()


# ---- 7. whichever plan ran last is the costmap's plan -------------------------------------------------------------------------------------
def test_linear_and_quadratic_plans_replace_each_other(emap):
    g = scenario("65x65", "noise")
    start, goal, flags, want = expected("65x65", "noise")[0]
    wl = lin.plan(g, default_weights(), flags, start, goal)
    assert wl["pot"].tobytes() != want["pot"].tobytes()
    dev = device_copy(emap, g)
    try:
        for k in range(2):
            same_plan(dev, want, start, goal, flags, f"quadratic {k}")
            _path, st = dev.nav_plan(centre(start), centre(goal), None, outline=bool(flags))
            pot, cells = dev.read_potential()
            assert pot.tobytes() == wl["pot"].tobytes() and cells.tolist() == wl["cells"].tolist() and st["goal_potential"] == wl["goal_potential"]
            assert dev.nav_status() == st
    finally:
        dev.close()


# ---- 8. stale plans and errors --------------------------------------------------------------------------------------------------------------
def test_generation_rule_and_the_error_cases():
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    g = scenario("65x65", "noise")
    start, goal, flags, want = expected("65x65", "noise")[0]
    dev = device_copy(m, g)
    w = np.array(default_weights(), np.int32)
    wp = w.ctypes.data_as(C.POINTER(C.c_int))
    nan, inf = float("nan"), float("inf")

    def plan(id_=None, s=centre(start), e=centre(goal), wt=wp, fl=flags, st=True, xy=None, cap=0):
        status = _lib.NavplanStatus()
        status.n_path = -77
        rc = lib.gem_costmap_navplan_quadratic(h, dev.id if id_ is None else id_, (C.c_double * 2)(*s) if s else None,
                                               (C.c_double * 2)(*e) if e else None, wt, fl, xy, cap, C.byref(status) if st else None)
        return rc, status

    def read():
        return lib.gem_costmap_navplan_read(h, dev.id, None, None, 0)

    def unchanged(what):
        pot = np.zeros((65, 65), np.int32)
        cells = np.zeros(want["n_path"], np.int32)
        assert lib.gem_costmap_navplan_read(h, dev.id, pot.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p), cells.size) == 0, what
        assert pot.tobytes() == want["pot"].tobytes() and cells.tolist() == want["cells"].tolist(), what

    try:
        assert read() == INV                                              # no plan yet
        rc, st = plan()
        assert rc == 0 and st.n_path == want["n_path"] and st.found == 1
        unchanged("the first plan")
        for bad in (-1, 5, 8, 1 << 20):
            assert plan(id_=bad)[0] == INV
        for fl in (2, 3, 4, -1):
            rc, st = plan(fl=fl)
            assert rc == INV and st.n_path == -77
        assert plan(wt=None)[0] == INV and plan(s=None)[0] == INV and plan(e=None)[0] == INV and plan(st=False)[0] == INV
        neg = w.copy(); neg[3] = -1
        assert plan(wt=neg.ctypes.data_as(C.POINTER(C.c_int)))[0] == INV
        top = w.copy(); top[200] = 463                                    # the weight limit
        rc, st = plan(wt=top.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc == INV and st.n_path == -77 and b"462" in lib.gem_last_error(h)
        for v in (nan, inf, -inf):
            assert plan(s=(v, 3.0))[0] == INV and plan(s=(0.0, v))[0] == INV and plan(e=(v, 3.0))[0] == INV and plan(e=(0.0, v))[0] == INV
        xy = np.full((4, 2), -1.0)
        assert plan(xy=xy.ctypes.data_as(C.c_void_p), cap=-1)[0] == INV and (xy == -1.0).all()
        w2 = ElevationMap(32, 0.05)                                       # a handle with a communicator
        w2.comm_init_loopback(9545, 1, 0, tile_strips=False)
        status = _lib.NavplanStatus()
        s2, e2 = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(1.0, 1.0)
        assert w2._lib.gem_costmap_navplan_quadratic(w2._h, 0, s2, e2, wp, 0, None, 0, C.byref(status)) == INV
        w2.close()
        unchanged("after the errors")
        assert dev.read().tobytes() == g.tobytes()

        # out_xy too short: an error, the first cap points written and the status filled; the plan is on record
        rc, status = plan(xy=xy.ctypes.data_as(C.c_void_p), cap=4)
        assert rc == INV and status.n_path == want["n_path"] and status.found == 1
        assert xy.tobytes() == lin.centres(want["cells"][:4], 65, RES, *ORIGIN).tobytes()
        unchanged("after the short call")
        top[200] = 462                                                    # accepted: byte 200 costs 462 now
        rc, st = plan(wt=top.ctypes.data_as(C.POINTER(C.c_int)))
        want462 = ref.plan(g, top, flags, start, goal)
        assert rc == 0 and st.goal_potential == want462["goal_potential"] and dev.read_potential()[0].tobytes() == want462["pot"].tobytes()
        assert plan()[0] == 0

        # an observe with an observation makes the plan stale until the next plan
        cloud = np.array([[ORIGIN[0] + 20.5 * RES, ORIGIN[1] + 20.5 * RES, 0.3]], np.float32)
        dev.observe([{"points": cloud, "origin": (ORIGIN[0] + 10.5 * RES, ORIGIN[1] + 10.5 * RES, 0.2), "obstacle_range": 5.0, "raytrace_range": 5.0}])
        assert read() == INV
        observed = dev.read()
        assert observed[20, 20] == 254
        want_o = ref.plan(observed, default_weights(), flags, start, goal)
        assert plan()[0] == 0 and dev.read_potential()[0].tobytes() == want_o["pot"].tobytes()

        # a roll that moves the map makes it stale too
        dev.roll_to(ORIGIN[0] + 65 * RES / 2 + 7 * RES, ORIGIN[1] + 65 * RES / 2 - 4 * RES)
        assert read() == INV
        geo = dev.geometry()
        rolled = dev.read()
        o2 = (geo["origin_x"], geo["origin_y"])
        want2 = ref.plan(rolled, default_weights(), 0, (5, 6), (50, 40))
        path, st2 = dev.nav_plan_quadratic(centre((5, 6), RES, o2), centre((50, 40), RES, o2), None, outline=False)
        pot, cells = dev.read_potential()
        assert pot.tobytes() == want2["pot"].tobytes() and cells.tolist() == want2["cells"].tolist()
        assert path.tobytes() == lin.centres(want2["cells"], 65, RES, *o2).tobytes()
    finally:
        dev.close()
        m.close()


# ---- 9. the C++ facade --------------------------------------------------------------------------------------------------------------------
def test_cpp_navquad_facade(tmp_path):
    exe = build_navquad_facade(tmp_path / "navquad_facade")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
