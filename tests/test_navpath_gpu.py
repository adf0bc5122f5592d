"""Paths on the last plan's potential for a batch of goals (gem_costmap_navplan_paths / _device) against the host twin on the read-back
potential, which tests/test_navpath_cpu.py pins to tests/navpath_ref.py.  Every comparison is exact: the result words as integers, the
points as bit patterns.

Costmaps of 2 x 2, 40 x 40 and 65 x 130 (the last spans the potential's 64 x 64 tiles and is no multiple of them).  Plan once, then 1 goal,
64 goals and 1024 goals (all cells of a 32 x 32 window), both forms, the waiting entry and the device entry; the GRID form against
gem_costmap_navplan_goal goal by goal; the plan's status, potential and path and the frontier search as they were before the batch;
refusals, also after roll_to and after an observe call; no allocation in a second identical call; max_points of 2 and of exactly a path's
length; the pinned cycle and oscillation goals of the CPU test."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import gem_amd
from gem_amd import ElevationMap, _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import navpath_ref as ref  # noqa: E402
from test_navpath_cpu import CYCLE, MAX_POINTS, OSC, build_navpath_facade, cycle_case, osc_case, scenario  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
RES, ORIGIN = 0.2, (-3.1, 2.7)
INV = _lib.GEM_OK - 1
FORMS = (ref.GRADIENT, ref.GRID)


@pytest.fixture(scope="module")
def emap():
    m = ElevationMap(32, 0.05)
    yield m
    m.close()


def centre(cell):
    """a world point well inside cell (x, y); off the map for a cell that is"""
    return (ORIGIN[0] + (cell[0] + 0.5) * RES, ORIGIN[1] + (cell[1] + 0.5) * RES)


def grid_of(name):
    """(grid, start, outline, the 32 x 32 window's corner)"""
    if name == "2x2":
        g, start, outline = scenario("2x2", "uniform")
        return g, start, outline, (-15, -14)
    if name == "40x40":
        g, start, outline = scenario("40x40", "noise20")
        return g, start, outline, (5, 8)
    rng = np.random.default_rng(65130)
    g = rng.integers(0, 68, (130, 65), dtype=np.uint8)
    g[rng.random(g.shape) < 0.2] = 254
    start = (60, 120)
    g[start[1], start[0]] = 0
    return g, start, False, (40, 50)                                      # the window lies across the seams at x = 64 and y = 64


def goal_sets(name):
    g, start, _outline, corner = grid_of(name)
    sy, sx = g.shape
    rng = np.random.default_rng(len(name))
    far = (3 % sx, 2 % sy)
    many = [start, far, (-1, 0), (sx, sy)] + [(int(rng.integers(-1, sx + 1)), int(rng.integers(-1, sy + 1))) for _ in range(60)]
    window = [(corner[0] + i, corner[1] + j) for j in range(32) for i in range(32)]
    return {1: [far], 64: many, 1024: window}


@pytest.fixture(scope="module")
def planned(emap):
    """name -> (costmap with a plan from its start, the read-back potential, start)"""
    made = {}

    def get(name):
        if name not in made:
            g, start, outline, _corner = grid_of(name)
            dev = emap.costmap(g.shape[1], g.shape[0], RES, ORIGIN[0], ORIGIN[1], 0)
            dev.write(g)
            _path, st = dev.nav_plan(centre(start), centre(start), None, outline=outline)
            assert st["found"] == 1 and st["start_cell"] == tuple(start)
            pot, _cells = dev.read_potential()
            made[name] = (dev, pot, tuple(start))
        return made[name]

    yield get
    for dev, _pot, _start in made.values():
        dev.close()


def twin_cells(goals, shape):
    """the cells the host maps the goals' centres to: (-1, -1) off the map"""
    sy, sx = shape
    return [(x, y) if 0 <= x < sx and 0 <= y < sy else (-1, -1) for x, y in goals]


def same(pts, res, want_pts, want_res, what):
    assert res.tolist() == want_res.tolist(), what
    for i in range(res.shape[0]):
        n = int(want_res[i, 1])
        assert pts[i, :n].tobytes() == want_pts[i, :n].tobytes(), (what, i)


@pytest.mark.parametrize("n_goals", [1, 64, 1024])
@pytest.mark.parametrize("name", ["2x2", "40x40", "65x130"])
def test_batch_equals_the_twin_on_the_read_back_potential(emap, planned, name, n_goals):
    dev, pot, start = planned(name)
    goals = goal_sets(name)[n_goals]
    assert len(goals) == n_goals
    world = [centre(c) for c in goals]
    cap = 512
    for form in FORMS:
        want_pts, want_res = gem_amd.nav_paths_host(pot, start, twin_cells(goals, pot.shape), form, cap)
        pts, res = dev.nav_paths(world, form, cap, raw=True)
        same(pts, res, want_pts, want_res, f"{name} {n_goals} form {form}")
        dpts, dres = dev.nav_paths_device(world, form, cap)
        emap.synchronize()
        same(dpts.cpu().numpy(), dres.cpu().numpy(), want_pts, want_res, f"{name} {n_goals} form {form}, device entry")
        _none, res2 = dev.nav_paths(world, form, cap, points=False, raw=True)
        assert _none is None and res2.tolist() == want_res.tolist()       # without a point buffer: the results alone
    if name != "2x2" and n_goals > 1:
        statuses = set(want_res[:, 0].tolist())
        assert ref.FOUND in statuses and len(statuses) > 1, statuses


@pytest.mark.parametrize("name", ["2x2", "40x40", "65x130"])
def test_grid_form_equals_navplan_goal_and_the_facade_converts(emap, planned, name):
    """every goal of the three sets, goal by goal against gem_costmap_navplan_goal"""
    dev, pot, start = planned(name)
    g = grid_of(name)[0]
    before = (dev.nav_status(), dev.read_potential())
    batches = []
    for goals in goal_sets(name).values():                                # (the batches first: nav_plan_to replaces the last path)
        world = [centre(c) for c in goals]
        paths, results = dev.nav_paths(world, ref.GRID, 512)
        raw_pts, raw_res = dev.nav_paths(world, ref.GRID, 512, raw=True)
        batches.append((goals, world, paths, results, raw_pts, raw_res))
    assert (dev.nav_status(), dev.read_potential()[1].tolist()) == (before[0], before[1][1].tolist())
    try:
        for goals, world, paths, results, raw_pts, raw_res in batches:
            for i, goal in enumerate(goals):
                want_path, st = dev.nav_plan_to(world[i])
                r = results[i]
                assert (r["status"] == ref.FOUND) == bool(st["found"]), (goal, r, st)
                assert r["goal_cell"] == st["goal_cell"] and r["goal_potential"] == st["goal_potential"]
                assert r["n_points"] == st["n_path"] == paths[i].shape[0] == raw_res[i, 1], (goal, r, st)   # 0 off the map or unreached
                assert r["status"] in (ref.FOUND, ref.OFF_MAP, ref.UNREACHED_GOAL), (goal, r)
                assert paths[i].tobytes() == want_path.tobytes(), goal        # reversed, cell centres in double
                if st["found"]:
                    assert raw_pts[i, 0].tolist() == [float(goal[0]), float(goal[1])]                 # walk order: goal first
    finally:                                                              # nav_plan_to replaced the last path: the plan again, for the tests behind
        outline = grid_of(name)[2]
        dev.nav_plan(centre(start), centre(start), None, outline=outline)
    after = (dev.nav_status(), dev.read_potential())
    assert after[1][0].tobytes() == before[1][0].tobytes() and g.tobytes() == dev.read().tobytes()


def test_the_plan_and_the_frontier_search_stay_as_they_were(emap):
    g = np.zeros((50, 70), np.uint8)
    g[:, 45:] = 255                                                       # unknown space to the right: a frontier along column 45
    g[10:30, 20] = 254
    dev = emap.costmap(70, 50, RES, ORIGIN[0], ORIGIN[1], 0)
    try:
        dev.write(g)
        w = gem_amd.nav_weights(allow_unknown=False)
        _path, st = dev.nav_plan(centre((5, 5)), centre((30, 40)), w, outline=False)
        assert st["found"] == 1 and st["n_path"] > 20
        fst = dev.frontiers()
        assert fst["n_kept"] >= 1
        before = (dev.nav_status(), dev.read_potential(), dev.read_frontiers())
        goals = [centre((x, y)) for y in range(0, 50, 3) for x in range(0, 70, 3)]
        for form in FORMS:
            _pts, res = dev.nav_paths(goals, form, 400, raw=True)
            assert (res[:, 0] == ref.FOUND).sum() > 100
            dev.nav_paths_device(goals, form, 400)
            emap.synchronize()
        after = (dev.nav_status(), dev.read_potential(), dev.read_frontiers())
        assert after[0] == before[0]
        assert after[1][0].tobytes() == before[1][0].tobytes() and after[1][1].tolist() == before[1][1].tolist()
        assert after[2][0] == before[2][0] and after[2][1].tobytes() == before[2][1].tobytes()
        assert dev.read().tobytes() == g.tobytes()
    finally:
        dev.close()


def test_second_identical_call_allocates_nothing(emap, planned):
    dev, _pot, _start = planned("65x130")
    world = [centre(c) for c in goal_sets("65x130")[1024]]
    first = dev.nav_paths(world, ref.GRADIENT, 700, raw=True)
    a1 = emap.debug_get("arena_allocations")
    for form in FORMS:
        again = dev.nav_paths(world, form, 700, raw=True)
        dev.nav_paths(world[:64], form, 300, raw=True)                   # smaller: the arenas only grow
    assert emap.debug_get("arena_allocations") == a1
    assert again[1].shape == first[1].shape


def test_caps_of_two_and_of_exactly_the_paths_length(emap, planned):
    dev, pot, start = planned("65x130")
    far = int(np.where(pot == ref.UNREACHED, -1, pot).argmax())          # the reached cell of the largest potential
    goal = (far % pot.shape[1], far // pot.shape[1])
    for form in FORMS:
        _p, res = dev.nav_paths([centre(goal)], form, MAX_POINTS, raw=True)
        assert res[0, 0] == ref.FOUND
        n = int(res[0, 1])
        assert n > 100
        for cap, status in ((n, ref.FOUND), (n - 1, ref.CAP), (2, ref.CAP)):
            want_pts, want_res = gem_amd.nav_paths_host(pot, start, [goal], form, cap)
            assert want_res[0, 0] == status and want_res[0, 1] == min(n, cap)
            pts, res = dev.nav_paths([centre(goal)], form, cap, raw=True)
            same(pts, res, want_pts, want_res, f"form {form} cap {cap}")


def test_the_pinned_cycle_and_oscillation_goals(emap):
    for what, (pot_want, start, goals) in (("cycle", cycle_case()[:2] + ([cycle_case()[2]],)), ("osc", osc_case())):
        spec = CYCLE if what == "cycle" else OSC                          # the CPU test's grid again, planned on the device
        sx, sy = spec["size"]
        rng = np.random.default_rng(spec["seed"])
        if what == "cycle":
            g = rng.integers(0, 68, (sy, sx)).astype(np.uint8)
        else:
            g = np.zeros((sy, sx), np.uint8)
        g[rng.random(g.shape) < spec["blocked"]] = 254
        g[start[1], start[0]] = 0
        dev = emap.costmap(sx, sy, RES, ORIGIN[0], ORIGIN[1], 0)
        try:
            dev.write(g)
            dev.nav_plan(centre(start), centre(start), None, outline=False)
            pot, _cells = dev.read_potential()
            assert pot.tobytes() == pot_want.tobytes()
            for cap in (MAX_POINTS, 2 * MAX_POINTS):
                want_pts, want_res = gem_amd.nav_paths_host(pot, start, list(goals), ref.GRADIENT, cap)
                if what == "cycle":
                    assert want_res[0, 0] == ref.CAP and want_res[0, 1] == cap
                pts, res = dev.nav_paths([centre(c) for c in goals], ref.GRADIENT, cap, raw=True)
                same(pts, res, want_pts, want_res, f"{what} cap {cap}")
        finally:
            dev.close()


def test_refusals_and_stale_plans():
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    g, start, outline = scenario("40x40", "noise5")
    dev = m.costmap(40, 40, RES, ORIGIN[0], ORIGIN[1], 0)
    dev.write(g)
    res = np.full((4, 8), -77, np.int32)
    pts = np.full((4, 16, 2), -1.0, np.float32)
    nan, inf = float("nan"), float("inf")

    def call(id_=None, goals=(centre((3, 3)), centre((7, 9))), n=None, form=ref.GRADIENT, cap=16, out_pts=True, out=True, fn="gem_costmap_navplan_paths"):
        arr = np.ascontiguousarray(goals, np.float64) if goals is not None else None
        return getattr(lib, fn)(h, dev.id if id_ is None else id_, arr.ctypes.data_as(C.c_void_p) if arr is not None else None,
                                (len(goals) if goals is not None else 2) if n is None else n, form, cap,
                                pts.ctypes.data_as(C.c_void_p) if out_pts else None, res.ctypes.data_as(C.c_void_p) if out else None)

    try:
        for fn in ("gem_costmap_navplan_paths", "gem_costmap_navplan_paths_device"):
            assert call(fn=fn) == INV                                         # no plan yet
        _path, st = dev.nav_plan(centre(start), centre(start), None, outline=outline)
        assert st["found"] == 1
        before = dev.read_potential()
        a0 = m.debug_get("arena_allocations")
        for fn in ("gem_costmap_navplan_paths", "gem_costmap_navplan_paths_device"):
            for bad in (-1, 5, 8, 1 << 20):
                assert call(id_=bad, fn=fn) == INV
            assert call(goals=None, fn=fn) == INV and call(out=False, fn=fn) == INV
            for v in (nan, inf, -inf):
                assert call(goals=((v, 3.0), (0.0, 0.0)), fn=fn) == INV and call(goals=((0.0, 0.0), (1.0, v)), fn=fn) == INV
            for n in (0, -1, 1025):
                assert call(n=n, fn=fn) == INV
            for cap in (-1, 0, 1, (1 << 20) + 1):
                assert call(cap=cap, out_pts=False, fn=fn) == INV
            assert call(goals=[centre((3, 3))] * 1024, cap=(1 << 14) + 1, out_pts=False, fn=fn) == INV     # n_goals * max_points above 2^24
            for form in (-1, 2, 9):
                assert call(form=form, fn=fn) == INV
        assert (res == -77).all() and (pts == -1.0).all() and m.debug_get("arena_allocations") == a0     # nothing was written or allocated
        w2 = ElevationMap(32, 0.05)                                       # a handle with a communicator
        w2.comm_init_loopback(9546, 1, 0, tile_strips=False)
        two = np.zeros((2, 2), np.float64)
        for fn in ("gem_costmap_navplan_paths", "gem_costmap_navplan_paths_device"):
            assert getattr(w2._lib, fn)(w2._h, 0, two.ctypes.data_as(C.c_void_p), 2, 1, 16, None, res.ctypes.data_as(C.c_void_p)) == INV
        w2.close()
        assert call() == 0 and res[0, 0] in (ref.FOUND, ref.CAP) and res[2, 0] == -77                     # ... and the good call works
        after = dev.read_potential()
        assert after[0].tobytes() == before[0].tobytes()

        # a roll that moves nothing keeps the plan; one that moves the map makes it stale until the next plan
        dev.update_origin(ORIGIN[0] + 0.3 * RES, ORIGIN[1])
        assert call() == 0
        dev.roll_to(ORIGIN[0] + 40 * RES / 2 + 7 * RES, ORIGIN[1] + 40 * RES / 2 - 4 * RES)
        for fn in ("gem_costmap_navplan_paths", "gem_costmap_navplan_paths_device"):
            assert call(fn=fn) == INV
        geo = dev.geometry()
        o2 = (geo["origin_x"], geo["origin_y"])
        here = (o2[0] + 20.5 * RES, o2[1] + 20.5 * RES)
        dev.nav_plan(here, here, None, outline=False)
        there = ((o2[0] + 3.5 * RES, o2[1] + 3.5 * RES), (o2[0] + 30.5 * RES, o2[1] + 9.5 * RES))
        assert call(goals=there) == 0
        # an observe call with an observation makes it stale too
        cloud = np.array([[here[0] + 1.0, here[1] + 0.4, 0.5]], np.float32)
        dev.observe([{"points": cloud, "origin": (here[0], here[1], 0.3)}], 2.0, None)
        for fn in ("gem_costmap_navplan_paths", "gem_costmap_navplan_paths_device"):
            assert call(goals=there, fn=fn) == INV
        dev.nav_plan(here, here, None, outline=False)
        assert call(goals=there) == 0
    finally:
        dev.close()
        m.close()


def test_cpp_navpath_facade(tmp_path):
    exe = build_navpath_facade(tmp_path / "navpath_facade")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
