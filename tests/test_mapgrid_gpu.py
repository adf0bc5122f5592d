"""Path and goal distance grids on the device costmap (gem_costmap_mapgrid_prepare / _read / _score) against the set form of
tests/mapgrid_ref.py.  Every comparison is exact: grids by tobytes(), started and the goal cell as integers, scores as integers.

  1. geometries at which a word boundary, a partial last word or a thin grid can go wrong (75 x 75, 130 x 90, 64 x 64, 65 x 3,
     1 x 200, 200 x 1), each empty, with 30 % blocked noise of 253 / 254 / 255, with a wall at columns 63 - 64 with one gap, and with a
     source in each of the four corners;
  2. long searches: a one-cell serpentine on 75 x 75 (2886 levels), 512 x 512 (the cap) empty and with 20 % noise, 513 x 512 refused;
  3. the run: off the map, in, out and in again; a second point on 255; a first point on 254; never on the map; an empty plan; PATH,
     GOAL and both in one call;
  4. scoring 300 trajectories of 7 poses around and beyond the map's edge: Last and Sum, with and without stop-on-failure, xshift 0
     and 0.325, a -4 behind a -3 and the reverse, host and device forms;
  5. the enqueued cycle mark -> clear footprint -> reset window -> merge -> inflate -> prepare -> both scorings with no host wait in
     between, and no allocation in a second identical loop;
  6. a stale grid after roll_to, and the other error cases (GEM_ERR_INVALID, grids unchanged);
  7. the C++ facade (tests/cpp/mapgrid_check.cpp) as a child process."""
import ctypes as C
import functools
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gem_amd import ElevationMap, _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import costmap_ref as cref  # noqa: E402
import footprint_ref as fref  # noqa: E402
import inflate_ref as iref  # noqa: E402
import mapgrid_ref as ref  # noqa: E402
from test_costmap_gpu import lattice_cloud  # noqa: E402
from test_mapgrid_cpu import build_mapgrid_check  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
GEOMETRIES = {"75x75": (75, 75), "130x90": (130, 90), "64x64": (64, 64), "65x3": (65, 3), "1x200": (1, 200), "200x1": (200, 1)}   # size_x, size_y
RES, ORIGIN = 0.05, (-3.1, 2.7)
INV = _lib.GEM_OK - 1
PATH, GOAL, BOTH = _lib.MAPGRID_PATH, _lib.MAPGRID_GOAL, _lib.MAPGRID_PATH | _lib.MAPGRID_GOAL
STOP, SUM = _lib.MAPGRID_STOP_ON_FAILURE, _lib.MAPGRID_SUM


@pytest.fixture(scope="module")
def emap():
    m = ElevationMap(32, 0.05)
    yield m
    m.close()


def ref_map(grid, res=RES, origin=ORIGIN):
    cm = cref.Costmap(grid.shape[1], grid.shape[0], res, *origin, 0)
    cm.grid[:] = grid
    return cm


def centre(cm, x, y):
    """a world point well inside cell (x, y)"""
    return (cm.ox + (x + 0.5) * cm.res, cm.oy + (y + 0.5) * cm.res)


def device_copy(m, cm):
    dev = m.costmap(cm.size_x, cm.size_y, cm.res, cm.ox, cm.oy, 0)
    dev.write(cm.grid)
    return dev


def same_grids(dev, want, which=BOTH, what=""):
    for bit, name in ((PATH, "path"), (GOAL, "goal")):
        if not which & bit:
            continue
        got, started, goal = dev.read_map_grid(bit)
        assert (started, goal) == (want["started"], want["goal_cell"]), f"{what} {name}: started {started}, goal cell {goal}"
        assert got.dtype == np.int32 and got.tobytes() == want[name].tobytes(), f"{what} {name}: {int((got != want[name]).sum())} cells differ"


def check(m, cm, plan, what=""):
    want = ref.grids(cm, plan)
    dev = device_copy(m, cm)
    try:
        dev.prepare_map_grid(plan, BOTH)
        same_grids(dev, want, BOTH, what)
    finally:
        dev.close()
    return want


@functools.lru_cache(maxsize=None)
def scenario(geom, kind):
    """(grid, plans): never changed"""
    sx, sy = GEOMETRIES[geom]
    rng = np.random.default_rng(sx * 1000 + sy)
    g = np.zeros((sy, sx), np.uint8)
    cm0 = ref_map(g)
    diagonal = [centre(cm0, 0, 0), centre(cm0, sx // 2, sy // 2), centre(cm0, sx - 1, sy - 1)]
    plans = [diagonal]
    if kind == "noise":
        g = rng.integers(0, 253, (sy, sx), dtype=np.uint8)
        blk = rng.random((sy, sx)) < 0.3
        g[blk] = rng.integers(253, 256, int(blk.sum()), dtype=np.uint8)
        free = np.argwhere(g < 253)
        y, x = free[len(free) // 2]
        plans = [[centre(cm0, int(x), int(y))], diagonal]
    elif kind == "wall":
        gap = sy // 3
        for col in (63, 64):
            if col < sx:
                g[:, col] = 254
                g[gap, col] = 0
        if sx == 1:                                                      # a thin map: the wall lies across it
            g[63:65, 0] = 254
        plans = [[centre(cm0, 0, sy - 1)], [centre(cm0, sx - 1, 0)]]
    elif kind == "corners":
        plans = [[centre(cm0, x, y)] for x, y in ((0, 0), (sx - 1, 0), (0, sy - 1), (sx - 1, sy - 1))]
        plans.append([p[0] for p in plans])                              # and a plan through all four: the adjusted plan runs along the borders
    g.setflags(write=False)
    return g, plans


# ---- 1. geometries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["empty", "noise", "wall", "corners"])
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_geometries(emap, geom, kind):
    g, plans = scenario(geom, kind)
    cm = ref_map(g)
    OB, UN = ref.constants(g)
    seen = set()
    for k, plan in enumerate(plans):
        want = check(emap, cm, plan, f"{geom} {kind} plan {k}")
        seen |= set(np.unique(want["path"]).tolist()) | set(np.unique(want["goal"]).tolist())
    if kind in ("noise", "wall") and min(g.shape) > 3:
        assert OB in seen                                                # the blocked rim occurs
    if kind == "noise" and min(g.shape) > 3:
        assert UN in seen                                                # and so do cells the search cannot reach
    if kind == "empty":
        assert max(seen) < OB


# ---- 2. long searches -----------------------------------------------------------------------------------------------------------------
def test_serpentine_of_2886_levels(emap):
    n = 75
    g = np.zeros((n, n), np.uint8)
    for y in range(1, n, 2):
        g[y, :] = 254
        g[y, n - 1 if y % 4 == 1 else 0] = 0
    cm = ref_map(g)
    want = check(emap, cm, [centre(cm, 0, 0)], "serpentine")
    reached = want["path"][want["path"] < n * n]
    assert int(reached.max()) == 2886


@pytest.mark.parametrize("kind", ["empty", "noise"])
def test_the_cap_size(emap, kind):
    n = 512
    rng = np.random.default_rng(512)
    g = np.zeros((n, n), np.uint8)
    if kind == "noise":
        blk = rng.random((n, n)) < 0.2
        g[blk] = rng.integers(253, 256, int(blk.sum()), dtype=np.uint8)
        g[250:262, 250:262] = 0
    cm = ref_map(g)
    want = check(emap, cm, [centre(cm, 255, 256), centre(cm, 258, 256)], f"512 x 512 {kind}")
    assert want["started"] == 1 and int(want["path"][want["path"] < n * n].max()) >= 500


def test_a_map_above_the_cap_is_refused(emap):
    dev = emap.costmap(513, 512, RES, 0.0, 0.0, 0)
    try:
        plan = (C.c_double * 2)(1.0, 1.0)
        assert emap._lib.gem_costmap_mapgrid_prepare(emap._h, dev.id, plan, 1, BOTH) == INV
        assert emap._lib.gem_costmap_mapgrid_read(emap._h, dev.id, PATH, None, None, None) == INV      # nothing was prepared
    finally:
        dev.close()


# ---- 3. the run -------------------------------------------------------------------------------------------------------------------------
def run_map():
    g = np.array(scenario("130x90", "empty")[0])
    g[40:50, 70] = 254
    g[10, 20:30] = 253
    return g


def test_run_enters_leaves_and_enters_again(emap):
    cm = ref_map(run_map())
    far = (cm.ox - 1.0, cm.oy + 1.0)
    plan = [far, centre(cm, 3, 20), centre(cm, 12, 22), (cm.ox + 2.0, cm.oy - 0.4), centre(cm, 60, 30), centre(cm, 100, 80)]
    want = check(emap, cm, plan, "in, out, in")
    cells = ref.plan_cells(cm, ref.adjust_plan(plan, cm.res))
    a, b = ref.run(cm.grid, cells)
    assert a > 0 and b < len(cells) and cells[b] is None and any(c is not None for c in cells[b:])
    assert want["started"] == 1 and want["path"][30, 60] > 0 and want["goal_cell"] == cells[b - 1]


def test_run_ends_at_a_255_cell_and_starts_on_254(emap):
    g = run_map()
    cm = ref_map(g)
    g2 = g.copy()
    g2[25, 40] = 255
    cm2 = ref_map(g2)
    plan = [centre(cm, 39, 25), centre(cm, 40, 25), centre(cm, 41, 25), centre(cm, 60, 25)]
    want = check(emap, cm2, plan, "second point on 255")
    assert want["goal_cell"] == (39, 25) and want["path"][25, 41] == 4      # round the unknown cell
    g3 = g.copy()
    g3[25, 39] = 254
    want = check(emap, ref_map(g3), plan, "first point on 254")
    assert want["path"][25, 39] == 0 and want["path"][24, 39] == 1 and want["goal_cell"] == (60, 25)
    g4 = g.copy()
    g4[25, 39] = 255                                                     # the first point is skipped, the run starts at the second
    want = check(emap, ref_map(g4), plan, "first point on 255")
    assert want["path"][25, 40] == 0 and want["path"][25, 39] == g.size


def test_never_on_the_map_and_an_empty_plan(emap):
    cm = ref_map(run_map())
    OB, UN = ref.constants(cm.grid)
    rng = np.random.default_rng(3)
    poses = fref.poses_from_yaw(np.stack([rng.uniform(cm.ox, cm.ox + 6.0, 21), rng.uniform(cm.oy, cm.oy + 4.0, 21), rng.uniform(-3, 3, 21)], axis=1))
    dev = device_copy(emap, cm)
    try:
        for plan in ([(cm.ox - 1.0, cm.oy - 1.0), (cm.ox - 0.5, cm.oy + 100.0)], np.zeros((0, 2))):
            want = ref.grids(cm, plan)
            assert want["started"] == 0 and (want["path"] == UN).all()
            dev.prepare_map_grid(plan)
            same_grids(dev, want)
            assert dev.score_map_grid(PATH, poses, 7, 0.0, STOP).tolist() == [-2, -2, -2]
            assert dev.score_map_grid(GOAL, poses, 7, 0.0, SUM).tolist() == [7 * UN] * 3
    finally:
        dev.close()


def test_path_goal_and_both_give_the_same_grids(emap):
    cm = ref_map(np.array(scenario("130x90", "noise")[0]))
    free = np.argwhere(cm.grid < 253)
    (y0, x0), (y1, x1) = free[10], free[11]
    plan = [centre(cm, int(x0), int(y0)), centre(cm, int(x1), int(y1))]
    want = ref.grids(cm, plan)
    assert want["path"].tobytes() != want["goal"].tobytes()
    dev = device_copy(emap, cm)
    try:
        dev.prepare_map_grid(plan, PATH)
        same_grids(dev, want, PATH, "PATH alone")
        assert emap._lib.gem_costmap_mapgrid_read(emap._h, dev.id, GOAL, None, None, None) == INV      # not prepared yet
        dev.prepare_map_grid(plan, GOAL)
        same_grids(dev, want, BOTH, "GOAL alone, PATH kept")
        dev.prepare_map_grid(plan, BOTH)
        same_grids(dev, want, BOTH, "both")
    finally:
        dev.close()


# ---- 4. scoring -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scoring_case():
    g = np.array(scenario("130x90", "noise")[0])
    g[30:60, 40:90][g[30:60, 40:90] >= 253] = 0                           # a reachable region, so that distances of every kind occur
    g[44:47, 60:63] = 254
    cm = ref_map(g)
    plan = [centre(cm, 45, 35), centre(cm, 80, 55)]
    want = ref.grids(cm, plan)
    OB, UN = ref.constants(g)
    T, n = 7, 300
    rng = np.random.default_rng(11)
    # trajectories that start anywhere up to a metre beyond the edge and move by up to four cells a pose
    start = np.stack([rng.uniform(cm.ox - 1.0, cm.ox + 130 * RES + 1.0, n), rng.uniform(cm.oy - 1.0, cm.oy + 90 * RES + 1.0, n)], axis=1)
    inside = rng.random(n) < 0.6                                         # most start in the reachable region: whole trajectories on the map
    start[inside] = np.stack([rng.uniform(cm.ox + 45 * RES, cm.ox + 85 * RES, int(inside.sum())),
                              rng.uniform(cm.oy + 35 * RES, cm.oy + 55 * RES, int(inside.sum()))], axis=1)
    steps = rng.uniform(-4 * RES, 4 * RES, (n, T, 2)).cumsum(axis=1)
    xy = start[:, None, :] + steps
    xyt = np.concatenate([xy.reshape(-1, 2), rng.uniform(-np.pi, np.pi, (n * T, 1))], axis=1)
    # two made ones: an obstacle cell (-3) before a pose off the map (-4), and the reverse
    ob_cells = np.argwhere(want["path"] == OB)
    y, x = ob_cells[len(ob_cells) // 2]
    on, ob, off = centre(cm, 50, 40), centre(cm, int(x), int(y)), (cm.ox - 2.0, cm.oy + 1.0)
    made = [on, on, ob, on, off, on, on] + [on, off, on, ob, on, on, on]
    xyt[:2 * T, :2] = made
    xyt[:2 * T, 2] = 0.0
    return cm, plan, want, fref.poses_from_yaw(xyt), T


def test_scoring(emap):
    import torch
    cm, plan, want, poses, T = scoring_case()
    OB, UN = ref.constants(cm.grid)
    dev = device_copy(emap, cm)
    d_poses = torch.from_numpy(poses.copy()).to("cuda:0")
    try:
        dev.prepare_map_grid(plan)
        same_grids(dev, want)
        seen = set()
        for bit, name in ((PATH, "path"), (GOAL, "goal")):
            for flags in (0, SUM, STOP, STOP | SUM):
                for xshift in (0.0, 0.325):
                    exp = ref.score(cm, want[name], poses, T, xshift, flags)
                    got = dev.score_map_grid(bit, poses, T, xshift, flags)
                    assert got.dtype == np.int64 and got.tolist() == exp.tolist(), (name, flags, xshift)
                    d_got = dev.score_map_grid(bit, d_poses, T, xshift, flags)     # only enqueued
                    emap.synchronize()
                    assert d_got.dtype == torch.int64 and d_got.cpu().numpy().tolist() == exp.tolist(), (name, flags, xshift, "device")
                    if xshift == 0.0:
                        assert exp[:2].tolist() == ([-3, -4] if flags & STOP else [-4, -4])     # the first event in pose order decides
                    seen |= set(exp.tolist())
                    if flags == STOP:
                        assert {-4, -3, -2} <= set(exp.tolist()) and (exp >= 0).sum() > 30
                    if flags == SUM:
                        assert (exp > UN).any() and ((exp >= 0) & (exp < OB)).any()
    finally:
        dev.close()


def test_scoring_long_trajectories(emap):
    """30 and 9 poses a trajectory: the wider lane groups, and a pose count that is no multiple of the group"""
    cm, plan, want, poses, _ = scoring_case()
    dev = device_copy(emap, cm)
    try:
        dev.prepare_map_grid(plan)
        for T in (30, 9, 1):
            p = poses[14:14 + (len(poses) - 14) // T * T]
            for flags in (0, SUM, STOP | SUM):
                assert dev.score_map_grid(PATH, p, T, 0.0, flags).tolist() == ref.score(cm, want["path"], p, T, 0.0, flags).tolist(), (T, flags)
    finally:
        dev.close()


# ---- 5. the cycle -----------------------------------------------------------------------------------------------------------------------
def test_the_enqueued_cycle_and_a_second_loop_allocates_nothing(emap):
    sx = sy = 75
    res, origin = 0.2, (-3.1, 2.7)
    window = (5, 4, 70, 72)
    p = iref.Params(0.55, 0.41, 3.0, False)                              # R = 3
    rng = np.random.default_rng(5)
    layer_ref, master_ref = cref.Costmap(sx, sy, res, *origin), cref.Costmap(sx, sy, res, *origin, cref.FREE_SPACE)
    layer, master = emap.costmap(sx, sy, res, *origin), emap.costmap(sx, sy, res, *origin, cref.FREE_SPACE)
    stale = rng.integers(1, 253, (sy, sx), dtype=np.uint8)
    T, n_traj = 5, 200
    xyt = np.stack([rng.uniform(origin[0] + 3.0, origin[0] + 12.0, T * n_traj), rng.uniform(origin[1] + 3.0, origin[1] + 12.0, T * n_traj),
                    rng.uniform(-np.pi, np.pi, T * n_traj)], axis=1)
    poses = fref.poses_from_yaw(xyt)
    robot = (origin[0] + 7.5, origin[1] + 7.5, math.cos(0.3), math.sin(0.3))
    plan = [(origin[0] + 7.5, origin[1] + 7.5), (origin[0] + 11.0, origin[1] + 9.0), (origin[0] + 13.9, origin[1] + 13.9)]
    clouds = [lattice_cloud(rng, 3000, layer_ref) for _ in range(2)]

    def loop():
        out = []
        for pts in clouds:
            master_ref.grid[:] = stale
            master.write(stale)
            cref.mark_points(layer_ref, pts, 0.5)
            assert fref.clear_footprint(layer_ref, robot, fref.RECTANGLE)
            iref.reset_window(master_ref.grid, *window, cref.FREE_SPACE)
            cref.merge(layer_ref, master_ref, window, cref.MAX)
            master_ref.grid[:] = iref.inflate_exact(master_ref.grid, p, res, window)
            want_obstacle = fref.score_trajectories(fref.footprint_cost(master_ref, poses, fref.RECTANGLE, fref.INSCRIBED_LETHAL), T, 0)
            want = ref.grids(master_ref, plan)
            want_path = ref.score(master_ref, want["path"], poses, T, 0.0, STOP)
            want_goal = ref.score(master_ref, want["goal"], poses, T, 0.325, STOP | SUM)
            # the device: nine calls, nothing waits before the first scores come back
            layer.mark_points(pts, 0.5, None)
            ok, _ = layer.clear_footprint(robot, fref.RECTANGLE)
            master.reset_window(*window)
            layer.merge(master, window, cref.MAX)
            master.inflate(p.inflation_radius, p.inscribed_radius, p.cost_scaling_factor, p.inflate_unknown, window)
            master.prepare_map_grid(plan)
            got_obstacle = master.score_trajectories(poses, T, fref.RECTANGLE, fref.INSCRIBED_LETHAL)
            got_path = master.score_map_grid(PATH, poses, T, 0.0, STOP)
            got_goal = master.score_map_grid(GOAL, poses, T, 0.325, STOP | SUM)
            assert ok and got_obstacle.tolist() == want_obstacle.tolist()
            assert got_path.tolist() == want_path.tolist() and got_goal.tolist() == want_goal.tolist()
            same_grids(master, want, BOTH, "cycle")
            assert want["started"] == 1 and (want["path"] == sx * sy).any() and (want_path >= 0).any() and (want_path == -3).any()
            out.append(got_path.tolist())
        return out

    try:
        first = loop()
        a1 = emap.debug_get("arena_allocations")
        second = loop()
        assert emap.debug_get("arena_allocations") == a1
        assert len(first) == len(second) == 2                             # (the layer keeps its marks: the loops' grids differ)
    finally:
        layer.close(); master.close()


# ---- 6. stale grids and errors --------------------------------------------------------------------------------------------------------
def test_stale_after_a_roll_and_the_error_cases():
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    cm = ref_map(np.array(scenario("75x75", "noise")[0]))
    free = np.argwhere(cm.grid < 253)
    y0, x0 = free[len(free) // 2]
    plan = [centre(cm, int(x0), int(y0))]
    dev = device_copy(m, cm)
    nan, inf = float("nan"), float("inf")
    poses = fref.poses_from_yaw(np.array([[cm.ox + 1.0, cm.oy + 1.0, 0.2], [cm.ox + 2.0, cm.oy + 1.5, 0.1]]))
    pp = poses.ctypes.data_as(C.c_void_p)
    out = np.full(2, -99, np.int64)
    po = out.ctypes.data_as(C.c_void_p)

    def prepare(id_=None, pts=plan, n=None, which=BOTH):
        v = np.ascontiguousarray(pts, np.float64).reshape(-1, 2)
        return lib.gem_costmap_mapgrid_prepare(h, dev.id if id_ is None else id_, v.ctypes.data_as(C.POINTER(C.c_double)) if v.size else None,
                                               v.shape[0] if n is None else n, which)

    def score(id_=None, which=PATH, p=pp, n=2, T=1, xshift=0.0, flags=0, o=po):
        return lib.gem_costmap_mapgrid_score(h, dev.id if id_ is None else id_, which, p, n, T, xshift, flags, o)

    def read(id_=None, which=PATH):
        return lib.gem_costmap_mapgrid_read(h, dev.id if id_ is None else id_, which, None, None, None)

    try:
        assert read() == INV and score() == INV                           # never prepared
        assert prepare() == 0
        want = ref.grids(cm, plan)
        same_grids(dev, want)
        for bad in (-1, 5, 8, 1 << 20):
            assert prepare(id_=bad) == INV and read(id_=bad) == INV and score(id_=bad) == INV
        for which in (0, 4, 7, -1):
            assert prepare(which=which) == INV
        for which in (0, 3, 4):
            assert read(which=which) == INV and score(which=which) == INV
        assert prepare(pts=[], n=3) == INV and prepare(n=-1) == INV        # NULL with a count | a negative count
        for v in (nan, inf, -inf):
            assert prepare(pts=[plan[0], (v, 0.0)]) == INV and prepare(pts=[(0.0, v)]) == INV
            assert score(xshift=v) == INV
        assert prepare(pts=[(0.0, 0.0), (1e5, 0.0)]) == INV                # 2 000 000 points at this resolution
        assert score(flags=4) == INV and score(flags=-1) == INV
        assert score(p=None) == INV and score(o=None) == INV and score(n=-1) == INV
        assert score(T=0) == INV and score(T=(1 << 20) + 1) == INV and score(n=1 << 30, T=4) == INV
        w2 = ElevationMap(32, 0.05)                                       # a handle with a communicator
        w2.comm_init_loopback(9543, 1, 0, tile_strips=False)
        v = (C.c_double * 2)(0.0, 0.0)
        assert w2._lib.gem_costmap_mapgrid_prepare(w2._h, 0, v, 1, BOTH) == INV
        assert w2._lib.gem_costmap_mapgrid_read(w2._h, 0, PATH, None, None, None) == INV
        assert w2._lib.gem_costmap_mapgrid_score(w2._h, 0, PATH, pp, 2, 1, 0.0, 0, po) == INV
        w2.close()
        assert out.tolist() == [-99, -99]
        same_grids(dev, want, BOTH, "after the errors")
        assert dev.read().tobytes() == cm.grid.tobytes()
        assert score() == 0 and out.tolist() == ref.score(cm, want["path"], poses, 1).tolist()
        assert score(n=0, p=None, o=None) == 0                             # no trajectories: fine

        # a roll that moves nothing keeps the grids; one that moves the map makes them stale until the next prepare
        dev.update_origin(cm.ox + 0.3 * RES, cm.oy)
        same_grids(dev, want, BOTH, "a roll by less than a cell")
        sizes = cm.size_in_meters()
        dev.roll_to(cm.ox + sizes[0] / 2 + 7 * RES, cm.oy + sizes[1] / 2 - 4 * RES)
        assert read(which=PATH) == INV and read(which=GOAL) == INV and score() == INV
        geo = dev.geometry()
        rolled = cref.Costmap(cm.size_x, cm.size_y, RES, geo["origin_x"], geo["origin_y"], 0)
        rolled.grid[:] = dev.read()
        assert rolled.grid.tobytes() != cm.grid.tobytes()
        assert prepare(which=GOAL) == 0
        want2 = ref.grids(rolled, plan)
        same_grids(dev, want2, GOAL, "after the roll")
        assert read(which=PATH) == INV                                    # only the goal grid was prepared again
        assert prepare(which=PATH) == 0
        same_grids(dev, want2, BOTH, "both again")
        dev.close()
        dev = device_copy(m, cm)                                         # the same id, created anew: nothing is prepared
        assert read() == INV and score() == INV
    finally:
        dev.close()
        m.close()


# ---- 7. the C++ facade ------------------------------------------------------------------------------------------------------------------
def test_cpp_mapgrid_facade(tmp_path):
    exe = build_mapgrid_check(tmp_path / "mapgrid_check")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
