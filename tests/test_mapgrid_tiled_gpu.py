"""Path, goal and front distance grids on a device costmap of ANY size (gem_costmap_mapgrid_prepare_tiled / _prepare_front_tiled) against the
set form of tests/mapgrid_ref.py.  Every comparison is exact: grids by tobytes(), started and the goal cell as integers, scores as
integers, totals and answers by their bytes.

  1. geometries at which a tile seam, a partial last tile or a thin grid can go wrong (64 x 64, 65 x 65, 128 x 128, 130 x 70, 129 x 3,
     1 x 200, 200 x 1), each empty, with 30 % blocked noise, with a 254 wall on columns 63 - 64 and on rows 63 - 64 with one gap, with a
     source in each map corner, and with each of the four cells around a tile corner as the only source;
  2. above the cap of the LDS form: 513 x 512 (which prepare_map_grid still refuses), 65 x 2049, 1 x 4097, 600 x 600;
  3. the same bytes as the LDS form where both run: the 75 x 75 serpentine, 130 x 90 noise, 512 x 512 noise;
  4. many rounds and chunks: the one-cell serpentine on 130 x 130 (8514 levels) with the default chunk and with "mapgrid_chunk" 1;
  5. the run: the plans of test_mapgrid_gpu.py's case 3; 6. the slots: PATH, GOAL, both, front, one after the other, after inflate;
  7. downstream on 600 x 600 at 0.05 with grids from the tiled call alone: score_map_grid, best_trajectory, dwa_best, rollout_best;
  8. stale grids and every refusal, earlier grids untouched, no allocation in a second identical call;
  9. the C++ facade (tests/cpp/mapgrid_tiled_check.cpp) as a child process on 65 x 2049."""
import ctypes as C
import functools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import gem_amd
from gem_amd import ElevationMap, _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import critics_ref as cref  # noqa: E402
import footprint_ref as fref  # noqa: E402
import mapgrid_ref as ref  # noqa: E402
import rollout_ref as rref  # noqa: E402
import trajgen_ref as tref  # noqa: E402
from test_critics_cpu import as_c  # noqa: E402
from test_critics_gpu import FORWARD, SMALL, rejected_by, same as same_best  # noqa: E402
from test_mapgrid_gpu import RES, centre, device_copy, ref_map, run_map, same_grids, scenario  # noqa: E402
from test_rollout_cpu import TWO  # noqa: E402
from test_trajgen_cpu import CONFIG, GOAL as TG_GOAL, LIMITS  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
GEOMETRIES = {"64x64": (64, 64), "65x65": (65, 65), "128x128": (128, 128), "130x70": (130, 70), "129x3": (129, 3), "1x200": (1, 200),
              "200x1": (200, 1)}                                         # size_x, size_y
INV = _lib.GEM_OK - 1
PATH, GOAL, BOTH = _lib.MAPGRID_PATH, _lib.MAPGRID_GOAL, _lib.MAPGRID_PATH | _lib.MAPGRID_GOAL
STOP, SUM = _lib.MAPGRID_STOP_ON_FAILURE, _lib.MAPGRID_SUM


@pytest.fixture(scope="module")
def emap():
    m = ElevationMap(32, 0.05)
    yield m
    m.close()


def check(m, cm, plan, what="", want=None):
    """both grids of `plan` by the tiled call equal the reference's: (the reference's grids, the call's status)"""
    want = ref.grids(cm, plan) if want is None else want
    dev = device_copy(m, cm)
    try:
        st = dev.prepare_map_grid_tiled(plan, BOTH)
        assert (st["started"], st["goal_cell"]) == (want["started"], want["goal_cell"]), (what, st)
        assert st["chunks"] >= 1 and (st["rounds"] >= 1) == bool(want["started"]), (what, st)
        same_grids(dev, want, BOTH, what)
    finally:
        dev.close()
    return want, st


def noise(rng, sx, sy, share):
    g = rng.integers(0, 253, (sy, sx), dtype=np.uint8)
    blk = rng.random((sy, sx)) < share
    g[blk] = rng.integers(253, 256, int(blk.sum()), dtype=np.uint8)
    return g


# ---- 1. geometries x kinds -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiled_scenario(geom, kind):
    """(grid, plans): never changed"""
    sx, sy = GEOMETRIES[geom]
    rng = np.random.default_rng(sx * 1000 + sy)
    g = np.zeros((sy, sx), np.uint8)
    cm0 = ref_map(g)
    diagonal = [centre(cm0, 0, 0), centre(cm0, sx // 2, sy // 2), centre(cm0, sx - 1, sy - 1)]
    plans = [diagonal]
    if kind == "noise":
        g = noise(rng, sx, sy, 0.3)
        free = np.argwhere(g < 253)
        y, x = free[len(free) // 2]
        plans = [[centre(cm0, int(x), int(y))], diagonal]
    elif kind == "wall columns":
        gap = sy // 3
        for col in (63, 64):
            if col < sx:
                g[:, col] = 254
                g[gap, col] = 0
        plans = [[centre(cm0, 0, sy - 1)], [centre(cm0, sx - 1, 0)]]
    elif kind == "wall rows":
        gap = sx // 3
        for row in (63, 64):
            if row < sy:
                g[row, :] = 254
                g[row, gap] = 0
        plans = [[centre(cm0, sx - 1, 0)], [centre(cm0, 0, sy - 1)]]
    elif kind == "corners":
        plans = [[centre(cm0, x, y)] for x, y in ((0, 0), (sx - 1, 0), (0, sy - 1), (sx - 1, sy - 1))]
        plans.append([p[0] for p in plans])                              # and a plan through all four: the adjusted plan runs along the borders
    elif kind == "tile corner":
        around = [(x, y) for x, y in ((63, 63), (64, 63), (63, 64), (64, 64)) if x < sx and y < sy]
        g = noise(rng, sx, sy, 0.3)
        for x, y in around:
            g[y, x] = 0
        g[min(63, sy - 1), min(63, sx - 1)] = 254                        # ... one of the four is a blocked source
        plans = [[centre(cm0, x, y)] for x, y in around] or [diagonal]
    g.setflags(write=False)
    return g, plans


@pytest.mark.parametrize("kind", ["empty", "noise", "wall columns", "wall rows", "corners", "tile corner"])
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_geometries(emap, geom, kind):
    g, plans = tiled_scenario(geom, kind)
    cm = ref_map(g)
    OB, UN = ref.constants(g)
    seen = set()
    for k, plan in enumerate(plans):
        want, _ = check(emap, cm, plan, f"{geom} {kind} plan {k}")
        seen |= set(np.unique(want["path"]).tolist()) | set(np.unique(want["goal"]).tolist())
    if kind in ("noise", "wall columns") and min(g.shape) > 3 and g.shape[1] > 64:
        assert OB in seen                                                # the blocked rim occurs
    if kind == "wall rows" and g.shape[0] > 64 and g.shape[1] > 3:
        assert OB in seen
    if kind == "noise" and min(g.shape) > 3:
        assert OB in seen and UN in seen                                 # and so do cells the search cannot reach
    if kind == "empty":
        assert max(seen) < OB


# ---- 2. above the cap -------------------------------------------------------------------------------------------------------------------
def test_513_by_512_and_the_capped_entry_still_refuses(emap):
    sx, sy = 513, 512
    rng = np.random.default_rng(512)
    g = np.zeros((sy, sx), np.uint8)
    blk = rng.random((sy, sx)) < 0.2
    g[blk] = rng.integers(253, 256, int(blk.sum()), dtype=np.uint8)
    g[250:262, 250:262] = 0
    cm = ref_map(g)
    plan = [centre(cm, 255, 256), centre(cm, 258, 256)]
    want = ref.grids(cm, plan)
    assert want["started"] == 1 and int(want["path"][want["path"] < sx * sy].max()) >= 500
    dev = device_copy(emap, cm)
    try:
        v = np.ascontiguousarray(plan, np.float64)
        assert emap._lib.gem_costmap_mapgrid_prepare(emap._h, dev.id, v.ctypes.data_as(C.POINTER(C.c_double)), 2, BOTH) == INV
        assert emap._lib.gem_costmap_mapgrid_read(emap._h, dev.id, PATH, None, None, None) == INV      # nothing was prepared
        st = dev.prepare_map_grid_tiled(plan)
        assert (st["started"], st["goal_cell"]) == (1, want["goal_cell"])
        same_grids(dev, want, BOTH, "513 x 512")
        assert emap._lib.gem_costmap_mapgrid_prepare(emap._h, dev.id, v.ctypes.data_as(C.POINTER(C.c_double)), 2, BOTH) == INV
        same_grids(dev, want, BOTH, "513 x 512 after the refusal")
    finally:
        dev.close()


def test_65_by_2049(emap):
    g = noise(np.random.default_rng(2049), 65, 2049, 0.2)
    g[1000:1010, 28:38] = 0
    cm = ref_map(g)
    assert -(-65 // 64) * 2049 == 4098 > ref.MAX_WORDS
    want, st = check(emap, cm, [centre(cm, 30, 1004), centre(cm, 35, 1006)], "65 x 2049")
    assert int(want["goal"][want["goal"] < g.size].max()) > 1000 and (want["goal"] == g.size + 1).any()


def test_1_by_4097(emap):
    g = np.zeros((4097, 1), np.uint8)
    g[100, 0] = 254
    cm = ref_map(g)
    want, st = check(emap, cm, [centre(cm, 0, 2048)], "1 x 4097")
    d = want["path"]
    assert int((d < 4097).sum()) == 3996 and int((d == 4097).sum()) == 1 and int((d == 4098).sum()) == 100     # reached | OB | UN
    assert d[100, 0] == 4097 and d[101, 0] == 1947 and d[4096, 0] == 2048


def test_600_by_600(emap):
    n = 600
    g = noise(np.random.default_rng(600), n, n, 0.2)
    g[294:306, 294:306] = 0
    cm = ref_map(g)
    want, st = check(emap, cm, [centre(cm, 299, 300), centre(cm, 301, 300)], "600 x 600")
    d = want["goal"]
    assert int((d < n * n).sum()) > 250000 and int(d[d < n * n].max()) >= 590 and (d == n * n).any() and (d == n * n + 1).any()
    assert st["chunks"] >= 1 and st["rounds"] >= 5                        # the goal sits in the middle tile of ten: five seams to the edge


# ---- 3. equal to the LDS form where both run --------------------------------------------------------------------------------------------
def serpentine(n):
    g = np.zeros((n, n), np.uint8)
    for y in range(1, n, 2):
        g[y, :] = 254
        g[y, n - 1 if y % 4 == 1 else 0] = 0
    return g


@pytest.mark.parametrize("name", ["serpentine 75", "noise 130x90", "noise 512"])
def test_equal_to_the_lds_form(emap, name):
    if name == "serpentine 75":
        g = serpentine(75)
        plan = [centre(ref_map(g), 0, 0)]
    elif name == "noise 130x90":
        g = np.array(scenario("130x90", "noise")[0])
        plan = scenario("130x90", "noise")[1][1]
    else:
        g = noise(np.random.default_rng(5120), 512, 512, 0.2)
        g[250:262, 250:262] = 0
        cm0 = ref_map(g)
        plan = [centre(cm0, 255, 256), centre(cm0, 258, 256)]
    cm = ref_map(g)
    dev = device_copy(emap, cm)
    try:
        dev.prepare_map_grid(plan)
        lds = {bit: dev.read_map_grid(bit) for bit in (PATH, GOAL)}
        # the tiled grids replace them in the same slots: wipe the difference away first with another plan's grids
        dev.prepare_map_grid([centre(cm, g.shape[1] - 1, g.shape[0] - 1)])
        st = dev.prepare_map_grid_tiled(plan)
        for bit in (PATH, GOAL):
            got, started, goal = dev.read_map_grid(bit)
            assert got.tobytes() == lds[bit][0].tobytes() and (started, goal) == lds[bit][1:] == (st["started"], st["goal_cell"]), (name, bit)
        if name == "serpentine 75":
            assert int(lds[PATH][0][lds[PATH][0] < 75 * 75].max()) == 2886
    finally:
        dev.close()


# ---- 4. many rounds and chunks ----------------------------------------------------------------------------------------------------------
def test_many_rounds_and_chunks(emap):
    g = serpentine(130)
    cm = ref_map(g)
    plan = [centre(cm, 0, 0)]
    want = ref.grids(cm, plan)
    assert int(want["path"][want["path"] < 130 * 130].max()) == 8514
    try:
        _, st = check(emap, cm, plan, "serpentine 130, the default chunk", want)
        assert st["chunks"] > 1 and st["rounds"] > 6                      # 3 + 3 rounds a chunk are not enough
        emap.debug_set("mapgrid_chunk", 1)
        assert emap.debug_get("mapgrid_chunk") == 1
        _, st1 = check(emap, cm, plan, "serpentine 130, a round a chunk", want)
        assert st1["chunks"] >= st1["rounds"] > 6
        emap.debug_set("mapgrid_chunk", 0)
        one = ref_map(np.zeros((64, 64), np.uint8))
        _, st = check(emap, one, [centre(one, 20, 30)], "one tile")
        assert st["chunks"] == 1
    finally:
        emap.debug_set("mapgrid_chunk", 0)


# ---- 5. the run -------------------------------------------------------------------------------------------------------------------------
def test_the_run(emap):
    g = run_map()
    cm = ref_map(g)
    far = (cm.ox - 1.0, cm.oy + 1.0)
    plan = [far, centre(cm, 3, 20), centre(cm, 12, 22), (cm.ox + 2.0, cm.oy - 0.4), centre(cm, 60, 30), centre(cm, 100, 80)]
    want, _ = check(emap, cm, plan, "in, out, in")
    cells = ref.plan_cells(cm, ref.adjust_plan(plan, cm.res))
    a, b = ref.run(cm.grid, cells)
    assert a > 0 and b < len(cells) and cells[b] is None and want["goal_cell"] == cells[b - 1] and want["path"][30, 60] > 0
    plan = [centre(cm, 39, 25), centre(cm, 40, 25), centre(cm, 41, 25), centre(cm, 60, 25)]
    g2 = g.copy()
    g2[25, 40] = 255
    want, _ = check(emap, ref_map(g2), plan, "second point on 255")
    assert want["goal_cell"] == (39, 25) and want["path"][25, 41] == 4
    g3 = g.copy()
    g3[25, 39] = 254
    want, _ = check(emap, ref_map(g3), plan, "first point on 254")
    assert want["path"][25, 39] == 0 and want["path"][24, 39] == 1 and want["goal_cell"] == (60, 25)
    OB, UN = ref.constants(g)
    for plan in ([(cm.ox - 1.0, cm.oy - 1.0), (cm.ox - 0.5, cm.oy + 100.0)], np.zeros((0, 2))):       # never on the map | empty
        want, st = check(emap, cm, plan, "nothing accepted")
        assert st["started"] == 0 and st["goal_cell"] == (-1, -1) and st["rounds"] == 0 and st["chunks"] == 1 and (want["path"] == UN).all()


# ---- 6. the slots -----------------------------------------------------------------------------------------------------------------------
def test_slots(emap):
    g = np.array(tiled_scenario("130x70", "noise")[0])
    g[20:50, 40:100][g[20:50, 40:100] >= 253] = 0
    cm = ref_map(g)
    plan_a, plan_b = [centre(cm, 45, 25), centre(cm, 95, 45)], [centre(cm, 90, 22), centre(cm, 50, 48)]
    want_a, want_b = ref.grids(cm, plan_a), ref.grids(cm, plan_b)
    assert want_a["path"].tobytes() != want_a["goal"].tobytes() != want_b["goal"].tobytes()
    dev = device_copy(emap, cm)
    try:
        dev.prepare_map_grid_tiled(plan_a, PATH)
        same_grids(dev, want_a, PATH, "PATH alone")
        assert emap._lib.gem_costmap_mapgrid_read(emap._h, dev.id, GOAL, None, None, None) == INV      # not prepared yet
        dev.prepare_map_grid_tiled(plan_b, GOAL)
        same_grids(dev, want_b, GOAL, "GOAL alone")
        same_grids(dev, want_a, PATH, "PATH kept")
        dev.prepare_map_grid_tiled(plan_a, PATH)                         # a tiled PATH prepare leaves the GOAL grid's bytes
        same_grids(dev, want_b, GOAL, "GOAL kept")
        st = dev.prepare_map_grid_front_tiled(plan_a)
        got, started, goal = dev.read_map_grid_front()
        assert got.tobytes() == want_a["goal"].tobytes() and (started, goal) == (1, want_a["goal_cell"]) == (st["started"], st["goal_cell"])
        same_grids(dev, want_b, GOAL, "GOAL kept by front")
        dev.prepare_map_grid_tiled(plan_a, BOTH)
        same_grids(dev, want_a, BOTH, "both")
        dev.prepare_map_grid_tiled(plan_b, BOTH)                         # the second must not see the first's marks or values
        same_grids(dev, want_b, BOTH, "another plan")
        import inflate_ref as iref
        p = iref.Params(0.25, 0.1, 3.0, False)
        dev.inflate(p.inflation_radius, p.inscribed_radius, p.cost_scaling_factor, p.inflate_unknown)
        cm2 = ref_map(dev.read())
        assert cm2.grid.tobytes() != cm.grid.tobytes()
        dev.prepare_map_grid_tiled(plan_b, BOTH)
        same_grids(dev, ref.grids(cm2, plan_b), BOTH, "after inflate")
    finally:
        dev.close()


# ---- 7. downstream on 600 x 600 at 0.05 -------------------------------------------------------------------------------------------------
BLOCK = (slice(270, 330), slice(260, 340))                                # rows, columns of a cleared block in the middle


@functools.lru_cache(maxsize=None)
def big_case():
    n = 600
    g = noise(np.random.default_rng(601), n, n, 0.2)
    rows, cols = BLOCK
    sub = g[rows, cols]
    sub[sub >= 253] = 0
    g[rows.start + 10:rows.start + 13, cols.start + 30:cols.start + 33] = 254
    g[rows.start + 30:rows.start + 35, cols.start + 8:cols.start + 13] = 253
    g.setflags(write=False)
    cm = ref_map(g)
    plan = [centre(cm, cols.start + 2, rows.start + 2), centre(cm, 300, 300), centre(cm, cols.stop - 3, rows.stop - 3)]
    front = cref.front_plan(plan, FORWARD)
    want, want_front = ref.grids(cm, plan), ref.grids(cm, front)
    grids = {cref.GRID_PATH: want["path"], cref.GRID_GOAL: want["goal"], cref.GRID_FRONT: want_front["goal"]}
    T, nt = 7, 40
    rng = np.random.default_rng(12)
    x_lo, x_hi = cm.ox + cols.start * RES, cm.ox + cols.stop * RES
    y_lo, y_hi = cm.oy + rows.start * RES, cm.oy + rows.stop * RES
    start = np.stack([rng.uniform(x_lo, x_hi, nt), rng.uniform(y_lo, y_hi, nt)], axis=1)
    start[30:] = np.stack([rng.uniform(cm.ox - 1.0, cm.ox + n * RES + 1.0, nt - 30), rng.uniform(cm.oy - 1.0, cm.oy + n * RES + 1.0, nt - 30)], axis=1)
    start[35:] = [cm.ox - 0.5, cm.oy + 10.0]                               # five from beyond the edge: -4
    xy = start[:, None, :] + rng.uniform(-4 * RES, 4 * RES, (nt, T, 2)).cumsum(axis=1)
    xyt = np.concatenate([xy.reshape(-1, 2), rng.uniform(-np.pi, np.pi, (nt * T, 1))], axis=1)
    poses = fref.poses_from_yaw(xyt)
    ext = np.zeros((2, nt))
    ext[0] = np.where(rng.random(nt) < 0.1, -5.0, 0.0)
    ext[1] = np.abs(rng.normal(0.0, 0.5, nt))
    return {"cm": cm, "plan": plan, "front": front, "want": want, "want_front": want_front, "grids": grids, "poses": poses, "T": T, "ext": ext}


@pytest.fixture(scope="module")
def big_dev(emap):
    """the 600 x 600 map on the device, its three grids prepared by the tiled calls alone"""
    c = big_case()
    dev = device_copy(emap, c["cm"])
    dev.prepare_map_grid_tiled(c["plan"])
    dev.prepare_map_grid_front_tiled(c["front"])
    yield dev
    dev.close()


def test_downstream_scores(emap, big_dev):
    import torch
    c = big_case()
    same_grids(big_dev, c["want"], BOTH, "600 x 600 downstream")
    assert big_dev.read_map_grid_front()[0].tobytes() == c["want_front"]["goal"].tobytes()
    d_poses = torch.from_numpy(np.array(c["poses"])).to("cuda:0")
    seen = set()
    for bit, name in ((PATH, "path"), (GOAL, "goal")):
        for flags in (0, SUM, STOP, STOP | SUM):
            exp = ref.score(c["cm"], c["want"][name], c["poses"], c["T"], 0.0, flags)
            assert big_dev.score_map_grid(bit, c["poses"], c["T"], 0.0, flags).tolist() == exp.tolist(), (name, flags)
            d_got = big_dev.score_map_grid(bit, d_poses, c["T"], 0.0, flags)
            emap.synchronize()
            assert d_got.cpu().numpy().tolist() == exp.tolist(), (name, flags, "device")
            seen |= set(exp.tolist())
    assert -4 in seen and (-2 in seen or -3 in seen) and any(0 <= v < 600 * 600 for v in seen)


def test_downstream_best_trajectory(emap, big_dev):
    c = big_case()
    critics = cref.dwa_list()
    table = cref.score_table(c["cm"], c["grids"], critics, c["poses"], c["T"], SMALL, c["ext"])
    totals = cref.combine(critics, table)
    best = cref.find_best(totals)
    assert best[2] >= 3 and (rejected_by(critics, table) >= 0).any()
    i, cost, n_valid, tot = big_dev.best_trajectory(as_c(critics)[:len(critics)], c["poses"], c["T"], SMALL, c["ext"], None, totals=True)
    same_best(i, cost, n_valid, tot, totals, best, "600 x 600 best_trajectory")


def test_downstream_dwa_best(emap, big_dev):
    c = big_case()
    rows, cols = BLOCK
    config = dict(CONFIG, oscillation_flags=16, vsamples=(4, 1, 6))
    vel = (0.1, 0.0, 0.1)
    pos = (*centre(c["cm"], cols.start + 20, rows.start + 11), 0.0)       # ten cells in front of the lethal patch, heading for it
    limits = dict(LIMITS, max_vel_y=0.0, min_vel_y=0.0)
    T = tref.max_steps(limits, config, tref.lists(limits, config, pos, vel, TG_GOAL))
    poses, lens, ext, vels = tref.generate(limits, config, pos, vel, TG_GOAL, T)
    critics = cref.dwa_list()
    table = cref.score_table(c["cm"], c["grids"], critics, poses, T, SMALL, ext, lens)
    totals = cref.combine(critics, table, lens, T)
    best = cref.find_best(totals)
    assert 8 <= lens.size <= 64 and best[2] >= 1
    plan = gem_amd.trajgen_plan(limits, config, pos, vel, TG_GOAL)
    assert plan.max_steps == T and plan.n_traj == lens.size
    i, cost, n_valid, tot = big_dev.dwa_best(as_c(critics)[:len(critics)], plan, pos, vel, T, SMALL, totals=True)
    same_best(i, cost, n_valid, tot, totals, best, "600 x 600 dwa_best")


def test_downstream_rollout_best(emap, big_dev):
    c = big_case()
    rows, cols = BLOCK
    cfg = dict(TWO, vx_samples=4, vtheta_samples=6)
    pos, vel = (*centre(c["cm"], cols.start + 20, rows.start + 11), 0.3), (0.2, 0.0, 0.1)
    r = rref.evaluate_all(c["cm"], c["want"]["path"], c["want"]["goal"], cfg, pos, vel, 0, fref.RECTANGLE, 0)
    assert 8 <= r["cost"].size <= 64 and (r["cost"] >= 0).any()
    plan = gem_amd.rollout_plan(cfg, pos, vel, 0)
    assert plan.n_cand == r["cost"].size
    ans, cost, ahead = big_dev.rollout_best(plan, pos, vel, 0, fref.RECTANGLE, 0, costs=True)
    assert cost.tobytes() == r["cost"].tobytes() and ahead.tobytes() == r["ahead"].tobytes() and ans["bytes"] == r["answer"]["bytes"]


# ---- 8. errors and state ----------------------------------------------------------------------------------------------------------------
def test_stale_grids_refusals_and_no_allocation():
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    cm = ref_map(np.array(tiled_scenario("130x70", "noise")[0]))
    free = np.argwhere(cm.grid < 253)
    y0, x0 = free[len(free) // 2]
    plan = [centre(cm, int(x0), int(y0))]
    dev = device_copy(m, cm)
    nan, inf = float("nan"), float("inf")

    def prepare(id_=None, pts=plan, n=None, which=BOTH, front=False):
        v = np.ascontiguousarray(pts, np.float64).reshape(-1, 2)
        pv = v.ctypes.data_as(C.POINTER(C.c_double)) if v.size else None
        st = _lib.MapGridTiledStatus(7, (7, 7), 7, 7)
        if front:
            rc = lib.gem_costmap_mapgrid_prepare_front_tiled(h, dev.id if id_ is None else id_, pv, v.shape[0] if n is None else n, C.byref(st))
        else:
            rc = lib.gem_costmap_mapgrid_prepare_tiled(h, dev.id if id_ is None else id_, pv, v.shape[0] if n is None else n, which, C.byref(st))
        if rc != 0:
            assert (st.started, st.goal_cell[0], st.goal_cell[1], st.rounds, st.chunks) == (7, 7, 7, 7, 7)      # a refusal writes nothing
        return rc

    try:
        assert lib.gem_costmap_mapgrid_read(h, dev.id, PATH, None, None, None) == INV                 # never prepared
        assert prepare() == 0 and prepare(front=True) == 0
        want = ref.grids(cm, plan)
        same_grids(dev, want)
        for front in (False, True):
            for bad in (-1, 5, 8, 1 << 20):
                assert prepare(id_=bad, front=front) == INV
            assert prepare(pts=[], n=3, front=front) == INV and prepare(n=-1, front=front) == INV      # NULL with a count | a negative count
            for v in (nan, inf, -inf):
                assert prepare(pts=[plan[0], (v, 0.0)], front=front) == INV and prepare(pts=[(0.0, v)], front=front) == INV
            assert prepare(pts=[(0.0, 0.0), (1e5, 0.0)], front=front) == INV                          # 2 000 000 points at this resolution
        for which in (0, 4, 7, -1):
            assert prepare(which=which) == INV
        w2 = ElevationMap(32, 0.05)                                       # a handle with a communicator
        w2.comm_init_loopback(9544, 1, 0, tile_strips=False)
        v = (C.c_double * 2)(0.0, 0.0)
        assert w2._lib.gem_costmap_mapgrid_prepare_tiled(w2._h, 0, v, 1, BOTH, None) == INV
        assert w2._lib.gem_costmap_mapgrid_prepare_front_tiled(w2._h, 0, v, 1, None) == INV
        w2.close()
        same_grids(dev, want, BOTH, "after the errors")                   # every refusal left the earlier grids as they were
        assert dev.read_map_grid_front()[0].tobytes() == want["goal"].tobytes()
        assert dev.read().tobytes() == cm.grid.tobytes()
        v = np.ascontiguousarray(plan, np.float64)
        assert lib.gem_costmap_mapgrid_prepare_tiled(h, dev.id, v.ctypes.data_as(C.POINTER(C.c_double)), 1, BOTH, None) == 0     # a NULL status is fine
        same_grids(dev, want, BOTH, "a NULL status")

        a1 = m.debug_get("arena_allocations")                             # a second identical call allocates nothing
        assert prepare() == 0 and prepare(front=True) == 0
        assert m.debug_get("arena_allocations") == a1

        sizes = cm.size_in_meters()
        dev.roll_to(cm.ox + sizes[0] / 2 + 7 * RES, cm.oy + sizes[1] / 2 - 4 * RES)
        assert lib.gem_costmap_mapgrid_read(h, dev.id, PATH, None, None, None) == INV and lib.gem_costmap_mapgrid_read(h, dev.id, GOAL, None, None, None) == INV
        assert lib.gem_costmap_mapgrid_read_front(h, dev.id, None, None, None) == INV
        geo = dev.geometry()
        rolled = ref_map(dev.read(), origin=(geo["origin_x"], geo["origin_y"]))
        assert rolled.grid.tobytes() != cm.grid.tobytes()
        assert prepare(which=GOAL) == 0
        want2 = ref.grids(rolled, plan)
        same_grids(dev, want2, GOAL, "after the roll")
        assert lib.gem_costmap_mapgrid_read(h, dev.id, PATH, None, None, None) == INV                 # only the goal grid was prepared again
    finally:
        dev.close()
        m.close()


# ---- 9. the C++ facade ------------------------------------------------------------------------------------------------------------------
def build_tiled_check(out: Path) -> Path:
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc", "-std=c++17", "-O2", "-Wall", "-Werror",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "mapgrid_tiled_check.cpp"), "-o", str(out),
           f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_cpp_tiled_facade(tmp_path):
    sx, sy, res = 65, 2049, 0.05
    g = noise(np.random.default_rng(20490), sx, sy, 0.2)
    g[1000:1010, 28:38] = 0
    cm = ref_map(g, res=res, origin=(0.0, 0.0))
    plan = np.array([centre(cm, 30, 1004), centre(cm, 35, 1006)], np.float64)
    want = ref.grids(cm, plan)
    assert want["started"] == 1
    files = {"grid": g, "plan": plan, "path": want["path"], "goal": want["goal"]}
    for name, a in files.items():
        (tmp_path / name).write_bytes(np.ascontiguousarray(a).tobytes())
    exe = build_tiled_check(tmp_path / "mapgrid_tiled_check")
    out = subprocess.run([str(exe), "1", str(tmp_path / "grid"), str(sx), str(sy), repr(res), str(tmp_path / "plan"), str(tmp_path / "path"),
                          str(tmp_path / "goal")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
