"""The global plan on the device costmap (gem_costmap_navplan / _read) against tests/navplan_ref.py and the host twin.  Every comparison
is exact: potentials by tobytes(), paths and status as integers, world points as doubles.

  1. seam and edge geometries (64 x 64, 65 x 65, 130 x 90, 65 x 3, 1 x 200, 200 x 1), each empty, with 30 % noise of bytes 0 .. 255
     under the default table, with two walls at columns 63 - 64 with one gap, and with 30 % blocked noise; a start in each corner tile,
     the outline on and off;
  2. a one-cell serpentine on 130 x 130 with nav_chunk 4: many rounds, and status.chunks > 1 says the second chunk was taken;
  3. a cheap corridor that leaves a tile and re-enters it: a tile's edge improves twice;
  4. the start on a lethal byte, the goal on one, a goal walled in, start = goal, start and goal off the map;
  5. 1000 x 1000 (the reference's global costmap) with 20 % noise against the host twin, which test_navplan_cpu.py pins to the Python
     statement at the sizes of 1.;
  6. the chain: a 200 x 200 global map is marked and inflated, nav_plan runs, its world path goes to prepare_map_grid on a 75 x 75
     local costmap, and both grids equal mapgrid_ref fed the reference's path;
  7. no allocation in a second identical call;
  8. a stale read after roll_to and the other error cases, the potential unchanged afterwards;
  9. the C++ facade (tests/cpp/navplan_check.cpp) as a child process."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import gem_amd
from gem_amd import ElevationMap, _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import costmap_ref as cref  # noqa: E402
import inflate_ref as iref  # noqa: E402
import mapgrid_ref as mref  # noqa: E402
import navplan_ref as ref  # noqa: E402
from test_costmap_gpu import lattice_cloud  # noqa: E402
from test_navplan_cpu import (GEOMETRIES, KINDS, build_navplan_check, default_weights, expected, scenario, seam_corridor, serpentine,  # noqa: E402
                              special_cases)

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
    """one nav_plan on the device against a reference plan; returns the status"""
    sx = dev.size_x
    path, st = dev.nav_plan(centre(start), centre(goal), weights, outline=bool(flags & ref.OUTLINE))
    pot, cells = dev.read_potential()
    assert pot.dtype == np.int32 and pot.tobytes() == want["pot"].tobytes(), f"{what}: {int((pot != want['pot']).sum())} potentials differ"
    assert (st["found"], st["n_path"], st["goal_potential"]) == (want["found"], want["n_path"], want["goal_potential"]), (what, st)
    assert (st["start_cell"], st["goal_cell"]) == (want["start_cell"], want["goal_cell"]), (what, st)
    assert cells.tolist() == np.asarray(want["cells"]).tolist(), what
    assert path.tobytes() == ref.centres(want["cells"], sx, RES, *ORIGIN).tobytes(), what
    assert st["chunks"] >= 1 and st["rounds"] >= (1 if want["start_cell"] != (-1, -1) else 0), (what, st)
    return st


# ---- 1. geometries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_geometries(emap, geom, kind):
    g = scenario(geom, kind)
    dev = device_copy(emap, g)
    try:
        for start, goal, flags, want in expected(geom, kind):
            same_plan(dev, want, start, goal, flags, f"{geom} {kind} {start} -> {goal} flags {flags}")
        assert dev.read().tobytes() == g.tobytes()                        # the outline is not written into the costmap
    finally:
        dev.close()


# ---- 2. many rounds, the second chunk -------------------------------------------------------------------------------------------------
def test_serpentine_takes_the_second_chunk(emap):
    g = serpentine()
    want = ref.plan(g, default_weights(), 0, (0, 0), (0, 128))
    assert want["found"] == 1 and want["n_path"] > 60 * 130
    dev = device_copy(emap, g)
    try:
        emap.debug_set("nav_chunk", 4)
        st = same_plan(dev, want, (0, 0), (0, 128), 0, "serpentine, chunks of 4")
        assert st["chunks"] > 1 and st["rounds"] > 4, st                  # the host's loop was taken
        emap.debug_set("nav_chunk", 0)
        st = same_plan(dev, want, (0, 0), (0, 128), 0, "serpentine, the default chunk")
        assert st["chunks"] > 1, st                                       # 3 + 3 rounds a chunk are not enough either
    finally:
        emap.debug_set("nav_chunk", 0)
        dev.close()


# ---- 3. an edge that improves twice ---------------------------------------------------------------------------------------------------
def test_corridor_across_a_seam_and_back(emap):
    g = seam_corridor()
    want = ref.plan(g, default_weights(), 0, (40, 5), (30, 49))
    assert {int(c) % 100 for c in want["cells"]} >= {63, 64, 89}
    dev = device_copy(emap, g)
    try:
        for chunk in (1, 0):
            emap.debug_set("nav_chunk", chunk)
            st = same_plan(dev, want, (40, 5), (30, 49), 0, f"corridor, nav_chunk {chunk}")
            assert st["rounds"] >= 3, st                                  # left tile, right tile, left tile again
        want = ref.plan(g, default_weights(), ref.OUTLINE, (30, 49), (40, 5))
        same_plan(dev, want, (30, 49), (40, 5), ref.OUTLINE, "corridor, reversed")
    finally:
        emap.debug_set("nav_chunk", 0)
        dev.close()


# ---- 4. found, the path length, the potential ---------------------------------------------------------------------------------------
def test_special_starts_and_goals(emap):
    dev = None
    try:
        for name, g, start, goal, flags in special_cases():
            if dev is None:
                dev = device_copy(emap, g)
            want = ref.plan(g, default_weights(), flags, start, goal)
            same_plan(dev, want, start, goal, flags, name)
    finally:
        if dev is not None:
            dev.close()


# ---- 5. the reference's global costmap --------------------------------------------------------------------------------------------------
def test_1000_x_1000_equals_the_host_twin(emap):
    rng = np.random.default_rng(1000)
    g = np.zeros((1000, 1000), np.uint8)
    hit = rng.random(g.shape) < 0.2
    g[hit] = rng.integers(0, 256, int(hit.sum()), dtype=np.uint8)
    start, goal = (3, 4), (995, 990)
    g[start[1], start[0]] = 0
    g[goal[1], goal[0]] = 0
    pot, cells, hst = gem_amd.nav_plan_host(g, start, goal)
    assert hst["found"] == 1 and hst["n_path"] >= 990
    want = {"pot": pot, "cells": cells, "found": 1, "n_path": hst["n_path"], "goal_potential": hst["goal_potential"], "start_cell": start,
            "goal_cell": goal}
    dev = device_copy(emap, g)
    try:
        st = same_plan(dev, want, start, goal, ref.OUTLINE, "1000 x 1000")
        assert st["rounds"] >= 16                                         # sixteen tiles from the start's to the goal's
    finally:
        dev.close()


# ---- 6. the chain into the local planner's grids --------------------------------------------------------------------------------------
def test_global_plan_feeds_the_local_map_grid(emap):
    res, origin = 0.2, (-20.0, -20.0)
    rng = np.random.default_rng(6)
    p = iref.Params(1.0, 0.4, 3.0, False)                                # R = 5
    gref = cref.Costmap(200, 200, res, *origin, cref.FREE_SPACE)
    pts = lattice_cloud(rng, 4000, gref)
    cref.mark_points(gref, pts, 0.5)
    gref.grid[:] = iref.inflate_exact(gref.grid, p, res, None)
    assert (gref.grid == 254).any() and ((gref.grid > 0) & (gref.grid < 253)).any()
    start, goal = (60, 70), (150, 140)                                   # across the marked patch in the map's middle
    want = ref.plan(gref.grid, default_weights(), ref.OUTLINE, start, goal)
    assert want["found"] == 1
    want_xy = ref.centres(want["cells"], 200, res, *origin)
    lorigin = (origin[0] + (start[0] + 0.5) * res - 7.5, origin[1] + (start[1] + 0.5) * res - 7.5)
    lref = cref.Costmap(75, 75, res, *lorigin, cref.FREE_SPACE)
    lref.grid[:] = np.where(rng.random((75, 75)) < 0.08, 254, 0).astype(np.uint8)
    lref.grid[35:40, 35:40] = 0                                          # the robot's own cells are free
    want_grids = mref.grids(lref, [tuple(v) for v in want_xy.tolist()])
    assert want_grids["started"] == 1

    glob = emap.costmap(200, 200, res, *origin, cref.FREE_SPACE)
    local = emap.costmap(75, 75, res, *lorigin, cref.FREE_SPACE)
    try:
        glob.mark_points(pts, 0.5, None)
        glob.inflate(p.inflation_radius, p.inscribed_radius, p.cost_scaling_factor, p.inflate_unknown)
        local.write(lref.grid)
        path, st = glob.nav_plan(centre(start, res, origin), centre(goal, res, origin))
        assert glob.read().tobytes() == gref.grid.tobytes()
        assert st["found"] == 1 and path.tobytes() == want_xy.tobytes()
        local.prepare_map_grid(path)
        for bit, name in ((_lib.MAPGRID_PATH, "path"), (_lib.MAPGRID_GOAL, "goal")):
            got, started, gcell = local.read_map_grid(bit)
            assert (started, gcell) == (want_grids["started"], want_grids["goal_cell"]), name
            assert got.tobytes() == want_grids[name].tobytes(), name
    finally:
        glob.close(); local.close()


# ---- 7. nothing is allocated the second time ------------------------------------------------------------------------------------------
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


# ---- 8. stale plans and errors ---------------------------------------------------------------------------------------------------------
def test_stale_after_a_roll_and_the_error_cases():
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    g = scenario("65x65", "noise")
    start, goal, flags, want = expected("65x65", "noise")[0]
    dev = device_copy(m, g)
    w = np.array(default_weights(), np.int32)
    wp = w.ctypes.data_as(C.POINTER(C.c_int))
    nan, inf = float("nan"), float("inf")

    def plan(id_=None, s=centre(start), e=centre(goal), wt=wp, fl=flags, st=True):
        status = _lib.NavplanStatus()
        status.n_path = -77
        rc = lib.gem_costmap_navplan(h, dev.id if id_ is None else id_, (C.c_double * 2)(*s) if s else None, (C.c_double * 2)(*e) if e else None,
                                     wt, fl, None, 0, C.byref(status) if st else None)
        return rc, status

    def read(id_=None):
        return lib.gem_costmap_navplan_read(h, dev.id if id_ is None else id_, None, None, 0)

    def unchanged(what):
        pot = np.zeros((65, 65), np.int32)
        cells = np.zeros(want["n_path"], np.int32)
        assert lib.gem_costmap_navplan_read(h, dev.id, pot.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p), cells.size) == 0, what
        assert pot.tobytes() == want["pot"].tobytes() and cells.tolist() == want["cells"].tolist(), what

    def last_status(id_=None):
        status = _lib.NavplanStatus()
        status.n_path = -77
        return lib.gem_costmap_navplan_status(h, dev.id if id_ is None else id_, C.byref(status)), status

    try:
        assert read() == INV and last_status()[0] == INV                       # no plan yet
        rc, st = plan()
        assert rc == 0 and st.n_path == want["n_path"] and st.found == 1
        unchanged("the first plan")
        # the plan was made through the C entry, not through this Python object: its status and its path are the costmap's
        rc, st2 = last_status()
        assert rc == 0 and bytes(st2) == bytes(st) and lib.gem_costmap_navplan_status(h, dev.id, None) == INV
        assert dev.nav_status()["n_path"] == want["n_path"]
        pot, cells = dev.read_potential()
        assert pot.tobytes() == want["pot"].tobytes() and cells.tolist() == want["cells"].tolist()
        assert last_status(id_=5)[0] == INV and last_status(id_=-1)[0] == INV
        for bad in (-1, 5, 8, 1 << 20):
            assert plan(id_=bad)[0] == INV and read(id_=bad) == INV
        for fl in (2, 3, 4, -1):
            rc, st = plan(fl=fl)
            assert rc == INV and st.n_path == -77
        assert plan(wt=None)[0] == INV and plan(s=None)[0] == INV and plan(e=None)[0] == INV and plan(st=False)[0] == INV
        neg = w.copy(); neg[3] = -1
        assert plan(wt=neg.ctypes.data_as(C.POINTER(C.c_int)))[0] == INV
        big = w.copy(); big[200] = -(-(2 ** 31 - 1) // (65 * 65))          # 65 * 65 * max(w) >= 2^31 - 1
        assert plan(wt=big.ctypes.data_as(C.POINTER(C.c_int)))[0] == INV
        for v in (nan, inf, -inf):
            assert plan(s=(v, 3.0))[0] == INV and plan(s=(0.0, v))[0] == INV and plan(e=(v, 3.0))[0] == INV and plan(e=(0.0, v))[0] == INV
        w2 = ElevationMap(32, 0.05)                                       # a handle with a communicator
        w2.comm_init_loopback(9544, 1, 0, tile_strips=False)
        status = _lib.NavplanStatus()
        s2, e2 = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(1.0, 1.0)
        assert w2._lib.gem_costmap_navplan(w2._h, 0, s2, e2, wp, 0, None, 0, C.byref(status)) == INV
        assert w2._lib.gem_costmap_navplan_read(w2._h, 0, None, None, 0) == INV
        assert w2._lib.gem_costmap_navplan_status(w2._h, 0, C.byref(status)) == INV
        w2.close()
        unchanged("after the errors")
        assert dev.read().tobytes() == g.tobytes()
        cells = np.zeros(3, np.int32)                                     # a read into too few cells
        assert lib.gem_costmap_navplan_read(h, dev.id, None, cells.ctypes.data_as(C.c_void_p), 3) == INV and not cells.any()

        # out_xy too short: an error, the first cap points written and the status filled
        status = _lib.NavplanStatus()
        xy = np.full((4, 2), -1.0)
        rc = lib.gem_costmap_navplan(h, dev.id, (C.c_double * 2)(*centre(start)), (C.c_double * 2)(*centre(goal)), wp, flags,
                                     xy.ctypes.data_as(C.c_void_p), 4, C.byref(status))
        assert rc == INV and status.n_path == want["n_path"] and status.found == 1
        assert xy.tobytes() == ref.centres(want["cells"][:4], 65, RES, *ORIGIN).tobytes()
        unchanged("after the short call")

        # a roll that moves nothing keeps the plan; one that moves the map makes it stale until the next plan
        dev.update_origin(ORIGIN[0] + 0.3 * RES, ORIGIN[1])
        unchanged("a roll by less than a cell")
        dev.roll_to(ORIGIN[0] + 65 * RES / 2 + 7 * RES, ORIGIN[1] + 65 * RES / 2 - 4 * RES)
        assert read() == INV and last_status()[0] == INV
        geo = dev.geometry()
        rolled = dev.read()
        assert rolled.tobytes() != g.tobytes()
        o2 = (geo["origin_x"], geo["origin_y"])
        want2 = ref.plan(rolled, default_weights(), 0, (5, 6), (50, 40))
        path, st2 = dev.nav_plan(centre((5, 6), RES, o2), centre((50, 40), RES, o2), None, outline=False)
        pot, cells = dev.read_potential()
        assert pot.tobytes() == want2["pot"].tobytes() and cells.tolist() == want2["cells"].tolist()
        assert path.tobytes() == ref.centres(want2["cells"], 65, RES, *o2).tobytes()
        dev.close()
        dev = device_copy(m, g)                                          # the same id, created anew: no plan
        assert read() == INV
    finally:
        dev.close()
        m.close()


# ---- 9. the C++ facade ------------------------------------------------------------------------------------------------------------------
def test_cpp_navplan_facade(tmp_path):
    exe = build_navplan_check(tmp_path / "navplan_check")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
