"""Frontier search on the device costmap (gem_costmap_frontiers / _read, gem_costmap_navplan_goal) against tests/frontier_ref.py, the
host twin and navplan_ref.  Every comparison is exact: labels by tobytes(), records as the struct's bytes (the cost as a double's
bytes among them), status as integers.

  1. seam and edge geometries (64 x 64, 65 x 65, 130 x 90, 65 x 3, 1 x 200, 200 x 1), each with a known disc around the start, with
     noise, all known and all unknown but the start; the start in each corner tile, planned with allow_unknown = 0;
  2. a frontier whose only link is the diagonal across the point where four tiles meet, and one on the anti-diagonal;
  3. a one-cell serpentine on 130 x 130 with front_chunk 4 and with the default chunk: many rounds;
  4. a frontier whose smallest cell lies in the top-left tile and whose mass lies in the bottom-right one;
  5. the pick: the tie, min_frontier_size, each scale alone, a scale pair for which the winner changes;
  6. 1000 x 1000 (the reference's global costmap), a ragged known region with 20 % noise, against the host twin, which
     test_frontier_cpu.py pins to the Python statement at the sizes of 1.;
  7. the chain: mark, inflate, nav_plan(robot, robot), frontiers, nav_plan_to(the winner's access cell);
  8. nav_plan_to alone against navplan_ref for the goals of test_navplan_cpu.special_cases();
  9. no allocation in a second identical call;
 10. stale searches and the error cases, the last search and the potential unchanged afterwards;
 11. the C++ facade (tests/cpp/frontier_check.cpp) as a child process."""
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
import frontier_ref as fref  # noqa: E402
import inflate_ref as iref  # noqa: E402
import navplan_ref as nref  # noqa: E402
from test_costmap_gpu import lattice_cloud  # noqa: E402
from test_frontier_cpu import (PICK_PARAMS, RES, SCENES, build_frontier_check, check_pick_winners, climbing_expected, diagonal_scene, expected, far_root_scene,  # noqa: E402
                               frontier_struct, pick_scene, potential, ragged_scene, serpentine_scene, weights_known_only)
from test_navplan_cpu import GEOMETRIES, default_weights, special_cases  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
ORIGIN = (-3.1, 2.7)
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
    return (origin[0] + (cell[0] + 0.5) * res, origin[1] + (cell[1] + 0.5) * res)


def plan_from(dev, start, outline=False):
    """the plan a search works from: start = goal, allow_unknown = 0"""
    return dev.nav_plan(centre(start), centre(start), weights_known_only(), outline=outline)


def raw_search(m, dev, params=(0.0, 1.0, 1.0)):
    st = _lib.FrontierStatus()
    prm = _lib.FrontierParams(*params)
    rc = m._lib.gem_costmap_frontiers(m._h, dev.id, C.byref(prm), C.byref(st))
    return rc, st


def raw_read(m, dev, n_kept):
    lab = np.full((dev.size_y, dev.size_x), -5, np.int32)
    rec = (_lib.Frontier * max(n_kept, 1))()
    rc = m._lib.gem_costmap_frontiers_read(m._h, dev.id, rec, n_kept, lab.ctypes.data_as(C.c_void_p))
    return rc, rec, lab


def same_search(m, dev, want, params, what):
    """one search on the device against a reference search (a dict of fref.search's form); returns the status"""
    rc, st = raw_search(m, dev, params)
    assert rc == 0, what
    print(what, "n_cells", st.n_cells, "n_frontiers", st.n_frontiers, "n_kept", st.n_kept, "best", st.best, "rounds", st.rounds, "chunks", st.chunks)
    assert (st.n_cells, st.n_frontiers, st.n_kept, st.best) == (want["n_cells"], want["n_frontiers"], want["n_kept"], want["best"]), what
    if want["best"] >= 0:
        assert bytes(st.best_frontier) == bytes(frontier_struct(want["best_frontier"])), what
    else:
        assert st.best_frontier.root == -1 and st.best_frontier.size == 0 and st.best_frontier.cost == 0.0, what
    rc, rec, lab = raw_read(m, dev, st.n_kept)
    assert rc == 0, what
    assert lab.tobytes() == want["labels"].tobytes(), f"{what}: {int((lab != want['labels']).sum())} labels differ"
    for i, r in enumerate(want["kept"]):
        assert bytes(rec[i]) == bytes(frontier_struct(r)), (what, i, r)
    assert st.chunks >= 1 and st.rounds >= (1 if want["n_cells"] else 0), (what, st.rounds, st.chunks)
    return st


# ---- 1. geometries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SCENES)
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_geometries(emap, geom, kind):
    dev = None
    try:
        for corner in range(4):
            g, start, pot, want = expected(geom, kind, corner)
            if dev is None:
                dev = device_copy(emap, g)
            else:
                dev.write(g)
            plan_from(dev, start)
            same_search(emap, dev, want, (0.0, 1.0, 1.0), f"{geom} {kind} corner {corner}")
            assert dev.read().tobytes() == g.tobytes() and dev.read_potential()[0].tobytes() == pot.tobytes()
    finally:
        if dev is not None:
            dev.close()


# ---- 2. the four-tile corner ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("anti", [False, True])
def test_link_across_the_corner_of_four_tiles(emap, anti):
    g, start = diagonal_scene(anti)
    pot = potential(g, start)
    want = fref.search(g, pot, RES)
    four = fref.labels_flood(want["mask"], fref.N4)
    assert want["n_frontiers"] == 1 and len(np.unique(four[want["mask"]])) == 2      # 4-connectivity would not pass
    dev = device_copy(emap, g)
    try:
        plan_from(dev, start)
        same_search(emap, dev, want, (0.0, 1.0, 1.0), f"diagonal, anti {anti}")
    finally:
        dev.close()


@pytest.mark.parametrize("left", [False, True])
def test_label_climbs_through_a_tile_corner(emap, left):
    """a lower tile's top-right (`left`: top-left) corner cell changes and nothing else that faces the tile above it diagonally: that
    tile is reached by the corner mark alone, upwards"""
    g, start, _pot, want = climbing_expected(left)
    dev = device_copy(emap, g)
    try:
        plan_from(dev, start)
        same_search(emap, dev, want, (0.0, 1.0, 1.0), f"climbing, left {left}")
    finally:
        dev.close()


# ---- 3. many rounds, the second chunk -------------------------------------------------------------------------------------------------
def test_serpentine_takes_the_second_chunk(emap):
    g, start = serpentine_scene()
    want = fref.search(g, potential(g, start), RES)
    assert want["n_frontiers"] == 1 and want["all"][0]["size"] > 60 * 128
    dev = device_copy(emap, g)
    try:
        plan_from(dev, start)
        emap.debug_set("front_chunk", 4)
        st = same_search(emap, dev, want, (0.0, 1.0, 1.0), "serpentine, chunks of 4")
        assert st.chunks > 1 and st.rounds > 4, (st.chunks, st.rounds)    # the host's loop was taken
        emap.debug_set("front_chunk", 0)
        st = same_search(emap, dev, want, (0.0, 1.0, 1.0), "serpentine, the default chunk")
        assert st.chunks > 1, (st.chunks, st.rounds)                      # 3 + 3 rounds a chunk are not enough either
    finally:
        emap.debug_set("front_chunk", 0)
        dev.close()


# ---- 4. a root far from the bulk --------------------------------------------------------------------------------------------------------
def test_root_far_from_the_bulk(emap):
    g, start = far_root_scene()
    want = fref.search(g, potential(g, start), RES)
    assert want["n_frontiers"] == 1 and want["all"][0]["root"] == 5 * 130 + 5
    dev = device_copy(emap, g)
    try:
        plan_from(dev, start)
        st = same_search(emap, dev, want, (0.0, 1.0, 1.0), "far root")
        assert st.rounds >= 3                                            # the label crosses two seams against the scan direction
    finally:
        dev.close()


# ---- 5. the pick -----------------------------------------------------------------------------------------------------------------------
def test_the_pick(emap):
    g, start = pick_scene()
    pot = potential(g, start)
    dev = device_copy(emap, g)
    try:
        plan_from(dev, start)
        winners = {}
        for params in PICK_PARAMS:
            want = fref.search(g, pot, RES, *params)
            st = same_search(emap, dev, want, params, f"pick {params}")
            winners[params] = st.best_frontier.root if st.best >= 0 else None
        check_pick_winners(winners)
        # the Python facade: the same winner, its centroid, the kept list
        want = fref.search(g, pot, RES, 0.7, 1.0, 0.0)
        st = dev.frontiers(0.7, 1.0, 0.0)
        assert st["best"] == want["best"] and st["n_kept"] == 3
        assert {k: st["best_frontier"][k] for k in want["best_frontier"]} == want["best_frontier"]
        assert st["best_frontier"]["centroid"] == fref.centroid(want["best_frontier"], RES, *ORIGIN)
        kept, labels = dev.read_frontiers()
        assert labels.tobytes() == want["labels"].tobytes() and [{k: f[k] for k in r} for f, r in zip(kept, want["kept"])] == want["kept"]
        assert len(kept) == 3 and kept[2]["centroid"] == fref.centroid(want["kept"][2], RES, *ORIGIN)
    finally:
        dev.close()


# ---- 6. the reference's global costmap --------------------------------------------------------------------------------------------------
def test_1000_x_1000_equals_the_host_twin(emap):
    g, start = ragged_scene()
    pot = potential(g, start, outline=True)
    params = (1.0, 0.001, 2.0)
    kept, labels, hst = gem_amd.frontiers_host(g, pot, RES, *params)
    assert hst["n_frontiers"] > 100 and hst["n_cells"] > 2000 and 0 < hst["n_kept"] < hst["n_frontiers"]
    keys = ("root", "size", "sum_x", "sum_y", "access_potential", "access_cell", "cost")
    want = {"labels": labels, "kept": [{k: f[k] for k in keys} for f in kept], "n_cells": hst["n_cells"], "n_frontiers": hst["n_frontiers"],
            "n_kept": hst["n_kept"], "best": hst["best"], "best_frontier": {k: hst["best_frontier"][k] for k in keys}}
    dev = device_copy(emap, g)
    try:
        plan_from(dev, start, outline=True)
        same_search(emap, dev, want, params, "1000 x 1000")
    finally:
        dev.close()


# ---- 7. the chain ------------------------------------------------------------------------------------------------------------------------
def test_chain_mark_inflate_plan_search_and_on_to_the_winner(emap):
    res, origin = 0.2, (-20.0, -20.0)
    rng = np.random.default_rng(7)
    p = iref.Params(1.0, 0.4, 3.0, False)
    gref = cref.Costmap(200, 200, res, *origin, cref.FREE_SPACE)
    yy, xx = np.mgrid[0:200, 0:200]
    ang = np.arctan2(yy - 100, xx - 100)
    gref.grid[(xx - 100) ** 2 + (yy - 100) ** 2 > (70 + 12 * np.sin(6 * ang)) ** 2] = 255
    start_grid = gref.grid.copy()
    pts = lattice_cloud(rng, 4000, gref)
    cref.mark_points(gref, pts, 0.5)
    gref.grid[:] = iref.inflate_exact(gref.grid, p, res, None)
    robot = (60, 70)
    w = weights_known_only()
    plan0 = nref.plan(gref.grid, w, nref.OUTLINE, robot, robot)
    want = fref.search(gref.grid, plan0["pot"], res, 1.0, 0.001, 1.0)
    assert want["best"] >= 0 and want["n_frontiers"] >= 1
    ac = want["best_frontier"]["access_cell"]
    goal = (ac % 200, ac // 200)
    want_plan = nref.plan(gref.grid, w, nref.OUTLINE, robot, goal)
    assert want_plan["found"] == 1 and want_plan["goal_potential"] == want["best_frontier"]["access_potential"]

    glob = emap.costmap(200, 200, res, *origin, cref.FREE_SPACE)
    try:
        glob.write(start_grid)
        glob.mark_points(pts, 0.5, None)
        glob.inflate(p.inflation_radius, p.inscribed_radius, p.cost_scaling_factor, p.inflate_unknown)
        _path, st0 = glob.nav_plan(centre(robot, res, origin), centre(robot, res, origin), w)
        pot0 = glob.read_potential()[0]
        assert pot0.tobytes() == plan0["pot"].tobytes()
        st = same_search(emap, glob, want, (1.0, 0.001, 1.0), "chain")
        assert st.best_frontier.access_cell == ac
        path, pst = glob.nav_plan_to(centre(goal, res, origin))
        assert glob.read().tobytes() == gref.grid.tobytes()
        assert (pst["found"], pst["n_path"], pst["goal_potential"]) == (1, want_plan["n_path"], want_plan["goal_potential"])
        assert (pst["start_cell"], pst["goal_cell"], pst["chunks"], pst["rounds"]) == (robot, goal, 1, st0["rounds"])
        assert path.tobytes() == nref.centres(want_plan["cells"], 200, res, *origin).tobytes()
        pot, cells = glob.read_potential()
        assert pot.tobytes() == pot0.tobytes() == want_plan["pot"].tobytes() and cells.tolist() == want_plan["cells"].tolist()
        rc, rec, lab = raw_read(emap, glob, st.n_kept)                   # the potential is unchanged: the search stands
        assert rc == 0 and lab.tobytes() == want["labels"].tobytes()
    finally:
        glob.close()


# ---- 8. another goal on the last plan's potential ---------------------------------------------------------------------------------------
def test_navplan_goal_equals_a_plan_to_that_goal(emap):
    cases = special_cases()
    g = cases[0][1]
    dev = device_copy(emap, g)
    lib, h = emap._lib, emap._h
    try:
        for start, flags in sorted({(c[2], c[4]) for c in cases}):
            _p, st0 = dev.nav_plan(centre(start), centre(start), None, outline=bool(flags & nref.OUTLINE))
            pot0 = dev.read_potential()[0]
            for name, _g, s, goal, fl in cases:
                if (s, fl) != (start, flags):
                    continue
                want = nref.plan(g, default_weights(), flags, start, goal)
                path, st = dev.nav_plan_to(centre(goal))
                assert (st["found"], st["n_path"], st["goal_potential"]) == (want["found"], want["n_path"], want["goal_potential"]), (name, st)
                assert (st["start_cell"], st["goal_cell"]) == (want["start_cell"], want["goal_cell"]), (name, st)
                assert (st["rounds"], st["chunks"]) == (st0["rounds"], 1), (name, st)
                assert path.tobytes() == nref.centres(want["cells"], dev.size_x, RES, *ORIGIN).tobytes(), name
                pot, cells = dev.read_potential()
                assert pot.tobytes() == pot0.tobytes() == want["pot"].tobytes() and cells.tolist() == want["cells"].tolist(), name
                assert dev.nav_status() == st, name
        # a short out_xy: an error, the first cap points written and the status filled
        start, goal = (1, 1), (9, 7)
        dev.nav_plan(centre(start), centre(start), None, outline=False)
        want = nref.plan(g, default_weights(), 0, start, goal)
        assert want["n_path"] > 4
        status = _lib.NavplanStatus()
        xy = np.full((4, 2), -1.0)
        rc = lib.gem_costmap_navplan_goal(h, dev.id, (C.c_double * 2)(*centre(goal)), xy.ctypes.data_as(C.c_void_p), 4, C.byref(status))
        assert rc == INV and status.n_path == want["n_path"] and status.found == 1
        assert xy.tobytes() == nref.centres(want["cells"][:4], dev.size_x, RES, *ORIGIN).tobytes()
        assert dev.read_potential()[1].tolist() == want["cells"].tolist()
        # errors: nothing changed
        for bad in (float("nan"), float("inf")):
            assert lib.gem_costmap_navplan_goal(h, dev.id, (C.c_double * 2)(bad, 3.0), None, 0, C.byref(status)) == INV
        assert lib.gem_costmap_navplan_goal(h, dev.id, None, None, 0, C.byref(status)) == INV
        assert lib.gem_costmap_navplan_goal(h, dev.id, (C.c_double * 2)(*centre(goal)), None, 0, None) == INV
        assert lib.gem_costmap_navplan_goal(h, 5, (C.c_double * 2)(*centre(goal)), None, 0, C.byref(status)) == INV
        assert lib.gem_costmap_navplan_goal(h, dev.id, (C.c_double * 2)(*centre(goal)), xy.ctypes.data_as(C.c_void_p), -1, C.byref(status)) == INV
        assert dev.read_potential()[1].tolist() == want["cells"].tolist()
        dev.close()
        dev = device_copy(emap, g)                                       # created anew: no plan to walk on
        assert lib.gem_costmap_navplan_goal(h, dev.id, (C.c_double * 2)(*centre(goal)), None, 0, C.byref(status)) == INV
    finally:
        dev.close()


# ---- 9. nothing is allocated the second time ------------------------------------------------------------------------------------------
def test_second_identical_call_allocates_nothing(emap):
    g, start, pot, want = expected("130x90", "noise", 0)
    dev = device_copy(emap, g)
    try:
        plan_from(dev, start)
        same_search(emap, dev, want, (0.0, 1.0, 1.0), "first")
        a1 = emap.debug_get("arena_allocations")
        for k in range(2):
            same_search(emap, dev, want, (0.0, 1.0, 1.0), f"again {k}")
            dev.nav_plan_to(centre(start))
        assert emap.debug_get("arena_allocations") == a1
    finally:
        dev.close()


# ---- 10. stale searches and errors -------------------------------------------------------------------------------------------------------
def test_stale_searches_and_the_error_cases():
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    g, start, pot, want = expected("65x65", "noise", 1)
    assert want["n_kept"] > 100
    dev = device_copy(m, g)
    nan, inf = float("nan"), float("inf")

    def unchanged(what):
        rc, rec, lab = raw_read(m, dev, want["n_kept"])
        assert rc == 0 and lab.tobytes() == want["labels"].tobytes(), what
        for i, r in enumerate(want["kept"]):
            assert bytes(rec[i]) == bytes(frontier_struct(r)), (what, i)
        assert dev.read_potential()[0].tobytes() == pot.tobytes(), what

    try:
        assert raw_search(m, dev)[0] == INV and raw_read(m, dev, 0)[0] == INV      # no plan yet
        plan_from(dev, start)
        assert raw_read(m, dev, 0)[0] == INV                             # a read before any search
        same_search(m, dev, want, (0.0, 1.0, 1.0), "the first search")
        unchanged("the first search")
        prm, st = _lib.FrontierParams(0.0, 1.0, 1.0), _lib.FrontierStatus()
        st.n_kept = -77
        for bad in (-1, 5, 8, 1 << 20):
            assert lib.gem_costmap_frontiers(h, bad, C.byref(prm), C.byref(st)) == INV and st.n_kept == -77
            assert lib.gem_costmap_frontiers_read(h, bad, None, 0, None) == INV
        assert lib.gem_costmap_frontiers(h, dev.id, None, C.byref(st)) == INV and lib.gem_costmap_frontiers(h, dev.id, C.byref(prm), None) == INV
        for bad in (nan, inf, -inf, -1.0, 1.1e100):
            for k in range(3):
                v = [0.0, 1.0, 1.0]
                v[k] = bad
                rc, st2 = raw_search(m, dev, tuple(v))
                assert rc == INV, (bad, k)
        w2 = ElevationMap(32, 0.05)                                       # a handle with a communicator
        w2.comm_init_loopback(9546, 1, 0, tile_strips=False)
        assert w2._lib.gem_costmap_frontiers(w2._h, 0, C.byref(prm), C.byref(st)) == INV
        assert w2._lib.gem_costmap_frontiers_read(w2._h, 0, None, 0, None) == INV
        assert w2._lib.gem_costmap_navplan_goal(w2._h, 0, (C.c_double * 2)(0.0, 0.0), None, 0, C.byref(_lib.NavplanStatus())) == INV
        w2.close()
        rec = (_lib.Frontier * 1)()                                      # a read into too few records
        assert lib.gem_costmap_frontiers_read(h, dev.id, rec, 1, None) == INV and rec[0].size == 0
        unchanged("after the errors")
        assert dev.read().tobytes() == g.tobytes()

        # another goal keeps the search; a new plan makes it stale; a roll makes plan and search stale
        dev.nav_plan_to(centre((30, 30)))
        unchanged("after nav_plan_to")
        plan_from(dev, start)
        assert raw_read(m, dev, 0)[0] == INV
        same_search(m, dev, want, (0.0, 1.0, 1.0), "searched again")
        dev.update_origin(ORIGIN[0] + 0.3 * RES, ORIGIN[1])
        unchanged("a roll by less than a cell")
        dev.roll_to(ORIGIN[0] + 65 * RES / 2 + 7 * RES, ORIGIN[1] + 65 * RES / 2 - 4 * RES)
        assert raw_read(m, dev, 0)[0] == INV and raw_search(m, dev)[0] == INV
        geo = dev.geometry()
        rolled = dev.read()
        o2 = (geo["origin_x"], geo["origin_y"])
        dev.nav_plan(centre((5, 6), RES, o2), centre((5, 6), RES, o2), weights_known_only(), outline=False)
        pot2 = dev.read_potential()[0]
        want2 = fref.search(rolled, pot2, RES)
        assert want2["n_cells"] > 0
        same_search(m, dev, want2, (0.0, 1.0, 1.0), "after the roll")
        dev.close()
        dev = device_copy(m, g)                                          # the same id, created anew: no search
        assert raw_read(m, dev, 0)[0] == INV
    finally:
        dev.close()
        m.close()


# ---- 11. the C++ facade -------------------------------------------------------------------------------------------------------------------
def test_cpp_frontier_facade(tmp_path):
    exe = build_frontier_check(tmp_path / "frontier_check")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
