"""The best trajectory on the device costmap (gem_costmap_best_trajectory / _device, the FRONT grid) against tests/critics_ref.py.
Every comparison is exact: totals by tobytes(), the winner's index and the valid count as integers, its cost by its bytes.

  1. parity on 75 x 75 and 130 x 90 with 30 % blocked noise: DWA's seven critics in order, the same with SUM aggregates and the centre
     cost, a single critic of each kind, a zero scale in the middle; host and device forms;
  2. group widths and lengths: poses_per_traj 1 .. 65, 0 .. 31 vertices, 0 .. 65 trajectories, lengths random / all T / all 1, and in
     device memory the lengths 0 and T + 1 (-5.0);
  3. 70 000 trajectories of one pose (more than one stride of the grid), the winner planted at 69 999 and 12 345; then all rejected;
  4. ties inside a wave, across the waves of a workgroup and across workgroups;
  5. the FRONT grid against the goal grid of the shifted plan, PATH and GOAL untouched, which = 4 still refused by the old calls;
  6. the enqueued cycle with no host wait before the answer, and no allocation in a second identical loop;
  7. stale grids and every refusal, with the outputs untouched;
  8. the C++ facade (tests/cpp/critics_check.cpp) as a child process."""
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
import critics_ref as ref  # noqa: E402
import footprint_ref as fref  # noqa: E402
import inflate_ref as iref  # noqa: E402
import mapgrid_ref as mref  # noqa: E402
from test_costmap_gpu import lattice_cloud  # noqa: E402
from test_critics_cpu import as_c, build_critics_check  # noqa: E402
from test_mapgrid_gpu import GEOMETRIES, ORIGIN, RES, centre, device_copy, ref_map, scenario  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
INV = _lib.GEM_OK - 1
STOP, SUM = _lib.MAPGRID_STOP_ON_FAILURE, _lib.MAPGRID_SUM
FORWARD = 0.325
SMALL = [[-0.07, -0.05], [-0.07, 0.05], [0.07, 0.05], [0.07, -0.05]]       # a 4-vertex footprint of about three cells by two
CLEARED = {"75x75": (slice(20, 58), slice(18, 60)), "130x90": (slice(30, 60), slice(40, 90))}     # rows, columns


@pytest.fixture(scope="module")
def emap():
    m = ElevationMap(32, 0.05)
    yield m
    m.close()


# ---- the scenario (the reference side: computed once, never changed) ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def parity_case(geom):
    """the noise map of test_mapgrid_gpu.py with a reachable region, a plan across the diagonal whose cells are known (not 255), the
    three grids, and 300 trajectories of 7 poses around and beyond the map's edge (the generator of its case 4)"""
    sx, sy = GEOMETRIES[geom]
    g = np.array(scenario(geom, "noise")[0])
    rows, cols = CLEARED[geom]
    sub = g[rows, cols]                                                  # (a view) a reachable region, so that distances of every kind occur
    sub[sub >= 253] = 0
    g[rows.start + 10:rows.start + 13, cols.start + 15:cols.start + 18] = 254
    g[rows.start + 20:rows.start + 25, cols.start + 8:cols.start + 13] = 253      # inscribed cells: the obstacle critic passes them, the grids answer OB
    cm0 = ref_map(g)
    plan = [centre(cm0, 1, 1), centre(cm0, sx // 2, sy // 2), centre(cm0, sx - 12, sy - 12)]
    front = ref.front_plan(plan, FORWARD)
    for c in mref.plan_cells(cm0, mref.adjust_plan(front, RES)):           # the run is the whole plan
        assert c is not None
        if g[c[1], c[0]] == 255:
            g[c[1], c[0]] = 0
    g.setflags(write=False)
    cm = ref_map(g)
    want = mref.grids(cm, plan)
    want_front = mref.grids(cm, front)
    grids = {ref.GRID_PATH: want["path"], ref.GRID_GOAL: want["goal"], ref.GRID_FRONT: want_front["goal"]}
    T, n = 7, 300
    rng = np.random.default_rng(11)
    x_lo, x_hi = cm.ox + cols.start * RES, cm.ox + cols.stop * RES
    y_lo, y_hi = cm.oy + rows.start * RES, cm.oy + rows.stop * RES
    start = np.stack([rng.uniform(cm.ox - 1.0, cm.ox + sx * RES + 1.0, n), rng.uniform(cm.oy - 1.0, cm.oy + sy * RES + 1.0, n)], axis=1)
    inside = rng.random(n) < 0.6
    start[inside] = np.stack([rng.uniform(x_lo, x_hi, int(inside.sum())), rng.uniform(y_lo, y_hi, int(inside.sum()))], axis=1)
    steps = rng.uniform(-4 * RES, 4 * RES, (n, T, 2)).cumsum(axis=1)
    xy = start[:, None, :] + steps
    xyt = np.concatenate([xy.reshape(-1, 2), rng.uniform(-np.pi, np.pi, (n * T, 1))], axis=1)
    # three made ones: over the inscribed patch (a stop-on-failure grid rejects it) | off the map before that | a free cell all the way
    on, ob, off = centre(cm, cols.start + 5, rows.start + 5), centre(cm, cols.start + 10, rows.start + 22), (cm.ox - 2.0, cm.oy + 1.0)
    assert want["path"][rows.start + 22, cols.start + 10] == sx * sy + 1     # (the patch's inner cells touch no reached cell: UN, its rim OB)
    xyt[:3 * T, :2] = [on, on, ob, on, on, on, on] + [on, off, on, ob, on, on, on] + [on] * 7
    xyt[:3 * T, 2] = 0.0
    poses = fref.poses_from_yaw(xyt)
    ext = np.zeros((2, n))
    ext[0] = np.where(rng.random(n) < 0.1, -5.0, 0.0)                     # oscillation: rejects a tenth
    ext[1] = np.abs(rng.normal(0.0, 0.5, n))                              # twirling: |angular velocity|
    ext[0, :3] = 0.0
    ext[1, 2] = np.nan                                                    # behind every other critic of a good trajectory: not valid
    for a in (poses, ext):
        a.setflags(write=False)
    return {"cm": cm, "plan": plan, "front": front, "want": want, "want_front": want_front, "grids": grids, "poses": poses, "T": T, "ext": ext}


def critic_lists():
    zero = list(ref.dwa_list())
    zero[3] = dict(zero[3], scale=0.0)
    return {"dwa": ref.dwa_list(),
            "dwa sum centre": ref.dwa_list(obstacle_flags=fref.SUM | ref.CENTRE_COST | fref.INSCRIBED_LETHAL, grid_flags=mref.SUM),
            "obstacle alone": [ref.obstacle(1.0)],
            "grid alone": [ref.map_grid(0.5, ref.GRID_FRONT, FORWARD, STOP)],
            "external alone": [ref.external(2.0, 1)],
            "zero scale": zero}


@functools.lru_cache(maxsize=None)
def parity_reference(geom, name):
    """(score table, totals, (index, cost, n_valid))"""
    c = parity_case(geom)
    critics = critic_lists()[name]
    table = ref.score_table(c["cm"], c["grids"], critics, c["poses"], c["T"], SMALL, c["ext"])
    totals = ref.combine(critics, table)
    totals.setflags(write=False)
    return table, totals, ref.find_best(totals)


def rejected_by(critics, table):
    """per trajectory the index of the critic that rejected it, -1 without one"""
    out = np.full(table.shape[1], -1)
    for t in range(table.shape[1]):
        for k, c in enumerate(critics):
            if c["scale"] != 0 and table[k, t] < 0:
                out[t] = k
                break
    return out


# ---- running both forms -------------------------------------------------------------------------------------------------------------
def prepared(m, c):
    dev = device_copy(m, c["cm"])
    dev.prepare_map_grid(c["plan"])
    dev.prepare_map_grid_front(c["front"])
    return dev


def same(got_index, got_cost, got_n_valid, got_totals, totals, best, what):
    assert got_totals.dtype == np.float64 and got_totals.tobytes() == np.asarray(totals).tobytes(), \
        f"{what}: {int((got_totals.view(np.uint64) != np.asarray(totals).view(np.uint64)).sum())} totals differ"
    assert (int(got_index), np.float64(got_cost).tobytes(), int(got_n_valid)) == (best[0], np.float64(best[1]).tobytes(), best[2]), \
        f"{what}: got {(got_index, got_cost, got_n_valid)}, want {best}"


def host_form(dev, critics, poses, T, spec, ext, lens, totals, best, what):
    i, cost, n_valid, tot = dev.best_trajectory(as_c(critics)[:len(critics)], poses, T, spec, ext, lens, totals=True)
    same(i, cost, n_valid, tot, totals, best, what + " (host)")
    assert dev.best_trajectory(as_c(critics)[:len(critics)], poses, T, spec, ext, lens) == (i, cost, n_valid)     # without totals


def device_form(m, dev, critics, poses, T, spec, ext, lens, totals, best, what):
    import torch
    d_poses = torch.from_numpy(np.array(poses, np.float64)).to("cuda:0")                 # (a copy: the cases are read-only)
    d_ext = None if ext is None else torch.from_numpy(np.array(ext, np.float64)).to("cuda:0")
    d_lens = None if lens is None else torch.from_numpy(np.array(lens, np.int32)).to("cuda:0")
    d_best, d_tot = dev.best_trajectory(as_c(critics)[:len(critics)], d_poses, T, spec, d_ext, d_lens, totals=True)      # only enqueued
    m.synchronize()
    b = d_best.cpu()
    assert d_best.dtype == torch.int64 and d_tot.dtype == torch.float64 and int(b[3]) == 0
    same(int(b[0]), float(b.view(torch.float64)[2]), int(b[1]), d_tot.cpu().numpy(), totals, best, what + " (device)")


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["75x75", "130x90"])
def test_parity_of_host_and_device_forms(emap, geom):
    c = parity_case(geom)
    lists = critic_lists()
    # the case cannot pass empty: asserted on the reference's output
    table, totals, best = parity_reference(geom, "dwa")
    by = rejected_by(lists["dwa"], table)
    n = totals.size
    assert (by == 1).any() and (by == 0).any() and ((by == 4) | (by == 5)).any()                # obstacle | external | a stop-on-failure grid
    stop_codes = {int(v) for k in (4, 5) for v in table[k][by == k]}
    assert stop_codes & {-3, -2} and best[2] >= n // 10 and best[0] > 0
    assert np.isnan(totals).any() and (table[2] != table[5]).any()                              # a NaN external | FRONT is not GOAL
    assert c["grids"][ref.GRID_FRONT].tobytes() != c["grids"][ref.GRID_GOAL].tobytes()
    dev = prepared(emap, c)
    try:
        for name, critics in lists.items():
            _, totals, best = parity_reference(geom, name)
            host_form(dev, critics, c["poses"], c["T"], SMALL, c["ext"], None, totals, best, f"{geom} {name}")
            device_form(emap, dev, critics, c["poses"], c["T"], SMALL, c["ext"], None, totals, best, f"{geom} {name}")
        assert parity_reference(geom, "dwa sum centre")[1].tobytes() != parity_reference(geom, "dwa")[1].tobytes()
        assert parity_reference(geom, "zero scale")[1].tobytes() != parity_reference(geom, "dwa")[1].tobytes()
    finally:
        dev.close()


# ---- 2. group widths and lengths ------------------------------------------------------------------------------------------------------
WIDTH_CRITICS = [ref.obstacle(0.5, ref.CENTRE_COST), ref.map_grid(1.0, ref.GRID_PATH, 0.1, STOP), ref.map_grid(0.25, ref.GRID_GOAL, 0.0, mref.SUM),
                 ref.external(1.0, 0)]


@functools.lru_cache(maxsize=None)
def width_case(T, nv):
    """65 trajectories of T poses inside and around the reachable region: (poses, ext, spec, {lengths' name: (lens, table)})"""
    c = parity_case("75x75")
    cm = c["cm"]
    rows, cols = CLEARED["75x75"]
    n = 65
    rng = np.random.default_rng(1000 * T + nv)
    start = np.stack([rng.uniform(cm.ox + (cols.start - 3) * RES, cm.ox + (cols.stop + 3) * RES, n),
                      rng.uniform(cm.oy + (rows.start - 3) * RES, cm.oy + (rows.stop + 3) * RES, n)], axis=1)
    xy = start[:, None, :] + rng.uniform(-0.4 * RES, 0.4 * RES, (n, T, 2)).cumsum(axis=1)
    poses = fref.poses_from_yaw(np.concatenate([xy.reshape(-1, 2), rng.uniform(-np.pi, np.pi, (n * T, 1))], axis=1))
    ext = np.where(rng.random((1, n)) < 0.1, -1.0, rng.integers(0, 4, (1, n)) / 4.0)
    spec = fref.regular_polygon(nv, 0.12) if nv else []
    lens = {"all T": None, "random": rng.integers(1, T + 1, n).astype(np.int32), "all 1": np.ones(n, np.int32)}
    tables = {k: ref.score_table(cm, c["grids"], WIDTH_CRITICS, poses, T, spec, ext, v) for k, v in lens.items()}
    bad = np.array(lens["random"])
    bad[[0, n // 2, n - 1]] = [0, T + 1, -3]
    return poses, ext, spec, lens, tables, bad


@pytest.mark.parametrize("T", [1, 7, 9, 17, 33, 65])
def test_group_widths_and_lengths(emap, T):
    c = parity_case("75x75")
    dev = prepared(emap, c)
    valid = 0
    try:
        for nv in (0, 3, 8, 31):
            poses, ext, spec, lens, tables, bad = width_case(T, nv)
            for kind, ln in lens.items():
                for n in (0, 1, 63, 64, 65):
                    table = tables[kind][:, :n]
                    totals = ref.combine(WIDTH_CRITICS, table)
                    best = ref.find_best(totals)
                    args = (dev, WIDTH_CRITICS, poses[:n * T], T, spec, ext[:, :n], None if ln is None else ln[:n], totals, best, f"T {T} nv {nv} {kind} n {n}")
                    host_form(*args)
                    if n in (0, 65):
                        device_form(emap, *args)
                    valid += best[2]
            # lengths nobody could refuse in device memory: -5.0, whatever the poses
            totals = ref.combine(WIDTH_CRITICS, tables["random"], bad, T)
            assert totals[0] == totals[32] == totals[64] == -5.0
            device_form(emap, dev, WIDTH_CRITICS, poses, T, spec, ext, bad, totals, ref.find_best(totals), f"T {T} nv {nv} bad lengths")
            with pytest.raises(Exception):
                dev.best_trajectory(as_c(WIDTH_CRITICS)[:4], poses, T, spec, ext, bad)          # the host form refuses them
        assert valid > 100
    finally:
        dev.close()


# ---- 3. across workgroups -------------------------------------------------------------------------------------------------------------
def test_more_than_one_stride_of_the_grid(emap):
    c = parity_case("130x90")
    cm = c["cm"]
    rows, cols = CLEARED["130x90"]
    n = 70000
    critics = [ref.obstacle(1.0), ref.map_grid(1000.0, ref.GRID_GOAL, 0.0, STOP)]
    rng = np.random.default_rng(70000)
    xyt = np.stack([rng.uniform(cm.ox + cols.start * RES, cm.ox + cols.stop * RES, n), rng.uniform(cm.oy + rows.start * RES, cm.oy + rows.stop * RES, n),
                    rng.uniform(-np.pi, np.pi, n)], axis=1)
    poses = fref.poses_from_yaw(xyt)
    first = ref.combine(critics, ref.score_table(cm, c["grids"], critics, poses, 1, SMALL))
    w = ref.find_best(first)[0]
    winner = poses[w].copy()
    poses[first == first[w]] = poses[int(np.argmax(first))]                  # nobody else costs as little ...
    poses[[69999, 12345]] = winner                                          # ... but these two
    totals = ref.combine(critics, ref.score_table(cm, c["grids"], critics, poses, 1, SMALL))
    best = ref.find_best(totals)
    assert best[0] == 12345 and totals[69999] == totals[12345] and int((totals == best[1]).sum()) == 2 and best[2] > n // 2
    dev = prepared(emap, c)
    try:
        host_form(dev, critics, poses, 1, SMALL, None, None, totals, best, "70 000")
        device_form(emap, dev, critics, poses, 1, SMALL, None, None, totals, best, "70 000")
        gone = poses.copy()
        gone[:, 0] = cm.ox - 1.0                                             # every trajectory off the map
        totals = np.full(n, -3.0)
        host_form(dev, critics, gone, 1, SMALL, None, None, totals, (-1, -1.0, 0), "all rejected")
        device_form(emap, dev, critics, gone, 1, SMALL, None, None, totals, (-1, -1.0, 0), "all rejected")
    finally:
        dev.close()


# ---- 4. ties ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", [4, 20, 200])
def test_ties_go_to_the_smallest_index(emap, other):
    """identical trajectories at 3 and `other` (the same wave | another wave of the workgroup | another workgroup), both as good as the
    winner further back: 3 wins"""
    c = parity_case("75x75")
    critics = critic_lists()["dwa"]
    table, totals, best = parity_reference("75x75", "dwa")
    T, w = c["T"], best[0]
    assert w > 4 and w not in (20, 200)
    poses, ext, totals = np.array(c["poses"]), np.array(c["ext"]), np.array(totals)
    for t in (3, other):
        poses[t * T:(t + 1) * T] = poses[w * T:(w + 1) * T]
        ext[:, t] = ext[:, w]
        totals[t] = totals[w]
    again = ref.combine(critics, ref.score_table(c["cm"], c["grids"], critics, poses, T, SMALL, ext))
    assert again.tobytes() == totals.tobytes() and ref.find_best(totals)[0] == 3 and int((totals == best[1]).sum()) == 3
    dev = prepared(emap, c)
    try:
        host_form(dev, critics, poses, T, SMALL, ext, None, totals, ref.find_best(totals), f"tie 3 / {other}")
        device_form(emap, dev, critics, poses, T, SMALL, ext, None, totals, ref.find_best(totals), f"tie 3 / {other}")
    finally:
        dev.close()


# ---- 5. the FRONT grid ----------------------------------------------------------------------------------------------------------------
def test_the_front_grid(emap):
    import test_mapgrid_gpu as tm
    c = parity_case("130x90")
    dev = device_copy(emap, c["cm"])
    lib, h = emap._lib, emap._h
    poses = np.ascontiguousarray(c["poses"][:7])
    out = np.full(1, -99, np.int64)
    try:
        assert lib.gem_costmap_mapgrid_read_front(h, dev.id, None, None, None) == INV            # never prepared
        dev.prepare_map_grid(c["plan"])
        tm.same_grids(dev, c["want"])
        assert lib.gem_costmap_mapgrid_read_front(h, dev.id, None, None, None) == INV            # still not
        dev.prepare_map_grid_front(c["front"])
        got, started, goal = dev.read_map_grid_front()
        wf = c["want_front"]
        assert got.dtype == np.int32 and got.tobytes() == wf["goal"].tobytes() and (started, goal) == (wf["started"], wf["goal_cell"])
        assert wf["goal_cell"] != c["want"]["goal_cell"] and wf["goal"].tobytes() != c["want"]["goal"].tobytes()
        tm.same_grids(dev, c["want"], tm.BOTH, "PATH and GOAL after the front grid")
        dev.prepare_map_grid(c["plan"])                                     # ... and the front grid after them
        assert dev.read_map_grid_front()[0].tobytes() == wf["goal"].tobytes()
        for fn in (lambda: lib.gem_costmap_mapgrid_read(h, dev.id, 4, None, None, None),
                   lambda: lib.gem_costmap_mapgrid_score(h, dev.id, 4, poses.ctypes.data_as(C.c_void_p), 1, 7, 0.0, 0, out.ctypes.data_as(C.c_void_p)),
                   lambda: lib.gem_costmap_mapgrid_prepare(h, dev.id, (C.c_double * 2)(1.0, 1.0), 1, 4)):
            assert fn() == INV
        assert out.tolist() == [-99]
        # an empty front plan is valid: started = 0, the grid all UN
        dev.prepare_map_grid_front(np.zeros((0, 2)))
        got, started, goal = dev.read_map_grid_front()
        assert started == 0 and goal == (-1, -1) and (got == c["cm"].grid.size + 1).all()
    finally:
        dev.close()


# ---- 6. the cycle -----------------------------------------------------------------------------------------------------------------------
def test_the_enqueued_cycle_and_a_second_loop_allocates_nothing(emap):
    import torch
    sx = sy = 75
    res, origin = 0.2, (-3.1, 2.7)
    window = (5, 4, 70, 72)
    p = iref.Params(0.55, 0.41, 3.0, False)
    rng = np.random.default_rng(6)
    layer_ref, master_ref = cref.Costmap(sx, sy, res, *origin), cref.Costmap(sx, sy, res, *origin, cref.FREE_SPACE)
    layer, master = emap.costmap(sx, sy, res, *origin), emap.costmap(sx, sy, res, *origin, cref.FREE_SPACE)
    stale = rng.integers(1, 253, (sy, sx), dtype=np.uint8)
    T, n_traj = 5, 200
    xyt = np.stack([rng.uniform(origin[0] + 3.0, origin[0] + 12.0, T * n_traj), rng.uniform(origin[1] + 3.0, origin[1] + 12.0, T * n_traj),
                    rng.uniform(-np.pi, np.pi, T * n_traj)], axis=1)
    poses = fref.poses_from_yaw(xyt)
    ext = np.stack([np.where(rng.random(n_traj) < 0.1, -5.0, 0.0), np.abs(rng.normal(0.0, 0.5, n_traj))])
    lens = rng.integers(1, T + 1, n_traj).astype(np.int32)
    d_poses, d_ext, d_lens = (torch.from_numpy(a).to("cuda:0") for a in (poses, ext, lens))
    robot = (origin[0] + 7.5, origin[1] + 7.5, math.cos(0.3), math.sin(0.3))
    plan = [(origin[0] + 7.5, origin[1] + 7.5), (origin[0] + 11.0, origin[1] + 9.0), (origin[0] + 13.0, origin[1] + 12.9)]
    front = ref.front_plan(plan, 0.65)
    critics = ref.dwa_list(obstacle_flags=fref.INSCRIBED_LETHAL, forward=0.65)
    cs = as_c(critics)[:len(critics)]
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
            want, want_front = mref.grids(master_ref, plan), mref.grids(master_ref, front)
            grids = {ref.GRID_PATH: want["path"], ref.GRID_GOAL: want["goal"], ref.GRID_FRONT: want_front["goal"]}
            table = ref.score_table(master_ref, grids, critics, poses, T, fref.RECTANGLE, ext, lens)
            totals = ref.combine(critics, table, lens, T)
            best = ref.find_best(totals)
            # the device: nine calls, nothing waits before the answer
            layer.mark_points(pts, 0.5, None)
            ok, _ = layer.clear_footprint(robot, fref.RECTANGLE)
            master.reset_window(*window)
            layer.merge(master, window, cref.MAX)
            master.inflate(p.inflation_radius, p.inscribed_radius, p.cost_scaling_factor, p.inflate_unknown, window)
            master.prepare_map_grid(plan)
            master.prepare_map_grid_front(front)
            d_best, d_tot = master.best_trajectory(cs, d_poses, T, fref.RECTANGLE, d_ext, d_lens, totals=True)
            emap.synchronize()
            b = d_best.cpu()
            same(int(b[0]), float(b.view(torch.float64)[2]), int(b[1]), d_tot.cpu().numpy(), totals, best, "cycle")
            assert ok and best[0] >= 0 and 0 < best[2] < n_traj and (rejected_by(critics, table) == 1).any()
            out.append(best)
        return out

    try:
        first = loop()
        a1 = emap.debug_get("arena_allocations")
        second = loop()
        assert emap.debug_get("arena_allocations") == a1
        assert len(first) == len(second) == 2
    finally:
        layer.close(); master.close()


# ---- 7. stale grids and errors --------------------------------------------------------------------------------------------------------
def test_stale_grids_and_every_refusal():
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    c = parity_case("75x75")
    cm = c["cm"]
    dev = device_copy(m, cm)
    nan, inf = float("nan"), float("inf")
    T, n = 7, 4
    poses = np.array(c["poses"][:n * T])                                 # (a copy: the case is read-only)
    ext = np.zeros((2, n))
    spec = np.ascontiguousarray(SMALL, np.float64)
    tot = np.full(n, -99.0)
    best = _lib.BestTrajectory(-9, -9, -9.0, -9)
    lens = np.full(n, T, np.int32)
    dwa = ref.dwa_list()

    def call(critics=dwa, id_=None, n_critics=None, p=poses, ln=None, n_traj=n, T_=T, sp=spec, nv=4, e=ext, ncol=2, o=tot, b=best, fn="gem_costmap_best_trajectory"):
        cs = as_c(critics) if critics is not None else None
        return getattr(lib, fn)(h, dev.id if id_ is None else id_, cs, (len(critics) if critics is not None else 1) if n_critics is None else n_critics,
                                p.ctypes.data_as(C.c_void_p) if p is not None else None, ln.ctypes.data_as(C.c_void_p) if ln is not None else None,
                                n_traj, T_, sp.ctypes.data_as(C.POINTER(C.c_double)) if sp is not None else None, nv,
                                e.ctypes.data_as(C.c_void_p) if e is not None else None, ncol,
                                o.ctypes.data_as(C.c_void_p) if o is not None else None, C.byref(b) if b is not None else None)

    def with_(k, **kw):
        cs = [dict(x) for x in dwa]
        cs[k].update(kw)
        return cs

    try:
        assert call() == INV                                              # nothing prepared
        dev.prepare_map_grid(c["plan"])
        assert call() == INV                                              # the list names FRONT, which is not
        assert call(critics=[dwa[1], dwa[4], dwa[5]]) == 0 and best.index != -9      # ... a list without it runs
        tot[:] = -99.0
        best.index, best.n_valid, best.cost, best.reserved = -9, -9, -9.0, -9
        dev.prepare_map_grid_front(c["front"])
        for bad in (-1, 5, 8, 1 << 20):
            assert call(id_=bad) == INV
        assert call(critics=None) == INV and call(n_critics=0) == INV and call(critics=[dwa[0]] * 9) == INV and call(n_critics=-1) == INV
        assert call(with_(1, kind=0)) == INV and call(with_(1, kind=4)) == INV                    # an unknown kind
        assert call(with_(2, grid=0)) == INV and call(with_(2, grid=3)) == INV and call(with_(2, grid=8)) == INV
        assert call(with_(1, flags=8)) == INV and call(with_(2, flags=4)) == INV and call(with_(0, flags=1)) == INV and call(with_(1, flags=-1)) == INV
        for v in (-1.0, -1e-300, nan, inf, -inf):
            for k in (0, 1, 2):
                assert call(with_(k, scale=v)) == INV
        for v in (nan, inf, -inf):
            assert call(with_(2, xshift=v)) == INV
        assert call(with_(6, column=2)) == INV and call(with_(0, column=-1)) == INV and call(ncol=1) == INV and call(ncol=-1) == INV
        assert call(critics=[dwa[1], dwa[1]]) == INV                       # more than one OBSTACLE critic
        assert call(nv=-1) == INV and call(nv=33) == INV and call(sp=None) == INV
        bad_spec = spec.copy()
        bad_spec[2, 1] = nan
        assert call(sp=bad_spec) == INV
        assert call(critics=[dwa[0], dwa[6]], sp=None, nv=33) == 0         # ... the spec is an OBSTACLE critic's alone
        tot[:] = -99.0
        best.index, best.n_valid, best.cost, best.reserved = -9, -9, -9.0, -9
        assert call(p=None) == INV and call(e=None) == INV and call(b=None) == INV
        assert call(n_traj=-1) == INV and call(T_=0) == INV and call(T_=(1 << 20) + 1) == INV and call(n_traj=1 << 30, T_=4) == INV
        for v in (0, T + 1, -2):                                          # a length in host memory is refused
            ln = lens.copy()
            ln[2] = v
            assert call(ln=ln) == INV
        import torch
        d = {k: torch.from_numpy(a).to("cuda:0") for k, a in (("p", poses), ("e", ext))}
        d_tot, d_best = torch.full((n,), -99.0, dtype=torch.float64, device="cuda:0"), torch.full((4,), -9, dtype=torch.int64, device="cuda:0")

        def device_call(critics):
            return lib.gem_costmap_best_trajectory_device(h, dev.id, as_c(critics), len(critics), C.c_void_p(d["p"].data_ptr()), None, n, T,
                                                          spec.ctypes.data_as(C.POINTER(C.c_double)), 4, C.c_void_p(d["e"].data_ptr()), 2,
                                                          C.c_void_p(d_tot.data_ptr()), C.c_void_p(d_best.data_ptr()))

        assert device_call(with_(2, grid=3)) == INV and device_call(with_(1, scale=-1.0)) == INV
        w2 = ElevationMap(32, 0.05)                                       # a handle with a communicator
        w2.comm_init_loopback(9544, 1, 0, tile_strips=False)
        assert w2._lib.gem_costmap_best_trajectory(w2._h, 0, as_c(dwa), 7, poses.ctypes.data_as(C.c_void_p), None, n, T,
                                                   spec.ctypes.data_as(C.POINTER(C.c_double)), 4, ext.ctypes.data_as(C.c_void_p), 2, None, C.byref(best)) == INV
        assert w2._lib.gem_costmap_mapgrid_prepare_front(w2._h, 0, (C.c_double * 2)(0.0, 0.0), 1) == INV
        assert w2._lib.gem_costmap_mapgrid_read_front(w2._h, 0, None, None, None) == INV
        w2.close()
        # the front entries' own cases
        assert lib.gem_costmap_mapgrid_prepare_front(h, 9, (C.c_double * 2)(0.0, 0.0), 1) == INV
        assert lib.gem_costmap_mapgrid_prepare_front(h, dev.id, None, 3) == INV and lib.gem_costmap_mapgrid_prepare_front(h, dev.id, None, -1) == INV
        assert lib.gem_costmap_mapgrid_prepare_front(h, dev.id, (C.c_double * 2)(nan, 0.0), 1) == INV
        # nothing was written by any refusal
        m.synchronize()
        assert tot.tolist() == [-99.0] * n and (best.index, best.n_valid, best.cost, best.reserved) == (-9, -9, -9.0, -9)
        assert d_tot.cpu().tolist() == [-99.0] * n and d_best.cpu().tolist() == [-9] * 4
        assert dev.read_map_grid_front()[0].tobytes() == c["want_front"]["goal"].tobytes()
        table = ref.score_table(cm, c["grids"], dwa, poses, T, SMALL, ext)
        totals = ref.combine(dwa, table)
        assert call() == 0
        same(best.index, best.cost, best.n_valid, tot, totals, ref.find_best(totals), "after the refusals")
        assert call(n_traj=0, p=None, e=None, o=None) == 0 and (best.index, best.cost, best.n_valid) == (-1, -1.0, 0)      # no trajectories: fine

        # a roll that moves the map makes all three grids stale until they are prepared again
        sizes = cm.size_in_meters()
        dev.roll_to(cm.ox + sizes[0] / 2 + 7 * RES, cm.oy + sizes[1] / 2 - 4 * RES)
        assert call() == INV and lib.gem_costmap_mapgrid_read_front(h, dev.id, None, None, None) == INV
        dev.prepare_map_grid(c["plan"])
        assert call() == INV                                              # FRONT is still the old one
        assert call(critics=[dwa[1], dwa[4], dwa[5]]) == 0
        dev.prepare_map_grid_front(c["front"])
        geo = dev.geometry()
        rolled = cref.Costmap(cm.size_x, cm.size_y, RES, geo["origin_x"], geo["origin_y"], 0)
        rolled.grid[:] = dev.read()
        want, want_front = mref.grids(rolled, c["plan"]), mref.grids(rolled, c["front"])
        grids = {ref.GRID_PATH: want["path"], ref.GRID_GOAL: want["goal"], ref.GRID_FRONT: want_front["goal"]}
        totals = ref.combine(dwa, ref.score_table(rolled, grids, dwa, poses, T, SMALL, ext))
        assert call() == 0
        same(best.index, best.cost, best.n_valid, tot, totals, ref.find_best(totals), "after the roll")
    finally:
        dev.close()
        m.close()


# ---- 8. the C++ facade ------------------------------------------------------------------------------------------------------------------
def test_cpp_critics_facade(tmp_path):
    exe = build_critics_check(tmp_path / "critics_check")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
