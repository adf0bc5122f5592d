"""VoxelLayer on the device costmap (gem_costmap_voxels_*, gem_costmap_voxel_observe / _observe_device) against the restatement of
tests/voxlayer_ref.py.  Every comparison is exact: grids and columns by tobytes(), bounds by == on doubles.  The cases are those of
tests/test_voxlayer_cpu.py (`cases()`), whose answers the reference computes once.

  1. the cases: 75 x 75 @ 0.2, 130 x 90 @ 0.05 and 300 x 260 @ 0.1 on noise grids and noise columns, so that untouched cells are checked
     too; size_z 1, 10 and 16, origin_z 0 and -0.3, thresholds (15, 0), (2, 0) and (15, 2); 4097 random records plus the hand-made
     ones, raytrace_range 0.4 w and 2 w; the sensor in the first and the last voxel, on a voxel boundary, below origin_z and off the
     map; two clearing and two marking observations in one call; n = 0, 1, 63, 64, 65, 4097 at strides 12, 16 and 32; bounds NULL.
     A second identical call shows that the scratch was left clean;
  2. stream order: reset_window -> voxel_observe -> clear_footprint -> merge -> inflate enqueued without a host wait, read back once;
  3. the device form with torch tensors, and no allocation in a second identical loop;
  4. roll_to between two observes, and reset: the columns move with the bytes, the rest unknown;
  5. a plan made before voxel_observe is refused as stale;
  6. the overhang scene: marks above a ray keep the cell lethal, the 2-D layer clears it;
  7. the error cases (GEM_ERR_INVALID; grid, columns and bounds unchanged);
  8. the C++ facade (tests/cpp/voxlayer_check.cpp) as a child process."""
import ctypes as C
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gem_amd import ElevationMap, GemError, _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import costmap_ref as cref  # noqa: E402
import footprint_ref as fref  # noqa: E402
import inflate_ref as iref  # noqa: E402
import obstacle_ref as oref  # noqa: E402
import voxlayer_ref as ref  # noqa: E402
from test_voxlayer_cpu import (EMPTY, GEOMETRIES, LAYER_MAX, ORIGIN, build_voxlayer_check, cases, fresh, noise_columns, observation, sensor,  # noqa: E402
                               voxels, wanted, world)

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
INV = _lib.GEM_OK - 1


@pytest.fixture(scope="module")
def emap():
    m = ElevationMap(32, 0.05)
    yield m
    m.close()


def device_copy(m, cm, cols, vox):
    dev = m.costmap(cm.size_x, cm.size_y, cm.res, cm.ox, cm.oy)
    dev.write(cm.grid)
    dev.attach_voxels(*vox)
    dev.write_voxels(cols)
    return dev


def same(dev, want_grid, want_cols, what):
    got, cols = dev.read(), dev.read_voxels()
    assert got.tobytes() == want_grid, f"{what}: {int((got.reshape(-1) != np.frombuffer(want_grid, np.uint8)).sum())} cells differ"
    assert cols.tobytes() == want_cols, f"{what}: {int((cols.reshape(-1) != np.frombuffer(want_cols, np.uint32)).sum())} columns differ"


# ---- 1. the cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases()))
def test_cases(emap, name):
    geom, vox, observations, bounds = cases()[name]
    want_grid, want_cols, want_bounds = wanted(name)
    base, cols = fresh(geom)
    dev = device_copy(emap, base, cols, vox)
    try:
        got = dev.voxel_observe(list(observations), LAYER_MAX, None if bounds is None else list(bounds))
        assert got == want_bounds, (got, want_bounds)
        same(dev, want_grid, want_cols, name)
        # a second identical call on the result: the reference's answer to that, which is no change where no record is accepted
        again = cref.Costmap(*GEOMETRIES[geom], *ORIGIN)
        again.grid[:] = np.frombuffer(want_grid, np.uint8).reshape(again.grid.shape)
        cols2 = np.frombuffer(want_cols, np.uint32).reshape(cols.shape).copy()
        d = {}
        ref.observe(again, cols2, vox, list(observations), LAYER_MAX, None, detail=d)
        dev.voxel_observe(list(observations), LAYER_MAX)
        same(dev, again.grid.tobytes(), cols2.tobytes(), name + ", again")
        if not d["accepted"].any():
            assert again.grid.tobytes() == want_grid and cols2.tobytes() == want_cols
    finally:
        dev.close()
    if " n 0 " in name:
        assert want_grid == base.grid.tobytes() and want_cols == cols.tobytes()
    elif " stride " not in name:
        assert want_cols != cols.tobytes() and want_grid != base.grid.tobytes()


# ---- 2. stream order ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["75x75", "300x260"])
def test_the_enqueued_cycle(emap, geom):
    sx, sy, res = GEOMETRIES[geom]
    base, cloud = world(geom)
    vox = voxels("z10", (15, 0))
    window = (3, 4, sx - 5, sy - 2)
    p = iref.Params(3 * res - 0.05 * res, 2 * res + 0.05 * res, 3.0, False)
    layer_ref, cols_ref = fresh(geom)
    master_ref = cref.Costmap(sx, sy, res, *ORIGIN, cref.FREE_SPACE)
    old = np.random.default_rng(9).integers(1, 254, (sy, sx), dtype=np.uint8)      # what a cycle before left in the master
    master_ref.grid[:] = old
    s = sensor(base)
    obs = [observation(base, cloud, s, 0.4)]
    robot = (s[0], s[1], math.cos(0.3), math.sin(0.3))
    spec = [[-3 * res, -2 * res], [-3 * res, 2 * res], [3 * res, 2 * res], [3 * res, -2 * res]]
    iref.reset_window(master_ref.grid, *window, cref.FREE_SPACE)
    ref.observe(layer_ref, cols_ref, vox, obs, LAYER_MAX)
    assert fref.clear_footprint(layer_ref, robot, spec)
    cref.merge(layer_ref, master_ref, window, cref.MAX)
    master_ref.grid[:] = iref.inflate_exact(master_ref.grid, p, res, window)
    layer, master = device_copy(emap, base, noise_columns(geom), vox), emap.costmap(sx, sy, res, *ORIGIN, cref.FREE_SPACE)
    try:
        master.write(old)
        master.reset_window(*window)                                      # five calls, none of which waits for the device
        assert layer.voxel_observe(obs, LAYER_MAX, None) is None
        ok, _ = layer.clear_footprint(robot, spec)
        layer.merge(master, window, cref.MAX)
        master.inflate(p.inflation_radius, p.inscribed_radius, p.cost_scaling_factor, p.inflate_unknown, window)
        assert master.read().tobytes() == master_ref.grid.tobytes()
        same(layer, layer_ref.grid.tobytes(), cols_ref.tobytes(), "layer")
        assert ok and (master_ref.grid == 253).any() and (master_ref.grid == 254).any() and (master_ref.grid == 0).any()
    finally:
        layer.close(); master.close()


# ---- 3. device tensors ------------------------------------------------------------------------------------------------------------------
def test_device_tensors_and_a_second_loop_allocates_nothing(emap):
    import torch
    names = ["130x90 z10 range 0.4 w", "300x260 four observations", "75x75 n 65 stride 12", "75x75 n 4097 stride 32"]
    tensors = {n: [torch.from_numpy(o["points"].copy()).to("cuda:0") for o in cases()[n][2]] for n in names}
    devs = {n: device_copy(emap, *fresh(cases()[n][0]), cases()[n][1]) for n in names}

    def loop():
        for n in names:
            geom, vox, observations, bounds = cases()[n]
            devs[n].write(world(geom)[0].grid)
            devs[n].write_voxels(noise_columns(geom))
            obs = [{**o, "points": t} for o, t in zip(observations, tensors[n])]
            b = devs[n].voxel_observe(obs, LAYER_MAX, list(bounds))
            assert b == wanted(n)[2]
            same(devs[n], wanted(n)[0], wanted(n)[1], n)
            devs[n].write(world(geom)[0].grid)
            devs[n].write_voxels(noise_columns(geom))
            assert devs[n].voxel_observe(obs, LAYER_MAX, None) is None    # only enqueued
            same(devs[n], wanted(n)[0], wanted(n)[1], n + ", enqueued")

    try:
        loop()
        a1 = emap.debug_get("arena_allocations")
        loop()
        assert emap.debug_get("arena_allocations") == a1
        n = names[3]                                                      # host and device inputs do not mix
        with pytest.raises(ValueError):
            devs[n].voxel_observe([{**cases()[n][2][0], "points": tensors[n][0]}, cases()[n][2][0]], LAYER_MAX)
        emap.synchronize()
    finally:
        for d in devs.values():
            d.close()


# ---- 4. roll and reset ------------------------------------------------------------------------------------------------------------------
def rolled(a, cell_ox, cell_oy, fill):
    """Costmap2D::updateOrigin's copy: out(x, y) = a(x + cell_ox, y + cell_oy) where that lies in the map, fill elsewhere"""
    sy, sx = a.shape
    out = np.full_like(a, fill)
    ys, xs = np.mgrid[0:sy, 0:sx]
    src_y, src_x = ys + cell_oy, xs + cell_ox
    ok = (src_x >= 0) & (src_x < sx) & (src_y >= 0) & (src_y < sy)
    out[ok] = a[src_y[ok], src_x[ok]]
    return out


def test_roll_between_two_observes_and_reset(emap):
    geom = "75x75"
    sx, sy, res = GEOMETRIES[geom]
    base, cloud = world(geom)
    vox = voxels("z10", (15, 0))
    cm, cols = fresh(geom)
    s = sensor(base)
    first, second = [observation(base, cloud[:2000], s, 0.4)], [observation(base, cloud[2000:], (s[0] + 1.0, s[1] - 0.6, 0.8), 0.4)]
    dev = device_copy(emap, base, noise_columns(geom), vox)
    try:
        ref.observe(cm, cols, vox, first, LAYER_MAX)
        dev.voxel_observe(first, LAYER_MAX)
        # the roll: the robot 1.3 m right and 0.9 m down of the map's centre
        w, h = cm.size_in_meters()
        robot = (cm.ox + w / 2 + 1.3, cm.oy + h / 2 - 0.9)
        dev.roll_to(*robot)
        g = dev.geometry()
        cell_ox, cell_oy = int((robot[0] - w / 2 - cm.ox) / res), int((robot[1] - h / 2 - cm.oy) / res)
        assert (cell_ox, cell_oy) == (6, -4) and g["origin_x"] == cm.ox + cell_ox * res and g["origin_y"] == cm.oy + cell_oy * res
        moved = cref.Costmap(sx, sy, res, g["origin_x"], g["origin_y"])
        moved.grid[:] = rolled(cm.grid, cell_ox, cell_oy, cref.NO_INFORMATION)
        cols = rolled(cols, cell_ox, cell_oy, ref.UNKNOWN_COLUMN)
        same(dev, moved.grid.tobytes(), cols.tobytes(), "rolled")
        assert (cols == ref.UNKNOWN_COLUMN).sum() >= 6 * sy + 4 * (sx - 6)
        b = list(EMPTY)
        ref.observe(moved, cols, vox, second, LAYER_MAX, b)
        assert dev.voxel_observe(second, LAYER_MAX, list(EMPTY)) == b
        same(dev, moved.grid.tobytes(), cols.tobytes(), "observed after the roll")
        # reset_window leaves the columns alone, reset makes every column unknown
        dev.reset_window(0, 0, sx, 10)
        assert dev.read_voxels().tobytes() == cols.tobytes() and (dev.read()[:10] == cref.NO_INFORMATION).all()
        dev.reset()
        assert (dev.read() == cref.NO_INFORMATION).all() and (dev.read_voxels() == ref.UNKNOWN_COLUMN).all()
        # a window of the columns, written and read back
        part = (np.arange(1, 7 * 5 + 1, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32).reshape(5, 7)
        dev.write_voxels(part, (3, 9, 10, 14))
        whole = dev.read_voxels()
        assert whole[9:14, 3:10].tobytes() == part.tobytes() and (whole == ref.UNKNOWN_COLUMN).sum() == sx * sy - 35
        assert dev.read_voxels((3, 9, 10, 14)).tobytes() == part.tobytes()
        # detached, the costmap takes the paths it took before
        dev.detach_voxels()
        with pytest.raises(GemError):
            dev.read_voxels()
        dev.reset()
        dev.roll_to(robot[0] + 1.0, robot[1])
    finally:
        dev.close()


# ---- 5. a plan goes stale -----------------------------------------------------------------------------------------------------------------
def test_a_plan_made_before_voxel_observe_is_stale(emap):
    base, cloud = world("75x75")
    cm = cref.Costmap(75, 75, 0.2, *ORIGIN)
    cm.grid[:] = 0
    dev = device_copy(emap, cm, np.full((75, 75), ref.UNKNOWN_COLUMN, np.uint32), voxels("z10", (15, 0)))
    try:
        start, goal = (ORIGIN[0] + 2.0, ORIGIN[1] + 2.0), (ORIGIN[0] + 11.0, ORIGIN[1] + 9.0)
        path, st = dev.nav_plan(start, goal)
        assert st["found"] and len(path) > 10
        pot, cells = dev.read_potential()
        dev.frontiers()
        dev.voxel_observe([], LAYER_MAX)                                  # no observation: nothing changes
        assert dev.read_potential()[0].tobytes() == pot.tobytes()
        dev.voxel_observe([observation(base, cloud[:100], sensor(base))], LAYER_MAX)
        with pytest.raises(GemError, match="before the costmap last rolled or was observed"):
            dev.read_potential()
        with pytest.raises(GemError, match="observed"):
            dev.read_frontiers()
        dev.nav_plan(start, goal)                                         # a new plan is good again
        dev.read_potential()
    finally:
        dev.close()


# ---- 6. the overhang ----------------------------------------------------------------------------------------------------------------------
def test_an_overhang_survives_the_ray_below_it(emap):
    """The reason the layer exists.  A 20 x 20 map at 0.5 m, ten voxels of 0.2 m: cell (13, 10) is lethal with marks in z-voxel 6 (an
    overhang 1.2 .. 1.4 m up).  A ray at height 0.3 (z-voxel 1) crosses the cell: VoxelLayer keeps it lethal and frees its neighbours,
    ObstacleLayer on a copy clears it."""
    vox = ref.Voxels(10, 0.2, 0.0, 15, 0)
    cm = cref.Costmap(20, 20, 0.5, 0.0, 0.0)
    cm.grid[:] = 100
    cm.grid[10, 13] = 254
    cols = np.full((20, 20), ref.UNKNOWN_COLUMN, np.uint32)
    cols[10, 13] |= 1 << 22
    ray = [{"points": np.array([[9.25, 5.25, 0.3]], np.float32), "origin": (5.25, 5.25, 0.3), "raytrace_range": 100.0, "marking": False}]
    a, b = device_copy(emap, cm, cols, vox), device_copy(emap, cm, cols, vox)
    try:
        a.voxel_observe(ray, 2.0)
        g, c = a.read(), a.read_voxels()
        assert g[10, 13] == 254 and c[10, 13] == (ref.UNKNOWN_COLUMN | (1 << 22)) & ~(1 << 1)
        assert g[10, 10:17].tolist() == [0, 0, 0, 254, 0, 0, 0] and (g != 100).sum() == 7
        b.observe(ray, 2.0)
        g2 = b.read()
        assert g2[10, 13] == 0 and g2[10, 10:19].tolist() == [0] * 9 and b.read_voxels().tobytes() == cols.tobytes()
        want, want_cols = cm, cols.copy()
        ref.observe(want, want_cols, vox, ray, 2.0)
        assert g.tobytes() == want.grid.tobytes() and c.tobytes() == want_cols.tobytes()
    finally:
        a.close(); b.close()


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------------
def test_error_cases_leave_grid_columns_and_bounds_unchanged():
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    base, cols = fresh("75x75")
    cloud = world("75x75")[1]
    vox = voxels("z10", (15, 0))
    dev = device_copy(m, base, cols, vox)
    bare = m.costmap(75, 75, 0.2, *ORIGIN)                                # no voxels attached
    pts = np.ascontiguousarray(cloud[:64])
    b = (C.c_double * 4)(*EMPTY)
    nan, inf = float("nan"), float("inf")
    s = sensor(base)

    def one(**change):
        f = {"points": pts.ctypes.data, "n": 64, "point_step": 12, "flags": 3, "origin": s, "obstacle_range": 2.5, "raytrace_range": 3.0,
             "min_obstacle_height": 0.0, "max_obstacle_height": 2.0}
        f.update(change)
        return _lib.Observation(f["points"], f["n"], f["point_step"], f["flags"], (C.c_double * 3)(*f["origin"]), f["obstacle_range"],
                                f["raytrace_range"], f["min_obstacle_height"], f["max_obstacle_height"])

    def call(obs, n_obs=None, id_=None, layer_max=LAYER_MAX, entry="gem_costmap_voxel_observe", handle=None):
        arr = (_lib.Observation * max(len(obs), 1))(*obs)
        return getattr(lib, entry)(handle or h, dev.id if id_ is None else id_, arr if obs else None, len(obs) if n_obs is None else n_obs, layer_max, b)

    def unchanged():
        assert dev.read().tobytes() == base.grid.tobytes() and dev.read_voxels().tobytes() == cols.tobytes() and list(b) == EMPTY

    bad = [one(n=-1), one(n=(1 << 31) - 1), one(point_step=8), one(point_step=14), one(point_step=0), one(flags=0), one(flags=4), one(flags=7),
           one(origin=(nan, 0.0, 0.0)), one(origin=(0.0, inf, 0.0)), one(origin=(0.0, 0.0, -inf)), one(obstacle_range=-1.0), one(obstacle_range=nan),
           one(raytrace_range=-0.5), one(raytrace_range=nan), one(min_obstacle_height=2.5), one(min_obstacle_height=nan),
           one(max_obstacle_height=nan), one(points=None)]
    try:
        for entry in ("gem_costmap_voxel_observe", "gem_costmap_voxel_observe_device"):
            for o in bad:
                assert call([o], entry=entry) == INV
                assert call([one(n=0, points=None), o], entry=entry) == INV        # wherever it stands in the list
            for id_ in (-1, 5, 8, 1 << 20, bare.id):                      # no such costmap, or one without voxels
                assert call([one()], id_=id_, entry=entry) == INV
            assert call([one()], n_obs=-1, entry=entry) == INV and call([one()] * 9, entry=entry) == INV and call([], n_obs=1, entry=entry) == INV
            assert call([one()], layer_max=nan, entry=entry) == INV
            half = (1 << 30)                                              # more than 2^31 - 2 records in the call, none alone
            assert call([one(n=half), one(n=half)], entry=entry) == INV
            unchanged()
        # the voxel grid itself: a bad configuration, attached twice, read / write / destroy without one, windows and strides
        V = _lib.VoxelConfig
        for cfg in (V(0, 0.2, 0.0, 15, 0), V(17, 0.2, 0.0, 15, 0), V(10, 0.0, 0.0, 15, 0), V(10, -0.2, 0.0, 15, 0), V(10, nan, 0.0, 15, 0),
                    V(10, inf, 0.0, 15, 0), V(10, 0.2, nan, 15, 0), V(10, 0.2, inf, 15, 0), V(10, 0.2, 0.0, 17, 0), V(10, 0.2, 0.0, 15, 17)):
            assert lib.gem_costmap_voxels_create(h, bare.id, C.byref(cfg)) == INV
        assert lib.gem_costmap_voxels_create(h, bare.id, None) == INV and lib.gem_costmap_voxels_create(h, 6, C.byref(V(10, 0.2, 0.0, 15, 0))) == INV
        assert lib.gem_costmap_voxels_create(h, dev.id, C.byref(V(10, 0.2, 0.0, 15, 0))) == INV          # attached twice
        out = np.zeros((75, 75), np.uint32)
        op = out.ctypes.data_as(C.c_void_p)
        assert lib.gem_costmap_voxels_read(h, bare.id, 0, 0, 75, 75, op, 75) == INV and lib.gem_costmap_voxels_write(h, bare.id, 0, 0, 75, 75, op, 75) == INV
        assert lib.gem_costmap_voxels_destroy(h, bare.id) == INV
        for w in ((-1, 0, 75, 75), (0, 0, 76, 75), (0, 0, 75, 76), (10, 0, 9, 75)):
            assert lib.gem_costmap_voxels_read(h, dev.id, *w, op, 75) == INV and lib.gem_costmap_voxels_write(h, dev.id, *w, op, 75) == INV
        assert lib.gem_costmap_voxels_read(h, dev.id, 0, 0, 75, 75, None, 75) == INV and lib.gem_costmap_voxels_read(h, dev.id, 0, 0, 75, 75, op, 74) == INV
        assert lib.gem_costmap_voxels_write(h, dev.id, 0, 0, 75, 75, None, 75) == INV and lib.gem_costmap_voxels_write(h, dev.id, 0, 0, 75, 75, op, 74) == INV
        assert lib.gem_costmap_voxels_read(h, dev.id, 5, 5, 5, 9, None, 0) == 0                          # an empty window is no error
        unchanged()
        wide = np.zeros((75, 80), np.uint32)                              # a row stride above the width
        assert lib.gem_costmap_voxels_read(h, dev.id, 0, 0, 75, 75, wide.ctypes.data_as(C.c_void_p), 80) == 0
        assert wide[:, :75].tobytes() == cols.tobytes() and (wide[:, 75:] == 0).all()
        w = ElevationMap(32, 0.05)                                        # a handle that joins a communicator after its costmap got voxels
        wc = device_copy(w, base, cols, vox)
        assert call([one()], id_=wc.id, handle=w._h) == 0                 # the same call is good before ...
        w.comm_init_loopback(9562, 1, 0, tile_strips=False)
        assert call([one()], id_=wc.id, handle=w._h) == INV and call([one()], id_=wc.id, handle=w._h, entry="gem_costmap_voxel_observe_device") == INV
        wc.id = -1                                                        # (the handle's destruction frees it: no costmap call is taken now)
        w.close()
        b[:] = EMPTY
        unchanged()
        # what is no error: no observation, no record with NULL points, an infinite range, an infinite layer maximum
        assert call([]) == 0 and call([one(n=0, points=None, flags=1)]) == 0 and call([one(n=0, points=None)]) == 0
        unchanged()                                                       # (clearing without a record touches nothing: no touch of the sensor)
        assert call([one(raytrace_range=inf, obstacle_range=inf)], layer_max=inf) == 0
        cm, want_cols = fresh("75x75")
        want_b = list(EMPTY)
        ref.observe(cm, want_cols, vox, [{"points": pts, "origin": s, "raytrace_range": inf, "obstacle_range": inf}], inf, want_b)
        assert dev.read().tobytes() == cm.grid.tobytes() and dev.read_voxels().tobytes() == want_cols.tobytes() and list(b) == want_b
        assert cm.grid.tobytes() != base.grid.tobytes()
    finally:
        dev.close(); bare.close()
        m.close()


# ---- 8. the C++ facade ------------------------------------------------------------------------------------------------------------------------
def test_cpp_voxlayer_facade(tmp_path):
    exe = build_voxlayer_check(tmp_path / "voxlayer_check")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
