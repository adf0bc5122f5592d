"""ObstacleLayer on the device costmap (gem_costmap_observe / _observe_device) against the restatement of tests/obstacle_ref.py.  Every
comparison is exact: grids by tobytes(), bounds by == on doubles.  The cases are those of tests/test_obstacle_cpu.py (`cases()`), whose
answers the reference computes once; every one runs with both values of the debug key "obstacle_direct".

  1. the cases: 75 x 75 @ 0.2 and 130 x 90 @ 0.05 (bitmaps in LDS) and 300 x 260 @ 0.1 (global), all on noise grids so that untouched
     cells are checked too; 4097 random records plus the hand-made ones, raytrace_range 0.4 w and 2 w; the sensor in the first and the
     last cell, on a cell boundary and off the map; two clearing and two marking observations with different origins in one call;
     n = 0, 1, 63, 64, 65, 4097 at strides 12, 16 and 32; bounds NULL;
  2. stream order: reset_window -> observe -> clear_footprint -> merge -> inflate enqueued without a host wait, read back once;
  3. the device form with torch tensors, and no allocation in a second identical loop;
  4. a plan made before observe is refused as stale;
  5. the error cases (GEM_ERR_INVALID, grid and bounds unchanged);
  6. the C++ facade (tests/cpp/obstacle_check.cpp) as a child process."""
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
import obstacle_ref as ref  # noqa: E402
from test_obstacle_cpu import (EMPTY, GEOMETRIES, LAYER_MAX, ORIGIN, build_obstacle_check, cases, extent, observation, sensor, wanted,  # noqa: E402
                               world)

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
INV = _lib.GEM_OK - 1


@pytest.fixture(scope="module")
def emap():
    m = ElevationMap(32, 0.05)
    yield m
    m.debug_set("obstacle_direct", 1)
    m.close()


def device_copy(m, cm):
    dev = m.costmap(cm.size_x, cm.size_y, cm.res, cm.ox, cm.oy)
    dev.write(cm.grid)
    return dev


def same(dev, want_bytes, what):
    got = dev.read()
    assert got.tobytes() == want_bytes, f"{what}: {int((got.reshape(-1) != np.frombuffer(want_bytes, np.uint8)).sum())} cells differ"


# ---- 1. the cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases()))
def test_cases_in_both_forms(emap, name):
    geom, observations, bounds = cases()[name]
    want_grid, want_bounds = wanted(name)
    base = world(geom)[0]
    assert emap.debug_get("obstacle_direct") == 1                        # the default is the direct form: it measured faster
    for direct in (0, 1):
        emap.debug_set("obstacle_direct", direct)
        dev = device_copy(emap, base)
        try:
            got = dev.observe(list(observations), LAYER_MAX, None if bounds is None else list(bounds))
            assert got == want_bounds, (direct, got, want_bounds)
            same(dev, want_grid, f"obstacle_direct {direct}")
            # a second identical call changes nothing: the bitmaps were left clean
            dev.observe(list(observations), LAYER_MAX)
            same(dev, want_grid, f"obstacle_direct {direct}, again")
        finally:
            dev.close()
            emap.debug_set("obstacle_direct", 1)
    if " n 0 " in name:
        assert want_grid == base.grid.tobytes()
    elif "off the map" not in name and " n 1 " not in name:
        assert want_grid != base.grid.tobytes() and want_bounds != EMPTY


# ---- 2. stream order ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["75x75", "300x260"])
def test_the_enqueued_cycle(emap, geom):
    sx, sy, res = GEOMETRIES[geom]
    base, cloud = world(geom)
    window = (3, 4, sx - 5, sy - 2)
    p = iref.Params(3 * res - 0.05 * res, 2 * res + 0.05 * res, 3.0, False)
    layer_ref, master_ref = cref.Costmap(sx, sy, res, *ORIGIN), cref.Costmap(sx, sy, res, *ORIGIN, cref.FREE_SPACE)
    layer_ref.grid[:] = base.grid
    old = np.random.default_rng(9).integers(1, 254, (sy, sx), dtype=np.uint8)      # what a cycle before left in the master
    master_ref.grid[:] = old
    s = sensor(base)
    obs = [observation(base, cloud, s, 0.4)]
    robot = (s[0], s[1], math.cos(0.3), math.sin(0.3))
    spec = [[-3 * res, -2 * res], [-3 * res, 2 * res], [3 * res, 2 * res], [3 * res, -2 * res]]
    iref.reset_window(master_ref.grid, *window, cref.FREE_SPACE)
    ref.observe(layer_ref, obs, LAYER_MAX)
    assert fref.clear_footprint(layer_ref, robot, spec)
    cref.merge(layer_ref, master_ref, window, cref.MAX)
    master_ref.grid[:] = iref.inflate_exact(master_ref.grid, p, res, window)
    for direct in (0, 1):
        emap.debug_set("obstacle_direct", direct)
        layer, master = device_copy(emap, base), emap.costmap(sx, sy, res, *ORIGIN, cref.FREE_SPACE)
        try:
            master.write(old)
            master.reset_window(*window)                                  # five calls, none of which waits for the device
            assert layer.observe(obs, LAYER_MAX, None) is None
            ok, _ = layer.clear_footprint(robot, spec)
            layer.merge(master, window, cref.MAX)
            master.inflate(p.inflation_radius, p.inscribed_radius, p.cost_scaling_factor, p.inflate_unknown, window)
            same(master, master_ref.grid.tobytes(), "master")
            same(layer, layer_ref.grid.tobytes(), "layer")
            assert ok and (master_ref.grid == 253).any() and (master_ref.grid == 254).any() and (master_ref.grid == 0).any()
        finally:
            layer.close(); master.close()
            emap.debug_set("obstacle_direct", 1)


# ---- 3. device tensors ------------------------------------------------------------------------------------------------------------------
def test_device_tensors_and_a_second_loop_allocates_nothing(emap):
    import torch
    names = ["130x90 range 0.4 w", "300x260 four observations", "75x75 n 65 stride 12", "75x75 n 4097 stride 32"]
    tensors = {n: [torch.from_numpy(o["points"].copy()).to("cuda:0") for o in cases()[n][1]] for n in names}
    devs = {n: device_copy(emap, world(cases()[n][0])[0]) for n in names}

    def loop():
        for direct in (0, 1):
            emap.debug_set("obstacle_direct", direct)
            for n in names:
                geom, observations, bounds = cases()[n]
                devs[n].write(world(geom)[0].grid)
                obs = [{**o, "points": t} for o, t in zip(observations, tensors[n])]
                b = devs[n].observe(obs, LAYER_MAX, None)                 # only enqueued
                assert b is None
                b = devs[n].observe(obs, LAYER_MAX, list(bounds))
                assert b == wanted(n)[1]
                same(devs[n], wanted(n)[0], n)
        emap.debug_set("obstacle_direct", 1)

    try:
        loop()
        a1 = emap.debug_get("arena_allocations")
        loop()
        assert emap.debug_get("arena_allocations") == a1
        # uint8 records are the same records; host and device inputs do not mix; float64 is refused
        n = names[3]
        raw = tensors[n][0].view(torch.uint8).reshape(-1, 32)
        devs[n].write(world("75x75")[0].grid)
        assert devs[n].observe([{**cases()[n][1][0], "points": raw}], LAYER_MAX, list(EMPTY)) == wanted(n)[1]
        same(devs[n], wanted(n)[0], "uint8 records")
        with pytest.raises(ValueError):
            devs[n].observe([{**cases()[n][1][0], "points": tensors[n][0]}, cases()[n][1][0]], LAYER_MAX)
        with pytest.raises(ValueError):
            devs[n].observe([{**cases()[n][1][0], "points": tensors[n][0].double()}], LAYER_MAX)
        emap.synchronize()
    finally:
        emap.debug_set("obstacle_direct", 1)
        for d in devs.values():
            d.close()


# ---- 4. a plan goes stale -----------------------------------------------------------------------------------------------------------------
def test_a_plan_made_before_observe_is_stale(emap):
    base, cloud = world("75x75")
    cm = cref.Costmap(75, 75, 0.2, *ORIGIN)
    cm.grid[:] = 0
    dev = device_copy(emap, cm)
    try:
        start, goal = (ORIGIN[0] + 2.0, ORIGIN[1] + 2.0), (ORIGIN[0] + 11.0, ORIGIN[1] + 9.0)
        path, st = dev.nav_plan(start, goal)
        assert st["found"] and len(path) > 10
        pot, cells = dev.read_potential()
        dev.frontiers()
        dev.observe([], LAYER_MAX)                                        # no observation: nothing changes
        assert dev.read_potential()[0].tobytes() == pot.tobytes()
        dev.observe([observation(base, cloud[:100], sensor(base))], LAYER_MAX)
        with pytest.raises(GemError, match="before the costmap last rolled or was observed"):
            dev.read_potential()
        with pytest.raises(GemError, match="observed"):
            dev.read_frontiers()
        with pytest.raises(GemError):
            dev.nav_plan_to(goal)
        dev.nav_plan(start, goal)                                         # a new plan is good again
        dev.read_potential()
    finally:
        dev.close()


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------------
def test_error_cases_leave_grid_and_bounds_unchanged():
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    base, cloud = world("75x75")
    dev = device_copy(m, base)
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

    def call(obs, n_obs=None, id_=None, layer_max=LAYER_MAX, entry="gem_costmap_observe", handle=None):
        arr = (_lib.Observation * max(len(obs), 1))(*obs)
        return getattr(lib, entry)(handle or h, dev.id if id_ is None else id_, arr if obs else None, len(obs) if n_obs is None else n_obs, layer_max, b)

    def unchanged():
        assert dev.read().tobytes() == base.grid.tobytes() and list(b) == EMPTY

    bad = [one(n=-1), one(n=(1 << 31) - 1), one(point_step=8), one(point_step=14), one(point_step=0), one(flags=0), one(flags=4), one(flags=7),
           one(origin=(nan, 0.0, 0.0)), one(origin=(0.0, inf, 0.0)), one(origin=(0.0, 0.0, -inf)), one(obstacle_range=-1.0), one(obstacle_range=nan),
           one(raytrace_range=-0.5), one(raytrace_range=nan), one(min_obstacle_height=2.5), one(min_obstacle_height=nan),
           one(max_obstacle_height=nan), one(points=None)]
    try:
        for entry in ("gem_costmap_observe", "gem_costmap_observe_device"):
            for o in bad:
                assert call([o], entry=entry) == INV
                assert call([one(n=0, points=None), o], entry=entry) == INV        # wherever it stands in the list
            for id_ in (-1, 5, 8, 1 << 20):
                assert call([one()], id_=id_, entry=entry) == INV
            assert call([one()], n_obs=-1, entry=entry) == INV and call([one()] * 9, entry=entry) == INV and call([], n_obs=1, entry=entry) == INV
            assert call([one()], layer_max=nan, entry=entry) == INV
            half = (1 << 30)                                              # more than 2^31 - 2 records in the call, none alone
            assert call([one(n=half), one(n=half)], entry=entry) == INV
            unchanged()
        w = ElevationMap(32, 0.05)                                        # a handle with a communicator
        w.comm_init_loopback(9561, 1, 0, tile_strips=False)
        assert call([one()], id_=0, handle=w._h) == INV and call([one()], id_=0, handle=w._h, entry="gem_costmap_observe_device") == INV
        w.close()
        unchanged()
        assert lib.gem_debug_set(h, b"obstacle_direct", 2) == INV and lib.gem_debug_set(h, b"obstacle_direct", -1) == INV
        assert m.debug_get("obstacle_direct") == 1
        # what is no error: no observation, no record with NULL points, an infinite range, an infinite layer maximum
        assert call([]) == 0 and call([one(n=0, points=None, flags=1)]) == 0
        unchanged()
        assert call([one(n=0, points=None)]) == 0                         # clearing without a record still touches the sensor
        assert dev.read().tobytes() == base.grid.tobytes() and list(b) == [s[0], s[1], s[0], s[1]]
        b[:] = EMPTY
        assert call([one(raytrace_range=inf, obstacle_range=inf)], layer_max=inf) == 0
        cm = cref.Costmap(75, 75, 0.2, *ORIGIN)
        cm.grid[:] = base.grid
        want_b = list(EMPTY)
        ref.observe(cm, [{"points": pts, "origin": s, "raytrace_range": inf, "obstacle_range": inf}], inf, want_b)
        assert dev.read().tobytes() == cm.grid.tobytes() and list(b) == want_b and cm.grid.tobytes() != base.grid.tobytes()
    finally:
        dev.close()
        m.close()


# ---- 6. the C++ facade ------------------------------------------------------------------------------------------------------------------------
def test_cpp_obstacle_facade(tmp_path):
    exe = build_obstacle_check(tmp_path / "obstacle_check")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
