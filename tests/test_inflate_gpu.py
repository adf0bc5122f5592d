"""Inflation on the device costmap (gem_costmap_inflate, gem_costmap_reset_window) against inflate_exact of tests/inflate_ref.py.  Every
comparison is exact: grids by tobytes(), trajectory costs as integers.

  1. small grids that are multiples of no tile (75 x 75, 130 x 90), one cell wide or high (1 x 200, 200 x 1) and smaller than the radius
     (5 x 5 with R = 11), R = 1, 2, 11, 64, 127, both values of inflate_unknown, NO_INFORMATION inside and outside the inscribed radius,
     old costs above and below the new one;
  2. 1000 x 1000 with fewer than 300 seeds: on the four borders, in the corners, a pair across every 64-cell boundary; R = 11 and 64;
  3. windows: the whole map, an interior one with a seed exactly R outside it (inflates) and one R + 1 outside (does not), a corner, an
     empty one; twice equals once; no seed and all seeds leave the grid as it is;
  4. reset_window: the whole map, slivers, whole rows;
  5. the enqueued cycle mark -> clear footprint -> reset window -> merge -> inflate -> score with no host wait in between, and no
     allocation in a second identical loop;
  6. the error cases (GEM_ERR_INVALID, grid unchanged);
  7. the C++ facade (tests/cpp/inflate_check.cpp) as a child process."""
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
import inflate_ref as ref  # noqa: E402
from test_costmap_gpu import lattice_cloud  # noqa: E402
from test_inflate_cpu import RES, build_inflate_check, noise_grid, params_for  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
GEOMETRIES = {"75x75": (75, 75), "130x90": (130, 90), "1x200": (1, 200), "200x1": (200, 1)}      # size_x, size_y
RADII = [1, 2, 11, 64, 127]
INV = _lib.GEM_OK - 1
THRESH = 0.5


@pytest.fixture(scope="module")
def emap():
    m = ElevationMap(32, 0.05)
    yield m
    m.close()


def params(R, inflate_unknown=False):
    """2.4 cells inscribed; a scaling factor under which the costs reach the radius's end above zero"""
    return params_for(R, inscribed=0.12, weight=3.0 if R <= 11 else 0.5, inflate_unknown=inflate_unknown)


@functools.lru_cache(maxsize=None)
def world(geom):
    """a noise grid of the geometry: bytes 0 .. 252, a tenth 255, 0.6 % 254 and one in the first and the last cell; never changed"""
    sx, sy = GEOMETRIES[geom]
    g = noise_grid(np.random.default_rng(sx * 1000 + sy), sx, sy, 0.006)
    g[0, 0] = g[sy - 1, sx - 1] = 254
    g.setflags(write=False)
    return g


def device_copy(m, grid, default_value=_lib.COST_NO_INFORMATION):
    dev = m.costmap(grid.shape[1], grid.shape[0], RES, -3.1, 2.7, default_value)
    dev.write(grid)
    return dev


def inflate_dev(dev, p, window=None):
    dev.inflate(p.inflation_radius, p.inscribed_radius, p.cost_scaling_factor, p.inflate_unknown, window)


def same(dev, want, what=""):
    got = dev.read()
    assert got.tobytes() == want.tobytes(), f"{what}: {int((got != want).sum())} cells differ"


# ---- 1. small grids -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_small_grids(emap, geom, R):
    g = world(geom)
    for unknown in (False, True):
        p = params(R, unknown)
        want, d2 = ref.inflate_exact(g, p, RES, None, True)
        dev = device_copy(emap, g)
        try:
            inflate_dev(dev, p)
            same(dev, want, f"{geom} R {R} unknown {unknown}")
            inflate_dev(dev, p)                                           # twice equals once
            same(dev, want, "twice")
        finally:
            dev.close()
        hit = d2 != ref.NONE
        assert hit.any() and (want != g).any()
        if R >= 11 and min(g.shape) > 1:                                  # the cases of the rule all occur
            cost = ref.table(p, RES)[1][np.where(hit, d2, 0)]
            was_unknown = hit & (g == 255)
            assert (was_unknown & (want == 253)).any() and (was_unknown & (cost < 253) & (want == (cost if unknown else 255))).any()
            assert (hit & (g < 253) & (g > cost)).any() and (hit & (g < cost)).any()


def test_a_map_smaller_than_the_radius(emap):
    g = np.array([[0, 0, 0, 0, 255], [0, 0, 0, 254, 0], [7, 0, 0, 0, 0], [0, 0, 200, 0, 0], [255, 0, 0, 0, 0]], np.uint8)
    for R in (11, 127):
        for unknown in (False, True):
            p = params(R, unknown)
            dev = device_copy(emap, g)
            try:
                inflate_dev(dev, p)
                same(dev, ref.inflate_exact(g, p, RES), f"5x5 R {R}")
            finally:
                dev.close()


@pytest.mark.parametrize("R", [63, 64, 65, 127])
def test_a_lone_seed_reaches_exactly_R_along_its_row(emap, R):
    """the row pass takes a row's seeds from two pairs of 64-bit words: the distances 63, 64 and 65 lie on either side of the first pair"""
    g = np.full((3, 300), 3, np.uint8)
    g[1, 150] = 254
    p = params(R)
    want = ref.inflate_exact(g, p, RES)
    assert want[1, 150 - R] > 3 and want[1, 150 + R] > 3 and want[1, 150 - R - 1] == 3 and want[1, 150 + R + 1] == 3
    dev = device_copy(emap, g)
    try:
        inflate_dev(dev, p)
        same(dev, want, f"R {R}")
    finally:
        dev.close()


# ---- 2. the large grid ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def large_world():
    rng = np.random.default_rng(1000)
    n = 1000
    g = rng.integers(0, 253, (n, n), dtype=np.uint8)
    g[rng.random((n, n)) < 0.1] = 255
    seeds = [(0, 0), (n - 1, 0), (0, n - 1), (n - 1, n - 1)]                                       # the corners
    seeds += [(int(rng.integers(1, n - 1)), e) for e in (0, n - 1) for _ in range(6)]              # the borders
    seeds += [(e, int(rng.integers(1, n - 1))) for e in (0, n - 1) for _ in range(6)]
    for k in range(1, 16):                                                                          # a pair across every 64-cell boundary
        y, x = int(rng.integers(0, n)), int(rng.integers(0, n))
        seeds += [(64 * k - 1, y), (64 * k, y), (x, 64 * k - 1), (x, 64 * k)]
    seeds += [(int(rng.integers(0, n)), int(rng.integers(0, n))) for _ in range(150)]
    assert len(set(seeds)) < 300
    for x, y in seeds:
        g[y, x] = 254
    g.setflags(write=False)
    return g


@pytest.mark.parametrize("R", [11, 64])
def test_large_grid(emap, R):
    g = large_world()
    assert (g == 254).sum() < 300
    for unknown in (False, True):
        p = params(R, unknown)
        want = ref.inflate_exact(g, p, RES)
        dev = device_copy(emap, g)
        try:
            inflate_dev(dev, p)
            same(dev, want, f"1000x1000 R {R} unknown {unknown}")
        finally:
            dev.close()
        assert (want != g).sum() > 20000


# ---- 3. windows -----------------------------------------------------------------------------------------------------------------------
def test_windows(emap):
    R = 11
    g = np.array(world("130x90"))
    g[g == 254] = 17                                                      # only the seeds placed here
    window = (40, 30, 80, 60)
    inside, at_R, beyond, corner = (60, 45), (40 - R, 44), (79 + R + 1, 46), (3, 2)
    for x, y in (inside, at_R, beyond, corner):
        g[y, x] = 254
    for unknown in (False, True):
        p = params(R, unknown)
        dev = device_copy(emap, g)
        try:
            # an empty window: nothing
            for w in ((50, 40, 50, 70), (50, 40, 90, 40), (0, 0, 0, 0), (130, 90, 130, 90)):
                inflate_dev(dev, p, w)
                same(dev, g, f"empty {w}")
            # the interior window: the seed R cells left of its first column inflates, the one R + 1 right of its last column does not
            want = ref.inflate_exact(g, p, RES, window)
            inflate_dev(dev, p, window)
            same(dev, want, "interior")
            near = lambda c, a: a[c[1] - 2:c[1] + 3, c[0] - 2:c[0] + 3]   # noqa: E731
            assert (near(at_R, want) != near(at_R, g)).any() and (near(inside, want) != near(inside, g)).any()
            assert (near(beyond, want) == near(beyond, g)).all() and (near(corner, want) == near(corner, g)).all()
            assert want[at_R[1], 0:at_R[0] - R].tobytes() == g[at_R[1], 0:at_R[0] - R].tobytes()
            assert (want[at_R[1], at_R[0] - 3:at_R[0]] != g[at_R[1], at_R[0] - 3:at_R[0]]).any()    # cells outside the widened window change
            # a corner window on top, then the whole map: each from the grid the call before left
            want = ref.inflate_exact(want, p, RES, (0, 0, 10, 10))
            inflate_dev(dev, p, (0, 0, 10, 10))
            same(dev, want, "corner")
            assert (near((4, 4), want) != near((4, 4), g)).any()
            want = ref.inflate_exact(want, p, RES, None)
            inflate_dev(dev, p, None)
            same(dev, want, "whole")
            assert want.tobytes() == ref.inflate_exact(g, p, RES, None).tobytes()
        finally:
            dev.close()


@pytest.mark.parametrize("R", [11, 127])
def test_no_seed_and_all_seeds_leave_the_grid(emap, R):
    none = np.array(world("75x75"))
    none[none == 254] = 253
    full = np.full((75, 75), 254, np.uint8)
    for g in (none, full):
        dev = device_copy(emap, g)
        try:
            for unknown in (False, True):
                inflate_dev(dev, params(R, unknown))
                same(dev, g)
        finally:
            dev.close()
    assert ref.inflate_exact(full, params(R), RES).tobytes() == full.tobytes()


# ---- 4. reset_window ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["130x90", "1x200"])
def test_reset_window(emap, geom):
    g = np.array(world(geom))
    sx, sy = GEOMETRIES[geom]
    dev = device_copy(emap, g, 9)
    try:
        windows = [(sx // 2, 3, sx // 2 + 1, sy - 5), (0, sy // 2, sx, sy // 2 + 1), (0, 10, sx, 25), (sx, sy, sx, sy), (0, 5, 0, 9)]
        for w in windows + [(0, 0, sx, sy)]:                              # slivers, whole rows, empty ones, then the whole map
            ref.reset_window(g, *w, 9)
            dev.reset_window(*w)
            same(dev, g, f"reset {w}")
        assert (g == 9).all()
    finally:
        dev.close()


# ---- 5. the cycle -----------------------------------------------------------------------------------------------------------------------
def test_the_enqueued_cycle_and_a_second_loop_allocates_nothing(emap):
    sx = sy = 75
    res, origin = 0.2, (-3.1, 2.7)
    window = (5, 4, 70, 72)
    p = ref.Params(0.55, 0.41, 3.0, False)                                # R = 3; up to two cells away is inscribed
    assert ref.cells(p, res) == 3
    rng = np.random.default_rng(5)
    layer_ref, master_ref = cref.Costmap(sx, sy, res, *origin), cref.Costmap(sx, sy, res, *origin, cref.FREE_SPACE)
    layer, master = emap.costmap(sx, sy, res, *origin), emap.costmap(sx, sy, res, *origin, cref.FREE_SPACE)
    stale = rng.integers(1, 254, (sy, sx), dtype=np.uint8)                # what a cycle before left in the master
    T, n_traj = 5, 200
    xyt = np.stack([rng.uniform(origin[0] + 3.0, origin[0] + 12.0, T * n_traj), rng.uniform(origin[1] + 3.0, origin[1] + 12.0, T * n_traj),
                    rng.uniform(-np.pi, np.pi, T * n_traj)], axis=1)
    poses = fref.poses_from_yaw(xyt)
    robot = (origin[0] + 7.5, origin[1] + 7.5, math.cos(0.3), math.sin(0.3))
    clouds = [lattice_cloud(rng, 3000, layer_ref) for _ in range(2)]

    def loop():
        out = []
        for pts in clouds:
            master_ref.grid[:] = stale
            master.write(stale)
            cref.mark_points(layer_ref, pts, THRESH)
            assert fref.clear_footprint(layer_ref, robot, fref.RECTANGLE)
            ref.reset_window(master_ref.grid, *window, cref.FREE_SPACE)
            cref.merge(layer_ref, master_ref, window, cref.MAX)
            before = fref.score_trajectories(fref.footprint_cost(master_ref, poses, fref.RECTANGLE, fref.INSCRIBED_LETHAL), T, 0)
            master_ref.grid[:] = ref.inflate_exact(master_ref.grid, p, res, window)
            want = fref.score_trajectories(fref.footprint_cost(master_ref, poses, fref.RECTANGLE, fref.INSCRIBED_LETHAL), T, 0)
            # the device: six calls, nothing waits before the scores come back
            layer.mark_points(pts, THRESH, None)
            ok, _ = layer.clear_footprint(robot, fref.RECTANGLE)
            master.reset_window(*window)
            layer.merge(master, window, cref.MAX)
            master.inflate(p.inflation_radius, p.inscribed_radius, p.cost_scaling_factor, p.inflate_unknown, window)
            got = master.score_trajectories(poses, T, fref.RECTANGLE, fref.INSCRIBED_LETHAL)
            assert ok and got.tolist() == want.tolist()
            same(master, master_ref.grid, "master")
            same(layer, layer_ref.grid, "layer")
            assert (master_ref.grid == 253).any() and (master_ref.grid[window[1]:window[3], window[0]:window[2]] == 0).any()
            assert (master_ref.grid[0:4] == stale[0:4]).all()             # outside the window (and its reach) the old costs stay
            only_inflation = (before >= 0) & (want == -1)
            assert only_inflation.any() and (want >= 0).any()             # a 253 that only the inflation produced decides
            out.append(got.tolist())
        return out

    try:
        first = loop()
        a1 = emap.debug_get("arena_allocations")
        second = loop()
        assert emap.debug_get("arena_allocations") == a1
        assert len(first) == len(second) == 2
    finally:
        layer.close(); master.close()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------
def test_error_cases_leave_the_grid_unchanged():
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    g = world("75x75")
    dev = device_copy(m, g)
    nan, inf = float("nan"), float("inf")
    good = (11 * RES - 0.01, 0.12, 3.0, 0)

    def inflate(id_=None, p=good, w=(0, 0, 75, 75)):
        s = None if p is None else C.byref(_lib.InflationParams(*p))
        return lib.gem_costmap_inflate(h, dev.id if id_ is None else id_, s, *w)

    def reset(id_=None, w=(0, 0, 75, 75)):
        return lib.gem_costmap_reset_window(h, dev.id if id_ is None else id_, *w)

    bad_windows = [(-1, 0, 10, 10), (0, -1, 10, 10), (0, 0, 76, 10), (0, 0, 10, 76), (11, 0, 10, 10), (0, 11, 10, 10), (0, 0, 1 << 30, 5)]
    try:
        for bad in (-1, 5, 8, 1 << 20):
            assert inflate(id_=bad) == INV and reset(id_=bad) == INV
        assert inflate(p=None) == INV
        for k in range(3):
            for v in (nan, inf, -inf, -0.01):
                q = list(good); q[k] = v
                assert inflate(p=tuple(q)) == INV, (k, v)
        assert inflate(p=(127.5 * RES, 0.12, 3.0, 0)) == INV                # 128 cells
        for w in bad_windows:
            assert inflate(w=w) == INV and reset(w=w) == INV, w
        w2 = ElevationMap(32, 0.05)                                       # a handle with a communicator
        w2.comm_init_loopback(9541, 1, 0, tile_strips=False)
        assert w2._lib.gem_costmap_inflate(w2._h, 0, C.byref(_lib.InflationParams(*good)), 0, 0, 75, 75) == INV
        assert w2._lib.gem_costmap_reset_window(w2._h, 0, 0, 0, 75, 75) == INV
        w2.close()
        same(dev, g, "after the errors")
        assert inflate(p=(0.0, 0.12, 3.0, 0)) == 0                         # R == 0 is fine and changes nothing
        same(dev, g, "R = 0")
        assert inflate() == 0                                              # (the arguments are good ones)
        same(dev, ref.inflate_exact(g, params(11), RES), "good")
    finally:
        dev.close()
        m.close()


# ---- 7. the C++ facade ------------------------------------------------------------------------------------------------------------------
def test_cpp_inflate_facade(tmp_path):
    exe = build_inflate_check(tmp_path / "inflate_check")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
