"""What the costmap layers share (cost_bounds_out and cost_publish of gem_cost_pass.hpp and the element-typed grid kernels on the
device, read_bounds / read_window / write_window on the host), where no layer's own test reaches it.  Every comparison is exact.

  1. the element-wise kernels over both element sizes on one small map: a 5 x 7 costmap with voxels attached, a known pattern in the
     bytes and in the columns; a roll by (2, -1) cells and one by (9, 0), which leaves the map; a 3 x 2 window of either grid read and
     written at a row stride of 5;
  2. bounds[4] across the shared read-back: mark_points, observe (one clearing and one marking observation, either walk form) and
     voxel_observe with mark_threshold 1 (the marks touch behind the apply) on one handle from the same initial bounds, against
     tests/costmap_ref.py and the host twins.  70 x 70 cells take the LDS form of the passes, 70 x 118 (above kCostLdsCells = 8192)
     the global one; every cloud is longer than the 4096 inputs of a workgroup."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import gem_amd
from gem_amd import ElevationMap
from gem_amd.api import POINT_DTYPE

sys.path.insert(0, str(Path(__file__).resolve().parent))
import costmap_ref as cref  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
UNKNOWN_COLUMN = 0x0000FFFF


@pytest.fixture(scope="module")
def emap():
    m = ElevationMap(32, 0.05)
    yield m
    m.close()


# ---- 1. fill, roll and window over bytes and columns ----------------------------------------------------------------------------------
def rolled(a, cell_ox, cell_oy, fill):
    """Costmap2D::updateOrigin's copy: out(x, y) = a(x + cell_ox, y + cell_oy) where that lies in the map, fill elsewhere"""
    sy, sx = a.shape
    out = np.full_like(a, fill)
    for y in range(sy):
        for x in range(sx):
            if 0 <= x + cell_ox < sx and 0 <= y + cell_oy < sy:
                out[y, x] = a[y + cell_oy, x + cell_ox]
    return out


def strided(dev, name, window, array):
    """gem_costmap_read / _write / _voxels_read / _voxels_write of `window` on the rows of `array`, whose row length is the stride"""
    dev._call(name, *window, array.ctypes.data_as(C.c_void_p), array.shape[1])


def test_roll_and_strided_windows_of_bytes_and_columns(emap):
    sx, sy, res, ox, oy = 5, 7, 0.5, 1.0, -2.0
    grid = (np.arange(sx * sy, dtype=np.uint8) + 1).reshape(sy, sx)
    cols = (np.arange(1, sx * sy + 1, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32).reshape(sy, sx)
    window = (1, 2, 4, 4)                                                 # 3 x 2

    def check(what):
        assert dev.read().tobytes() == grid.tobytes() and dev.read_voxels().tobytes() == cols.tobytes(), what
        for name, want, dtype in (("gem_costmap_read", grid, np.uint8), ("gem_costmap_voxels_read", cols, np.uint32)):
            out = np.full((2, 5), 77, dtype)
            strided(dev, name, window, out)
            assert out[:, :3].tobytes() == want[2:4, 1:4].tobytes() and (out[:, 3:] == 77).all(), (what, name)

    dev = emap.costmap(sx, sy, res, ox, oy)
    try:
        dev.attach_voxels(10, 0.2, 0.0, 15, 0)
        assert (dev.read() == cref.NO_INFORMATION).all() and (dev.read_voxels() == UNKNOWN_COLUMN).all()      # the two fills
        dev.write(grid)
        dev.write_voxels(cols)
        check("written")
        for step in ((2, -1), (9, 0)):
            ox, oy = ox + step[0] * res, oy + step[1] * res
            dev.update_origin(ox, oy)
            g = dev.geometry()
            assert (g["origin_x"], g["origin_y"]) == (ox, oy)
            grid, cols = rolled(grid, *step, cref.NO_INFORMATION), rolled(cols, *step, UNKNOWN_COLUMN)
            check(f"rolled by {step}")
        assert (grid == cref.NO_INFORMATION).all() and (cols == UNKNOWN_COLUMN).all()                        # the second roll left the map
        # the window written from rows of 5: the rest of the rows is not the grid's business
        for name, want, dtype in (("gem_costmap_write", grid, np.uint8), ("gem_costmap_voxels_write", cols, np.uint32)):
            rows = (np.arange(10, dtype=np.uint64) * 40503 % 251 + 1).astype(dtype).reshape(2, 5)
            strided(dev, name, window, rows)
            want[2:4, 1:4] = rows[:, :3]
        check("a window written at stride 5")
        assert (grid != cref.NO_INFORMATION).sum() == 6 and (cols != UNKNOWN_COLUMN).sum() == 6
    finally:
        dev.close()


# ---- 2. the bounds of the three layers through one read-back ------------------------------------------------------------------------------
RES, ORIGIN = 0.1, (-3.0, 1.0)
INITIAL = [-100.0, 7.5, 0.75, 100.0]                                      # min_x, min_y, max_x, max_y: every call keeps the outer two and moves the inner two
VOXELS = (10, 0.2, 0.0, 15, 1)                                            # mark_threshold 1


def clouds(sx, sy):
    rng = np.random.default_rng(70)
    w, h = sx * RES, sy * RES
    pts = np.zeros(5000, POINT_DTYPE)                                     # some of them off the map
    pts["x"] = rng.uniform(ORIGIN[0] + 0.3, ORIGIN[0] + w + 0.4, pts.size)
    pts["y"] = rng.uniform(ORIGIN[1] - 0.4, ORIGIN[1] + h - 0.3, pts.size)
    pts["travers"] = rng.uniform(0.0, 1.0, pts.size)
    sensor = (ORIGIN[0] + 0.4 * w, ORIGIN[1] + 0.55 * h, 0.6)

    def sweep(n, reach):
        p = np.zeros((n, 4), np.float32)
        p[:, 0] = sensor[0] + rng.uniform(-reach, reach, n)
        p[:, 1] = sensor[1] + rng.uniform(-reach, reach, n)
        p[:, 2] = rng.uniform(-0.1, 1.9, n)
        return p

    common = {"origin": sensor, "obstacle_range": 2.5, "raytrace_range": 3.0, "min_obstacle_height": 0.0, "max_obstacle_height": 1.8}
    obs = [{**common, "points": sweep(4500, 2.0), "marking": False, "clearing": True},
           {**common, "points": sweep(4300, 1.5), "marking": True, "clearing": False}]
    return pts, obs


@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("size", [(70, 70), (70, 118)])
def test_bounds_of_mark_observe_and_voxel_observe(emap, size, direct):
    sx, sy = size
    pts, obs = clouds(sx, sy)
    want = cref.Costmap(sx, sy, RES, *ORIGIN)
    cols = np.full((sy, sx), UNKNOWN_COLUMN, np.uint32)
    dev = emap.costmap(sx, sy, RES, *ORIGIN)
    before = emap.debug_get("obstacle_direct")
    emap.debug_set("obstacle_direct", direct)
    try:
        dev.attach_voxels(*VOXELS)
        b = cref.mark_points(want, pts, 0.5, list(INITIAL))
        assert dev.mark_points(pts, 0.5, list(INITIAL)) == b and b != INITIAL
        assert dev.read().tobytes() == want.grid.tobytes()
        b = gem_amd.obstacle_host(want.grid, RES, ORIGIN, obs, 1.5, list(INITIAL))
        assert dev.observe(obs, 1.5, list(INITIAL)) == b and b != INITIAL
        assert dev.read().tobytes() == want.grid.tobytes()
        b = gem_amd.voxlayer_host(want.grid, cols, RES, ORIGIN, VOXELS, obs, 1.5, list(INITIAL))
        assert dev.voxel_observe(obs, 1.5, list(INITIAL)) == b and b != INITIAL
        assert dev.read().tobytes() == want.grid.tobytes() and dev.read_voxels().tobytes() == cols.tobytes()
        assert (want.grid == cref.LETHAL_OBSTACLE).any() and (want.grid == cref.FREE_SPACE).any()
        # nothing accepted: the caller's bounds come back as they went in, from all three
        far = np.zeros(1, POINT_DTYPE)
        far["x"] = 1e6
        nothing = [{**obs[1], "points": np.full((1, 4), 1e6, np.float32)}]
        assert dev.mark_points(far, 0.5, list(INITIAL)) == INITIAL and dev.observe(nothing, 1.5, list(INITIAL)) == INITIAL
        assert dev.voxel_observe(nothing, 1.5, list(INITIAL)) == INITIAL
    finally:
        emap.debug_set("obstacle_direct", before)
        dev.close()
