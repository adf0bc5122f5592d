"""The costmap layers on the device (gem_costmap_*) against the restatement of tests/costmap_ref.py.  Every comparison is exact: byte
grids by tobytes(), bounds and origins by == on doubles.

  1. PointMapLayer's loop over clouds on a 0.05 m lattice rasterised into 0.2 m cells, travers around the threshold (some exactly
     on it, NaN, +-inf), records outside on all four sides, on both edges, at NaN / inf coordinates; map sizes 1 x 1 .. 1000 x 1000
     and both sides of the implementation's one size switch; n = 0, 1, 63, 64, 65, 2e6; reversed; three times;
  2. a million records into one cell, alternating verdicts;
  3. mark_points_device, mark_grid_cloud, mark_global(i) and (-1) against mark_points of what the export calls return;
  4. ElevationMapLayer's loop (mark_visual) after a node-ordered frame loop, against the restatement driven from gem_show's traver
     plane and the capture geometry;
  5. rolling through all eight headings, interleaved with marks; roll_to against update_origin;
  6. merge in both modes, read and write over windows and strides;
  7. bounds NULL + gem_synchronize, and no allocation in a second identical loop;
  8. the error cases (GEM_ERR_INVALID, the grid unchanged);
  9. the C++ gem::Costmap (tests/cpp/costmap_facade_check.cpp) as a child process."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gem_amd import ElevationMap, _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import costmap_ref as ref  # noqa: E402
from local_ref import POINT  # noqa: E402
from test_costmap_cpu import build_costmap_facade_check  # noqa: E402
from test_local_map_gpu import HEADINGS, Pair, trajectory  # noqa: E402

# (no map is fused by most of these tests, and where one is its traversability comes from the oracle: nothing depends on the pipeline knobs)
pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
F32 = np.float32
FREE, LETHAL, NOINFO = ref.FREE_SPACE, ref.LETHAL_OBSTACLE, ref.NO_INFORMATION
THRESH = 0.5
EMPTY = [1e30, 1e30, -1e30, -1e30]                       # the bounds LayeredCostmap::updateMap starts from
# The implementation's only size-dependent switch (gem_costmap.hpp, kCostLdsCells = 8192): a costmap of at most that many cells
# keeps its stamps in LDS per workgroup, a larger one sends them to global memory.  128 x 64 = 8192 is the last LDS size, 128 x 65
# the first global one; 1 x 1, 75 x 40 and 75 x 75 lie below it, 1000 x 1000 above.
SIZES = [(1, 1), (75, 40), (75, 75), (128, 64), (128, 65), (1000, 1000)]
COUNTS = [0, 1, 63, 64, 65, 2_000_000]
ORIGIN = (-7.25, 4.125)                                  # floats: a record can sit exactly on an edge


def lattice_cloud(rng, n, cm):
    """n records on a 0.05 m lattice with jitter, bunched on a patch of about n / 16 costmap cells (so that nearly every marked cell
    sees both verdicts), travers scattered around the threshold; from 63 records on, twelve of them are the special ones."""
    out = np.zeros(n, POINT)
    if n == 0:
        return out
    side = max(1, int(np.ceil(np.sqrt(n / 16))))
    cx, cy = min(side, cm.size_x), min(side, cm.size_y)                  # the patch, in costmap cells, from the map's middle on
    x0 = cm.ox + cm.res * ((cm.size_x - cx) // 2)
    y0 = cm.oy + cm.res * ((cm.size_y - cy) // 2)
    fine = 0.05
    kx, ky = rng.integers(0, int(round(cx * cm.res / fine)), n), rng.integers(0, int(round(cy * cm.res / fine)), n)
    jit = lambda: np.where(rng.random(n) < 0.3, 0.0, rng.uniform(0.1, 0.9, n) * fine)     # some exactly on the lattice lines
    out["x"], out["y"] = (x0 + fine * kx + jit()).astype(F32), (y0 + fine * ky + jit()).astype(F32)
    out["z"], out["pad"] = rng.uniform(-1, 2, n).astype(F32), 1.0
    t = rng.uniform(THRESH - 0.3, THRESH + 0.3, n)
    t[rng.random(n) < 0.05] = THRESH                                     # exactly the threshold: lethal in this layer
    t[rng.random(n) < 0.03] = np.nan
    t[rng.random(n) < 0.01] = np.inf
    t[rng.random(n) < 0.01] = -np.inf
    out["travers"] = t.astype(F32)
    if n >= 63:
        ex, ey = cm.ox + cm.size_x * cm.res, cm.oy + cm.size_y * cm.res  # the far edges: out
        mid_x, mid_y = cm.ox + 0.5 * cm.size_x * cm.res, cm.oy + 0.5 * cm.size_y * cm.res
        special = [(cm.ox - 0.01, mid_y), (ex + 0.01, mid_y), (mid_x, cm.oy - 0.01), (mid_x, ey + 0.01),     # outside, four sides
                   (cm.ox, cm.oy), (ex, mid_y), (mid_x, ey), (float(np.nextafter(F32(cm.ox), F32(-1e9))), mid_y),   # on the edges
                   (np.nan, mid_y), (mid_x, np.inf), (-np.inf, mid_y), (np.nan, np.nan)]
        at = np.linspace(0, n - 1, len(special)).astype(int)             # (the first and the last record among them)
        for i, (sx, sy) in zip(at, special):
            out["x"][i], out["y"][i] = sx, sy
        # the second record and the last but one share a cell with opposite verdicts: whatever else happens, in order that cell
        # ends lethal and in reverse free (on a 1 x 1 map this is the whole answer)
        out["x"][1], out["y"][1] = out["x"][n - 2], out["y"][n - 2]
        out["travers"][1], out["travers"][n - 2] = THRESH + 0.25, THRESH - 0.25
    return out


def middle(values):
    """a threshold that IS one of the values (so the comparison at equality is exercised) with about half of them on either side"""
    v = np.sort(np.asarray(values, np.float64)[np.isfinite(values)])
    return float(v[v.size // 2])


def device_costmap(m, cm, default=NOINFO):
    return m.costmap(cm.size_x, cm.size_y, cm.res, cm.ox, cm.oy, default)


def same(dev, cm):
    g = dev.geometry()
    assert (g["origin_x"], g["origin_y"], g["size_x"], g["size_y"]) == (cm.ox, cm.oy, cm.size_x, cm.size_y)
    got = dev.read()
    assert got.shape == cm.grid.shape and got.tobytes() == cm.grid.tobytes(), f"{int((got != cm.grid).sum())} cells differ"


@pytest.fixture(scope="module")
def emap():
    m = ElevationMap(32, 0.05)
    yield m
    m.close()


# ---- 1. points --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_points(emap, size, n):
    rng = np.random.default_rng(1000 * size[0] + size[1] + n)
    cm = ref.Costmap(size[0], size[1], 0.2, *ORIGIN)
    pts = lattice_cloud(rng, n, cm)
    marked, both = ref.verdict_mix(cm, *ref.point_inputs(pts, THRESH))
    print(f"size {size} n {n}: {marked} cells marked, {both} with both verdicts")
    if n >= 63:                                          # (fewer records cannot give a cell two verdicts)
        assert marked > 0 and 2 * both >= marked         # last-writer-wins is what decides, by the restatement alone
    want_b = ref.mark_points(cm, pts, THRESH, list(EMPTY))
    rev = ref.Costmap(size[0], size[1], 0.2, *ORIGIN)
    want_rb = ref.mark_points(rev, pts[::-1], THRESH, list(EMPTY))
    if n >= 63:
        assert rev.grid.tobytes() != cm.grid.tobytes()   # the reversed cloud has a different answer
    dev = device_costmap(emap, cm)
    try:
        grids = []
        for _ in range(3):
            dev.reset()
            b = dev.mark_points(pts, THRESH, list(EMPTY))
            assert b == want_b, (b, want_b)
            same(dev, cm)
            grids.append(dev.read().tobytes())
        assert grids[0] == grids[1] == grids[2]
        dev.reset()
        b = dev.mark_points(pts[::-1], THRESH, list(EMPTY))
        assert b == want_rb
        same(dev, rev)
        # onto what is there: cells no record touches keep their value; bounds that already hold values are merged
        more = lattice_cloud(rng, min(n, 5000), cm)
        start = [cm.ox + 0.3, -1e30, 1e30, cm.oy + 0.1]
        assert dev.mark_points(more, 0.45, list(start)) == ref.mark_points(rev, more, 0.45, list(start))
        same(dev, rev)
    finally:
        dev.close()


# ---- 2. one cell ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(75, 75), (1000, 1000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_cell_a_million_records(emap, size):
    n = 1_000_000
    cm = ref.Costmap(size[0], size[1], 0.2, *ORIGIN)
    rng = np.random.default_rng(5)
    pts = np.zeros(n, POINT)
    pts["x"] = (cm.ox + 0.2 * 17 + rng.uniform(0.01, 0.19, n)).astype(F32)
    pts["y"] = (cm.oy + 0.2 * 23 + rng.uniform(0.01, 0.19, n)).astype(F32)
    pts["travers"] = np.where(np.arange(n) % 2 == 0, 0.9, 0.1).astype(F32)       # free, lethal, free, ... : the last is lethal
    dev = device_costmap(emap, cm)
    try:
        for cloud, want in ((pts, LETHAL), (pts[:-1], FREE)):
            c = ref.Costmap(size[0], size[1], 0.2, *ORIGIN)
            wb = ref.mark_points(c, cloud, THRESH, list(EMPTY))
            assert c.grid[23, 17] == want and (c.grid != NOINFO).sum() == 1
            dev.reset()
            assert dev.mark_points(cloud, THRESH, list(EMPTY)) == wb
            same(dev, c)
    finally:
        dev.close()


# ---- 3. the inputs that live on the device --------------------------------------------------------------------------------------------
def test_device_grid_cloud_and_global_inputs(oracle_mod):
    import torch
    L, res = 48, 0.1
    p = Pair(oracle_mod, L, res)
    p.gpu.global_enable(1 << 12)
    cm = ref.Costmap(20, 20, 0.2, -2.1, -1.9)            # 4 m: smaller than the 4.8 m map, so some records fall outside
    layer, other = device_costmap(p.gpu, cm), device_costmap(p.gpu, cm)
    rng = np.random.default_rng(9)

    def both_ways(mark, records, thr, what):
        """`mark` on `layer` == mark_points of `records` on `other` == the restatement"""
        c = ref.Costmap(cm.size_x, cm.size_y, cm.res, cm.ox, cm.oy)
        want = ref.mark_points(c, records, thr, list(EMPTY))
        layer.reset(); other.reset()
        assert mark(list(EMPTY)) == want, what
        assert other.mark_points(records, thr, list(EMPTY)) == want, what
        same(layer, c); same(other, c)
        return c

    for k, xy in enumerate(trajectory(16)):
        shift = p.move(xy)
        p.add(k, xy)
        p.capture(p.feature(), k)
        if k == 0:
            p.keep_previous()
        if p.gate(shift):
            p.spill(shift, k)
        g = p.gpu.local_grid_cloud()
        thr = middle(g["travers"])
        c = both_ways(lambda b: layer.mark_grid_cloud(thr, b), g, thr, f"grid cloud, frame {k}")
        if k == 15:
            assert g.size > 500 and (c.grid == LETHAL).sum() > 10 and (c.grid == FREE).sum() > 10
            d = torch.from_numpy(g.view(np.uint8).reshape(-1, 32).copy()).to("cuda:0")
            both_ways(lambda b: layer.mark_points(d, thr, b), g, thr, "mark_points_device")
        if k % 8 == 7:
            p.gpu.global_push_local(True)
            p.local.clear()
        p.raytracing()
        p.keep_previous()
    # two caller pushes that overlap the pushed submaps and each other, with their own verdicts
    for _ in range(2):
        p.gpu.global_push(lattice_cloud(rng, 20000, cm))
    S = p.gpu.global_count()
    assert S == 4
    for i in list(range(S)) + [-1]:
        recs = p.gpu.global_export(i)
        assert recs.size > 100
        thr = middle(recs["travers"])
        both_ways(lambda b: layer.mark_global(i, thr, b), recs, thr, f"submap {i}")
    layer.close(); other.close()


# ---- 4. the visual map ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,explicit", [(48, False), (49, True), (49, False), (48, True)])
def test_mark_visual_after_a_frame_loop(oracle_mod, L, explicit):
    res = 0.1
    p = Pair(oracle_mod, L, res, explicit=explicit)
    cm = ref.Costmap(20, 20, 0.2, -2.1, -1.9, FREE if explicit else NOINFO)
    dev = device_costmap(p.gpu, cm, cm.default)
    from_nan = 0
    for k, xy in enumerate(trajectory(24)):
        p.move(xy)
        p.add(k, xy)
        p.capture(p.feature(), k)                                         # move, add, map_feature, capture
        # the restatement's input: the traver plane of gem_show with the geometry the capture was taken with -- not the records
        if explicit:
            length, r = L * res + 0.125 * (k % 3), res
            pos = (float(p.center[0]) + 0.013, float(p.center[1]) - 0.021)
            plane = p.gpu.show(length, r, pos)["visual"][4]
        else:
            r = float(F32(res))
            length, pos = L * r, (float(p.center[0]), float(p.center[1]))
            plane = p.gpu.show()["visual"][4]
        geom = ref.VisualGeom(L, length, r, pos, p.gpu.pose()[1])
        ref.roll_to(cm, float(xy[0]), float(xy[1])); dev.roll_to(float(xy[0]), float(xy[1]))
        before = cm.grid.copy()
        thr = middle(plane)                                               # one kept cell sits exactly on it: free in this layer
        want = ref.mark_visual(cm, plane, geom, thr, list(EMPTY))
        assert dev.mark_visual(thr, list(EMPTY)) == want, f"frame {k}"
        same(dev, cm)
        # cells that are free only because a NaN cell was visited last: marking the kept cells alone leaves them different
        kept = ref.Costmap(cm.size_x, cm.size_y, cm.res, cm.ox, cm.oy); kept.grid = before
        px, py, lethal = ref.visual_inputs(plane, geom, thr)
        keep = ~np.isnan(np.asarray(plane, F32).reshape(-1))
        ref.write(kept, px[keep], py[keep], lethal[keep])
        from_nan += int(((cm.grid == FREE) & (kept.grid != FREE)).sum())
        p.raytracing()
        p.keep_previous()
    assert (cm.grid == LETHAL).sum() > 10 and (cm.grid == FREE).sum() > 10
    assert from_nan > 0, "no FREE_SPACE cell came from a NaN cell"
    dev.close()


# ---- 5. rolling -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(75, 75), (130, 90)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rolling_through_all_headings(emap, size):
    rng = np.random.default_rng(size[0])
    cm = ref.Costmap(size[0], size[1], 0.2, *ORIGIN, FREE if size[0] == 75 else NOINFO)
    a, b = device_costmap(emap, cm, cm.default), device_costmap(emap, cm, cm.default)     # a by roll_to, b by update_origin
    mx, my = cm.size_in_meters()
    robot = np.array([cm.ox + mx / 2, cm.oy + my / 2])
    steps = [0.07, 0.19, 0.2, 0.33, 1.7, 0.21 * size[0], 0.2 * size[0] + 3.0]          # sub-cell, one cell, multi-cell, beyond the map
    try:
        k = 0
        for d in HEADINGS + HEADINGS[::-1]:
            for s in steps:
                robot = robot + s * np.array(d, float)
                ref.roll_to(cm, robot[0], robot[1])
                a.roll_to(robot[0], robot[1])
                b.update_origin(robot[0] - mx / 2, robot[1] - my / 2)
                same(a, cm); same(b, cm)
                pts = lattice_cloud(rng, 3000, cm)
                want = ref.mark_points(cm, pts, THRESH, list(EMPTY))
                assert a.mark_points(pts, THRESH, list(EMPTY)) == want and b.mark_points(pts, THRESH, list(EMPTY)) == want
                same(a, cm); same(b, cm)
                k += 1
        assert k == 16 * len(steps)
    finally:
        a.close(); b.close()


# ---- 6. merge, read, write --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [ref.OVERWRITE, ref.MAX])
def test_merge_read_write(emap, mode):
    rng = np.random.default_rng(21 + mode)
    sx, sy = 75, 40
    layer, master = ref.Costmap(sx, sy, 0.2, *ORIGIN), ref.Costmap(sx, sy, 0.2, *ORIGIN, FREE)
    dl, dm = device_costmap(emap, layer), device_costmap(emap, master, FREE)
    try:
        pts = lattice_cloud(rng, 40000, layer)
        ref.mark_points(layer, pts, THRESH); dl.mark_points(pts, THRESH)
        layer.grid[5:9, :] = NOINFO; dl.write(layer.grid[5:9, 10:30], (10, 5, 30, 9))   # some unknown cells inside the marked patch
        layer.grid[5:9, :10] = dl.read((0, 5, 10, 9)); layer.grid[5:9, 30:] = dl.read((30, 5, sx, 9))
        same(dl, layer)
        assert all((layer.grid == v).any() for v in (FREE, LETHAL, NOINFO))
        for window in ((0, 0, sx, sy), (7, 3, 61, 33), (0, 0, 0, 0), (74, 39, 75, 40)):
            master.grid[:] = rng.choice(np.array([FREE, 100, LETHAL, NOINFO], np.uint8), (sy, sx))       # what other layers left
            dm.write(master.grid)
            same(dm, master)
            ref.merge(layer, master, window, mode)
            dl.merge(dm, window, mode)
            same(dm, master); same(dl, layer)
        # partial windows with a row stride wider than the window; the bytes beyond the width are not written
        for (i0, j0, i1, j1), stride in (((7, 3, 61, 33), 64), ((0, 39, 75, 40), 200), ((74, 0, 75, 40), 3), ((10, 10, 10, 20), 5)):
            out = np.full((j1 - j0, stride), 7, np.uint8)
            emap._check(emap._lib.gem_costmap_read(emap._h, dm.id, i0, j0, i1, j1, out.ctypes.data_as(C.c_void_p), stride), "gem_costmap_read")
            assert out[:, :i1 - i0].tobytes() == master.grid[j0:j1, i0:i1].tobytes() and (out[:, i1 - i0:] == 7).all()
        wide = np.full((6, 90), 9, np.uint8)
        wide[:, :50] = rng.integers(0, 256, (6, 50))
        emap._check(emap._lib.gem_costmap_write(emap._h, dm.id, 20, 30, 70, 36, wide.ctypes.data_as(C.c_void_p), 90), "gem_costmap_write")
        master.grid[30:36, 20:70] = wide[:, :50]
        same(dm, master)
    finally:
        dl.close(); dm.close()


# ---- 7. enqueue only --------------------------------------------------------------------------------------------------------------
def test_null_bounds_only_enqueue_and_a_second_loop_allocates_nothing(oracle_mod):
    L, res = 48, 0.1
    p = Pair(oracle_mod, L, res)
    m = p.gpu
    m.global_enable(1 << 16)
    cm = ref.Costmap(75, 75, 0.2, -7.4, -7.6)
    big = ref.Costmap(1000, 1000, 0.2, -100.0, -100.0)
    sync, lazy, dbig = device_costmap(m, cm), device_costmap(m, cm), device_costmap(m, big)
    rng = np.random.default_rng(2)
    clouds = [lattice_cloud(rng, 30000, cm) for _ in range(3)]
    for c in clouds:
        m.global_push(c)

    def loop():
        out = []
        for k, xy in enumerate(trajectory(6)):
            p.move(xy)
            p.add(k, xy)
            p.capture(p.feature(), k)
            for dev, bounds in ((sync, list(EMPTY)), (lazy, None)):
                dev.roll_to(float(xy[0]), float(xy[1]))
                dev.mark_points(clouds[k % 3], THRESH, bounds)
                dev.mark_grid_cloud(THRESH, bounds)
                dev.mark_visual(0.45, bounds)
                dev.mark_global(-1, THRESH, bounds)
            dbig.mark_global(k % 3, THRESH, None)
            m.synchronize()
            a, b = sync.read(), lazy.read()
            assert a.tobytes() == b.tobytes() and (a != NOINFO).sum() > 100
            out.append(a.tobytes())
            p.raytracing()
            p.keep_previous()
        return out

    first = loop()
    a1 = m.debug_get("arena_allocations")
    for dev in (sync, lazy, dbig):
        dev.reset()
    p.gpu.move([0.0, 0.0, 0.5]); p.ref.move([0.0, 0.0, 0.5]); p.center = np.zeros(2, F32)
    for dev in (sync, lazy):
        dev.update_origin(cm.ox, cm.oy)
    loop()
    assert m.debug_get("arena_allocations") == a1
    assert len(first) == 6
    for dev in (sync, lazy, dbig):
        dev.close()


# ---- 8. errors --------------------------------------------------------------------------------------------------------------------
def test_error_cases_leave_the_grid_unchanged():
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    INV = _lib.GEM_OK - 1
    cm = ref.Costmap(30, 20, 0.2, *ORIGIN)
    dev, same_size, other_size = device_costmap(m, cm), device_costmap(m, cm), m.costmap(31, 20, 0.2)
    pts = lattice_cloud(np.random.default_rng(3), 5000, cm)
    want_b = ref.mark_points(cm, pts, THRESH, list(EMPTY))
    assert dev.mark_points(pts, THRESH, list(EMPTY)) == want_b
    vp = pts.ctypes.data_as(C.c_void_p)
    b = (C.c_double * 4)(*EMPTY)
    idc = C.c_int()

    def unchanged():
        same(dev, cm)
        assert list(b) == EMPTY

    def cfg(sx=4, sy=4, res=0.2, ox=0.0, oy=0.0):
        return C.byref(_lib.CostmapConfig(sx, sy, res, ox, oy, 255))

    nan, inf = float("nan"), float("inf")
    # creation: a zero size, a resolution that is not positive and finite, a non-finite origin
    for c in (cfg(sx=0), cfg(sy=0), cfg(res=0.0), cfg(res=-0.2), cfg(res=nan), cfg(res=inf), cfg(ox=nan), cfg(oy=-inf), cfg(sx=1 << 16, sy=1 << 15)):
        assert lib.gem_costmap_create(h, c, C.byref(idc)) == INV
    assert lib.gem_costmap_create(h, None, C.byref(idc)) == INV
    # a bad id, every entry
    for bad in (-1, 3, 8, 1 << 20):
        assert lib.gem_costmap_destroy(h, bad) == INV and lib.gem_costmap_reset(h, bad) == INV
        assert lib.gem_costmap_geometry(h, bad, C.byref(_lib.CostmapConfig())) == INV
        assert lib.gem_costmap_update_origin(h, bad, 0.0, 0.0) == INV and lib.gem_costmap_roll_to(h, bad, 0.0, 0.0) == INV
        assert lib.gem_costmap_mark_points(h, bad, vp, 10, THRESH, b) == INV and lib.gem_costmap_mark_points_device(h, bad, vp, 10, THRESH, b) == INV
        assert lib.gem_costmap_mark_grid_cloud(h, bad, THRESH, b) == INV and lib.gem_costmap_mark_visual(h, bad, THRESH, b) == INV
        assert lib.gem_costmap_mark_global(h, bad, -1, THRESH, b) == INV
        assert lib.gem_costmap_merge(h, bad, dev.id, 0, 0, 1, 1, 0) == INV and lib.gem_costmap_merge(h, dev.id, bad, 0, 0, 1, 1, 0) == INV
        assert lib.gem_costmap_read(h, bad, 0, 0, 1, 1, vp, 1) == INV and lib.gem_costmap_write(h, bad, 0, 0, 1, 1, vp, 1) == INV
    unchanged()
    # clouds and thresholds
    for n in (-1, (1 << 31) - 1, 1 << 40):
        assert lib.gem_costmap_mark_points(h, dev.id, vp, n, THRESH, b) == INV
        assert lib.gem_costmap_mark_points_device(h, dev.id, vp, n, THRESH, b) == INV
    assert lib.gem_costmap_mark_points(h, dev.id, None, 5, THRESH, b) == INV
    for t in (nan, inf, -inf):
        assert lib.gem_costmap_mark_points(h, dev.id, vp, 10, t, b) == INV
        assert lib.gem_costmap_mark_grid_cloud(h, dev.id, t, b) == INV and lib.gem_costmap_mark_visual(h, dev.id, t, b) == INV
        assert lib.gem_costmap_mark_global(h, dev.id, -1, t, b) == INV
    unchanged()
    # no local map, then no capture; no submap stack, then an index out of range
    assert lib.gem_costmap_mark_grid_cloud(h, dev.id, THRESH, b) == INV and lib.gem_costmap_mark_visual(h, dev.id, THRESH, b) == INV
    m.local_enable(16)
    assert lib.gem_costmap_mark_grid_cloud(h, dev.id, THRESH, b) == INV and lib.gem_costmap_mark_visual(h, dev.id, THRESH, b) == INV
    assert lib.gem_costmap_mark_global(h, dev.id, -1, THRESH, b) == INV
    m.global_enable(16)
    m.global_push(pts[:100])
    for i in (-2, 1, 7):
        assert lib.gem_costmap_mark_global(h, dev.id, i, THRESH, b) == INV
    unchanged()
    # origins: not finite, or a step whose cell count does not fit an int
    for x, y in ((nan, 0.0), (0.0, inf), (ORIGIN[0] + 0.2 * (2.0 ** 31 + 1000), ORIGIN[1]), (ORIGIN[0], ORIGIN[1] - 0.2 * (2.0 ** 31 + 1000)), (1e300, 0.0)):
        assert lib.gem_costmap_update_origin(h, dev.id, x, y) == INV
    assert lib.gem_costmap_roll_to(h, dev.id, nan, 0.0) == INV and lib.gem_costmap_roll_to(h, dev.id, 0.0, -1e300) == INV
    unchanged()
    # windows outside the map, sizes that differ, a merge mode that is neither
    for w in ((-1, 0, 5, 5), (0, -1, 5, 5), (0, 0, 31, 5), (0, 0, 5, 21), (6, 0, 5, 5), (0, 6, 5, 5)):
        assert lib.gem_costmap_merge(h, same_size.id, dev.id, *w, 0) == INV
        assert lib.gem_costmap_read(h, dev.id, *w, vp, 64) == INV and lib.gem_costmap_write(h, dev.id, *w, vp, 64) == INV
    assert lib.gem_costmap_merge(h, other_size.id, dev.id, 0, 0, 5, 5, 0) == INV
    assert lib.gem_costmap_merge(h, same_size.id, dev.id, 0, 0, 5, 5, 2) == INV
    assert lib.gem_costmap_read(h, dev.id, 0, 0, 5, 5, None, 5) == INV and lib.gem_costmap_read(h, dev.id, 0, 0, 5, 5, vp, 4) == INV
    assert lib.gem_costmap_write(h, dev.id, 0, 0, 5, 5, None, 5) == INV and lib.gem_costmap_write(h, dev.id, 0, 0, 5, 5, vp, 4) == INV
    unchanged()
    # eight costmaps per handle
    extra = [m.costmap(2, 2, 1.0) for _ in range(5)]
    assert lib.gem_costmap_create(h, cfg(), C.byref(idc)) == INV
    freed = extra[0].id
    extra[0].close()
    assert lib.gem_costmap_create(h, cfg(), C.byref(idc)) == 0 and idc.value == freed       # a destroyed id is free again
    unchanged()
    # a handle with a communicator
    w = ElevationMap(32, 0.05)
    w.comm_init_loopback(9533, 1, 0, tile_strips=False)
    assert w._lib.gem_costmap_create(w._h, cfg(), C.byref(idc)) == INV
    assert w._lib.gem_costmap_reset(w._h, 0) == INV
    # a destroyed id is gone
    i = dev.id
    dev.close()
    assert lib.gem_costmap_reset(h, i) == INV


# ---- 9. the C++ facade ------------------------------------------------------------------------------------------------------------
def test_cpp_costmap_facade(tmp_path):
    exe = build_costmap_facade_check(tmp_path / "costmap_facade_check")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
