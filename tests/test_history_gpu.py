"""The history cloud on the device (gem_history_*, gem_costmap_mark_history) against the restatement of tests/history_ref.py, the
restatements it stands on (local_ref for the spills, costmap_ref for the marks) and the device's own independent path (history_export
followed by mark_points).  Every comparison is exact: records and byte grids by tobytes(), bounds by == on doubles, counts by ==.

  1. a node-ordered frame loop whose spills append: the export after every frame, with and without the grid cloud; a second handle
     that never downloads a spill ends with the same bytes;
  2. appends of 0 .. 10000 records, host and device forms in turn, growing from a capacity of 64;
  3. the rebuild after a loop closure (reset_from_global), a spill behind it, clear;
  4. the culled mark on both forms of the mark kernel: blocks inside, outside, straddling an edge, of NaN only, a partial last one;
     cull on and off, three times over;
  5. rolling: the culled set changes with every roll, mark_history + mark_grid_cloud after each;
  6. bounds NULL + gem_synchronize, and no allocation in a second identical loop;
  7. the error cases (GEM_ERR_INVALID: size, export and costmap unchanged);
  8. the C++ gem::History (tests/cpp/history_check.cpp) as a child process."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gem_amd import ElevationMap, SensorModel, _lib, synth

sys.path.insert(0, str(Path(__file__).resolve().parent))
import costmap_ref as cref  # noqa: E402
import history_ref as ref  # noqa: E402
import local_ref  # noqa: E402
from local_ref import POINT  # noqa: E402
from test_history_cpu import build_history_check  # noqa: E402
from test_local_map_gpu import HEADINGS, Pair, trajectory  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
F32 = np.float32
FREE, LETHAL, NOINFO = cref.FREE_SPACE, cref.LETHAL_OBSTACLE, cref.NO_INFORMATION
THRESH = 0.5
EMPTY = [1e30, 1e30, -1e30, -1e30]                       # the bounds LayeredCostmap::updateMap starts from
ORIGIN = (-7.25, 4.125)                                  # floats: a record can sit exactly on an edge
B = ref.BLOCK
NAN, INF = np.nan, np.inf


def device_costmap(m, cm, default=NOINFO):
    return m.costmap(cm.size_x, cm.size_y, cm.res, cm.ox, cm.oy, default)


def same(dev, cm):
    g = dev.geometry()
    assert (g["origin_x"], g["origin_y"], g["size_x"], g["size_y"]) == (cm.ox, cm.oy, cm.size_x, cm.size_y)
    got = dev.read()
    assert got.shape == cm.grid.shape and got.tobytes() == cm.grid.tobytes(), f"{int((got != cm.grid).sum())} cells differ"


def cluster(rng, n, x0, x1, y0, y1):
    """n records on a 0.05 m lattice inside [x0, x1) x [y0, y1) (many per 0.2 m cell, so a cell sees both verdicts), travers scattered
    around the threshold, some exactly on it (lethal in this layer), some NaN"""
    out = np.zeros(n, POINT)
    out["x"] = (x0 + 0.05 * rng.integers(0, max(1, int((x1 - x0) / 0.05)), n) + rng.uniform(0.0, 0.04, n)).astype(F32)
    out["y"] = (y0 + 0.05 * rng.integers(0, max(1, int((y1 - y0) / 0.05)), n) + rng.uniform(0.0, 0.04, n)).astype(F32)
    out["z"], out["pad"] = rng.uniform(-1, 2, n).astype(F32), 1.0
    out["intensity"] = rng.uniform(0, 100, n).astype(F32)
    t = rng.uniform(THRESH - 0.3, THRESH + 0.3, n)
    t[rng.random(n) < 0.05] = THRESH
    t[rng.random(n) < 0.03] = NAN
    out["travers"] = t.astype(F32)
    return out


def to_device(points):
    import torch
    return torch.from_numpy(np.ascontiguousarray(points).view(np.uint8).reshape(points.shape[0], 32).copy()).to("cuda:0")


def add_like_pair(m, seed, xy, L, res, n):
    """the cloud Pair.add fuses, into another device map"""
    rng = np.random.default_rng(seed)
    c = synth.random_cloud(seed, n, 0.4 * L * res, z_sigma=0.15)
    rgb = rng.integers(0, 1 << 24, c.shape[0]).astype(np.uint32)
    m.add(synth._frame_for(synth.pose_matrix(xy[0], xy[1], 0.5, 0.1 * seed), SensorModel.velodyne()), c, rgb=rgb)


# ---- 1. the frame loop ------------------------------------------------------------------------------------------------------------
def test_frame_loop_spills_append(oracle_mod):
    L, res, n_add = 48, 0.1, 20000
    p = Pair(oracle_mod, L, res)
    p.gpu.history_enable(64)                              # grows several times
    quiet = ElevationMap(L, res)                          # the same node, but no spill ever crosses the link
    quiet.set_lowest_tracking(True)
    quiet.set_layer("lowest", p.ref.layer("lowest"))
    quiet.local_enable(1 << 12)
    quiet.history_enable(64)
    hist = ref.History()
    a0 = p.gpu.debug_get("arena_allocations")
    for k, xy in enumerate(trajectory(24, step=1.2, per_heading=3)):
        shift = p.move(xy)
        quiet.move([xy[0], xy[1], 0.5])
        p.add(k, xy, n_add)
        add_like_pair(quiet, k, xy, L, res, n_add)
        feat = p.feature()
        quiet.map_feature(fetch=False)
        quiet.set_layer("traver", feat["traver"])
        p.capture(feat, k)
        quiet.local_capture()
        if k == 0:
            p.keep_previous(); quiet.local_keep_previous()
        if p.gate(shift):
            before = dict(p.local)
            want, _ = local_ref.spill(p.prev, p.center, shift, before)       # the restatement alone, on a copy of the local map
            hist.append(want)
            p.spill(shift, k)                                                 # (asserts the device's records against the same)
            n, _ = quiet.local_spill(p.center, shift, download=False)
            assert n == want.size
        assert p.gpu.history_size() == len(hist)
        assert p.gpu.history_export(False).tobytes() == hist.export().tobytes(), f"frame {k}"
        assert p.gpu.history_export(True).tobytes() == hist.export(local_ref.grid_cloud(p.cap)).tobytes(), f"frame {k}"
        p.raytracing(); quiet.raytracing()
        p.keep_previous(); quiet.local_keep_previous()
    assert len(hist) > 2 * B, len(hist)                   # by the restatement alone: more than two blocks, several growths from 64
    assert p.gpu.debug_get("arena_allocations") > a0
    assert quiet.history_size() == len(hist) and quiet.history_export().tobytes() == hist.export().tobytes()
    assert p.gpu.debug_get("history_blocks") == ref.n_blocks(len(hist))
    quiet.close()


# ---- 2. appends -------------------------------------------------------------------------------------------------------------------
def test_appends_host_and_device_forms_growing_from_64():
    m = ElevationMap(32, 0.05)
    m.history_enable(64)
    rng = np.random.default_rng(11)
    counts = [0, 1, 63, 64, 65, 4095, 4096, 4097, 10000]
    rng.shuffle(counts)
    hist = ref.History()
    assert m.history_size() == 0 and m.history_export().size == 0
    for k, n in enumerate(counts):
        pts = cluster(rng, n, -5.0, 5.0, -5.0, 5.0)
        pts["b"], pts["covariance"] = rng.integers(0, 256, n), rng.uniform(0, 1, n).astype(F32)
        m.history_append(to_device(pts) if k % 2 else pts)
        hist.append(pts)
        assert m.history_size() == len(hist)
        assert m.history_export().tobytes() == hist.export().tobytes(), f"append {k} of {n}"
    assert len(hist) == sum(counts)
    m.history_enable(64)                                  # on an enabled handle it starts over
    assert m.history_size() == 0 and m.history_export().size == 0
    m.history_enable(0)
    n = C.c_longlong()
    assert m._lib.gem_history_size(m._h, C.byref(n)) == _lib.GEM_OK - 1
    m.close()


# ---- 3. the rebuild ---------------------------------------------------------------------------------------------------------------
def test_rebuild_from_the_stack_after_a_loop_closure(oracle_mod):
    L, res = 48, 0.1
    p = Pair(oracle_mod, L, res)
    m = p.gpu
    m.global_enable(1 << 12)
    m.history_enable(64)
    hist = ref.History()
    rng = np.random.default_rng(9)
    centres = []
    spills_after = 0
    for k, xy in enumerate(trajectory(22)):
        shift = p.move(xy)
        p.add(k, xy)
        p.capture(p.feature(), k)
        if k == 0:
            p.keep_previous()
        if p.gate(shift):
            want, _ = local_ref.spill(p.prev, p.center, shift, dict(p.local))
            hist.append(want)
            spilled = p.spill(shift, k)
            spills_after += spilled if k >= 16 else 0
        if k < 16 and k % 8 == 7:
            m.global_push_local(True)
            p.local.clear()
            centres.append([float(p.center[0]), float(p.center[1])])
        if k == 15:                                       # the loop closure arrives: four submaps, fused, then the history is rebuilt
            for _ in range(2):
                m.global_push(cluster(rng, 20000, -2.0, 2.0, -2.0, 2.0))
                centres.append([0.0, 0.0])
            assert m.global_count() == 4
            t = np.tile(np.eye(4, dtype=F32), (4, 1, 1))
            t[:, 0, 3] = [0.0, 0.05, -0.1, 0.15]
            before = m.global_export(-1)
            fused = m.global_loop_closure(t, centres, radius=25.0, resolution=0.1)
            stack = m.global_export(-1)
            assert fused > 100 and stack.size < before.size and stack.size > 1000
            assert m.history_size() == len(hist) and len(hist) > 0
            m.history_reset_from_global()
            hist.reset_from([m.global_export(i) for i in range(4)])
            assert m.history_size() == stack.size and m.history_export().tobytes() == stack.tobytes() == hist.export().tobytes()
        assert m.history_export().tobytes() == hist.export().tobytes(), f"frame {k}"
        p.raytracing()
        p.keep_previous()
    assert spills_after > 0 and len(hist) == m.global_export(-1).size + spills_after      # later spills went behind the rebuilt cloud
    m.history_clear()
    assert m.history_size() == 0 and m.history_export().size == 0
    assert m.debug_get("history_blocks") == 0


# ---- 4. the culled mark -----------------------------------------------------------------------------------------------------------
def marked_history(rng, cm):
    """clusters of 4096 m plus or minus a few records at distinct places, in append order, and the indices of the two records that
    share the cell (1, 1) with opposite verdicts"""
    ox, oy, ex, ey = cm.ox, cm.oy, cm.ox + cm.size_x * cm.res, cm.oy + cm.size_y * cm.res
    mid_x, mid_y = 0.5 * (ox + ex), 0.5 * (oy + ey)
    below = lambda v: float(np.nextafter(F32(v), F32(-INF)))
    inside = lambda n: cluster(rng, n, mid_x - 3.0, mid_x + 3.0, mid_y - 3.0, mid_y + 3.0)
    parts = [inside(B + 7),                                                           # blocks inside
             cluster(rng, 3 * B - 5, ex + 100.0, ex + 104.0, mid_y, mid_y + 4.0),     # far beyond the far x edge: whole blocks outside
             cluster(rng, B + 3, ox - 3.0, ox + 3.0, mid_y - 2.0, mid_y + 2.0),       # across the near x edge
             cluster(rng, 2 * B, mid_x, mid_x + 1.0, mid_y, mid_y + 1.0),             # (made all-NaN below: one block of only NaN)
             cluster(rng, 2 * B + 1, mid_x - 2.0, mid_x + 2.0, oy - 60.0, oy - 50.0),  # below the near y edge
             cluster(rng, B - 9, mid_x - 2.0, mid_x + 2.0, ey - 2.0, ey + 2.0),       # across the far y edge
             inside(B - 9),
             inside(1000)]                                                            # the last block is partial
    parts[3]["x"], parts[3]["y"] = NAN, NAN
    rec = np.concatenate(parts)
    # the special records, spread over the last two inside clusters: on each edge and just outside it, NaN and +-inf coordinates, travers at
    # the threshold and NaN
    special = [(ox, mid_y), (below(ox), mid_y), (mid_x, oy), (mid_x, below(oy)), (ex, mid_y), (below(ex), mid_y), (mid_x, ey), (mid_x, below(ey)),
               (ox - 0.01, mid_y), (ex + 0.01, mid_y), (mid_x, oy - 0.01), (mid_x, ey + 0.01), (ex + 0.2, mid_y), (mid_x, ey + 0.2),
               (NAN, mid_y), (mid_x, NAN), (INF, mid_y), (mid_x, -INF), (-INF, INF), (NAN, NAN)]
    last0 = rec.size - 1000 - (B - 9)
    at = np.linspace(last0 + 10, rec.size - 3, len(special)).astype(int)
    for i, (sx, sy) in zip(at, special):
        rec["x"][i], rec["y"][i] = sx, sy
    rec["travers"][at[0]], rec["travers"][at[5]], rec["travers"][at[2]] = THRESH, NAN, THRESH + 0.25
    # cell (1, 1) holds two records only: the second record of the history (free) and the last but one (lethal)
    first, last = 1, rec.size - 2
    for i, t in ((first, THRESH + 0.25), (last, THRESH - 0.25)):
        rec["x"][i], rec["y"][i], rec["travers"][i] = ox + 1.5 * cm.res, oy + 1.5 * cm.res, t
    return [rec[a:b] for a, b in zip(np.cumsum([0] + [q.size for q in parts[:-1]]), np.cumsum([q.size for q in parts]))], first, last


@pytest.mark.parametrize("size", [(75, 75), (128, 65)], ids=lambda s: f"{s[0]}x{s[1]}")     # the LDS form | the global form of the mark
def test_culled_mark(size):
    rng = np.random.default_rng(100 * size[0] + size[1])
    cm = cref.Costmap(size[0], size[1], 0.2, *ORIGIN)
    parts, first, last = marked_history(rng, cm)
    hist = ref.History()
    m = ElevationMap(32, 0.05)
    m.history_enable(64)
    for k, q in enumerate(parts):
        m.history_append(to_device(q) if k % 2 else q)
        hist.append(q)
    rec = hist.rec
    assert m.history_size() == rec.size and rec.size % B != 0
    # what the input exercises, by the restatement alone
    nb = ref.n_blocks(rec.size)
    skip = ref.culled_blocks(cm, rec)
    ok, idx = cref.world_to_map_v(cm, rec["x"].astype(np.float64), rec["y"].astype(np.float64))
    per_block = np.add.reduceat(ok.astype(int), np.arange(0, rec.size, B))
    sizes = np.diff(np.append(np.arange(0, rec.size, B), rec.size))
    assert 0 < skip.sum() < nb and not per_block[skip].any()
    assert (per_block[~skip] == sizes[~skip]).any() and ((per_block[~skip] > 0) & (per_block[~skip] < sizes[~skip])).any()   # inside | straddling
    t = ref.boxes(rec)
    assert any(tuple(b.tolist()) == ref.EMPTY_BOX for b in t)                            # a block of only NaN
    assert first // B != last // B and idx[first] == idx[last] == cm.size_x + 1 and (idx[ok] == idx[first]).sum() == 2
    want_b = ref.mark_history(cm, hist, THRESH, list(EMPTY))
    rev = cref.Costmap(size[0], size[1], 0.2, *ORIGIN)
    cref.mark_points(rev, rec[::-1], THRESH)
    assert cm.grid[1, 1] == LETHAL and rev.grid[1, 1] == FREE and rev.grid.tobytes() != cm.grid.tobytes()
    marked, both = cref.verdict_mix(cm, *cref.point_inputs(rec, THRESH))
    assert marked > 100 and 2 * both >= marked
    dev, other = device_costmap(m, cm), device_costmap(m, cm)
    assert m.debug_get("history_cull") == 1 and m.debug_get("history_blocks") == nb
    try:
        grids = []
        for cull in (1, 0):
            m.debug_set("history_cull", cull)
            for _ in range(3):
                dev.reset(); other.reset()
                b = dev.mark_history(THRESH, list(EMPTY))
                culled = m.debug_get("history_blocks_culled")
                print(f"size {size} cull {cull}: {culled} of {nb} blocks culled, restatement {int(skip.sum())}")
                assert b == want_b, (b, want_b)
                same(dev, cm)
                assert culled == (int(skip.sum()) if cull else 0)
                assert other.mark_points(m.history_export(), THRESH, list(EMPTY)) == want_b
                same(other, cm)
                grids.append(dev.read().tobytes())
        assert all(g == grids[0] for g in grids) and len(grids) == 6
        # onto what is there, with bounds that already hold values, another threshold
        start = [cm.ox + 0.3, -1e30, 1e30, cm.oy + 0.1]
        m.debug_set("history_cull", 1)
        assert dev.mark_history(0.45, list(start)) == ref.mark_history(cm, hist, 0.45, list(start))
        same(dev, cm)
        # an empty history marks nothing and culls nothing
        m.history_clear()
        assert dev.mark_history(THRESH, list(EMPTY)) == EMPTY and m.debug_get("history_blocks_culled") == 0
        same(dev, cm)
    finally:
        dev.close(); other.close(); m.close()


# ---- 5. rolling -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(75, 75), (130, 90)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rolling_changes_the_culled_set(size):
    """eight clusters on a ring, the robot visits them in turn: every roll brings another cluster into the window; the grid cloud is
    the capture of a map moved with the robot"""
    L, res = 32, 0.1
    rng = np.random.default_rng(size[1])
    m = ElevationMap(L, res)
    m.local_enable(64)
    m.history_enable(1 << 12)
    hist = ref.History()
    R = 22.0
    for k, d in enumerate(HEADINGS):
        c = R * np.array(d, float)
        q = cluster(rng, B + 11 * k - 30, c[0] - 1.0, c[0] + 1.0, c[1] - 1.0, c[1] + 1.0)
        m.history_append(q); hist.append(q)
    cm = cref.Costmap(size[0], size[1], 0.2, -7.4, -7.6, FREE if size[0] == 75 else NOINFO)
    dev = device_costmap(m, cm, cm.default)
    layers = {"elevation": rng.uniform(-0.5, 0.5, (L, L)).astype(F32), "traver": rng.uniform(0.0, 1.0, (L, L)).astype(F32),
              "variance": rng.uniform(1e-4, 1e-2, (L, L)).astype(F32)}
    try:
        previous = None
        for k, d in enumerate(HEADINGS + HEADINGS[-2::-1]):           # (no heading twice in a row)
            robot = (R - 2.0 + 0.37 * k) * np.array(d, float)
            m.move([robot[0], robot[1], 0.5])
            for name, v in layers.items():
                m.set_layer(name, v)
            m.local_capture()
            grid_pc = m.local_grid_cloud()
            assert grid_pc.size > 500
            cref.roll_to(cm, robot[0], robot[1]); dev.roll_to(robot[0], robot[1])
            skip = ref.culled_blocks(cm, hist.rec)
            assert 0 < skip.sum() < skip.size and (previous is None or (skip != previous).any()), f"roll {k}"
            previous = skip
            b_hist = ref.mark_history(cm, hist, THRESH, list(EMPTY))
            assert dev.mark_history(THRESH, list(EMPTY)) == b_hist, f"roll {k}"
            assert m.debug_get("history_blocks_culled") == skip.sum()
            b_all = cref.mark_points(cm, grid_pc, THRESH, list(b_hist))  # visualCloud_ + grid_pc: one cloud, the bounds carried on
            assert dev.mark_grid_cloud(THRESH, list(b_hist)) == b_all, f"roll {k}"
            same(dev, cm)
        assert (cm.grid == LETHAL).sum() > 100 and (cm.grid == FREE).sum() > 100
    finally:
        dev.close(); m.close()


# ---- 6. enqueue only --------------------------------------------------------------------------------------------------------------
def test_null_bounds_only_enqueue_and_a_second_loop_allocates_nothing():
    m = ElevationMap(32, 0.05)
    cm = cref.Costmap(75, 75, 0.2, *ORIGIN)
    big = cref.Costmap(1000, 1000, 0.2, -100.0, -100.0)
    sync, lazy, dbig = device_costmap(m, cm), device_costmap(m, cm), device_costmap(m, big)
    rng = np.random.default_rng(2)
    mid = (cm.ox + 7.5, cm.oy + 7.5)
    clouds = [cluster(rng, n, mid[0] - 4.0 + 9.0 * k, mid[0] + 4.0 + 9.0 * k, mid[1] - 4.0, mid[1] + 4.0) for k, n in enumerate((5000, B + 1, 3 * B - 7, 100))]
    held = [to_device(c) for c in clouds]

    def loop():
        m.history_enable(64)
        out = []
        for k, c in enumerate(clouds):
            m.history_append(held[k] if k % 2 else c)
            sync.mark_history(THRESH, list(EMPTY))
            lazy.mark_history(THRESH, None)
            dbig.mark_history(THRESH, None)
            m.synchronize()
            a, b = sync.read(), lazy.read()
            assert a.tobytes() == b.tobytes() and (a != NOINFO).sum() > 100
            out.append(a.tobytes())
        return out, dbig.read().tobytes()

    first = loop()
    a1 = m.debug_get("arena_allocations")
    for dev in (sync, lazy, dbig):
        dev.reset()
    second = loop()
    assert m.debug_get("arena_allocations") == a1
    assert first == second and len(first[0]) == 4
    c = cref.Costmap(big.size_x, big.size_y, big.res, big.ox, big.oy)
    cref.mark_points(c, np.concatenate(clouds), THRESH)
    assert first[1] == c.grid.tobytes()
    for dev in (sync, lazy, dbig):
        dev.close()
    m.close()


# ---- 7. errors --------------------------------------------------------------------------------------------------------------------
def test_error_cases_leave_everything_unchanged():
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    INV = _lib.GEM_OK - 1
    cm = cref.Costmap(30, 20, 0.2, *ORIGIN)
    dev = device_costmap(m, cm)
    rng = np.random.default_rng(3)
    pts = cluster(rng, 5000, cm.ox - 1.0, cm.ox + 5.0, cm.oy - 1.0, cm.oy + 3.0)
    vp = pts.ctypes.data_as(C.c_void_p)
    d_pts = to_device(pts)
    dp = C.c_void_p(d_pts.data_ptr())
    b = (C.c_double * 4)(*EMPTY)
    n = C.c_longlong(-7)
    nan, inf = float("nan"), float("inf")
    # not enabled: every entry
    assert lib.gem_history_append(h, vp, 10) == INV and lib.gem_history_append_device(h, dp, 10) == INV
    assert lib.gem_history_reset_from_global(h) == INV and lib.gem_history_clear(h) == INV
    assert lib.gem_history_size(h, C.byref(n)) == INV and lib.gem_history_export(h, 0, None, 0, C.byref(n)) == INV and n.value == -7
    assert lib.gem_costmap_mark_history(h, dev.id, THRESH, b) == INV
    assert lib.gem_history_enable(h, -1) == INV and lib.gem_history_enable(h, 1 << 31) == INV
    assert m.debug_get("history_blocks") == 0 and m.debug_get("history_blocks_culled") == 0
    same(dev, cm)
    m.history_enable(64)
    m.history_append(pts)
    hist = ref.History(); hist.append(pts)
    want_b = ref.mark_history(cm, hist, THRESH, list(EMPTY))
    assert dev.mark_history(THRESH, list(EMPTY)) == want_b

    def unchanged():
        assert m.history_size() == len(hist) and m.history_export().tobytes() == hist.export().tobytes()
        same(dev, cm)
        assert list(b) == EMPTY

    # clouds: n < 0, NULL with n > 0, a length that would pass 2^31 - 2 (checked before anything is read: the buffer holds 5000 records)
    limit = (1 << 31) - 2
    for fn, ptr in ((lib.gem_history_append, vp), (lib.gem_history_append_device, dp)):
        assert fn(h, ptr, -1) == INV and fn(h, None, 5) == INV
        assert fn(h, ptr, limit - len(hist) + 1) == INV and fn(h, ptr, limit) == INV and fn(h, ptr, 1 << 40) == INV
        assert fn(h, None, 0) == 0 and fn(h, ptr, 0) == 0                 # nothing to append is fine
    unchanged()
    # no submap stack; the grid cloud without a local map, then without a capture; max_points below the count
    assert lib.gem_history_reset_from_global(h) == INV
    out = np.empty(len(hist) + 10, POINT)
    op = out.ctypes.data_as(C.c_void_p)
    assert lib.gem_history_export(h, 1, op, out.size, C.byref(n)) == INV and lib.gem_history_export(h, 1, None, 0, C.byref(n)) == INV
    m.local_enable(16)
    assert lib.gem_history_export(h, 1, op, out.size, C.byref(n)) == INV
    assert lib.gem_history_export(h, 0, op, len(hist) - 1, C.byref(n)) == INV and lib.gem_history_export(h, 0, op, 0, C.byref(n)) == INV
    assert n.value == -7
    assert lib.gem_history_export(h, 0, None, 0, C.byref(n)) == 0 and n.value == len(hist)      # NULL: the count only
    assert lib.gem_history_size(h, None) == INV
    unchanged()
    # the mark: a bad costmap id, a threshold that is not finite
    for bad in (-1, 3, 8, 1 << 20):
        assert lib.gem_costmap_mark_history(h, bad, THRESH, b) == INV
    for t in (nan, inf, -inf):
        assert lib.gem_costmap_mark_history(h, dev.id, t, b) == INV
    assert lib.gem_debug_set(h, b"history_cull", 2) == INV and lib.gem_debug_set(h, b"history_cull", -1) == INV
    assert m.debug_get("history_cull") == 1
    unchanged()
    # a spill with the history enabled but no capture fails as it did
    c2 = (C.c_float * 2)(0.3, 0.0)
    k, rep = C.c_int(), C.c_int()
    assert lib.gem_local_spill(h, c2, c2, op, C.byref(k), C.byref(rep)) == INV
    unchanged()
    # a handle with a communicator
    w = ElevationMap(32, 0.05)
    w.comm_init_loopback(9541, 1, 0, tile_strips=False)
    assert w._lib.gem_history_enable(w._h, 64) == INV and w._lib.gem_history_size(w._h, C.byref(n)) == INV
    assert w._lib.gem_costmap_mark_history(w._h, 0, THRESH, b) == INV
    w.close()
    # switched off: gone, and the costmap stays
    m.history_enable(0)
    assert lib.gem_history_size(h, C.byref(n)) == INV and lib.gem_costmap_mark_history(h, dev.id, THRESH, b) == INV
    same(dev, cm)
    dev.close(); m.close()


# ---- 8. the C++ facade ------------------------------------------------------------------------------------------------------------
def test_cpp_history_facade(tmp_path):
    exe = build_history_check(tmp_path / "history_check")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
