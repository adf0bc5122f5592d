"""gem_local_compose / gem_local_compose_distances against tests/compose_ref.py on the device's own previous capture: the road and
obstacle records and their order, the three counts, the threshold and every point's distance, BIT-IDENTICAL, no tolerance.

  1. node order (move -> add -> map_feature -> show / capture -> raytracing -> keep_previous) on maps of 64, 200 and 600 cells, every capture of every run compared; after
     the moves the start index is not zero, so the unwrapped-index handling is exercised;
  2. geometry that defeats the LDS tile -- 5 % occupancy, isolated cells, a 2 m step scene -- with gem_debug_get("compose_far_points")
     > 0, and a full flat map where it must read 0.  A plain plateau edge is a half plane of neighbours, exactly what a cell at the
     map's rim has, and the flat map's rim has to close inside the tile; so the step scene also carries a free-standing wall of the
     same 2 m, one cell wide (a step on both of its sides), whose cells find their 20 neighbours only along the wall;
  3. positions where a float ulp is a visible part of a cell (2e4) and larger than a cell (1e6: coincident x / y, d2 = 0 ties);
  4. mean_k 1, 8, 20, 32, both sqrt forms, stddev_mul 0 and 3, travers thresholds 0, positive and above every value (empty road);
  5. NULL outputs, the error cases, n <= mean_k;
  6. no allocation on a second call; a call from a second thread while the first runs the frame loop; the C++ facade."""
import ctypes as C
import struct
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

from gem_amd import ElevationMap, _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import compose_ref  # noqa: E402
import local_ref  # noqa: E402
from test_compose_cpu import build_compose_facade_check  # noqa: E402
from test_local_map_gpu import Pair, trajectory  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
EMPTY = F32(-10.0)
INV = _lib.GEM_OK - 1


def bits(v):
    return struct.pack("<d", float(v))


def scene_map(L, res, elevation, traver=None, seed=0, move=None):
    """a device map, moved first (a start index other than zero; a move empties the cells that enter the window), whose layers are
    then set directly, in storage order; elevation -10 = empty cell"""
    rng = np.random.default_rng(seed)
    m = ElevationMap(L, res)
    if move is not None:
        m.move([move[0], move[1], 0.0])
        assert tuple(m.pose()[1]) != (0, 0)
    m.set_layer("elevation", np.asarray(elevation, F32))
    m.set_layer("traver", rng.uniform(-0.2, 1.0, (L, L)).astype(F32) if traver is None else np.asarray(traver, F32))
    m.set_layer("variance", rng.uniform(1e-4, 1e-2, (L, L)).astype(F32))
    m.set_layer("intensity", rng.uniform(0, 100, (L, L)).astype(F32))
    for c in ("color_r", "color_g", "color_b"):
        m.set_layer(c, rng.integers(0, 256, (L, L)))
    m.local_enable(1 << 10)
    return m


def capture_previous(m, *args):
    """capture, read the capture's own grid cloud, make it the previous one"""
    m.local_capture(*args)
    g = m.local_grid_cloud()
    m.local_keep_previous()
    return g


def compare(m, g, what, mean_k=20, stddev_mul=1.0, tt=0.0, sqrt_double=False, ref=None):
    """every record, count, the threshold and every distance against the restatement on `g`; returns the far count"""
    road, obstacle, removed, thr = m.local_compose(mean_k, stddev_mul, tt, sqrt_double)
    far = m.debug_get("compose_far_points")
    dist = m.local_compose_distances(mean_k, stddev_mul, tt, sqrt_double)
    r_road, r_obstacle, r_removed, r_thr, r_dist = ref if ref is not None else compose_ref.compose(g, mean_k, stddev_mul, tt, sqrt_double, workers=16)
    wrong = int(np.count_nonzero(dist.view(np.uint32) != r_dist.view(np.uint32))) if dist.shape == r_dist.shape else -1
    print(f"[compose] {what}: n {g.shape[0]} mean_k {mean_k} mul {stddev_mul} tt {tt} sqrt_double {int(sqrt_double)} far {far} | "
          f"road {road.shape[0]}/{r_road.shape[0]} obstacle {obstacle.shape[0]}/{r_obstacle.shape[0]} removed {removed}/{r_removed} "
          f"threshold {thr!r}/{r_thr!r} distances differing {wrong}")
    assert dist.shape == r_dist.shape and wrong == 0
    assert bits(thr) == bits(r_thr)
    assert (road.shape[0], obstacle.shape[0], removed) == (r_road.shape[0], r_obstacle.shape[0], r_removed)
    assert road.tobytes() == r_road.tobytes() and obstacle.tobytes() == r_obstacle.tobytes()
    assert road.shape[0] + obstacle.shape[0] + removed == g.shape[0]
    return far


# ---- 1. node order ---------------------------------------------------------------------------------------------------------------
def node_order(oracle_mod, L, res, frames, points):
    p = Pair(oracle_mod, L, res)
    checked = 0
    for k, xy in enumerate(trajectory(frames, step=4 * res, per_heading=2)):
        p.move(xy)
        p.add(k, xy, n=points)
        feat = p.feature()
        p.capture(feat, k)                                # (asserts the grid cloud against the oracle's show)
        g = p.gpu.local_grid_cloud()
        p.raytracing()
        p.keep_previous()
        assert g.shape[0] > 20
        compare(p.gpu, g, f"node L={L} frame {k} start {tuple(p.gpu.pose()[1])}", sqrt_double=bool(k & 1))
        checked += 1
    assert checked == frames and tuple(p.gpu.pose()[1]) != (0, 0)


def test_node_order_64(oracle_mod):
    node_order(oracle_mod, 64, 0.1, 6, 3000)


@pytest.mark.one_pipeline
def test_node_order_200(oracle_mod):
    node_order(oracle_mod, 200, 0.05, 4, 40000)


@pytest.mark.one_pipeline
def test_node_order_600(oracle_mod):
    node_order(oracle_mod, 600, 0.05, 3, 250000)


# ---- 2. geometry that defeats the LDS tile, and geometry that must not ------------------------------------------------------------
@pytest.mark.one_pipeline
def test_sparse_map_takes_the_far_kernel():
    L, rng = 200, np.random.default_rng(11)
    e = rng.uniform(-0.3, 0.3, (L, L)).astype(F32)
    e[rng.random((L, L)) >= 0.05] = EMPTY
    m = scene_map(L, 0.05, e, seed=11, move=(0.35, -0.2))
    g = capture_previous(m)
    assert 1500 < g.shape[0] < 2500
    assert compare(m, g, "5 % occupied") > 0
    assert compare(m, g, "5 % occupied", mean_k=32, sqrt_double=True) > 0


@pytest.mark.one_pipeline
def test_isolated_cells_take_the_far_kernel():
    L = 200
    e = np.full((L, L), EMPTY, F32)
    e[5::31, 3::29] = np.random.default_rng(12).uniform(-1, 1, e[5::31, 3::29].shape).astype(F32)
    m = scene_map(L, 0.05, e, seed=12, move=(-0.25, 0.4))
    g = capture_previous(m)
    assert g.shape[0] == 49
    assert compare(m, g, "isolated cells") == g.shape[0]              # nobody finds 20 neighbours within 8 rings
    assert compare(m, g, "isolated cells", mean_k=1) == g.shape[0]


@pytest.mark.one_pipeline
def test_step_scene_takes_the_far_kernel():
    L, rng = 200, np.random.default_rng(13)
    e = rng.normal(0.0, 0.01, (L, L)).astype(F32)
    e[120:, :] += F32(2.0)                                # the plateau: a 2 m step edge across the whole map
    e[40, 20:180] += F32(2.0)                             # the wall: 2 m, one cell wide
    m = scene_map(L, 0.05, e, seed=13, move=(0.1, 0.15))
    g = capture_previous(m)
    assert g.shape[0] == L * L
    assert compare(m, g, "2 m step scene") > 0


@pytest.mark.one_pipeline
def test_full_flat_map_stays_in_the_tile():
    L = 200
    for k, move in enumerate((None, (0.45, -0.3))):
        m = scene_map(L, 0.05, np.full((L, L), 0.25, F32), seed=14, move=move)
        g = capture_previous(m)
        assert g.shape[0] == L * L
        assert compare(m, g, f"flat map {k}") == 0
    m = scene_map(96, 0.1, np.random.default_rng(15).normal(0, 0.01, (96, 96)).astype(F32), seed=15)
    assert compare(m, capture_previous(m), "nearly flat map, L = 96") == 0


# ---- 3. float-coarse positions -----------------------------------------------------------------------------------------------------
@pytest.mark.one_pipeline
@pytest.mark.parametrize("centre", [(2.0e4 + 0.013, -2.0e4 - 0.021), (1.0e6 + 0.013, -1.0e6 - 0.021)])
def test_float_coarse_positions(centre):
    L, res = 200, 0.05
    e = np.random.default_rng(16).normal(0.0, 0.03, (L, L)).astype(F32)
    e[np.random.default_rng(17).random((L, L)) < 0.2] = EMPTY
    m = scene_map(L, res, e, seed=16, move=(0.2, 0.3))
    g = capture_previous(m, L * res, res, centre)
    if centre[0] > 1e5:                                   # neighbouring columns share a float x: coincident points exist
        assert np.unique(g["x"]).size < L
    xyz = np.stack([g["x"], g["y"], g["z"]], axis=1)
    assert np.abs(xyz[:, 0] - F32(centre[0])).max() <= 0.5 * L * res + 0.1
    compare(m, g, f"centre {centre}")
    compare(m, g, f"centre {centre}", mean_k=8, sqrt_double=True, stddev_mul=3.0)


# ---- 4. the parameters -------------------------------------------------------------------------------------------------------------
@pytest.fixture
def rough_map():
    L, rng = 128, np.random.default_rng(21)
    e = rng.normal(0.0, 0.08, (L, L)).astype(F32)
    e[rng.random((L, L)) < 0.1] = EMPTY
    e[rng.random((L, L)) < 0.002] += F32(1.5)             # spikes
    m = scene_map(L, 0.05, e, seed=21, move=(0.15, -0.1))
    return m, capture_previous(m)


@pytest.mark.one_pipeline
def test_mean_k_and_sqrt_forms(rough_map):
    m, g = rough_map
    for mean_k in (1, 8, 20, 32):
        for sd in (False, True):
            compare(m, g, "rough", mean_k=mean_k, sqrt_double=sd)


@pytest.mark.one_pipeline
def test_multiplier_and_travers_thresholds(rough_map):
    m, g = rough_map
    xyz = np.stack([g["x"], g["y"], g["z"]], axis=1)
    dist = compose_ref.distances(xyz, 20, workers=16)
    for mul in (0.0, 1.0, 3.0):
        for tt in (0.0, 0.3, 10.0):
            thr = compose_ref.threshold(dist, mul)
            keep = dist.astype(np.float64) <= thr
            t = g["travers"].astype(np.float64)
            ref = (g[keep & (t > tt)], g[keep & (t <= tt)], int(g.shape[0] - keep.sum()), thr, dist)
            compare(m, g, "rough", stddev_mul=mul, tt=tt, ref=ref)
            if tt == 10.0:
                assert m.local_compose(20, mul, tt)[0].shape[0] == 0           # above every value: an empty road
    removed0, removed3 = m.local_compose(20, 0.0)[2], m.local_compose(20, 3.0)[2]
    assert removed0 > removed3 > 0


@pytest.mark.one_pipeline
def test_small_clouds_remove_nothing():
    L = 64
    for n in (0, 1, 20, 21):
        e = np.full((L, L), EMPTY, F32)
        e.reshape(-1)[np.arange(n) * 97 + 5] = 0.5
        m = scene_map(L, 0.1, e, traver=np.full((L, L), 0.5, F32), seed=n)
        g = capture_previous(m)
        assert g.shape[0] == n
        road, obstacle, removed, thr = m.local_compose(20)
        dist = m.local_compose_distances(20)
        if n <= 20:
            assert removed == 0 and road.tobytes() == g.tobytes() and obstacle.shape[0] == 0 and thr == float("inf")
            assert dist.shape[0] == n and np.isinf(dist).all() and m.debug_get("compose_far_points") == 0
        else:
            compare(m, g, "n = mean_k + 1")


# ---- 5. NULL outputs and errors ----------------------------------------------------------------------------------------------------
@pytest.mark.one_pipeline
def test_null_outputs(rough_map):
    m, g = rough_map
    lib, h = m._lib, m._h
    road, obstacle, removed, thr = m.local_compose()
    p = _lib.ComposeParams(20, 1.0, 0.0, 0)
    counts, t = (C.c_int * 3)(), C.c_double()
    assert lib.gem_local_compose(h, C.byref(p), None, None, counts, C.byref(t)) == 0
    assert tuple(counts) == (road.shape[0], obstacle.shape[0], removed) and bits(t.value) == bits(thr)
    buf = np.zeros(g.shape[0] + 1, local_ref.POINT)
    assert lib.gem_local_compose(h, C.byref(p), buf.ctypes.data_as(C.c_void_p), None, None, None) == 0
    assert buf[:road.shape[0]].tobytes() == road.tobytes() and not buf[road.shape[0]:].view(np.uint8).any()
    buf[:] = 0
    assert lib.gem_local_compose(h, C.byref(p), None, buf.ctypes.data_as(C.c_void_p), counts, None) == 0
    assert buf[:obstacle.shape[0]].tobytes() == obstacle.tobytes() and counts[1] == obstacle.shape[0]
    n = C.c_int()
    assert lib.gem_local_compose_distances(h, C.byref(p), None, C.byref(n)) == 0 and n.value == g.shape[0]
    assert m.local_compose(want_road=False, want_obstacle=False)[:3] == (road.shape[0], obstacle.shape[0], removed)


@pytest.mark.one_pipeline
def test_error_cases():
    L = 32
    rng = np.random.default_rng(3)
    m = ElevationMap(L, 0.1)
    m.set_layer("elevation", rng.uniform(0, 1, (L, L)).astype(F32)); m.set_layer("traver", rng.uniform(0, 1, (L, L)).astype(F32))
    lib, h = m._lib, m._h
    ok = _lib.ComposeParams(20, 1.0, 0.0, 0)
    counts, t, n = (C.c_int * 3)(7, 7, 7), C.c_double(7.0), C.c_int(7)
    buf = np.zeros(L * L, local_ref.POINT)
    vp = buf.ctypes.data_as(C.c_void_p)

    def both(p):
        a = lib.gem_local_compose(h, p, vp, vp, counts, C.byref(t))
        b = lib.gem_local_compose_distances(h, p, vp, C.byref(n))
        return a, b

    assert both(C.byref(ok)) == (INV, INV)                                    # not enabled
    m.local_enable(16)
    assert both(C.byref(ok)) == (INV, INV)                                    # no capture
    m.local_capture()
    assert both(C.byref(ok)) == (INV, INV)                                    # no keep_previous yet
    m.local_keep_previous()
    assert both(None) == (INV, INV)
    for bad in (_lib.ComposeParams(0, 1.0, 0.0, 0), _lib.ComposeParams(33, 1.0, 0.0, 0), _lib.ComposeParams(-1, 1.0, 0.0, 0),
                _lib.ComposeParams(20, float("nan"), 0.0, 0), _lib.ComposeParams(20, float("inf"), 0.0, 0)):
        assert both(C.byref(bad)) == (INV, INV)
    assert tuple(counts) == (7, 7, 7) and t.value == 7.0 and n.value == 7 and not buf.view(np.uint8).any()       # nothing written
    assert b"mean_k" in lib.gem_last_error(h) or b"stddev_mul" in lib.gem_last_error(h)
    g = m.local_grid_cloud()
    compare(m, g, "after the errors")                                          # ... and the handle is as usable as before
    w = ElevationMap(L, 0.1)
    w.comm_init_loopback(9518, 1, 0, tile_strips=False)
    assert w._lib.gem_local_compose(w._h, C.byref(ok), None, None, counts, None) == INV
    m.local_enable(0)
    assert both(C.byref(ok)) == (INV, INV)                                    # switched off


# ---- 6. allocation, threads, the facade --------------------------------------------------------------------------------------------
@pytest.mark.one_pipeline
def test_no_allocation_on_the_second_call():
    L, rng = 160, np.random.default_rng(31)
    e = rng.normal(0, 0.05, (L, L)).astype(F32)
    e[rng.random((L, L)) < 0.3] = EMPTY
    m = scene_map(L, 0.05, e, seed=31)

    def loop():
        out = []
        for k, xy in enumerate(trajectory(6, step=0.15, per_heading=1)):
            m.move([xy[0], xy[1], 0.0])
            m.set_layer("elevation", e)                   # (a move empties the cells that enter the window)
            g = capture_previous(m)
            out.append(compare(m, g, f"allocation loop {k}", mean_k=(20, 32)[k & 1]))
        return out

    a0 = m.debug_get("arena_allocations")
    first = loop()
    a1 = m.debug_get("arena_allocations")
    second = loop()
    a2 = m.debug_get("arena_allocations")
    assert len(first) == len(second) == 6 and a1 > a0 and a2 == a1, (a0, a1, a2)


@pytest.mark.one_pipeline
def test_second_thread_while_the_frame_loop_runs(oracle_mod):
    """The composing thread calls while the callback thread fuses, captures and ray-traces.  The frame loop leaves keep_previous alone
    meanwhile: its captures go to the other slot, so the previous capture -- and the answer -- must stay what they were."""
    L, res = 96, 0.1
    p = Pair(oracle_mod, L, res)
    for k, xy in enumerate(trajectory(3, step=0.3, per_heading=1)):
        p.move(xy); p.add(k, xy, n=20000)
        p.capture(p.feature(), k)
        g = p.gpu.local_grid_cloud()
        p.keep_previous()
    ref = compose_ref.compose(g, workers=16)
    stop, errors, frames = threading.Event(), [], [0]

    def frame_loop():
        try:
            k = 3
            while not stop.is_set() and k < 200:
                xy = (0.6 + 0.01 * k, 0.3)
                p.gpu.move([xy[0], xy[1], 0.5])
                from gem_amd import SensorModel, synth
                cloud = synth.random_cloud(k, 20000, 0.4 * L * res, z_sigma=0.15)
                p.gpu.add(synth._frame_for(synth.pose_matrix(xy[0], xy[1], 0.5, 0.0), SensorModel.velodyne()), cloud)
                p.gpu.map_feature(fetch=False)
                p.gpu.local_capture()
                p.gpu.raytracing()
                k += 1
                frames[0] += 1
        except Exception as e:                            # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=frame_loop)
    t.start()
    try:
        for i in range(12):
            compare(p.gpu, g, f"second thread, call {i}", ref=ref)
    finally:
        stop.set()
        t.join(120)
    assert not errors, errors
    assert frames[0] > 0 and not t.is_alive()


@pytest.mark.one_pipeline
def test_cpp_compose_facade(tmp_path):
    """... with the spike scene's exact removed count from the restatement: L = 32, res = 0.1f, centre 0, start 0, every cell at
    0.25 m but [16][16] at 50.25 m; the count does not depend on which cell of the lattice the spike is, away from the rim."""
    L, r = 32, float(F32(0.1))
    u = np.arange(L)
    x = ((0.0 + (0.5 * (L * r) - 0.5 * r)) + r * (-u).astype(np.float64)).astype(F32)
    rec = np.zeros(L * L, local_ref.POINT)
    X, Y = np.meshgrid(x, x, indexing="ij")
    rec["x"], rec["y"], rec["z"], rec["travers"] = X.reshape(-1), Y.reshape(-1), 0.25, 0.5
    rec["z"][16 * L + 16] = 50.25
    removed = compose_ref.compose(rec, 20, 3.0, 0.0, sqrt_double=True)[2]
    assert removed >= 1
    exe = build_compose_facade_check(tmp_path / "compose_facade_check")
    res = subprocess.run([str(exe), "1", str(removed)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
