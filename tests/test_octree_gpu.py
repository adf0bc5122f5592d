"""gem_octree_build / gem_octree_read / gem_local_compose_octrees against tests/octree_ref.py: the fullMapToMsg byte stream of the
road and obstacle ColorOcTrees, BYTE-IDENTICAL, no tolerance.

  1. hand cases and caller clouds against the literal pointer tree: one point, the eight-leaf collapse and the ninth point's expand,
     dense 2^3 / 4^3 / 8^3 / 16^3-leaf blocks (eight lanes per block, one wave per block, the host routine), keys on both sides of the
     origin (all 48 key bits vary) and far from it, invalid and out-of-range points, a device tensor;
  2. node order (move -> add -> map_feature -> capture -> raytracing -> keep_previous) on maps of 64 and 200 cells against the literal
     form, of 600 cells against the array form (which test_octree_cpu.py pins to the literal one); gem_local_compose_octrees equals
     gem_octree_build over the lists gem_local_compose returns, with that call's counts and threshold;
  3. a rolling surface and 0.6 m steps: the reference's own statistics say blocks were walked jointly (a per-leaf build fails here);
  4. non-default parameters, road and obstacle at different resolutions, NULL and size-only reads, the error cases, no allocation
     on a second call, a call from a second thread while the first runs the frame loop, the C++ facade."""
import ctypes as C
import struct
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest
import torch

from gem_amd import ElevationMap, _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import octree_ref as R  # noqa: E402
from test_compose_gpu import capture_previous, scene_map  # noqa: E402
from test_local_map_gpu import Pair, trajectory  # noqa: E402
from test_octree_cpu import build_octree_facade_check, cloud, eight  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
INV = _lib.GEM_OK - 1
STAT_KEYS = ("points_in", "points_keyed", "leaves_depth16", "pruned_leaves", "nodes", "bytes")


def bits(v):
    return struct.pack("<d", float(v))


def first_difference(a, b):
    n = min(len(a), len(b))
    x = np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8)
    return int(np.argmax(x)) // 8 if x.any() else n // 8


def check(m, slot, c, res, what, form="literal", **kw):
    """build `c` into `slot`, read it back, compare bytes and statistics with the reference; returns the reference's statistics of the
    array form (the coupled blocks) when form is 'array' or 'both'"""
    p = R.Params(res, **kw)
    st = m.octree_build(slot, c, res, **kw)
    got = m.octree_read(slot)
    want, ws = (R.build_literal if form != "array" else R.build_array)(c, p)
    print(f"[octree] {what}: res {res} points {st['points_in']} keyed {st['points_keyed']} nodes {st['nodes']} bytes {st['bytes']} "
          f"leaves {st['leaves_depth16']} pruned {st['pruned_leaves']} blocks {st['coupled_blocks']} fallback {st['fallback_points']} | "
          f"reference bytes {len(want)} first differing node {first_difference(got, want)}")
    assert len(got) == len(want) and got == want
    for k in STAT_KEYS:
        assert st[k] == ws[k], k
    if form == "literal":
        return ws
    arr = R.build_array(c, p)[1] if form == "both" else ws
    assert st["coupled_blocks"] == arr["coupled_blocks"] and st["fallback_points"] == arr["fallback_points"]
    return arr


@pytest.fixture
def emap():
    return ElevationMap(32, 0.1)


# ---- 1. hand cases and caller clouds -------------------------------------------------------------------------------------------------
@pytest.mark.one_pipeline
def test_hand_cases(emap):
    m = emap
    st = check(m, 2, cloud([(0.05, 0.05, 0.05, 10, 20, 30)]), 0.1, "one point")
    assert st["nodes"] == 17
    check(m, 2, cloud([(0.05, 0.05, 0.05, 100, 100, 100)] * 5 + [(0.05, 0.05, 0.05, 0, 0, 0)]), 0.1, "six hits")
    check(m, 2, cloud([(0.05, 0.05, 0.05, 255, 255, 255), (0.05, 0.05, 0.05, 9, 8, 7)]), 0.1, "white first")
    st = check(m, 3, cloud(eight()), 0.1, "eight leaves", form="both")
    assert st["coupled_blocks"] == [1, 0, 0] and st["pruned_leaves"] == 1
    st = check(m, 3, cloud(eight() + [(0.05, 0.05, 0.05, 1, 2, 3)]), 0.1, "ninth point")
    assert st["expands"] == 1
    c = cloud([(0.05, 0.05, 0.05, 200, 100, 50), (0.05, 0.05, 0.05, 20, 40, 250)])
    check(m, 2, c, 0.1, "two hits")
    a = m.octree_read(2)
    check(m, 2, c[::-1].copy(), 0.1, "two hits, permuted")
    assert m.octree_read(2) != a


@pytest.mark.one_pipeline
def test_invalid_and_out_of_range_points(emap):
    m = emap
    c = cloud([(np.nan, 0, 0, 1, 2, 3), (0, 4000.0, 0, 1, 2, 3), (0, 0, -np.inf, 1, 2, 3)])
    st = m.octree_build(2, c, 0.1)
    assert st["points_in"] == 3 and st["points_keyed"] == 0 and st["bytes"] == 0 and m.octree_read(2) == b""
    assert m.octree_build(2, c[:0], 0.1)["bytes"] == 0 and m.octree_size(2) == 0                      # the empty cloud
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-3.0, 3.0, (4000, 3))
    xyz[::7, 0] = np.nan; xyz[3::11, 2] = np.inf; xyz[5::13, 1] = 1.0e7; xyz[6::17, 1] = -1.0e7
    c = R.make_cloud(xyz, rng.integers(0, 256, (4000, 3)))
    st = check(m, 2, c, 0.25, "invalid mixed in", form="both")
    assert 0 < st["points_keyed"] < 4000
    # the ends of the key range: +-32768 * res (res = 0.25: exact)
    e = cloud([(-8192.0, 0, 0, 1, 2, 3), (-8192.25, 0, 0, 4, 5, 6), (8191.75, 8191.75, 8191.75, 7, 8, 9), (8192.0, 0, 0, 1, 1, 1),
               (-0.25, -0.25, -0.25, 9, 9, 9), (0.0, 0.0, 0.0, 3, 3, 3)])
    assert check(m, 3, e, 0.25, "key range ends", form="both")["points_keyed"] == 4


@pytest.mark.one_pipeline
def test_dense_blocks_take_their_walkers(emap):
    m = emap
    st = check(m, 2, R.dense_block(1, 0.2, hits=3, seed=1, extra=60), 0.2, "2^3 block", form="both")
    assert st["coupled_blocks"][0] >= 1
    st = check(m, 2, R.dense_block(2, 0.1, hits=2, seed=2, extra=80), 0.1, "4^3 block", form="both")
    assert st["coupled_blocks"][1] == 1 and st["fallback_points"] == 0
    st = check(m, 2, R.dense_block(2, 0.1, hits=7, seed=5), 0.1, "4^3 block, saturated", form="both")
    assert st["coupled_blocks"][1] == 1 and st["pruned_leaves"] == 1
    st = check(m, 3, R.dense_block(3, 0.1, hits=2, seed=4, extra=30), 0.1, "8^3 block (host)", form="both")
    assert st["coupled_blocks"][2] == 1 and st["fallback_points"] == 1024
    st = check(m, 3, R.dense_block(4, 0.1, hits=1, seed=7, extra=100, base=(0, -1, 0)), 0.1, "16^3 block (host)", form="both")
    assert st["coupled_blocks"][2] == 8 and st["fallback_points"] == 4096
    # several blocks of every kind in one cloud, on both sides of the origin
    parts = [R.dense_block(1, 0.1, hits=3, seed=10 + k, base=(k - 4, 2 * k - 7, k % 3 - 1)) for k in range(9)]
    parts += [R.dense_block(2, 0.1, hits=2, seed=30 + k, base=(k - 1, -k, k - 2)) for k in range(3)]
    c = np.concatenate(parts)
    c = c[np.random.default_rng(3).permutation(c.shape[0])]
    st = check(m, 2, c, 0.1, "many blocks", form="both")
    assert st["coupled_blocks"][0] >= 9 and st["coupled_blocks"][1] == 3


@pytest.mark.one_pipeline
def test_caller_clouds(emap):
    m = emap
    rng = np.random.default_rng(17)
    for k, (centre, spread, n, res) in enumerate((((0.0, 0.0, 0.0), 2.0, 30000, 0.2), ((100.0, -50.0, 3.0), 1.5, 30000, 0.1),
                                                  ((0.0, 0.0, 0.0), 0.4, 20000, 0.05), ((-1500.0, 900.0, 40.0), 6.0, 5000, 0.1))):
        xyz = np.asarray(centre) + rng.normal(0.0, spread, (n, 3)) * (1.0, 1.0, 0.1)
        c = R.make_cloud(xyz, rng.integers(0, 256, (n, 3)))
        check(m, 2 + (k & 1), c, res, f"caller cloud {k}", form="both")
    # ... the same bytes from a device tensor
    want = m.octree_read(3)
    d = torch.from_numpy(c.view(np.uint8).reshape(-1, 32).copy()).to("cuda:0")
    st = m.octree_build(2, d, 0.1)
    m.synchronize()
    assert m.octree_read(2) == want and st["points_in"] == c.shape[0]


@pytest.mark.one_pipeline
def test_non_default_parameters(emap):
    m = emap
    c = R.dense_block(2, 0.1, hits=4, seed=6, extra=500)
    for kw in (dict(prob_hit=0.9, clamp_min=0.2, clamp_max=0.99), dict(prob_hit=0.55), dict(clamp_max=0.8), dict(prob_hit=0.55, clamp_max=0.9999)):
        check(m, 2, c, 0.1, f"params {kw}", form="both", **kw)
    assert R.Params(0.1, prob_hit=0.55, clamp_max=0.9999).S > 40                     # a long table


# ---- 2. node order, compose_octrees ----------------------------------------------------------------------------------------------------
def compose_both(m, what, form, road_res=0.2, obstacle_res=0.1, **kw):
    """gem_local_compose's lists built through gem_octree_build, against the reference; then gem_local_compose_octrees against both.
    Returns the reference's array-form statistics of the two trees (or the literal form's)."""
    road, obstacle, removed, thr = m.local_compose(**kw)
    sr = check(m, 2, road, road_res, f"{what}: road list", form=form)
    so = check(m, 3, obstacle, obstacle_res, f"{what}: obstacle list", form=form)
    want = (m.octree_read(2), m.octree_read(3))
    nr, no, rem, t, st = m.local_compose_octrees(road_res, obstacle_res, **kw)
    assert (nr, no, rem) == (road.shape[0], obstacle.shape[0], removed) and bits(t) == bits(thr)
    assert m.octree_read(0) == want[0] and m.octree_read(1) == want[1]
    assert st[0]["bytes"] == len(want[0]) and st[1]["bytes"] == len(want[1]) and st[0]["points_in"] == nr and st[1]["points_in"] == no
    assert m.octree_read(2) == want[0] and m.octree_read(3) == want[1]            # the user slots are their own
    return sr, so


def node_order(oracle_mod, L, res, frames, points, form):
    p = Pair(oracle_mod, L, res)
    for k, xy in enumerate(trajectory(frames, step=4 * res, per_heading=2)):
        p.move(xy)
        p.add(k, xy, n=points)
        feat = p.feature()
        p.capture(feat, k)
        p.raytracing()
        p.keep_previous()
        compose_both(p.gpu, f"node L={L} frame {k}", form, sqrt_double=bool(k & 1))
    assert tuple(p.gpu.pose()[1]) != (0, 0)


def test_node_order_64(oracle_mod):
    node_order(oracle_mod, 64, 0.1, 4, 3000, "both")


@pytest.mark.one_pipeline
def test_node_order_200(oracle_mod):
    node_order(oracle_mod, 200, 0.05, 3, 40000, "both")


@pytest.mark.one_pipeline
def test_node_order_600(oracle_mod):
    node_order(oracle_mod, 600, 0.05, 2, 250000, "array")


# ---- 3. surfaces that couple leaves ------------------------------------------------------------------------------------------------------
@pytest.mark.one_pipeline
@pytest.mark.parametrize("kind", ["rolling", "steps"])
def test_surfaces_with_full_blocks(kind):
    """The road half (travers 1) is the half whose plateaus lie on the 0.2 m tree's block boundaries, the obstacle half (travers -1)
    the one raised by 0.1 m (octree_ref.scene_elevation).  The reference's statistics on the device's own lists must show blocks walked
    jointly in both trees, none of 512 leaves."""
    L = 200
    e = R.scene_elevation(L, 0.05, kind, seed=3).astype(F32)
    t = np.ones((L, L), F32)
    t[:, L // 2:] = -1.0
    m = scene_map(L, 0.05, e, traver=t, seed=41, move=(0.35, -0.2))
    g = capture_previous(m)
    assert g.shape[0] == L * L
    sr, so = compose_both(m, kind, "both")
    for s in (sr, so):
        assert s["coupled_blocks"][0] > 0 and s["coupled_blocks"][2] == 0 and s["fallback_points"] == 0
    if kind == "steps":
        assert sr["pruned_leaves"] > 0


# ---- 4. reads, errors, allocation, threads, the facade -----------------------------------------------------------------------------------
@pytest.mark.one_pipeline
def test_null_and_size_only_reads(emap):
    m = emap
    lib, h = m._lib, m._h
    c = R.dense_block(1, 0.2, hits=2, seed=8, extra=100)
    st = m.octree_build(2, c, 0.2)
    want = m.octree_read(2)
    n = C.c_size_t(0)
    assert lib.gem_octree_read(h, 2, None, 0, C.byref(n)) == 0 and n.value == len(want) == st["bytes"]
    assert lib.gem_octree_read(h, 2, None, 0, None) == 0
    buf = np.zeros(len(want) + 16, np.uint8)
    n.value = 0
    assert lib.gem_octree_read(h, 2, buf.ctypes.data_as(C.c_void_p), len(want) - 8, C.byref(n)) == INV          # too small: the size, no bytes
    assert n.value == len(want) and not buf.any()
    assert lib.gem_octree_read(h, 2, buf.ctypes.data_as(C.c_void_p), buf.shape[0], C.byref(n)) == 0
    assert buf[:len(want)].tobytes() == want and not buf[len(want):].any()
    p = _lib.OctreeParams(0.2, 0.0, 0.0, 0.0, 0)
    assert lib.gem_octree_build(h, 3, C.byref(p), c.ctypes.data_as(C.c_void_p), c.shape[0], None) == 0           # stats may be NULL
    assert m.octree_read(3) == want
    assert m.octree_size(0) == 0 and m.octree_read(1) == b""                                                    # never built


@pytest.mark.one_pipeline
def test_error_cases_leave_the_slots_unchanged():
    L = 32
    rng = np.random.default_rng(3)
    m = ElevationMap(L, 0.1)
    m.set_layer("elevation", rng.uniform(0, 1, (L, L)).astype(F32)); m.set_layer("traver", rng.uniform(-1, 1, (L, L)).astype(F32))
    lib, h = m._lib, m._h
    c = R.dense_block(1, 0.2, hits=2, seed=9, extra=50)
    m.octree_build(2, c, 0.2)
    want = m.octree_read(2)
    st = _lib.OctreeStats()
    st.nodes = 77
    vp = c.ctypes.data_as(C.c_void_p)
    ok = _lib.OctreeParams(0.2, 0.0, 0.0, 0.0, 0)
    bad = [_lib.OctreeParams(0.0, 0, 0, 0, 0), _lib.OctreeParams(-0.1, 0, 0, 0, 0), _lib.OctreeParams(float("nan"), 0, 0, 0, 0),
           _lib.OctreeParams(float("inf"), 0, 0, 0, 0), _lib.OctreeParams(0.2, 0.5, 0, 0, 0), _lib.OctreeParams(0.2, 0.3, 0, 0, 0),
           _lib.OctreeParams(0.2, 0.500001, 0, 0.999999, 0), _lib.OctreeParams(0.2, 0, 0, 0.4, 0)]
    for p in bad:
        assert lib.gem_octree_build(h, 2, C.byref(p), vp, c.shape[0], C.byref(st)) == INV
        assert lib.gem_octree_build_device(h, 2, C.byref(p), vp, c.shape[0], C.byref(st)) == INV
    assert lib.gem_octree_build(h, 2, None, vp, c.shape[0], C.byref(st)) == INV
    assert lib.gem_octree_build(h, 4, C.byref(ok), vp, c.shape[0], C.byref(st)) == INV
    assert lib.gem_octree_build(h, -1, C.byref(ok), vp, c.shape[0], C.byref(st)) == INV
    assert lib.gem_octree_build(h, 2, C.byref(ok), None, 5, C.byref(st)) == INV
    assert lib.gem_octree_build(h, 2, C.byref(ok), vp, -1, C.byref(st)) == INV
    n = C.c_size_t(5)
    assert lib.gem_octree_read(h, 4, None, 0, C.byref(n)) == INV and n.value == 5
    cp = _lib.ComposeParams(20, 1.0, 0.0, 0)
    counts, t = (C.c_int * 3)(7, 7, 7), C.c_double(7.0)
    st2 = (_lib.OctreeStats * 2)()

    def compose(p=cp, r=ok, o=ok):
        byref = lambda x: None if x is None else C.byref(x)
        return lib.gem_local_compose_octrees(h, byref(p), byref(r), byref(o), counts, C.byref(t), st2)

    assert compose() == INV                                                   # not enabled
    m.local_enable(16)
    assert compose() == INV                                                   # no capture
    m.local_capture()
    assert compose() == INV                                                   # no keep_previous yet
    m.local_keep_previous()
    assert compose(p=None) == INV and compose(p=_lib.ComposeParams(0, 1.0, 0.0, 0)) == INV
    assert compose(r=bad[0]) == INV and compose(o=bad[4]) == INV and compose(r=None) == INV
    assert tuple(counts) == (7, 7, 7) and t.value == 7.0 and st.nodes == 77
    assert m.octree_read(2) == want and m.octree_size(0) == 0 and m.octree_size(1) == 0
    assert compose() == 0 and m.octree_size(0) + m.octree_size(1) > 0          # ... and the handle is as usable as before
    road, obstacle, removed, thr = m.local_compose()
    assert tuple(counts) == (road.shape[0], obstacle.shape[0], removed) and bits(t.value) == bits(thr)
    assert m.octree_read(0) == R.build_literal(road, R.Params(0.2))[0]
    w = ElevationMap(L, 0.1)
    w.comm_init_loopback(9519, 1, 0, tile_strips=False)
    assert w._lib.gem_octree_build(w._h, 2, C.byref(ok), vp, c.shape[0], None) == INV
    assert w._lib.gem_local_compose_octrees(w._h, C.byref(cp), C.byref(ok), C.byref(ok), counts, None, None) == INV


@pytest.mark.one_pipeline
def test_no_allocation_on_the_second_call():
    L, rng = 160, np.random.default_rng(31)
    e = rng.normal(0, 0.05, (L, L)).astype(F32)
    m = scene_map(L, 0.05, e, seed=31)
    user = R.make_cloud(rng.normal(0, 1.0, (L * L, 3)), rng.integers(0, 256, (L * L, 3)))

    def loop():
        out = []
        for k, xy in enumerate(trajectory(4, step=0.15, per_heading=1)):
            m.move([xy[0], xy[1], 0.0])
            m.set_layer("elevation", e)
            capture_previous(m)
            m.local_compose_octrees()
            m.octree_build(2, user[:L * L - 100 * k], 0.1)
            out.append((m.octree_read(0), m.octree_read(1), m.octree_read(2)))
        return out

    a0 = m.debug_get("arena_allocations")
    first = loop()
    a1 = m.debug_get("arena_allocations")
    second = loop()
    a2 = m.debug_get("arena_allocations")
    assert len(first) == 4 and a1 > a0 and a2 == a1, (a0, a1, a2)
    assert all(len(x[0]) and len(x[1]) and len(x[2]) for x in first)


@pytest.mark.one_pipeline
def test_second_thread_while_the_frame_loop_runs(oracle_mod):
    """The composing thread builds the two trees while the callback thread fuses, captures and ray-traces; the frame loop leaves
    keep_previous alone meanwhile, so the previous capture -- and the bytes -- must stay what they were."""
    L, res = 96, 0.1
    p = Pair(oracle_mod, L, res)
    for k, xy in enumerate(trajectory(3, step=0.3, per_heading=1)):
        p.move(xy); p.add(k, xy, n=20000)
        p.capture(p.feature(), k)
        p.keep_previous()
    road, obstacle, removed, thr = p.gpu.local_compose()
    want = (R.build_literal(road, R.Params(0.2))[0], R.build_literal(obstacle, R.Params(0.1))[0])
    stop, errors, frames = threading.Event(), [], [0]

    def frame_loop():
        try:
            k = 3
            while not stop.is_set() and k < 200:
                xy = (0.6 + 0.01 * k, 0.3)
                p.gpu.move([xy[0], xy[1], 0.5])
                from gem_amd import SensorModel, synth
                c = synth.random_cloud(k, 20000, 0.4 * L * res, z_sigma=0.15)
                p.gpu.add(synth._frame_for(synth.pose_matrix(xy[0], xy[1], 0.5, 0.0), SensorModel.velodyne()), c)
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
            nr, no, rem, tt, _ = p.gpu.local_compose_octrees()
            assert (nr, no, rem) == (road.shape[0], obstacle.shape[0], removed) and bits(tt) == bits(thr)
            assert p.gpu.octree_read(0) == want[0] and p.gpu.octree_read(1) == want[1], f"call {i}"
    finally:
        stop.set()
        t.join(120)
    assert not errors, errors
    assert frames[0] > 0 and not t.is_alive()


@pytest.mark.one_pipeline
def test_cpp_octree_facade(tmp_path):
    exe = build_octree_facade_check(tmp_path / "octree_facade_check")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
