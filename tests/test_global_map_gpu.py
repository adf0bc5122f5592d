"""The submap stack on the device (gem_global_*) against the restatement of tests/global_ref.py, bit for bit, order included (a NaN
key's x or y compares as NaN: its payload is the platform's):

  1. a node-ordered frame loop (move -> add -> map_feature -> capture -> spill -> raytracing -> keep_previous) with push_local every
     8 frames: every push against local_ref's export followed by the grid cloud, then a loop closure on the pushed stack;
  2. caller pushes of synthetic clouds with duplicate keys, overlaps, variances in and out of (0, 1), a NaN and an inf record;
  3. a loop closure with small random yaw / translation transforms, resolution 0.05 (a double) and 0 (the map's float): every
     submap, the fused count and the index -1 export;
  4. a second loop closure on the result;
  5. growth from a capacity of 16, and no allocation in a repeated run;
  6. the error cases (GEM_ERR_INVALID, the stack unchanged);
  7. the C++ gem::GlobalMap (tests/cpp/global_facade_check.cpp) as a child process."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gem_amd import ElevationMap, _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import global_ref  # noqa: E402
from test_global_map_cpu import build_global_facade_check  # noqa: E402
from test_local_map_gpu import Pair, trajectory  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def synthetic(rng, n, cx, cy=0.0, half=(6.0, 1.0), res=0.05):
    """n records around (cx, cy) on a res grid, most jittered: repeated cells give duplicate keys; variances in and out of (0, 1)"""
    out = np.zeros(n, global_ref.POINT)
    cells_x, cells_y = int(half[0] / res), int(half[1] / res)
    jitter = lambda: np.where(rng.random(n) < 0.3, 0.0, rng.uniform(-0.3, 0.3, n) * res)     # some on the cell borders
    out["x"] = (cx + res * rng.integers(-cells_x, cells_x, n) + jitter()).astype(F32)
    out["y"] = (cy + res * rng.integers(-cells_y, cells_y, n) + jitter()).astype(F32)
    out["z"] = rng.uniform(-1, 2, n).astype(F32)
    out["pad"] = 1.0
    for f in ("r", "g", "b"):
        out[f] = rng.integers(0, 256, n)
    out["covariance"] = rng.uniform(-0.2, 1.2, n).astype(F32)
    out["covariance"][rng.random(n) < 0.05] = 0.0
    out["covariance"][rng.random(n) < 0.05] = 1.0
    out["intensity"] = rng.uniform(0, 100, n).astype(F32)
    out["travers"] = rng.uniform(0, 1, n).astype(F32)
    out[n // 3]["x"] = np.nan
    out[n // 2]["y"] = np.inf
    return out


def transforms(rng, n):
    t = np.zeros((n, 4, 4), F32)
    for i in range(n):
        a = rng.uniform(-0.02, 0.02)
        c, s = np.cos(a), np.sin(a)
        t[i] = [[c, -s, 0, rng.uniform(-0.2, 0.2)], [s, c, 0, rng.uniform(-0.2, 0.2)], [0, 0, 1, rng.uniform(-0.05, 0.05)], [0, 0, 0, 1]]
    return t


def check_stack(m: ElevationMap, stack):
    assert m.global_count() == len(stack)
    for i, s in enumerate(stack):
        assert global_ref.same(m.global_export(i), s), f"submap {i}"
    assert global_ref.same(m.global_export(-1), global_ref.export_all(stack))


def pushed(m: ElevationMap, seed=11, S=6, n=5000, spacing=10.0):
    rng = np.random.default_rng(seed)
    stack = []
    for i in range(S):
        c = synthetic(rng, n, spacing * i)
        assert m.global_push(c) == i
        global_ref.push(stack, c)
    return stack, rng


def test_node_ordered_loop_push_local(oracle_mod):
    L, res = 48, 0.1
    p = Pair(oracle_mod, L, res)
    p.gpu.global_enable(1 << 12)
    stack, centres = [], []
    for k, xy in enumerate(trajectory(32)):
        shift = p.move(xy)
        p.add(k, xy)
        feat = p.feature()
        p.capture(feat, k)
        if k == 0:
            p.keep_previous()
        if p.gate(shift):
            p.spill(shift, k)
        if k % 8 == 7:
            i = p.gpu.global_push_local(True)
            assert i == global_ref.push_local(stack, p.local, p.cap)
            p.local.clear()
            assert p.gpu.local_size() == 0
            assert p.gpu.global_export(i).tobytes() == stack[i].tobytes(), f"push at frame {k}"
            centres.append([float(p.center[0]), float(p.center[1])])
        p.raytracing()
        p.keep_previous()
    assert len(stack) == 4 and all(s.size > 100 for s in stack)
    check_stack(p.gpu, stack)
    t = transforms(np.random.default_rng(1), len(stack))
    fused = p.gpu.global_loop_closure(t, centres, radius=25.0, resolution=0.1)
    assert fused == global_ref.loop_closure(stack, len(stack), t, centres, 25.0, 0.1)
    assert fused > 0
    check_stack(p.gpu, stack)


@pytest.mark.one_pipeline
@pytest.mark.parametrize("resolution", [0.05, 0.0])
def test_loop_closure_twice(resolution):
    m = ElevationMap(32, 0.05)
    m.global_enable(1 << 14)
    stack, rng = pushed(m)
    check_stack(m, stack)
    S = len(stack)
    centres = np.array([[10.0 * i, 0.0] for i in range(S)], F32)
    t = transforms(rng, S)
    fused = m.global_loop_closure(t, centres, 25.0, resolution)
    want = global_ref.loop_closure(stack, S, t, centres, 25.0, resolution, map_resolution=0.05)
    assert fused == want and fused > 100
    check_stack(m, stack)
    # a second loop closure on the result, clamped to the first four submaps, with a coincident centre (the k == i step)
    t2 = transforms(rng, S + 2)
    c2 = np.array([[0, 0], [0, 0], [10, 0.5], [20, -0.5], [40, 0], [50, 0], [60, 0], [70, 0]], F32)
    fused = m.global_loop_closure(t2, c2, 25.0, resolution)
    assert fused == global_ref.loop_closure(stack, S + 2, t2, c2, 25.0, resolution, map_resolution=0.05)
    check_stack(m, stack)


@pytest.mark.one_pipeline
def test_growth_and_no_allocation_once_grown():
    m = ElevationMap(32, 0.05)

    def run():
        m.global_enable(16)
        stack, rng = pushed(m, seed=4, S=5, n=3000)
        t = transforms(rng, 5)
        centres = [[10.0 * i, 0.0] for i in range(5)]
        fused = m.global_loop_closure(t, centres, 25.0, 0.05)
        assert fused == global_ref.loop_closure(stack, 5, t, centres, 25.0, 0.05)
        check_stack(m, stack)
        return fused, m.global_export(-1)

    a0 = m.debug_get("arena_allocations")
    f1, e1 = run()
    a1 = m.debug_get("arena_allocations")
    f2, e2 = run()
    a2 = m.debug_get("arena_allocations")
    assert f1 == f2 and global_ref.same(e1, e2)
    assert a1 > a0 and a2 == a1, (a0, a1, a2)


@pytest.mark.one_pipeline
def test_error_cases():
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    INV = _lib.GEM_OK - 1
    idx, ns, nl = C.c_int(), C.c_int(), C.c_longlong()
    one = np.zeros(1, global_ref.POINT)
    vp = one.ctypes.data_as(C.c_void_p)
    eye = np.tile(np.eye(4, dtype=F32).T.ravel(), 3).astype(F32)
    cen = np.zeros(6, F32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    # not enabled
    assert lib.gem_global_push_local(h, 1, C.byref(idx)) == INV
    assert lib.gem_global_push(h, vp, 1, C.byref(idx)) == INV
    assert lib.gem_global_loop_closure(h, 3, fp(eye), fp(cen), 25.0, 0.0, C.byref(nl)) == INV
    assert lib.gem_global_export(h, -1, None, 0, C.byref(nl)) == INV
    assert lib.gem_global_count(h, C.byref(ns)) == INV
    m.global_enable(16)
    stack, _ = pushed(m, seed=8, S=3, n=500)
    before = m.global_export(-1)

    def unchanged():
        assert m.global_count() == 3 and global_ref.same(m.global_export(-1), before)

    # push_local without a local map, then without a capture
    assert lib.gem_global_push_local(h, 1, C.byref(idx)) == INV
    m.local_enable(16)
    assert lib.gem_global_push_local(h, 1, C.byref(idx)) == INV
    unchanged()
    assert lib.gem_global_loop_closure(h, -1, fp(eye), fp(cen), 25.0, 0.0, C.byref(nl)) == INV
    assert lib.gem_global_loop_closure(h, 2, None, fp(cen), 25.0, 0.0, C.byref(nl)) == INV
    assert lib.gem_global_loop_closure(h, 2, fp(eye), None, 25.0, 0.0, C.byref(nl)) == INV
    for r in (float("inf"), float("nan"), -1.0):
        assert lib.gem_global_loop_closure(h, 3, fp(eye), fp(cen), r, 0.0, C.byref(nl)) == INV
    unchanged()
    for i in (-2, 3):
        assert lib.gem_global_export(h, i, None, 0, C.byref(nl)) == INV
    buf = np.empty(before.size, global_ref.POINT)
    assert lib.gem_global_export(h, -1, buf.ctypes.data_as(C.c_void_p), before.size - 1, C.byref(nl)) == INV
    assert lib.gem_global_push(h, None, 4, C.byref(idx)) == INV
    assert lib.gem_global_push(h, vp, -1, C.byref(idx)) == INV
    unchanged()
    # n_opt 0 and 1 with NULL arrays are fine and change nothing
    assert lib.gem_global_loop_closure(h, 0, None, None, 25.0, 0.0, C.byref(nl)) == 0 and nl.value == 0
    assert lib.gem_global_loop_closure(h, 1, None, None, 25.0, 0.0, C.byref(nl)) == 0 and nl.value == 0
    unchanged()
    # a handle with a communicator
    w = ElevationMap(32, 0.05)
    w.comm_init_loopback(9519, 1, 0, tile_strips=False)
    assert w._lib.gem_global_enable(w._h, 16) == INV
    assert w._lib.gem_global_count(w._h, C.byref(ns)) == INV
    m.global_enable(0)
    assert lib.gem_global_count(h, C.byref(ns)) == INV                       # switched off


@pytest.mark.one_pipeline
def test_cpp_global_facade(tmp_path):
    exe = build_global_facade_check(tmp_path / "global_facade_check")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
