"""The rolling-window local map on the device (gem_local_*) against the restatement of tests/local_ref.py, driven from the oracle's
show(), bit for bit:

  1. a node-ordered frame loop (move -> add -> map_feature -> capture -> spill -> raytracing with lowest tracking -> keep_previous)
     over a trajectory that turns through all eight shift-sign cases, on even and odd L, default and explicit show geometry:
     every spill, its replaced count, every grid cloud and the final export;
  2. the capture is taken before raytracing: a cell raytracing deletes afterwards still spills;
  3. growth from a capacity of 16, and no allocation in a second identical loop;
  4. export with clear in the middle of a loop;
  5. the error cases (GEM_ERR_INVALID, layers untouched);
  6. the C++ gem::LocalMap (tests/cpp/local_facade_check.cpp) as a child process."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gem_amd import ElevationMap, SensorModel, _lib, synth

sys.path.insert(0, str(Path(__file__).resolve().parent))
import local_ref  # noqa: E402
from test_local_map_cpu import build_local_facade_check  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
HEADINGS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]     # all eight shift-sign cases


def trajectory(frames, step=0.2, per_heading=5):
    p, out = np.zeros(2), []
    for k in range(frames):
        d = HEADINGS[(k // per_heading) % len(HEADINGS)]
        if k:
            p = p + step * np.array(d, float)
        out.append(p.copy())
    return out


class Pair:
    """the device map and the oracle in lockstep, plus the restated local map"""

    def __init__(self, oracle_mod, L, res, capacity=1 << 12, explicit=False):
        self.L, self.res, self.explicit = L, res, explicit
        self.gpu, self.ref = ElevationMap(L, res), oracle_mod.OracleMap(L, res)
        self.gpu.set_lowest_tracking(True)
        self.gpu.set_layer("lowest", self.ref.layer("lowest"))
        self.gpu.local_enable(capacity)
        self.local, self.cap, self.prev = {}, None, None
        self.center = np.zeros(2, F32)

    def move(self, xy, z=0.5):
        g = self.gpu.move([xy[0], xy[1], z]); o = self.ref.move([xy[0], xy[1], z])
        assert np.array_equal(g[0], np.asarray(o[0], F32)) and tuple(g[1]) == tuple(o[1])
        shift = (np.asarray(g[0], F32) - self.center).astype(F32)
        self.center = np.asarray(g[0], F32)
        return shift

    def add(self, seed, xy, n=3000):
        rng = np.random.default_rng(seed)
        c = synth.random_cloud(seed, n, 0.4 * self.L * self.res, z_sigma=0.15)
        rgb = rng.integers(0, 1 << 24, c.shape[0]).astype(np.uint32)
        f = synth._frame_for(synth.pose_matrix(xy[0], xy[1], 0.5, 0.1 * seed), SensorModel.velodyne())
        self.gpu.add(f, c, rgb=rgb); self.ref.add(f, c, rgb=rgb)

    def feature(self):
        o = self.ref.map_feature()
        self.gpu.map_feature(fetch=False)
        self.gpu.set_layer("traver", o["traver"])         # (rough / slope agree to a tolerance only; they are not in the records)
        return o

    def capture(self, feat, k=0):
        if self.explicit:                                 # visualMap_'s own geometry, not the map's: doubles, an off-centre position
            length, res = self.L * self.res + 0.125 * (k % 3), self.res
            pos = (float(self.center[0]) + 0.013, float(self.center[1]) - 0.021)
            o = self.ref.show(feat["rough"], feat["slope"], map_length=length, resolution=res, position=pos)
            self.gpu.local_capture(length, res, pos)
        else:
            res = float(F32(self.res))
            length, pos = self.L * res, (float(self.center[0]), float(self.center[1]))
            o = self.ref.show(feat["rough"], feat["slope"])
            self.gpu.local_capture()
        self.cap = local_ref.capture(o, self.L, length, res, pos, self.ref.pose()[1])
        g = self.gpu.local_grid_cloud()
        assert g.tobytes() == local_ref.grid_cloud(self.cap).tobytes()

    def keep_previous(self):
        self.gpu.local_keep_previous()
        self.prev = self.cap

    def spill(self, shift, frame):
        g, rg = self.gpu.local_spill(self.center, shift)
        o, ro = local_ref.spill(self.prev, self.center, shift, self.local)
        assert g.size == o.size and g.tobytes() == o.tobytes(), f"frame {frame}: {g.size} spilled, restatement {o.size}"
        assert rg == ro, f"frame {frame}: replaced {rg} != {ro}"
        assert self.gpu.local_size() == len(self.local)
        return g.size

    def raytracing(self):
        self.gpu.raytracing(); self.ref.raytracing()
        assert np.array_equal(self.gpu.layer("elevation"), self.ref.layer("elevation"))

    def gate(self, shift):
        # if (abs(delta_x) >= resolution_ || abs(delta_y) >= resolution_ && initFlag == 0 && JumpFlag == 0)   (EMg.cpp:715)
        return abs(float(shift[0])) >= self.res or abs(float(shift[1])) >= self.res

    def check_export(self, clear=False):
        g = self.gpu.local_export(clear)
        assert g.tobytes() == local_ref.export(self.local).tobytes()
        if clear:
            self.local.clear()
            assert self.gpu.local_size() == 0


def run_frames(p: Pair, frames, seed0=0, clear_at=None, adds=True):
    spilled = 0
    for k, xy in enumerate(trajectory(frames)):
        shift = p.move(xy)
        if adds:
            p.add(seed0 + k, xy)
        feat = p.feature()
        p.capture(feat, k)
        if k == 0:
            p.keep_previous()                             # the init frame: prevMap_ = map_.visualMap_ (EMg.cpp:620-621)
        if p.gate(shift):
            spilled += p.spill(shift, k)
        if clear_at is not None and k == clear_at:
            p.check_export(clear=True)
        p.raytracing()
        p.keep_previous()
    return spilled


@pytest.mark.parametrize("L,explicit", [(48, False), (49, True), (49, False), (48, True)])
def test_trajectory_bit_identical(oracle_mod, L, explicit):
    p = Pair(oracle_mod, L, 0.1, explicit=explicit)
    spilled = run_frames(p, 40)
    assert spilled > 200 and len(p.local) > 100
    p.check_export()
    assert p.gpu.local_size() == len(p.local)


@pytest.mark.one_pipeline
def test_capture_before_raytracing(oracle_mod):
    """an obstacle cell raytracing deletes after the capture is in the previous capture, and spills when it leaves the window"""
    L, res = 32, 0.1
    p = Pair(oracle_mod, L, res)
    p.move((0.0, 0.0))
    e = np.zeros((L, L), F32); t = np.full((L, L), 0.9, F32)
    e[5, 9], t[5, 9] = 5.0, 0.0                          # a tall obstacle away from the centre row / column
    for name, v in (("elevation", e), ("traver", t), ("variance", np.full((L, L), 1e-4, F32)), ("lowest", np.zeros((L, L), F32))):
        p.gpu.set_layer(name, v); p.ref.set_layer(name, v)
    feat = {"rough": np.zeros((L, L), F32), "slope": np.zeros((L, L), F32)}
    p.capture(feat)
    p.keep_previous()
    p.raytracing()
    assert p.gpu.layer("elevation")[5, 9] == -10.0        # deleted after the capture
    shift = np.array([L * res, 0.0], F32)                # the whole window is left behind
    p.center = p.center + shift
    n = p.spill(shift, 0)
    assert n == L * L
    g = p.gpu.local_export()
    assert np.any(g["z"] == F32(5.0)) and np.count_nonzero(g["travers"] == 0.0) == 1


@pytest.mark.one_pipeline
def test_growth_and_no_allocation_once_grown(oracle_mod):
    L, res = 48, 0.1
    p = Pair(oracle_mod, L, res, capacity=16)
    rng = np.random.default_rng(5)
    layers = {"elevation": rng.uniform(-0.5, 0.5, (L, L)).astype(F32), "traver": rng.uniform(-0.2, 1.0, (L, L)).astype(F32),
              "variance": rng.uniform(1e-4, 1e-2, (L, L)).astype(F32), "intensity": rng.uniform(0, 100, (L, L)).astype(F32),
              "color_r": rng.integers(0, 256, (L, L)), "color_g": rng.integers(0, 256, (L, L)), "color_b": rng.integers(0, 256, (L, L))}
    layers["traver"][rng.random((L, L)) < 0.05] = np.nan

    def loop():
        p.move((0.0, 0.0))
        for name, v in layers.items():
            p.gpu.set_layer(name, v); p.ref.set_layer(name, v)
        p.gpu.local_enable(16)
        p.local, p.cap, p.prev = {}, None, None
        total = 0
        for k, xy in enumerate(trajectory(24, step=0.3, per_heading=3)):
            shift = p.move(xy, 0.0)
            feat = {"rough": np.zeros((L, L), F32), "slope": np.zeros((L, L), F32)}
            p.capture(feat, k)
            if k == 0:
                p.keep_previous()
            if p.gate(shift):
                total += p.spill(shift, k)
            p.keep_previous()
        p.check_export()
        return total

    a0 = p.gpu.debug_get("arena_allocations")
    first = loop()
    a1 = p.gpu.debug_get("arena_allocations")
    second = loop()
    a2 = p.gpu.debug_get("arena_allocations")
    assert first == second and len(p.local) > 64 * 16
    assert a1 > a0 and a2 == a1, (a0, a1, a2)


def test_clear_then_continue(oracle_mod):
    p = Pair(oracle_mod, 40, 0.1, capacity=64)
    run_frames(p, 20, seed0=100, clear_at=11)
    p.check_export(clear=True)
    assert p.gpu.local_size() == 0


@pytest.mark.one_pipeline
def test_error_cases(oracle_mod):
    L = 32
    m = ElevationMap(L, 0.1)
    lib, h = m._lib, m._h
    c2 = (C.c_float * 2)(0.3, 0.0)
    n, rep, nl = C.c_int(), C.c_int(), C.c_longlong()
    rng = np.random.default_rng(3)
    m.set_layer("elevation", rng.uniform(0, 1, (L, L)).astype(F32)); m.set_layer("traver", rng.uniform(0, 1, (L, L)).astype(F32))
    before = {k: m.layer(k) for k in ("elevation", "traver", "variance", "intensity")}
    buf = np.empty(L * L, local_ref.POINT)
    vp = buf.ctypes.data_as(C.c_void_p)
    INV = _lib.GEM_OK - 1
    # not enabled
    assert lib.gem_local_capture(h, 0.0, 0.0, None) == INV
    assert lib.gem_local_keep_previous(h) == INV
    assert lib.gem_local_grid_cloud(h, vp, C.byref(n)) == INV
    assert lib.gem_local_spill(h, c2, c2, vp, C.byref(n), C.byref(rep)) == INV
    assert lib.gem_local_export(h, vp, L * L, C.byref(nl), 0) == INV
    assert lib.gem_local_size(h, C.byref(nl)) == INV
    m.local_enable(16)
    # before any capture
    assert lib.gem_local_spill(h, c2, c2, vp, C.byref(n), C.byref(rep)) == INV
    assert lib.gem_local_keep_previous(h) == INV
    m.local_capture()
    assert lib.gem_local_spill(h, c2, c2, vp, C.byref(n), C.byref(rep)) == INV     # nothing kept as previous yet
    m.local_keep_previous()
    assert lib.gem_local_spill(h, c2, c2, vp, C.byref(n), C.byref(rep)) == 0 and n.value > 0
    # max_points too small
    assert lib.gem_local_export(h, vp, n.value - 1, C.byref(nl), 0) == INV
    assert lib.gem_local_export(h, vp, n.value, C.byref(nl), 0) == 0 and nl.value == m.local_size()
    for k, v in before.items():
        assert np.array_equal(m.layer(k), v, equal_nan=True), k
    # a handle with a communicator
    w = ElevationMap(L, 0.1)
    w.comm_init_loopback(9517, 1, 0, tile_strips=False)
    assert w._lib.gem_local_enable(w._h, 16) == INV
    assert w._lib.gem_local_capture(w._h, 0.0, 0.0, None) == INV
    m.local_enable(0)
    assert lib.gem_local_size(h, C.byref(nl)) == INV                          # switched off


@pytest.mark.one_pipeline
def test_cpp_local_facade(tmp_path):
    exe = build_local_facade_check(tmp_path / "local_facade_check")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
