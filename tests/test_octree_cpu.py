"""The ColorOcTree contract of gem_octree_build (include/gem_hip.h), on the CPU: hand-checkable cases on the literal form of
tests/octree_ref.py, the array form against it, and the two facts the device build rests on."""
from __future__ import annotations

import math
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import octree_ref as R  # noqa: E402


def nodes_of(data):
    return [struct.unpack("<fBBBB", data[i:i + 8]) for i in range(0, len(data), 8)]


def cloud(points):
    """[(x, y, z, r, g, b)]"""
    a = np.asarray(points, dtype=np.float64).reshape(-1, 6)
    return R.make_cloud(a[:, :3], a[:, 3:].astype(np.uint8))


HIT = np.float32(math.log(0.7 / 0.3))
CMAX = np.float32(math.log(0.971 / 0.029))


def test_constants():
    p = R.Params(0.1)
    assert p.hit == HIT and p.cmax == CMAX and p.cmin == np.float32(math.log(0.1192 / 0.8808))
    assert p.S == 5 and p.f[5] == CMAX and p.f[4] < CMAX            # five hits reach cmax
    assert all(p.f[i] < p.f[i + 1] for i in range(5))


def test_one_point():
    data, st = R.build_literal(cloud([(0.05, 0.05, 0.05, 10, 20, 30)]), R.Params(0.1))
    assert len(data) == 136 and st["nodes"] == 17
    n = nodes_of(data)
    # key 32768 on every axis: bit 15 set, the rest clear -> child 7 under the root, child 0 below
    assert [m[4] for m in n] == [1 << 7] + [1] * 15 + [0]
    assert all(m[0] == HIT and m[1:4] == (10, 20, 30) for m in n)


def test_saturation_and_blend_after_it():
    pts = [(0.05, 0.05, 0.05, 100, 100, 100)] * 5
    d5, _ = R.build_literal(cloud(pts), R.Params(0.1))
    d6, _ = R.build_literal(cloud(pts + [(0.05, 0.05, 0.05, 0, 0, 0)]), R.Params(0.1))
    assert nodes_of(d5)[-1][0] == CMAX and nodes_of(d6)[-1][0] == CMAX
    assert nodes_of(d6)[-1][1:4] != nodes_of(d5)[-1][1:4]


def test_blend_by_hand():
    # second hit: value = 2 * hit (float), p = 1 - 1 / (1 + exp(value)); channel = (uint8)(prev * p + c * (0.99 - p))
    data, _ = R.build_literal(cloud([(0.05, 0.05, 0.05, 200, 100, 50), (0.05, 0.05, 0.05, 20, 40, 250)]), R.Params(0.1))
    v = np.float32(HIT + HIT)
    p = 1.0 - 1.0 / (1.0 + math.exp(float(v)))
    assert abs(p - 0.8448) < 1e-3                                                       # (7/3)^2 / (1 + (7/3)^2) = 49 / 58
    want = tuple(int(a * p + c * (0.99 - p)) for a, c in ((200, 20), (100, 40), (50, 250)))
    assert want == (171, 90, 78)
    assert nodes_of(data)[-1] == (v,) + want + (0,)


def test_white_point_leaves_colour_unset():
    data, _ = R.build_literal(cloud([(0.05, 0.05, 0.05, 255, 255, 255), (0.05, 0.05, 0.05, 9, 8, 7)]), R.Params(0.1))
    assert nodes_of(data)[-1][1:4] == (9, 8, 7)                                        # the second point SETS, it does not blend


def eight(res=0.1):
    return [((i & 1) * res + 0.05, ((i >> 1) & 1) * res + 0.05, ((i >> 2) & 1) * res + 0.05, 10 * (i + 1), 100, 200 - 10 * i)
            for i in range(8)]


def test_eight_leaves_collapse():
    data, st = R.build_literal(cloud(eight()), R.Params(0.1))
    assert st["prunes"] == 1 and st["nodes"] == 16 and st["pruned_leaves"] == 1 and st["leaves_depth16"] == 0
    last = nodes_of(data)[-1]
    # at the prune the eighth leaf is still white: the mean is over seven set colours; then the eighth point blends onto the parent
    r7 = sum(10 * (i + 1) for i in range(7)) // 7
    b7 = sum(200 - 10 * i for i in range(7)) // 7
    p = R.blend_p(HIT)
    assert last == (HIT, R.blend(r7, 80, p), R.blend(100, 100, p), R.blend(b7, 130, p), 0)


def test_ninth_point_expands():
    pts = eight() + [(0.05, 0.05, 0.05, 1, 2, 3)]
    data, st = R.build_literal(cloud(pts), R.Params(0.1))
    assert st["expands"] == 1 and st["nodes"] == 16 + 8
    n = nodes_of(data)
    parent_col = nodes_of(R.build_literal(cloud(eight()), R.Params(0.1))[0])[-1][1:4]
    assert n[15][4] == 255
    assert all(m[1:4] == parent_col and m[0] == HIT for m in n[17:])                 # the siblings carry the parent's colour
    assert n[16][0] == np.float32(HIT + HIT)


def test_keys():
    rf = 1.0 / 0.1
    assert R.axis_key(np.float32(-0.05), rf) == 32767
    assert R.axis_key(np.float32(-0.1), rf) == 32766                                   # the float is just below -0.1: floor(10 x) = -2
    assert R.axis_key(np.float32(0.0), rf) == 32768
    assert R.axis_key(np.float32(-8192.0), 4.0) == 0 and R.axis_key(np.float32(-8192.25), 4.0) is None          # -32768 * res
    assert R.axis_key(np.float32(8191.75), 4.0) == 65535 and R.axis_key(np.float32(8192.0), 4.0) is None         # +32768 * res
    assert R.axis_key(np.float32(-3276.8), rf) is None                                 # the float is below -3276.8
    for bad in (np.nan, np.inf, -np.inf):
        assert R.axis_key(np.float32(bad), rf) is None
    c = cloud([(np.nan, 0, 0, 1, 2, 3), (0, 4000.0, 0, 1, 2, 3), (0, 0, -np.inf, 1, 2, 3)])
    data, st = R.build_literal(c, R.Params(0.1))
    assert data == b"" and st["points_keyed"] == 0 and st["points_in"] == 3
    assert R.build_array(c, R.Params(0.1))[0] == b""


def test_empty_tree():
    assert R.build_literal(cloud([]), R.Params(0.2))[0] == b""
    assert R.build_array(cloud([]), R.Params(0.2))[0] == b""


def test_order_matters():
    c = cloud([(0.05, 0.05, 0.05, 200, 100, 50), (0.05, 0.05, 0.05, 20, 40, 250)])
    assert R.build_literal(c, R.Params(0.1))[0] != R.build_literal(c[::-1], R.Params(0.1))[0]


def test_params_rejected():
    for kw in (dict(resolution=0.0), dict(resolution=np.inf), dict(resolution=0.1, prob_hit=0.5),
               dict(resolution=0.1, prob_hit=0.500001, clamp_max=0.999999), dict(resolution=0.1, clamp_max=0.4)):
        with pytest.raises(ValueError):
            R.Params(**kw)
    assert R.Params(0.1, prob_hit=0.9, clamp_min=0.2, clamp_max=0.99).S == 3


# ---- fact 1: a leaf's value depends only on its hit count ------------------------------------------------------------------------
def test_value_is_a_function_of_the_hit_count():
    c = R.dense_block(1, 0.2, hits=7, seed=3, extra=40)
    p = R.Params(0.2)
    t = R.LiteralTree(p)
    t.insert(c)
    hits = {}
    for rec in c:
        k = R.point_key(rec, 1.0 / p.resolution)
        if k is not None:
            hits[R.morton(k)] = hits.get(R.morton(k), 0) + 1
    for m, h in hits.items():
        assert t.search(m).value == p.f[min(h, p.S)]
    assert t.stats["prunes"] > 0 and t.stats["expands"] > 0


# ---- array form == literal form --------------------------------------------------------------------------------------------------
ARRAY_CASES = {
    "level1": lambda: (R.dense_block(1, 0.2, hits=3, seed=1, extra=60), R.Params(0.2)),
    "level2": lambda: (R.dense_block(2, 0.1, hits=2, seed=2, extra=80), R.Params(0.1)),
    "level2_sat": lambda: (R.dense_block(2, 0.1, hits=7, seed=5), R.Params(0.1)),
    "level3": lambda: (R.dense_block(3, 0.1, hits=2, seed=4, extra=30), R.Params(0.1)),
    "steps": lambda: (R.lattice_scene(96, 0.05, "steps"), R.Params(0.2)),
    "rolling": lambda: (R.lattice_scene(64, 0.05, "rolling"), R.Params(0.1)),
    "params": lambda: (R.dense_block(2, 0.1, hits=4, seed=6, extra=50), R.Params(0.1, prob_hit=0.9, clamp_min=0.2, clamp_max=0.99)),
}


@pytest.mark.parametrize("name", sorted(ARRAY_CASES))
def test_array_form_equals_literal(name):
    c, p = ARRAY_CASES[name]()
    lit, ls = R.build_literal(c, p)
    arr, st = R.build_array(c, p)
    assert arr == lit
    for k in ("points_in", "points_keyed", "nodes", "bytes", "leaves_depth16", "pruned_leaves"):
        assert st[k] == ls[k], k
    if name == "level1":
        assert ls["prunes"] > 0 and ls["expands"] > 0 and st["coupled_blocks"][0] >= 1
    if name.startswith("level2"):
        assert ls["prunes_level"][2] > 0 and ls["expands"] > 0 and st["coupled_blocks"][1] == 1
    if name == "level3":
        assert st["coupled_blocks"][2] == 1 and st["fallback_points"] == 1024
    if name == "steps":
        assert ls["prunes"] > 0 and st["coupled_blocks"][0] > 0 and st["coupled_blocks"][2] == 0


# ---- fact 2: the prune / expand history is local to the maximal full block -------------------------------------------------------
def test_block_regrouping_equals_sequential_and_leaf_regrouping_does_not():
    c, p = R.lattice_scene(96, 0.05, "steps"), R.Params(0.2)
    seq, st = R.build_literal(c, p)
    assert st["prunes"] > 0
    assert R.build_literal(R.regroup(c, p, "block"), p)[0] == seq
    assert R.build_literal(R.regroup(c, p, "leaf"), p)[0] != seq
    c2, p2 = R.dense_block(2, 0.1, hits=3, seed=9, extra=200), R.Params(0.1)
    assert R.build_literal(R.regroup(c2, p2, "block"), p2)[0] == R.build_literal(c2, p2)[0]


# ---- the C++ facade ---------------------------------------------------------------------------------------------------------------
def build_octree_facade_check(out: Path) -> Path:
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc", "-std=c++17", "-O1", "-Wall", "-Werror",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "octree_facade_check.cpp"), "-o", str(out),
           f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_octree_facade_builds():
    """gem::LocalMap::compose_octrees / build_octree compile with hipcc against the installed header and the library; without a GPU
    the check exits early."""
    import tempfile
    from gem_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as td:
        exe = build_octree_facade_check(Path(td) / "octree_facade_check")
        res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: built)"), res.stdout + res.stderr


def test_python_binding_matches_the_header():
    """the ctypes twins of gem_octree_params / gem_octree_stats have the C layout (a double-aligned struct of 40 / 80 bytes)"""
    import ctypes as C
    from gem_amd import _lib
    assert C.sizeof(_lib.OctreeParams) == 40 and C.sizeof(_lib.OctreeStats) == 80
    for name in ("gem_octree_build", "gem_octree_build_device", "gem_local_compose_octrees", "gem_octree_read"):
        assert name in _lib.SIGNATURES
