"""The VoxelGrid pre-filter without a device: hand-derived known answers for every rule of the contract (include/gem_hip.h,
gem_voxel_device) against tests/voxel_ref.py -- the reference the GPU tests compare with bit for bit -- and the product's host side:
the launch-file presets and the ctypes twin of gem_voxel_params against the header."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import voxel_ref as vr  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
F32 = np.float32
NAN = np.float32(np.nan)


def pts(*rows):
    return np.array(rows, F32).reshape(-1, 4)


def test_two_point_voxel_and_order_of_voxels():
    a = pts([0.01, 0.02, 0.03, 1.0], [0.31, 0.02, 0.03, 5.0], [0.07, 0.05, 0.09, 3.0])
    out, _, m = vr.stage(a, leaf=0.1)
    assert m == 2
    # voxel (0, 0, 0): points 0 and 2, summed in input order from +0; voxel (3, 0, 0) holds point 1 alone
    want0 = [(F32(0) + F32(0.01) + F32(0.07)) / F32(2), (F32(0) + F32(0.02) + F32(0.05)) / F32(2),
             (F32(0) + F32(0.03) + F32(0.09)) / F32(2), F32(2.0)]
    assert np.array_equal(out[0], np.array(want0, F32))
    assert np.array_equal(out[1], a[1])
    assert np.isnan(out[2, :3]).all() and out[2, 3] == 0.0


def test_crowded_voxel_sums_in_input_order():
    # intensities 1e8, 1, -1e8 in one voxel: sequentially (1e8 + 1) - 1e8 = 0 in float; any other order gives 1/3 or 0 differently
    a = pts([0.5, 0.5, 0.5, 1e8], [0.52, 0.5, 0.5, 1.0], [0.5, 0.55, 0.5, -1e8], [0.5, 0.5, 0.58, 0.0])
    out, _, m = vr.stage(a, leaf=1.0)
    assert m == 1
    assert out[0, 3] == F32(0.0)
    b = a[[0, 2, 1, 3]]
    assert vr.stage(b, leaf=1.0)[0][0, 3] == F32(1.0) / F32(4)


def test_negative_zero_sums_to_positive_zero():
    a = pts([-0.0, -0.0, -0.0, -0.0], [-0.0, -0.0, -0.0, -0.0])
    out, _, m = vr.stage(a, leaf=0.1)
    assert m == 1
    assert (out[0].view(np.uint32) == 0).all()            # +0.0: the sums start from +0.0f


def test_uint32_voxel_order():
    # d = 1290 per axis (1290^3 <= INT32_MAX: no overflow) but div = 1291 (min's fraction above max's), so the far voxel's idx is
    # 1291^3 - 1 > INT32_MAX: as uint32 it sorts LAST, as int32 it would sort first
    a = pts([1290.1, 1290.1, 1290.1, 2.0], [0.9, 0.9, 0.9, 1.0], [600.5, 0.9, 0.9, 3.0])
    out, _, m = vr.stage(a, leaf=1.0)
    assert m == 3
    assert list(out[:3, 3]) == [1.0, 3.0, 2.0]
    assert 1291 ** 3 - 1 > 2 ** 31 - 1 and 1290 ** 3 <= 2 ** 31 - 1


def test_negative_limits():
    a = pts([-1.0, 0, 0, 1], [-0.5, 0, 0, 2], [0.99, 0, 0, 3], [1.0, 0, 0, 4], [5.0, 0, 0, 5])
    out, _, m = vr.stage(a, leaf=0.01, field="x", lo=-1.0, hi=1.0, negative=True)
    assert m == 3
    assert list(out[:3, 3]) == [1.0, 4.0, 5.0]             # inside the open interval (-1, 1) is dropped, the limits are kept


def test_nan_intensity_under_an_intensity_field():
    a = pts([0.0, 0.0, 0.0, NAN], [5.0, 0.0, 0.0, 50.0], [9.0, 0.0, 0.0, 2.0])
    out, _, m = vr.stage(a, leaf=1.0, field="intensity", lo=0.0, hi=10.0)
    assert m == 2                                          # NaN fails both comparisons: kept; 50 is out
    assert np.isnan(out[0, 3]) and out[1, 3] == 2.0


def test_float_against_double_limit():
    # float(0.1) > 0.1: the point at x = 0.1f shapes the bounds (float test) but is not output (double test)
    a = pts([F32(0.1), 0.0, 0.0, 7.0], [-0.25, 0.0, 0.0, 1.0])
    inb, surv = vr._tests(a, "x", -10.0, 0.1, False)
    assert inb.tolist() == [True, True] and surv.tolist() == [False, True]
    out, _, m = vr.stage(a, leaf=0.1, field="x", lo=-10.0, hi=0.1)
    assert m == 1 and out[0, 3] == 1.0
    # the bounds it shaped: with a leaf that makes the extent overflow, the stage passes its input through
    o2, _, m2 = vr.stage(pts([F32(0.1), 0, 0, 7], [-0.25, 1e3, 1e3, 1]), leaf=1e-4, field="x", lo=-10.0, hi=0.1)
    assert m2 == 2


def test_overflow_passes_the_input_through():
    a = pts([0, 0, 0, 1], [NAN, 1, 1, 2], [900, 900, 900, 3], [5, 5, 5, 4])
    rgb = np.array([1, 2, 3, 4], np.uint32)
    out, ro, m = vr.stage(a, rgb, leaf=1e-3)
    assert m == 4
    assert np.array_equal(out.view(np.uint32), a.view(np.uint32)) and np.array_equal(ro, rgb)   # NaN point included


def test_zero_survivors():
    out, _, m = vr.stage(pts([NAN, 0, 0, 1], [0, np.inf, 0, 1]), leaf=0.1)
    assert m == 0 and np.isnan(out[:, :3]).all() and (out[:, 3] == 0).all()
    out, _, m = vr.stage(pts([20, 0, 0, 1]), leaf=0.1, field="x", lo=-10, hi=10)
    assert m == 0
    assert vr.stage(np.zeros((0, 4), F32), leaf=0.1)[2] == 0


def test_rgb_centroid():
    a = pts([0, 0, 0, 0], [0.01, 0, 0, 0], [0.02, 0, 0, 0])
    rgb = np.array([(10 << 16) | (0 << 8) | 255, (11 << 16) | (1 << 8) | 255, (12 << 16) | (1 << 8) | 254], np.uint32)
    _, ro, m = vr.stage(a, rgb, leaf=1.0)
    assert m == 1 and ro[0] == (11 << 16) | (0 << 8) | 254     # 33/3, 2/3 -> 0, 764/3 = 254.67 -> 254


def test_chain_equals_single_stages():
    rng = np.random.default_rng(4)
    a = np.concatenate([rng.normal(0, 20, (5000, 3)), rng.uniform(0, 100, (5000, 1))], 1).astype(F32)
    a[rng.random(5000) < 0.05, 1] = NAN
    rgb = rng.integers(0, 1 << 24, 5000).astype(np.uint32)
    from gem_amd import VoxelStage
    chain = VoxelStage.filter_kitti_launch()
    out, ro, m = vr.voxel(a, rgb, chain)
    cur, cr, k = a, rgb, a.shape[0]
    for st in chain:
        o, r, k = vr.stage(cur[:k] if cur is not a else cur, cr[:k] if cr is not rgb else cr, **vr.stage_args(st))
        cur, cr = o, r
    assert m == k and 0 < m < a.shape[0]
    assert np.array_equal(out[:m].view(np.uint32), cur[:m].view(np.uint32)) and np.array_equal(ro[:m], cr[:m])
    assert np.isnan(out[m:, :3]).all() and (ro[m:] == 0).all()


def test_launch_presets():
    from gem_amd import VoxelStage, _lib
    (f,) = VoxelStage.filter_launch()
    assert (f.leaf_size, f.field, f.limit_min, f.limit_max, f.limit_negative) == (0.1, "x", -10.0, 10.0, False)
    k = VoxelStage.filter_kitti_launch()
    assert [(s.leaf_size, s.field, s.limit_min, s.limit_max, s.limit_negative) for s in k] == \
        [(0.2, "x", -40.0, 40.0, False), (0.2, "z", -25.0, 25.0, False), (0.2, "y", -40.0, 40.0, False)]
    p = f.to_struct()
    assert list(p.leaf) == [float(F32(0.1))] * 3 and p.field == _lib.VOXEL_FIELD_X and p.limit_max == 10.0
    d = VoxelStage().to_struct()                               # PCL's defaults
    assert d.field == _lib.VOXEL_FIELD_NONE and d.limit_min == -vr.FLT_MAX and d.limit_max == vr.FLT_MAX
    with pytest.raises(ValueError):
        VoxelStage(0.1, "rgb").to_struct()
    rng = np.random.default_rng(9)
    a = rng.normal(0, 15, (20000, 4)).astype(F32)
    for stages in (VoxelStage.filter_launch(), k):
        assert 0 < vr.voxel(a, None, stages)[2] < a.shape[0]


def test_ctypes_params_match_the_header(tmp_path):
    from gem_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gem_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(gem_voxel_params), offsetof(gem_voxel_params, leaf),\n'
                   '         offsetof(gem_voxel_params, field), offsetof(gem_voxel_params, limit_min), offsetof(gem_voxel_params, limit_max),\n'
                   '         offsetof(gem_voxel_params, limit_negative), offsetof(gem_voxel_params, reserved), GEM_VOXEL_FIELD_NONE,\n'
                   '         GEM_VOXEL_FIELD_X, GEM_VOXEL_FIELD_Y, GEM_VOXEL_FIELD_Z, GEM_VOXEL_FIELD_INTENSITY);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    cc = next((c for c in ("cc", "gcc", "clang", "g++") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    if cc is None:
        pytest.fail("no host C compiler")
    lang = ["-x", "c"] if cc != "g++" else []
    subprocess.run([cc, *lang, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = _lib.VoxelParams
    want = [C.sizeof(P), P.leaf.offset, P.field.offset, P.limit_min.offset, P.limit_max.offset, P.limit_negative.offset,
            P.reserved.offset, _lib.VOXEL_FIELD_NONE, _lib.VOXEL_FIELD_X, _lib.VOXEL_FIELD_Y, _lib.VOXEL_FIELD_Z, _lib.VOXEL_FIELD_INTENSITY]
    assert got == want
