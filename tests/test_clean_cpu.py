"""cleanPointCloud (SensorProcessorBase.cpp:89) without a GPU: the host half of include/gem_hip.h's raw-cloud entries --
gem_clean_params_for_model through ctypes, the SensorModel / C++ processors that call it -- and the numpy reference
(tests/clean_ref.py) the GPU tests compare the device compaction with."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))

import clean_ref  # noqa: E402

DBL_MIN, DBL_MAX = sys.float_info.min, sys.float_info.max


@pytest.fixture(scope="module")
def lib():
    from gem_amd import _lib
    return _lib.load()


def params(lib, model, lo=DBL_MIN, hi=DBL_MAX):
    from gem_amd import _lib
    out = _lib.CleanParams()
    rc = lib.gem_clean_params_for_model(model, lo, hi, C.byref(out))
    return rc, out


@pytest.mark.parametrize("model", [0, 2, 3])          # laser, stereo, perfect
def test_laser_stereo_perfect_remove_nan(lib, model):
    rc, p = params(lib, model, 0.2, 3.25)             # (cutoffs are the structured-light processor's only)
    assert rc == 0 and p.mode == clean_ref.REMOVE_NAN


def test_structured_light_reference_defaults(lib):
    """numeric_limits<double>::min() / ::max() (StructuredLightSensorProcessor.cpp:40-41) rounded to float: +0.0f and +inf."""
    rc, p = params(lib, 1)
    assert rc == 0 and p.mode == clean_ref.PASSTHROUGH_Z
    assert p.z_min == 0.0 and not np.signbit(np.float32(p.z_min))
    assert np.isposinf(p.z_max)
    assert (p.mode, np.float32(p.z_min), np.float32(p.z_max)) == clean_ref.params_for_model(1)


def test_structured_light_d435_cutoffs(lib):
    rc, p = params(lib, 1, 0.2, 3.25)                 # realsense_d435.yaml
    assert rc == 0 and p.mode == clean_ref.PASSTHROUGH_Z
    assert np.float32(p.z_min) == np.float32(0.2) and np.float32(p.z_max) == np.float32(3.25)
    from gem_amd import SensorModel
    m = SensorModel.realsense_d435()
    q = m.clean_params()
    assert (q.mode, q.z_min, q.z_max) == (p.mode, p.z_min, p.z_max)
    assert SensorModel.velodyne().clean_params().mode == clean_ref.REMOVE_NAN
    assert SensorModel.perfect().clean_params().mode == clean_ref.REMOVE_NAN


def test_cutoffs_round_to_nearest(lib):
    f32max = float(np.finfo(np.float32).max)
    half_ulp = 2.0 ** 103
    for v in (0.1, -0.1, 1.0 / 3.0, 5e-46, -5e-46, 1e-39, f32max, f32max + half_ulp * 0.99, f32max + half_ulp, -f32max - half_ulp, 1e300):
        rc, p = params(lib, 1, v, v)
        assert rc == 0
        want = clean_ref.to_float32(v)
        assert np.float32(p.z_min).tobytes() == want.tobytes(), (v, p.z_min, want)
    assert params(lib, 1, float("nan"), 1.0)[0] != 0
    assert params(lib, 4)[0] != 0 and params(lib, -1)[0] != 0
    assert lib.gem_clean_params_for_model(0, 0.0, 1.0, None) != 0


def test_numpy_reference_known_answers(lib):
    """the reference's own known answers -- and the limits it filters with are the library's (gem_clean_params_for_model)"""
    for args in ((1, 0.2, 3.25), (1, DBL_MIN, DBL_MAX), (0, DBL_MIN, DBL_MAX), (2, 0.2, 3.25)):
        rc, p = params(lib, *args)
        assert rc == 0
        mode, lo, hi = clean_ref.params_for_model(args[0], args[1], args[2])
        assert (p.mode, np.float32(p.z_min).tobytes(), np.float32(p.z_max).tobytes()) == (mode, lo.tobytes(), hi.tobytes()), args
    nan, inf = np.nan, np.inf
    pts = np.array([[0, 0, 1, 1], [nan, 0, 1, 2], [0, inf, 1, 3], [0, 0, -inf, 4], [1, 2, 0.2, 5], [1, 2, 3.25, 6],
                    [1, 2, -0.0, 7], [1, 2, 0.0, 8], [1, 2, 3.3, 9], [nan, nan, nan, 10]], np.float32)
    xyzi, rgb, orig = clean_ref.clean(pts, np.arange(10, dtype=np.uint32) * 3, clean_ref.REMOVE_NAN)
    assert orig.tolist() == [0, 4, 5, 6, 7, 8] and rgb.tolist() == [0, 12, 15, 18, 21, 24]
    assert np.array_equal(xyzi[:, 3], [1, 5, 6, 7, 8, 9])
    _, zlo, zhi = clean_ref.params_for_model(1, 0.2, 3.25)
    assert clean_ref.clean(pts, None, clean_ref.PASSTHROUGH_Z, zlo, zhi)[2].tolist() == [0, 4, 5]
    _, zlo, zhi = clean_ref.params_for_model(1)
    assert clean_ref.clean(pts, None, clean_ref.PASSTHROUGH_Z, zlo, zhi)[2].tolist() == [0, 4, 5, 6, 7, 8]     # -0.0 >= +0.0f: kept
    assert clean_ref.clean(pts, None, clean_ref.NONE)[2].tolist() == list(range(10))
    assert clean_ref.clean(np.zeros((0, 4), np.float32))[2].size == 0


def test_cpp_processors_clean_params(lib, tmp_path):
    """gem::SensorProcessorBase::cleanParams per processor (tests/cpp/clean_facade_check.cpp, host part): the structured-light
    processor reads cutoff_min_depth / cutoff_max_depth with the reference's defaults, not param()'s 0."""
    from conftest import HAS_GPU
    exe = build_clean_facade_check(tmp_path)
    if not HAS_GPU:
        res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: cleanParams)"), res.stdout + res.stderr


def build_clean_facade_check(tmp_path) -> Path:
    exe = tmp_path / "clean_facade_check"
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "clean_facade_check.cpp"),
           "-o", str(exe), f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe
