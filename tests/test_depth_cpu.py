"""CPU tests of the depth-image entries (include/gem_hip.h): they are declared, exported and bound; gem_depth_image matches its
ctypes mirror field by field; gem_depth_constants equals tests/depth_ref.py bit for bit and rejects what the header says it rejects;
depth_ref gives the answers one can work out by hand; synth.depth_image_c3 is C3; the C++ facade compiles and its host part runs."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import depth_ref  # noqa: E402

F32 = np.float32
GEM_ERR_INVALID = -1
ENTRIES = ("gem_depth_constants", "gem_depth_unproject_device", "gem_add_depth", "gem_add_depth_device")


def image(**kw):
    from gem_amd import _lib
    f = dict(width=640, height=480, format=_lib.DEPTH_U16, row_stride=0, fx=380.0, fy=380.0, cx=319.5, cy=239.5, depth_unit=0.0,
             intensity=1.0, color_format=_lib.COLOR_NONE, color_row_stride=0)
    f.update(kw)
    return _lib.DepthImage(**f)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_depth_entries_are_declared_exported_and_bound():
    from gem_amd import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "gem_hip.h").read_text(), flags=re.S)
    for n in ENTRIES:
        assert re.search(r"\b" + n + r"\s*\(", header), f"{n} is not declared in gem_hip.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes prototype"
    assert lib.gem_abi_version() == 9


def test_depth_image_layout_matches_the_header(tmp_path):
    from gem_amd import _lib
    fields = [n for n, _ in _lib.DepthImage._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gem_hip.h"\nint main(void){printf("%zu", sizeof(gem_depth_image));\n'
                   + "".join(f'printf(" %zu", offsetof(gem_depth_image, {f}));\n' for f in fields)
                   + 'printf(" %d %d %d %d %d\\n", GEM_DEPTH_U16, GEM_DEPTH_F32, GEM_COLOR_NONE, GEM_COLOR_BGR8, GEM_COLOR_RGB8);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    exp = [C.sizeof(_lib.DepthImage)] + [getattr(_lib.DepthImage, f).offset for f in fields] + \
          [_lib.DEPTH_U16, _lib.DEPTH_F32, _lib.COLOR_NONE, _lib.COLOR_BGR8, _lib.COLOR_RGB8]
    assert len(fields) == 12 and got == exp


@pytest.mark.parametrize("fmt", [0, 1])
def test_depth_constants_match_the_reference_bit_for_bit(fmt):
    from gem_amd import _lib
    lib = _lib.load()
    for fx in (380.0, 381.7, 1e-3, 1e6):
        for unit in (0.0, 0.001, 0.00025, 1.0):
            for cx, cy in ((319.5, 239.5), (-10.25, 500.5), (320.1, 0.3)):
                img = image(format=fmt, fx=fx, fy=fx * 1.01, cx=cx, cy=cy, depth_unit=unit)
                out = (C.c_float * 4)()
                assert lib.gem_depth_constants(C.byref(img), out) == _lib.GEM_OK
                want = depth_ref.constants(img)
                assert np.array_equal(bits(np.array(out[:], F32)), bits(want)), (fmt, fx, unit, list(out), want)
    # the unit of a uint16 image is float(0.001), not the double 0.001; a float image has none
    k = depth_ref.constants(image(format=0, fx=380.0))
    assert k[0] == F32(float(F32(0.001)) / 380.0) and depth_ref.constants(image(format=1, fx=380.0, depth_unit=0.5))[0] == F32(1.0 / 380.0)


def test_invalid_images_are_rejected_without_a_handle():
    from gem_amd import _lib
    lib = _lib.load()
    out = (C.c_float * 4)()
    nan, inf = float("nan"), float("inf")
    assert lib.gem_depth_constants(None, out) == GEM_ERR_INVALID
    assert lib.gem_depth_constants(C.byref(image()), None) == GEM_ERR_INVALID
    bad = [dict(width=-1), dict(height=-3), dict(width=8193, height=8192), dict(format=2), dict(format=-1), dict(color_format=3), dict(color_format=-1),
           dict(row_stride=1279), dict(row_stride=1278), dict(row_stride=1281), dict(format=1, row_stride=2558), dict(format=1, row_stride=2562),
           dict(color_format=1, color_row_stride=1919), dict(fx=0.0), dict(fy=0.0), dict(fx=nan), dict(fy=inf), dict(fx=-inf), dict(cx=nan), dict(cy=inf),
           dict(depth_unit=-0.001), dict(depth_unit=nan), dict(depth_unit=inf), dict(format=1, depth_unit=-1.0)]
    for kw in bad:
        assert lib.gem_depth_constants(C.byref(image(**kw)), out) == GEM_ERR_INVALID, kw
    good = [dict(), dict(width=0), dict(height=0), dict(width=8192, height=8192), dict(row_stride=1280), dict(row_stride=1282), dict(format=1, row_stride=2564),
            dict(color_format=2, color_row_stride=1921), dict(fx=-380.0), dict(cx=-1e9)]
    for kw in good:
        assert lib.gem_depth_constants(C.byref(image(**kw)), out) == _lib.GEM_OK, kw
    # the entries that take a handle: a NULL handle is GEM_ERR_INVALID before anything else is looked at
    img = image()
    assert lib.gem_depth_unproject_device(None, C.byref(img), None, None, None, None, None) == GEM_ERR_INVALID
    assert lib.gem_add_depth(None, None, C.byref(img), None, None, None, None, 0) == GEM_ERR_INVALID
    assert lib.gem_add_depth_device(None, None, C.byref(img), None, None, None, None, 0) == GEM_ERR_INVALID


def test_reference_answers_one_can_work_out_by_hand():
    # a pixel at the principal point: (0, 0, z)
    img = image(width=5, height=3, cx=2.0, cy=1.0, fx=380.0, fy=380.0, intensity=7.5)
    d = np.zeros((3, 5), np.uint16); d[1, 2] = 1500
    x, rgb = depth_ref.unproject(img, d)
    assert rgb is None and x.shape == (15, 4)
    p = x[1 * 5 + 2]
    assert p[0] == 0 and p[1] == 0 and p[2] == F32(1500) * F32(0.001) and p[3] == F32(7.5)
    # d = 1000 counts one focal length right of the principal point: x = (380 * 1000) * (float)(0.001f / 380), its bits pinned
    img = image(width=640, height=2, cx=100.0, cy=1.0, fx=380.0, fy=380.0)
    d = np.zeros((2, 640), np.uint16); d[1, 480] = 1000
    p = depth_ref.unproject(img, d)[0][640 + 480]
    k = F32(float(F32(0.001)) / 380.0)
    want = F32(F32(380.0) * F32(1000.0)) * k
    assert bits(np.array([k]))[0] == 0x36309a2f                   # (float)(0.001f / 380)
    assert bits(p[:1])[0] == bits(np.array([want]))[0] == 0x3f800000          # 380000 * k rounds to exactly 1.0f
    assert p[1] == 0 and bits(p[2:3])[0] == bits(np.array([F32(1000.0) * F32(0.001)]))[0] == 0x3f800000
    # d = 0: three quiet NaNs and the intensity
    q = depth_ref.unproject(img, d)[0][0]
    assert list(bits(q[:3])) == [0x7fc00000] * 3 and q[3] == F32(1.0)
    # float images: NaN and +-inf are invalid; zeros, negative and denormal depths are valid
    img = image(width=6, height=1, format=1, cx=0.0, cy=0.0)
    d = np.array([[np.nan, np.inf, -np.inf, 0.0, -2.0, 1e-45]], F32)
    x = depth_ref.unproject(img, d)[0]
    assert np.isnan(x[:3, :3]).all() and np.isfinite(x[3:, :3]).all() and x[4, 2] == -2.0 and x[5, 2] == F32(1e-45)
    # colour: 0x00RRGGBB from either byte order, for invalid pixels too
    c = np.arange(18, dtype=np.uint8).reshape(1, 6, 3)
    assert depth_ref.unproject(image(width=6, height=1, format=1, color_format=1), d, c)[1][1] == (5 << 16) | (4 << 8) | 3
    assert depth_ref.unproject(image(width=6, height=1, format=1, color_format=2), d, c)[1][1] == (3 << 16) | (4 << 8) | 5
    # PASSTHROUGH_Z: the limits are inclusive, their neighbours outside are dropped
    lo, hi = F32(0.2), F32(3.25)
    d = np.array([[np.nextafter(lo, F32(-1)), lo, hi, np.nextafter(hi, F32(9)), 1.0, np.nan]], F32)
    x = depth_ref.unproject(image(width=6, height=1, format=1, cx=0.0, cy=0.0), d, clean=(2, lo, hi))[0]
    assert list(np.isnan(x[:, 2])) == [True, False, False, True, False, True]


def test_synthetic_c3_depth_image():
    from gem_amd import _lib, synth
    wl = synth.config_c3()
    for fmt in ("u16", "f32"):
        img, d, bgr = synth.depth_image_c3(fmt=fmt)
        img2, d2, bgr2 = synth.depth_image_c3(fmt=fmt)
        assert np.array_equal(d.view(np.uint8), d2.view(np.uint8)) and np.array_equal(bgr, bgr2)
        assert (img.width, img.height, img.fx, img.cx, img.cy, img.color_format) == (640, 480, 380.0, 320.0, 240.0, _lib.COLOR_BGR8)
        assert d.shape == (480, 640) and bgr.shape == (480, 640, 3) and bgr.dtype == np.uint8
        x, rgb = depth_ref.unproject(img, d, bgr)
        valid = np.flatnonzero(np.isfinite(x[:, 2]))
        assert np.array_equal(valid, wl.orig_index)               # invalid exactly where config_c3 drops the ray
        # ... and the depths are config_c3's, to the format's rounding
        assert np.max(np.abs(x[valid, 2].astype(np.float64) - wl.clouds[0][:, 2])) <= (0.00051 if fmt == "u16" else 0.0)
        assert rgb.shape == (640 * 480,) and rgb.max() < 1 << 24
    assert not np.array_equal(synth.depth_image_c3(seed=4)[2], synth.depth_image_c3(seed=3)[2])


def build_depth_facade_check(tmp_path) -> Path:
    exe = tmp_path / "depth_facade_check"
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", str(ROOT / "include"),
           str(ROOT / "tests" / "cpp" / "depth_facade_check.cpp"), "-o", str(exe), f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_cpp_facade_compiles_and_its_host_part_runs(tmp_path):
    from gem_amd import _lib
    _lib.load()
    exe = build_depth_facade_check(tmp_path)
    res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout.strip().startswith("OK"), res.stdout + res.stderr


def test_gem_reserve_plans_every_depth_image_with_tight_rows(tmp_path):
    """gem_amd/csrc/gem_plan.hpp on its own: what gem_reserve allocates in the staging arena for max_points (depth_stage_bytes) holds
    the plan of every image of up to that many pixels with tight rows -- both formats, with and without colour, host and device images
    (depth_plan, what add_cloud sizes the arena by) -- and the four parts of a plan do not overlap.  A host-only HIP build."""
    from gem_amd.build import hipcc_path
    src = tmp_path / "depth_plan.cpp"
    src.write_text('#include "gem_plan.hpp"\n#include <cstdio>\nusing namespace gem;\nint main(){ long long bad = 0;\n'
                   'for (long long P : {1ll, 63ll, 4096ll, 19200ll, 307200ll, 1ll << 26}) for (long long n : {1ll, P / 2 + 1, P}) '
                   'for (int esz : {2, 4}) for (int colour = 0; colour < 2; ++colour) for (int dev = 0; dev < 2; ++dev) {\n'
                   '  const size_t db = dev ? 0 : (size_t)n * esz, cb = dev || !colour ? 0 : (size_t)n * 3;\n'
                   '  const DepthPlan p = depth_plan(n, db, cb);\n'
                   '  bad += p.bytes > depth_stage_bytes(P) || p.o_color < db || p.o_xyzi < p.o_color + cb || p.o_rgb < p.o_xyzi + (size_t)n * 16 ||\n'
                   '         p.bytes < p.o_rgb + (size_t)n * 4 || (p.o_color | p.o_xyzi | p.o_rgb) % 256; }\n'
                   'std::printf(bad ? "FAILED %lld\\n" : "ok\\n", bad); return bad != 0; }\n')
    exe = tmp_path / "depth_plan"
    res = subprocess.run([hipcc_path(), "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "gem_amd" / "csrc"),
                          str(src), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
