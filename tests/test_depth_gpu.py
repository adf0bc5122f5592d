"""Depth images on the device (include/gem_hip.h: depth_image_proc::convert, restated) against the numpy statement (tests/depth_ref.py).
Every comparison is on uint32 views: both sides round the same three operations, so there is no tolerance.

  1. gem_depth_unproject_device: both formats, the three colour formats, sizes around the four-pixel group and the workgroup, tight and
     padded strides, base pointers off the wide loads' alignment, the special depth values, the PassThrough limits and their
     neighbours, every clean mode;
  2. gem_add_depth / gem_add_depth_device over three frames with a move in between = gem_add_raw of the reference cloud, all ten
     layers, on every pipeline, for the four sensor models, with and without colour;
  3. ... behind the VoxelGrid stage of filter.launch = gem_add_voxel of the reference cloud;
  4. gem_reserve covers a stream of host depth frames: no arena and no pinned-buffer allocation;
  5. the invalid arguments: GEM_ERR_INVALID and an untouched map;
  6. one C3 frame (640 x 480, uint16 + BGR8, structured light) = gem_add_raw of its reference cloud;
  7. the C++ facade's addDepth (tests/cpp/depth_facade_check.cpp) as a child process."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gem_amd import ElevationMap, SensorModel, VoxelStage, _lib, synth

sys.path.insert(0, str(Path(__file__).resolve().parent))
import clean_ref  # noqa: E402
import depth_ref  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
LAYERS = ("elevation", "variance", "intensity", "traver", "lowest", "color_r", "color_g", "color_b", "rough", "slope")
Z_LO, Z_HI = F32(0.2), F32(3.25)
GEM_ERR_INVALID = -1


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def clean_params(mode, lo=-np.inf, hi=np.inf):
    p = _lib.CleanParams()
    p.mode, p.z_min, p.z_max = int(mode), float(lo), float(hi)
    return p


def make_image(w, h, fmt, colour=_lib.COLOR_NONE, **kw):
    f = dict(width=w, height=h, format=fmt, row_stride=0, fx=380.0, fy=381.7, cx=319.5, cy=239.5, depth_unit=0.0, intensity=3.5,
             color_format=colour, color_row_stride=0)
    f.update(kw)
    return _lib.DepthImage(**f)


def special_depths(fmt, unit):
    """the values that decide something: invalid ones, the extremes, the PassThrough limits and their neighbours"""
    if fmt == _lib.DEPTH_U16:
        u = float(F32(unit) if unit else F32(0.001))
        out = [0, 1, 65535]
        for lim in (float(Z_LO), float(Z_HI)):
            c = int(round(lim / u))
            out += [c - 1, c, c + 1]
        return np.array(out, np.uint16)
    out = [np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, 1e-45, np.finfo(F32).max]
    for lim in (Z_LO, Z_HI):
        out += [np.nextafter(lim, F32(-np.inf)), lim, np.nextafter(lim, F32(np.inf))]
    return np.array(out, F32)


def depth_values(rng, n, fmt, unit, rotate):
    if fmt == _lib.DEPTH_U16:
        d = rng.integers(0, 65536, n).astype(np.uint16)
        d[rng.random(n) < 0.1] = 0
    else:
        d = rng.uniform(0.05, 6.0, n).astype(F32)
        d[rng.random(n) < 0.1] = np.nan
    s = np.roll(special_depths(fmt, unit), rotate)
    k = min(n, s.size)
    d[rng.permutation(n)[:k]] = s[:k]
    return d


def laid_out(values, w, h, per_row_extra, offset):
    """the [h, w * c] elements in a flat array with `per_row_extra` elements of padding behind each row, starting `offset` elements in;
    padding and slack hold a pattern a kernel that read them would show"""
    values = values.reshape(h, -1)
    row = values.shape[1] + per_row_extra
    flat = np.full(offset + h * row + 8, 77, values.dtype)
    for v in range(h):
        flat[offset + v * row: offset + v * row + values.shape[1]] = values[v]
    return flat, row * values.dtype.itemsize


SIZES = [(1, 1), (3, 2), (5, 7), (63, 3), (64, 4), (65, 3), (255, 1), (257, 2), (640, 480)]
# (depth elements of padding per row, depth base offset in elements, colour bytes of padding per row, colour base offset in bytes)
LAYOUTS = {"tight": (0, 0, 0, 0), "odd_strides": (1, 0, 1, 0), "off_base": (0, 1, 5, 1), "aligned_padding": (8, 0, 8, 0)}


# ---- 1. the unprojection itself --------------------------------------------------------------------------------------------------
@pytest.mark.one_pipeline
def test_depth_unproject_matches_numpy():
    import torch
    m = ElevationMap(64, 0.1)
    rng = np.random.default_rng(61)
    case = 0
    pass_z = clean_params(_lib.CLEAN_PASSTHROUGH_Z, Z_LO, Z_HI)
    cleans = {"null": None, "none": clean_params(_lib.CLEAN_NONE), "remove_nan": clean_params(_lib.CLEAN_REMOVE_NAN), "passthrough": pass_z}
    masked_points = 0
    for w, h in SIZES:
        for fmt in (_lib.DEPTH_U16, _lib.DEPTH_F32):
            for lname, (dpad, doff, cpad, coff) in LAYOUTS.items():
                case += 1
                unit = 0.0 if case % 2 else 0.00025
                cx, cy = ((319.5, 239.5), (-10.25, 500.5))[(case // 2) % 2]
                d = depth_values(rng, w * h, fmt, unit, case)
                dflat, dstride = laid_out(d, w, h, dpad, doff)
                bgr = rng.integers(0, 256, (h, w * 3), dtype=np.uint8)
                cflat, cstride = laid_out(bgr, w, h, cpad, coff)
                t_d = torch.from_numpy(dflat.view(np.int16) if fmt == _lib.DEPTH_U16 else dflat).cuda()[doff:]
                t_c = torch.from_numpy(cflat).cuda()[coff:]
                ref_plain = None
                for colour in (_lib.COLOR_NONE, _lib.COLOR_BGR8, _lib.COLOR_RGB8):
                    img = make_image(w, h, fmt, colour, row_stride=0 if lname == "tight" else dstride, color_row_stride=0 if lname == "tight" else cstride,
                                     depth_unit=unit, cx=cx, cy=cy)
                    want, want_rgb = depth_ref.unproject(img, dflat[doff:], cflat[coff:] if colour else None)
                    if ref_plain is not None:
                        assert np.array_equal(bits(want), bits(ref_plain))
                    ref_plain = want
                    want_masked = depth_ref.unproject(img, dflat[doff:], None, (clean_ref.PASSTHROUGH_Z, Z_LO, Z_HI))[0]
                    names = ("null", "passthrough") if w * h > 100_000 else tuple(cleans)
                    got_plain = None
                    for cname in names:
                        out, rgb = m.depth_unproject(img, t_d, t_c if colour else None, cleans[cname])
                        got = out.cpu().numpy()
                        what = (w, h, fmt, lname, colour, cname)
                        exp = want_masked if cname == "passthrough" else want
                        bad = np.flatnonzero((bits(got) != bits(exp)).any(1))
                        assert bad.size == 0, f"{what}: {bad.size} points differ, first {bad[:3]}: {got[bad[:3]]} != {exp[bad[:3]]}"
                        if colour:
                            assert np.array_equal(rgb.cpu().numpy().view(np.uint32), want_rgb), what
                        else:
                            assert rgb is None
                        if cname == "null":
                            got_plain = got
                        if cname == "passthrough":
                            # ... and it is the fuse entries' mask (clean_ref) applied to the plain output
                            twin = got_plain.copy()
                            drop = ~clean_ref.keep_mask(twin, clean_ref.PASSTHROUGH_Z, Z_LO, Z_HI)
                            twin[drop, :3] = depth_ref.QNAN
                            assert np.array_equal(bits(got), bits(twin)), what
                            masked_points += int((drop & np.isfinite(got_plain[:, 2])).sum())
    assert masked_points > 100_000                  # the cutoffs dropped valid pixels
    # the limits themselves are kept, their outer neighbours dropped (both formats see them: special_depths)
    img = make_image(6, 1, _lib.DEPTH_F32)
    d = np.array([np.nextafter(Z_LO, F32(-1)), Z_LO, np.nextafter(Z_LO, F32(1)), np.nextafter(Z_HI, F32(0)), Z_HI, np.nextafter(Z_HI, F32(9))], F32)
    out, _ = m.depth_unproject(img, torch.from_numpy(d).cuda(), None, pass_z)
    assert list(np.isnan(out.cpu().numpy()[:, 2])) == [True, False, False, False, False, True]
    # no pixels: nothing to do, not an error
    out, _ = m.depth_unproject(make_image(0, 5, _lib.DEPTH_U16), torch.zeros(4, dtype=torch.int16).cuda())
    assert out.shape == (0, 4)
    m.close()


# ---- the fuse workloads -------------------------------------------------------------------------------------------------------------
W, H = 160, 120
STEREO = lambda: SensorModel(2, (0.1, 0.001, 380.0, 1.0, 0.002, 0.001, 30.0), original_width=W)
MODELS = {"laser": SensorModel.velodyne, "structured_light": SensorModel.realsense_d435, "stereo": STEREO, "perfect": SensorModel.perfect}
_C3 = {}


def c3():
    """C3 at a quarter of its resolution: every fourth pixel of its uint16 image, the intrinsics scaled with it; shared, never changed"""
    if not _C3:
        img, d, bgr = synth.depth_image_c3()
        wl = synth.config_c3()
        _C3.update(depth=np.ascontiguousarray(d[::4, ::4]), bgr=np.ascontiguousarray(bgr[::4, ::4]), T=wl.frames[0].T.astype(np.float64),
                   pos=wl.map_position)
        assert _C3["depth"].shape == (H, W)
    return _C3


def small_frame(seed, fmt=_lib.DEPTH_U16, colour=True):
    """(image, depth, bgr) of frame `seed`: the shared scene with its own noise and holes"""
    s = c3()
    rng = np.random.default_rng(seed)
    d = s["depth"].astype(np.int64) + rng.integers(-4, 5, (H, W))
    d[rng.random((H, W)) < 0.05] = 0
    d = np.clip(d, 0, 65535).astype(np.uint16)
    bgr = s["bgr"] ^ np.uint8(seed)
    img = make_image(W, H, fmt, _lib.COLOR_BGR8 if colour else _lib.COLOR_NONE, fx=95.0, fy=95.0, cx=80.0, cy=60.0, depth_unit=0.001, intensity=50.0)
    if fmt == _lib.DEPTH_F32:
        f = d.astype(F32) * F32(0.001)
        f[d == 0] = np.nan
        d = f
    return img, d, (bgr if colour else None)


def model_frame(model, step):
    sm = MODELS[model]()
    sm.ignore_points_above, sm.ignore_points_below = float("inf"), float("-inf")
    sm.original_width = W
    T = c3()["T"].copy()
    T[0, 3] += 0.05 * step
    T[1, 3] -= 0.03 * step
    return synth._frame_for(T, sm)


def same_maps(got, want, what):
    for name in LAYERS:
        bad = np.flatnonzero(bits(got.layer(name)).ravel() != bits(want.layer(name)).ravel())
        assert bad.size == 0, f"{what} {name}: {bad.size} cells differ"
    assert got.stats()["points_in"] == want.stats()["points_in"] == W * H


# ---- 2. gem_add_depth* = gem_add_raw of the reference cloud ----------------------------------------------------------------------
@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("model", list(MODELS))
def test_add_depth_map_parity(model, colour):
    import torch
    host, dev, twin = (ElevationMap(128, 0.05) for _ in range(3))
    pos = np.asarray(c3()["pos"], F32)
    for m in (host, dev, twin):
        m.move(pos)
    for step, seed in enumerate((21, 22, 23)):
        fmt = _lib.DEPTH_F32 if step == 1 else _lib.DEPTH_U16
        img, d, bgr = small_frame(seed, fmt, colour)
        f = model_frame(model, step)
        cp = f.model.clean_params()
        if step == 2:
            for m in (host, dev, twin):
                m.move(pos + np.array([0.15, -0.1, 0.0], F32))
                m.mapvar_update(1e-5)
        cloud, rgb = depth_ref.unproject(img, d, bgr)
        host.add_depth(f, img, d, bgr)
        t_d = torch.from_numpy(d.view(np.int16) if fmt == _lib.DEPTH_U16 else d).cuda()
        dev.add_depth(f, img, t_d, torch.from_numpy(bgr).cuda() if colour else None)
        twin.add_raw(f, cloud, rgb=rgb, clean=cp)
        same_maps(host, twin, f"add_depth host {model} step {step}")
        same_maps(dev, twin, f"add_depth device {model} step {step}")
    seen = (twin.layer("elevation") != -10).sum()
    assert seen > 1000
    if model == "structured_light":                # its cutoffs dropped what the other models fuse
        assert cp.mode == _lib.CLEAN_PASSTHROUGH_Z and np.isfinite(cloud[:, 2]).sum() > clean_ref.keep_mask(cloud, cp.mode, cp.z_min, cp.z_max).sum()
    if colour:
        assert (twin.layer("color_r") != 0).sum() > 1000
    for m in (host, dev, twin):
        m.close()


# ---- 3. ... behind the VoxelGrid stage ---------------------------------------------------------------------------------------------
def test_add_depth_voxel_map_parity():
    import torch
    host, dev, twin = (ElevationMap(128, 0.05) for _ in range(3))
    for m in (host, dev, twin):
        m.move(np.asarray(c3()["pos"], F32))
    img, d, bgr = small_frame(31)
    f = model_frame("laser", 0)
    stages = VoxelStage.filter_launch()
    cloud, rgb = depth_ref.unproject(img, d, bgr)
    host.add_depth(f, img, d, bgr, stages=stages)
    dev.add_depth(f, img, torch.from_numpy(d.view(np.int16)).cuda(), torch.from_numpy(bgr).cuda(), stages=stages)
    twin.add_voxel(f, stages, cloud, rgb=rgb)
    same_maps(host, twin, "add_depth host voxel")
    same_maps(dev, twin, "add_depth device voxel")
    assert (twin.layer("elevation") != -10).sum() > 500
    for m in (host, dev, twin):
        m.close()


# ---- 4. gem_reserve covers the depth source ----------------------------------------------------------------------------------------
@pytest.mark.one_pipeline
def test_reserve_then_no_allocation_for_depth_frames():
    m, twin = ElevationMap(128, 0.05), ElevationMap(128, 0.05)
    m.reserve(W * H, 1, True)
    before = m.debug_get("arena_allocations"), m.debug_get("hstage_allocations")
    assert before[0] > 0
    for x in (m, twin):
        x.move(np.asarray(c3()["pos"], F32))
    for step, seed in enumerate((41, 42, 43)):
        img, d, bgr = small_frame(seed, _lib.DEPTH_F32 if step == 1 else _lib.DEPTH_U16)
        f = model_frame("structured_light", step)
        m.add_depth(f, img, d, bgr)
        cloud, rgb = depth_ref.unproject(img, d, bgr)
        twin.add_raw(f, cloud, rgb=rgb)
    same_maps(m, twin, "reserved stream")
    assert (m.debug_get("arena_allocations"), m.debug_get("hstage_allocations")) == before, "a depth frame inside the reserved bounds allocated"
    m.close(); twin.close()


# ---- 5. invalid arguments ------------------------------------------------------------------------------------------------------------
@pytest.mark.one_pipeline
def test_invalid_arguments_change_nothing():
    import torch
    m = ElevationMap(128, 0.05)
    m.move(np.asarray(c3()["pos"], F32))
    img, d, bgr = small_frame(51)
    f = model_frame("laser", 0)
    m.add_depth(f, img, d, bgr)
    before = bits(m.layer("elevation")).copy()
    assert (m.layer("elevation") != -10).sum() > 500
    lib, h = m._lib, m._h
    p = f.to_struct()
    t_d, t_c = torch.from_numpy(d.view(np.int16)).cuda(), torch.from_numpy(bgr).cuda()
    xyzi, rgb = torch.empty((W * H, 4), dtype=torch.float32).cuda(), torch.empty(W * H, dtype=torch.int32).cuda()
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    nan, inf = float("nan"), float("inf")
    ok_clean, bad_clean = clean_params(_lib.CLEAN_PASSTHROUGH_Z, 0.2, 3.25), clean_params(3)
    stages = (_lib.VoxelParams * 1)(VoxelStage.filter_launch()[0].to_struct())

    def calls(image, depth=True, colour=True, clean=None, st=None, ns=0, frame=p):
        """the three entries that take a handle, on the same arguments"""
        i = None if image is None else C.byref(image)
        c = None if clean is None else C.byref(clean)
        return [lib.gem_add_depth(h, C.byref(frame), i, hp(d) if depth else None, hp(bgr) if colour else None, c, st, ns),
                lib.gem_add_depth_device(h, C.byref(frame), i, vp(t_d) if depth else None, vp(t_c) if colour else None, c, st, ns),
                lib.gem_depth_unproject_device(h, i, vp(t_d) if depth else None, vp(t_c) if colour else None, c, vp(xyzi), vp(rgb))]

    def variant(**kw):
        g = _lib.DepthImage.from_buffer_copy(img)
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    assert calls(None) == [GEM_ERR_INVALID] * 3
    assert calls(img, depth=False) == [GEM_ERR_INVALID] * 3
    assert calls(img, colour=False) == [GEM_ERR_INVALID] * 3
    assert calls(img, clean=bad_clean) == [GEM_ERR_INVALID] * 3
    for kw in (dict(width=-W), dict(height=-1), dict(width=8193, height=8192), dict(format=2), dict(color_format=7), dict(row_stride=W * 2 - 2),
               dict(row_stride=W * 2 + 1), dict(color_row_stride=W * 3 - 1), dict(fx=0.0), dict(fy=nan), dict(fx=inf), dict(cx=nan), dict(cy=-inf),
               dict(depth_unit=-1.0), dict(depth_unit=nan), dict(depth_unit=inf)):
        assert calls(variant(**kw)) == [GEM_ERR_INVALID] * 3, kw
    # the add entries' own cases: both front ends at once, bad stages, a stereo frame of another width, no frame
    assert calls(img, clean=ok_clean, st=stages, ns=1)[:2] == [GEM_ERR_INVALID] * 2
    assert calls(img, st=stages, ns=0)[:2] == [GEM_ERR_INVALID] * 2
    assert calls(img, st=None, ns=1)[:2] == [GEM_ERR_INVALID] * 2
    assert calls(img, st=stages, ns=5)[:2] == [GEM_ERR_INVALID] * 2
    stereo = model_frame("stereo", 0)
    stereo.model.original_width = W + 1
    assert calls(img, frame=stereo.to_struct())[:2] == [GEM_ERR_INVALID] * 2
    assert lib.gem_add_depth(h, None, C.byref(img), hp(d), hp(bgr), None, None, 0) == GEM_ERR_INVALID
    # a misaligned XYZI output
    assert lib.gem_depth_unproject_device(h, C.byref(img), vp(t_d), vp(t_c), None, C.c_void_p(xyzi.data_ptr() + 4), vp(rgb)) == GEM_ERR_INVALID
    assert m.stats()["points_in"] == W * H
    assert np.array_equal(bits(m.layer("elevation")), before)
    # an image without pixels adds nothing and is no error; the map answers as before
    assert calls(variant(width=0), depth=False, colour=False) == [_lib.GEM_OK] * 3
    assert np.array_equal(bits(m.layer("elevation")), before)
    m.close()


# ---- 6. one C3 frame ------------------------------------------------------------------------------------------------------------------
@pytest.mark.one_pipeline
def test_c3_depth_frame():
    wl = synth.config_c3(structured_light=True)
    img, d, bgr = synth.depth_image_c3()
    m, twin = ElevationMap(wl.length, wl.resolution), ElevationMap(wl.length, wl.resolution)
    for x in (m, twin):
        x.move(wl.map_position)
    f = wl.frames[0]
    assert f.model.original_width == img.width
    m.add_depth(f, img, d, bgr)
    cloud, rgb = depth_ref.unproject(img, d, bgr)
    twin.add_raw(f, cloud, rgb=rgb)
    for name in LAYERS:
        assert np.array_equal(bits(m.layer(name)), bits(twin.layer(name))), name
    assert m.stats()["points_in"] == 640 * 480 and (m.layer("elevation") != -10).sum() > 5000
    m.close(); twin.close()


# ---- 7. the C++ facade -----------------------------------------------------------------------------------------------------------------
@pytest.mark.one_pipeline            # (a C++ child process: the fixture's knobs never reach it)
def test_cpp_add_depth_on_gpu(tmp_path):
    from test_depth_cpu import build_depth_facade_check
    exe = build_depth_facade_check(tmp_path)
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
