"""numpy reference of the depth-image unprojection, the semantics include/gem_hip.h pins (depth_image_proc::convert<T>, ROS noetic,
range_max = 0, restated -- not verified against an installation):

  constants (double, one rounding each)   unit = depth_unit (0 -> 0.001f) for U16, 1 for F32; kx = (float)(unit / fx),
                                          ky = (float)(unit / fy), cxf = (float)cx, cyf = (float)cy
  per pixel (u, v), i = v * width + u, float32 throughout, every operation rounded:
    U16  d = the count, invalid iff d == 0, df = (float)d, z = df * depth_unit
    F32  d = the value, invalid iff not finite (negative, zero and denormal depths are valid), df = z = d
    valid    x = (((float)u - cxf) * df) * kx, y = (((float)v - cyf) * df) * ky
    invalid  x = y = z = NaN (0x7fc00000)
    I = intensity, rgb = 0x00RRGGBB of the colour pixel, for every pixel
  clean (PASSTHROUGH_Z): the points clean_ref drops get x = y = z = NaN

A plain module the CPU and GPU tests import (not a conftest)."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import clean_ref  # noqa: E402

U16, F32FMT = 0, 1
NONE, BGR8, RGB8 = 0, 1, 2
F32 = np.float32
QNAN = np.array([0x7fc00000], np.uint32).view(F32)[0]


def unit_of(image) -> np.float32:
    u = F32(image.depth_unit)
    return F32(0.001) if u == 0 else u


def constants(image) -> np.ndarray:
    """[kx, ky, cxf, cyf] as float32"""
    unit = float(unit_of(image)) if image.format == U16 else 1.0
    with np.errstate(over="ignore"):
        return np.array([F32(unit / float(image.fx)), F32(unit / float(image.fy)), F32(float(image.cx)), F32(float(image.cy))], F32)


def rows(image, buf, itemsize: int, per_pixel: int, stride: int) -> np.ndarray:
    """the [height, width * per_pixel] elements of an image whose rows lie `stride` bytes apart in the flat buffer `buf`"""
    w, h = int(image.width), int(image.height)
    raw = np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    stride = stride or w * per_pixel * itemsize
    out = np.empty((h, w * per_pixel * itemsize), np.uint8)
    for v in range(h):
        out[v] = raw[v * stride: v * stride + w * per_pixel * itemsize]
    return out


def unproject(image, depth, color=None, clean=None):
    """-> (xyzi [n, 4] float32, rgb [n] uint32 or None).  depth / color: arrays laid out as `image` says (flat buffers with the
    image's strides, or [H, W] / [H, W, 3] arrays when the rows are tight); clean: None or (mode, z_min, z_max)."""
    w, h = int(image.width), int(image.height)
    kx, ky, cxf, cyf = constants(image)
    if image.format == U16:
        d = rows(image, depth, 2, 1, int(image.row_stride)).view(np.uint16).reshape(h, w)
        valid = d != 0
        df = d.astype(F32)
        with np.errstate(all="ignore"):
            z = df * unit_of(image)
    else:
        d = rows(image, depth, 4, 1, int(image.row_stride)).view(F32).reshape(h, w)
        valid = np.isfinite(d)
        df = d.copy()
        z = d.copy()
    u = np.arange(w, dtype=np.int64).astype(F32)[None, :]
    v = np.arange(h, dtype=np.int64).astype(F32)[:, None]
    with np.errstate(all="ignore"):
        x = ((u - cxf) * df) * kx
        y = ((v - cyf) * df) * ky
    assert x.dtype == F32 and y.dtype == F32 and z.dtype == F32
    out = np.empty((h, w, 4), F32)
    out[..., 0], out[..., 1], out[..., 2] = x, y, z
    out[~valid, :3] = QNAN
    out[..., 3] = F32(image.intensity)
    out = out.reshape(-1, 4)
    if clean is not None:
        mode, lo, hi = clean
        if mode == clean_ref.PASSTHROUGH_Z:
            out[~clean_ref.keep_mask(out, mode, lo, hi), :3] = QNAN
    rgb = None
    if color is not None and image.color_format != NONE:
        c = rows(image, color, 1, 3, int(image.color_row_stride)).reshape(h, w, 3).astype(np.uint32)
        r, b = (c[..., 2], c[..., 0]) if image.color_format == BGR8 else (c[..., 0], c[..., 2])
        rgb = ((r << 16) | (c[..., 1] << 8) | b).reshape(-1)
    return out, rgb
