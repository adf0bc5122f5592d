"""The VoxelGrid contract of gem_voxel_device (include/gem_hip.h) restated in numpy: one pcl::VoxelGrid<pcl::PCLPointCloud2>
stage as pcl_ros's nodelet runs it, and a chain of stages.  Imported by tests/test_voxel_cpu.py and tests/test_voxel_gpu.py.

Float arithmetic stays float32 wherever the contract says float; np.add.at in float32 over input order gives the sequential sums
from +0.0f."""
import numpy as np

F32 = np.float32
FLT_MAX = float(np.finfo(F32).max)
INT_MAX = 2 ** 31 - 1
FIELDS = {None: 0, "": 0, "x": 1, "y": 2, "z": 3, "intensity": 4}


def to_float(v: float) -> F32:
    """double -> float, round to nearest (+-inf beyond FLT_MAX + half an ulp)"""
    with np.errstate(over="ignore"):
        return F32(v)


def f2i(v) -> np.ndarray:
    """(int) of float32 values as x86 converts them: truncation, INT_MIN outside the int range"""
    v = np.asarray(v, F32)
    ok = (v >= F32(-2147483648.0)) & (v < F32(2147483648.0))
    out = np.full(v.shape, -2 ** 31, np.int64)
    out[ok] = np.trunc(v[ok]).astype(np.int64)
    return out


def _tests(xyzi, field, lo, hi, negative):
    """(bounds set, survivors): the limit test against the float-cast limits, and against the double limits"""
    finite = np.isfinite(xyzi[:, :3]).all(axis=1)
    f = FIELDS[field] if not isinstance(field, (int, np.integer)) else int(field)
    if f == 0:
        return finite, finite.copy()
    v = xyzi[:, (0, 1, 2, 3)[f - 1]]
    lo_f, hi_f = to_float(lo), to_float(hi)
    v64 = v.astype(np.float64)
    with np.errstate(invalid="ignore"):
        if negative:
            pf = ~((v < hi_f) & (v > lo_f))
            pd = ~((v64 < hi) & (v64 > lo))
        else:
            pf = ~((v > hi_f) | (v < lo_f))
            pd = ~((v64 > hi) | (v64 < lo))
    return finite & pf, finite & pd


def stage(xyzi, rgb=None, leaf=0.1, field=None, lo=-FLT_MAX, hi=FLT_MAX, negative=False):
    """one stage on k points -> (xyzi [k, 4], rgb [k] uint32 or None, m): the m centroids, then NaN x, y, z with intensity 0 (rgb 0)
    -- or, on overflow, the input unchanged (m = k)."""
    xyzi = np.ascontiguousarray(xyzi, F32).reshape(-1, 4)
    k = xyzi.shape[0]
    rgb = None if rgb is None else np.ascontiguousarray(rgb).view(np.uint32).reshape(-1)
    leaf = np.broadcast_to(np.asarray(leaf, np.float64), (3,)).astype(F32)
    out = np.zeros((k, 4), F32)
    out[:, :3] = np.nan
    rgb_out = None if rgb is None else np.zeros(k, np.uint32)
    inb, surv = _tests(xyzi, field, lo, hi, negative)
    if not inb.any():
        return out, rgb_out, 0
    pts = xyzi[inb, :3]
    mn, mx = pts.min(axis=0), pts.max(axis=0)
    inv = (F32(1.0) / leaf).astype(F32)
    e = ((mx - mn).astype(F32) * inv).astype(F32)
    overflow = not bool(np.all(e < F32(2147483648.0)))
    if not overflow:
        d = np.trunc(e).astype(np.int64) + 1
        d01 = int(d[0]) * int(d[1])
        overflow = d01 > INT_MAX or d01 * int(d[2]) > INT_MAX
    if overflow:
        return xyzi.copy(), (None if rgb is None else rgb.copy()), k
    min_b = f2i(np.floor((mn * inv).astype(F32)))
    max_b = f2i(np.floor((mx * inv).astype(F32)))
    div = (max_b - min_b + 1) & 0xFFFFFFFF
    mul = np.array([1, int(div[0]), (int(div[0]) * int(div[1])) & 0xFFFFFFFF], np.uint64)
    q = xyzi[surv]
    if q.shape[0] == 0:
        return out, rgb_out, 0
    ijk = (f2i(np.floor((q[:, :3] * inv).astype(F32))) - min_b) & 0xFFFFFFFF
    idx = ((ijk.astype(np.uint64) * mul).sum(axis=1) & 0xFFFFFFFF).astype(np.uint32)
    keys, inverse, counts = np.unique(idx, return_inverse=True, return_counts=True)
    m = keys.size
    inverse = inverse.reshape(-1)
    sums = np.zeros((m, 4), F32)                       # +0.0f
    np.add.at(sums, inverse, q)                        # sequential, input order inside every voxel
    c = counts.astype(F32)
    out[:m] = sums / c[:, None]
    if rgb is not None:
        cr = rgb[surv]
        ch = np.stack([(cr >> 16) & 255, (cr >> 8) & 255, cr & 255], axis=1).astype(F32)
        cs = np.zeros((m, 3), F32)
        np.add.at(cs, inverse, ch)
        avg = np.trunc(cs / c[:, None]).astype(np.uint32)
        rgb_out[:m] = (avg[:, 0] << 16) | (avg[:, 1] << 8) | avg[:, 2]
    return out, rgb_out, m


def stage_args(st):
    """a VoxelStage (gem_amd.api) -> the keyword arguments of stage()"""
    return dict(leaf=st.leaf_size, field=st.field, lo=st.limit_min, hi=st.limit_max, negative=st.limit_negative)


def voxel(xyzi, rgb=None, stages=()):
    """a chain of stages (VoxelStage objects or stage() keyword dicts) on n points -> (xyzi [n, 4], rgb [n] or None, m):
    stage s + 1 reads stage s's m points; the output is padded to n with the NaN tail."""
    xyzi = np.ascontiguousarray(xyzi, F32).reshape(-1, 4)
    n = xyzi.shape[0]
    cur, cur_rgb, m = xyzi, (None if rgb is None else np.ascontiguousarray(rgb).view(np.uint32).reshape(-1)), n
    for st in stages:
        kw = st if isinstance(st, dict) else stage_args(st)
        o, r, m2 = stage(cur[:m], None if cur_rgb is None else cur_rgb[:m], **kw)
        cur = np.zeros((n, 4), F32)
        cur[:, :3] = np.nan
        cur[:o.shape[0]] = o
        if cur_rgb is not None:
            nr = np.zeros(n, np.uint32)
            nr[:r.shape[0]] = r
            cur_rgb = nr
        m = m2
    return cur, cur_rgb, m
