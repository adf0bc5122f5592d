"""numpy restatement of the VoxelLayer contract of include/gem_hip_voxlayer.h, on top of costmap_ref.Costmap and obstacle_ref's
observation dicts: the pieces of ROS noetic costmap_2d (voxel_layer.cpp updateBounds / raytraceFreespace) and voxel_grid (voxel_grid.h
markVoxelInMap, clearVoxelLineInMap, raytraceLine, bresenham3D, bitsBelowThreshold) that gem_costmap_voxel_observe and
gem_voxlayer_host stand for.  Neither library is available to these tests: this is a restatement from memory, unverified against them.

The contract is stated twice.  `observe_loop` is the LITERAL form: observation by observation and record by record in order, a ray
walked by bresenham3D's own loop with its two errors, a cell's byte written as the library writes it (at every cleared voxel, at every
marked voxel), touch(px, py) only when the record's own markVoxelInMap returned true.  `observe` is the SET-FUNCTION form: vectorised,
the closed form of the line, the byte rule of the header per cell, and the header's one named departure in the bounds.
tests/test_voxlayer_cpu.py pins the two to identical grids and columns, to equal bounds at mark_threshold 0 and to contained bounds
above it.  All arithmetic is numpy float64 = C double, every operation rounded on its own.

A voxel grid is `Voxels` (size_z, z_resolution, origin_z, unknown_threshold, mark_threshold); the columns are uint32 [size_y, size_x]."""
import collections

import numpy as np

import costmap_ref as cref
from obstacle_ref import UINT_MAX, cell_distance, check, field, raytrace_bounds, std_max, std_min, xyz, _fold

Voxels = collections.namedtuple("Voxels", "size_z z_resolution origin_z unknown_threshold mark_threshold")
UNKNOWN_COLUMN = 0x0000FFFF
INT_LIMIT = 2147483648.0
POPCOUNT16 = np.array([bin(i).count("1") for i in range(1 << 16)], np.int64)


def mask(z):
    return ((1 << 16) | 1) << int(z)


def below(n, thr):
    """bitsBelowThreshold: popcount(n) <= thr"""
    return bin(int(n)).count("1") <= thr


def marked(col):
    return int(col) >> 16


def unknown(col):
    return ((int(col) >> 16) ^ int(col)) & 0xFFFF


# ---- worldToMap3D ---------------------------------------------------------------------------------------------------------------------
def world_to_map_3d_float(cm, vox, wx, wy, wz):
    """(fx, fy, fz) as float64, or None"""
    f = np.float64
    wx, wy, wz = f(wx), f(wy), f(wz)
    if not (np.isfinite(wx) and np.isfinite(wy) and np.isfinite(wz)):
        return None
    if wx < cm.ox or wy < cm.oy or wz < vox.origin_z:
        return None
    fx, fy, fz = (wx - f(cm.ox)) / f(cm.res), (wy - f(cm.oy)) / f(cm.res), (wz - f(vox.origin_z)) / f(vox.z_resolution)
    return (fx, fy, fz) if fx < cm.size_x and fy < cm.size_y and fz < vox.size_z else None


def world_to_map_3d(cm, vox, wx, wy, wz):
    """(mx, my, mz) as ints, or None: the same pre-test, the quotients truncated, the tests on the integers"""
    f = np.float64
    wx, wy, wz = f(wx), f(wy), f(wz)
    if not (np.isfinite(wx) and np.isfinite(wy) and np.isfinite(wz)):
        return None
    if wx < cm.ox or wy < cm.oy or wz < vox.origin_z:
        return None
    qx, qy, qz = (wx - f(cm.ox)) / f(cm.res), (wy - f(cm.oy)) / f(cm.res), (wz - f(vox.origin_z)) / f(vox.z_resolution)
    if not (qx < INT_LIMIT and qy < INT_LIMIT and qz < INT_LIMIT):
        return None
    mx, my, mz = int(qx), int(qy), int(qz)
    return (mx, my, mz) if mx < cm.size_x and my < cm.size_y and mz < vox.size_z else None


# ---- raytraceLine / bresenham3D ---------------------------------------------------------------------------------------------------------
def _deltas(x0, y0, z0, x1, y1, z1):
    return int(x1) - int(x0), int(y1) - int(y0), int(z1) - int(z0)


def dominant(dx, dy, dz):
    """0, 1 or 2: x if |dx| >= max(|dy|, |dz|), else y if |dy| >= |dz|, else z"""
    return 0 if abs(dx) >= max(abs(dy), abs(dz)) else (1 if abs(dy) >= abs(dz) else 2)


def ray_end(x0, y0, z0, x1, y1, z1, max_length=UINT_MAX):
    """min((unsigned)(scale * da), da) on double voxel coordinates"""
    f = np.float64
    d = _deltas(x0, y0, z0, x1, y1, z1)
    da = abs(d[dominant(*d)])
    with np.errstate(all="ignore"):
        dist = np.sqrt((f(x0) - f(x1)) * (f(x0) - f(x1)) + (f(y0) - f(y1)) * (f(y0) - f(y1)) + (f(z0) - f(z1)) * (f(z0) - f(z1)))
        scale = std_min(f(1.0), f(max_length) / dist)
    return min(int(scale * f(da)), da)


def raytrace_line(x0, y0, z0, x1, y1, z1, max_length=UINT_MAX):
    """voxel_grid.h raytraceLine + bresenham3D literally, in (x, y, z) steps instead of offsets and masks: the voxels at() visits"""
    d = _deltas(x0, y0, z0, x1, y1, z1)
    ad = [abs(v) for v in d]
    step = [1 if v > 0 else -1 for v in d]                               # sign(): 0 gives -1, which a zero count never uses
    a = dominant(*d)
    b, c = [k for k in range(3) if k != a]
    end = ray_end(x0, y0, z0, x1, y1, z1, max_length)
    abs_da, abs_db, abs_dc = ad[a], ad[b], ad[c]
    error_b = error_c = abs_da // 2
    pos, out = [int(x0), int(y0), int(z0)], []
    for _ in range(end):
        out.append(tuple(pos))
        pos[a] += step[a]
        error_b += abs_db
        error_c += abs_dc
        if error_b >= abs_da:
            pos[b] += step[b]
            error_b -= abs_da
        if error_c >= abs_da:
            pos[c] += step[c]
            error_c -= abs_da
    out.append(tuple(pos))
    return out


def line_closed(x0, y0, z0, x1, y1, z1):
    """the whole line by the closed form: voxel k lies k steps along the dominant axis, (da / 2 + k * db) / da along the others"""
    p0 = (int(x0), int(y0), int(z0))
    d = _deltas(x0, y0, z0, x1, y1, z1)
    a = dominant(*d)
    da = abs(d[a])
    out = []
    for k in range(da + 1):
        out.append(tuple(p0[i] + (1 if d[i] >= 0 else -1) * (k if i == a else ((da // 2 + k * abs(d[i])) // da if da else 0)) for i in range(3)))
    return out


# ---- the per-record arithmetic, one record at a time --------------------------------------------------------------------------------
def map_end(cm):
    f = np.float64
    return f(cm.ox) + (f(cm.size_x) - f(1) + f(0.5)) * f(cm.res), f(cm.oy) + (f(cm.size_y) - f(1) + f(0.5)) * f(cm.res)


def clip_record(cm, vox, origin, wx, wy, wz, layer_max_h):
    """raytraceFreespace's shortening and clips of one record: the point the ray ends at"""
    f = np.float64
    ox, oy, oz = (f(v) for v in origin)
    wx, wy, wz = f(wx), f(wy), f(wz)
    origin_x, origin_y, origin_z, res, lmh = f(cm.ox), f(cm.oy), f(vox.origin_z), f(cm.res), f(layer_max_h)
    map_end_x, map_end_y = map_end(cm)
    with np.errstate(all="ignore"):
        d = np.sqrt((wx - ox) * (wx - ox) + (wy - oy) * (wy - oy) + (wz - oz) * (wz - oz))
        fac = std_max(std_min(f(1.0), (d - f(2) * res) / d), f(0.0))
        wx, wy, wz = fac * (wx - ox) + ox, fac * (wy - oy) + oy, fac * (wz - oz) + oz
        a, b, c, t = wx - ox, wy - oy, wz - oz, f(1.0)
        if wz > lmh:
            t = std_max(f(0.0), std_min(t, (lmh - f(0.01) - oz) / c))
        elif wz < origin_z:
            t = std_min(t, (origin_z - oz) / c)
        if wx < origin_x:
            t = std_min(t, (origin_x - ox) / a)
        if wy < origin_y:
            t = std_min(t, (origin_y - oy) / b)
        if wx > map_end_x:
            t = std_min(t, (map_end_x - ox) / a)
        if wy > map_end_y:
            t = std_min(t, (map_end_y - oy) / b)
        return ox + a * t, oy + b * t, oz + c * t


def observe_loop(cm, columns, vox, observations, layer_max_h=2.0, bounds=None):
    """VoxelLayer::updateBounds, literally: every clearing observation, then every marking one, bytes written as they go"""
    check(observations, layer_max_h)
    flat, cols = cm.grid.reshape(-1), columns.reshape(-1)
    for o in observations:                                               # raytraceFreespace
        if not field(o, "clearing"):
            continue
        ox, oy, oz = (float(v) for v in o["origin"])
        start = world_to_map_3d_float(cm, vox, ox, oy, oz)
        if start is None:
            continue
        cell_range = cell_distance(field(o, "raytrace_range"), cm.res)
        for wx, wy, wz in zip(*xyz(o)):
            if not (field(o, "min_obstacle_height") <= wz <= field(o, "max_obstacle_height")):
                continue
            wx, wy, wz = clip_record(cm, vox, (ox, oy, oz), wx, wy, wz, layer_max_h)
            end = world_to_map_3d_float(cm, vox, wx, wy, wz)
            if end is None:
                continue
            for x, y, z in raytrace_line(*start, *end, cell_range):      # ClearVoxelInMap
                i = y * cm.size_x + x
                col = int(cols[i]) & ~mask(z)
                cols[i] = col
                if below(marked(col), vox.mark_threshold):
                    flat[i] = cref.FREE_SPACE if below(unknown(col), vox.unknown_threshold) else cref.NO_INFORMATION
            if bounds is not None:
                cref._touch(bounds, *raytrace_bounds(ox, oy, wx, wy, field(o, "raytrace_range")))
    for o in observations:                                               # the marking loop of updateBounds
        if not field(o, "marking"):
            continue
        f = np.float64
        ox, oy, oz = (f(v) for v in o["origin"])
        with np.errstate(all="ignore"):
            sq_range = f(field(o, "obstacle_range")) * f(field(o, "obstacle_range"))
            for px, py, pz in zip(*xyz(o)):
                if not (field(o, "min_obstacle_height") <= pz <= field(o, "max_obstacle_height")):
                    continue
                if pz > layer_max_h:
                    continue
                sq = (px - ox) * (px - ox) + (py - oy) * (py - oy) + (pz - oz) * (pz - oz)
                if sq >= sq_range:
                    continue
                m = world_to_map_3d(cm, vox, px, py, f(vox.origin_z) if pz < vox.origin_z else pz)
                if m is None:
                    continue
                i = m[1] * cm.size_x + m[0]
                col = int(cols[i]) | mask(m[2])                          # markVoxelInMap: true iff the marked bits are not below
                cols[i] = col
                if not below(marked(col), vox.mark_threshold):
                    flat[i] = cref.LETHAL_OBSTACLE
                    if bounds is not None:
                        cref._touch(bounds, float(px), float(py))
    return bounds


# ---- vectorised -------------------------------------------------------------------------------------------------------------------------
def _map3_v(cm, vox, wx, wy, wz):
    """worldToMap3DFloat over arrays: ok, fx, fy, fz"""
    with np.errstate(all="ignore"):
        ok = np.isfinite(wx) & np.isfinite(wy) & np.isfinite(wz)
        ok &= ~(wx < cm.ox) & ~(wy < cm.oy) & ~(wz < vox.origin_z)
        fx, fy, fz = (wx - cm.ox) / cm.res, (wy - cm.oy) / cm.res, (wz - vox.origin_z) / np.float64(vox.z_resolution)
        ok &= (fx < cm.size_x) & (fy < cm.size_y) & (fz < vox.size_z)
    return ok, fx, fy, fz


def _vmin(a, b):
    """std::min(a, b) element by element"""
    return np.where(b < a, b, a)


def _vmax(a, b):
    return np.where(a < b, b, a)


def clear_records(cm, vox, o, layer_max_h):
    """the clearing arithmetic of one observation over all its records: a dict of arrays [n] -- ok, d (the integer deltas [n, 3]),
    axis, da, end, ex, ey and the clips taken (ceiling, floor, left, bottom, right, top) -- and start (the sensor's voxel); None when
    worldToMap3DFloat refuses the origin"""
    f = np.float64
    ox, oy, oz = (f(v) for v in o["origin"])
    start = world_to_map_3d_float(cm, vox, ox, oy, oz)
    if start is None:
        return None
    wx, wy, wz = xyz(o)
    origin_x, origin_y, origin_z, res, lmh = f(cm.ox), f(cm.oy), f(vox.origin_z), f(cm.res), f(layer_max_h)
    map_end_x, map_end_y = map_end(cm)
    with np.errstate(all="ignore"):
        in_window = (field(o, "min_obstacle_height") <= wz) & (wz <= field(o, "max_obstacle_height"))
        d = np.sqrt((wx - ox) * (wx - ox) + (wy - oy) * (wy - oy) + (wz - oz) * (wz - oz))
        fac = _vmax(_vmin(np.ones_like(d), (d - f(2) * res) / d), np.zeros_like(d))
        wx, wy, wz = fac * (wx - ox) + ox, fac * (wy - oy) + oy, fac * (wz - oz) + oz
        a, b, c, t = wx - ox, wy - oy, wz - oz, np.ones_like(d)
        ceiling = wz > lmh
        floor = ~ceiling & (wz < origin_z)
        t = np.where(ceiling, _vmax(np.zeros_like(d), _vmin(t, (lmh - f(0.01) - oz) / c)), t)
        t = np.where(floor, _vmin(t, (origin_z - oz) / c), t)
        left, bottom, right, top = wx < origin_x, wy < origin_y, wx > map_end_x, wy > map_end_y
        t = np.where(left, _vmin(t, (origin_x - ox) / a), t)
        t = np.where(bottom, _vmin(t, (origin_y - oy) / b), t)
        t = np.where(right, _vmin(t, (map_end_x - ox) / a), t)
        t = np.where(top, _vmin(t, (map_end_y - oy) / b), t)
        wx, wy, wz = ox + a * t, oy + b * t, oz + c * t
        ok, fx, fy, fz = _map3_v(cm, vox, wx, wy, wz)
        ok &= in_window
        fx, fy, fz = np.where(ok, fx, start[0]), np.where(ok, fy, start[1]), np.where(ok, fz, start[2])
        s0 = np.array([int(v) for v in start], np.int64)
        delta = np.stack([fx.astype(np.int64), fy.astype(np.int64), fz.astype(np.int64)], axis=1) - s0[None, :]
        ad = np.abs(delta)
        axis = np.where(ad[:, 0] >= np.maximum(ad[:, 1], ad[:, 2]), 0, np.where(ad[:, 1] >= ad[:, 2], 1, 2))
        da = ad[np.arange(len(ad)), axis]
        dist = np.sqrt((start[0] - fx) * (start[0] - fx) + (start[1] - fy) * (start[1] - fy) + (start[2] - fz) * (start[2] - fz))
        cell_range = cell_distance(field(o, "raytrace_range"), cm.res)
        scale = _vmin(np.ones_like(dist), f(cell_range) / dist)
        end = np.minimum((scale * da.astype(f)).astype(np.int64), da)
        ddx, ddy = wx - ox, wy - oy
        full = np.sqrt(ddx * ddx + ddy * ddy)
        r = f(field(o, "raytrace_range")) / full
        s = np.where(r < 1.0, r, 1.0)
        ex, ey = ox + ddx * s, oy + ddy * s
    return {"ok": ok, "delta": delta, "axis": axis, "da": da, "end": end, "ex": ex, "ey": ey, "start": s0, "ceiling": ceiling, "floor": floor,
            "left": left, "bottom": bottom, "right": right, "top": top}


def mark_records(cm, vox, o, layer_max_h):
    """the marking arithmetic of one observation: ok (accepted), idx (the cell), z, px, py"""
    f = np.float64
    px, py, pz = xyz(o)
    ox, oy, oz = (f(v) for v in o["origin"])
    with np.errstate(all="ignore"):
        ok = (field(o, "min_obstacle_height") <= pz) & (pz <= field(o, "max_obstacle_height")) & ~(pz > layer_max_h)
        sq = (px - ox) * (px - ox) + (py - oy) * (py - oy) + (pz - oz) * (pz - oz)
        ok &= ~(sq >= f(field(o, "obstacle_range")) * f(field(o, "obstacle_range")))
        zz = np.where(pz < vox.origin_z, f(vox.origin_z), pz)
        ok &= np.isfinite(px) & np.isfinite(py) & np.isfinite(zz) & ~(px < cm.ox) & ~(py < cm.oy) & ~(zz < vox.origin_z)
        qx, qy, qz = (px - cm.ox) / cm.res, (py - cm.oy) / cm.res, (zz - vox.origin_z) / f(vox.z_resolution)
        ok &= (qx < INT_LIMIT) & (qy < INT_LIMIT) & (qz < INT_LIMIT)
        mx, my, mz = (np.where(ok, q, 0.0).astype(np.int64) for q in (qx, qy, qz))
    ok &= (mx < cm.size_x) & (my < cm.size_y) & (mz < vox.size_z)
    return {"ok": ok, "idx": my * cm.size_x + mx, "z": mz, "px": px, "py": py}


def observe(cm, columns, vox, observations, layer_max_h=2.0, bounds=None, chunk=2048, detail=None):
    """... as the set function of the header: every ray by the closed form, then the byte rule per cell.  `detail`, a dict, receives
    the per-cell classes (touched, accepted, lethal, freed, unknown, kept) and the clearing records' arrays per observation."""
    check(observations, layer_max_h)
    cells = cm.size_x * cm.size_y
    flat, cols = cm.grid.reshape(-1), columns.reshape(-1)
    hit = np.zeros(cells * 16, bool)                                     # voxel (cell, z) lies on a ray
    rays = []
    for o in observations:
        if not field(o, "clearing"):
            continue
        c = clear_records(cm, vox, o, layer_max_h)
        rays.append(c)
        if c is None:
            continue
        sel = np.flatnonzero(c["ok"])
        for at in range(0, sel.size, chunk):
            s = sel[at:at + chunk]
            delta, axis, da, end = c["delta"][s], c["axis"][s], c["da"][s], c["end"][s]
            k = np.arange(int(end.max()) + 1, dtype=np.int64)[None, :]
            take = k <= end[:, None]
            pos = []
            for i in range(3):
                adi, sign = np.abs(delta[:, i])[:, None], np.where(delta[:, i] >= 0, 1, -1)[:, None]
                minor = (da[:, None] // 2 + k * adi) // np.maximum(da[:, None], 1)
                pos.append(c["start"][i] + sign * np.where((axis == i)[:, None], k, minor))
            hit[((pos[1] * cm.size_x + pos[0]) * 16 + pos[2])[take]] = True
        _fold(bounds, c["ex"][sel], c["ey"][sel])
    hit = hit.reshape(cells, 16)
    touched = hit.any(axis=1)
    cleared = (hit.astype(np.uint32) << np.arange(16, dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint32)
    col_c = cols & ~(cleared | (cleared << np.uint32(16)))
    marks = np.zeros(cells * 16, bool)
    accepted = []
    for o in observations:
        if not field(o, "marking"):
            continue
        m = mark_records(cm, vox, o, layer_max_h)
        accepted.append(m)
        marks[(m["idx"] * 16 + m["z"])[m["ok"]]] = True
    marks = (marks.reshape(cells, 16).astype(np.uint32) << np.arange(16, dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint32)
    marks |= marks << np.uint32(16)
    col_f = col_c | marks
    lethal = (marks != 0) & (POPCOUNT16[col_f >> 16] > vox.mark_threshold)
    written = touched & ~lethal & (POPCOUNT16[col_c >> 16] <= vox.mark_threshold)
    few = POPCOUNT16[((col_c >> 16) ^ col_c) & 0xFFFF] <= vox.unknown_threshold
    flat[written & few] = cref.FREE_SPACE
    flat[written & ~few] = cref.NO_INFORMATION
    flat[lethal] = cref.LETHAL_OBSTACLE
    cols[:] = col_f
    for m in accepted:                                                   # the named departure: every accepted record of a lethal cell touches
        sel = m["ok"] & lethal[np.where(m["ok"], m["idx"], 0)]
        _fold(bounds, m["px"][sel], m["py"][sel])
    if detail is not None:
        detail.update({"touched": touched, "accepted": marks != 0, "lethal": lethal, "freed": written & few, "unknown": written & ~few,
                       "kept": touched & ~lethal & ~written, "rays": rays})
    return bounds
