"""numpy restatement of the ObstacleLayer contract of include/gem_hip_obstacle.h, on top of costmap_ref.Costmap / world_to_map and the
line of footprint_ref: the pieces of ROS noetic costmap_2d (obstacle_layer.cpp updateBounds / raytraceFreespace / updateRaytraceBounds,
observation_buffer.cpp's height window, costmap_2d.h raytraceLine / bresenham2D / cellDistance) that gem_costmap_observe and
gem_obstacle_host stand for.  costmap_2d is not available to these tests: this is a restatement, unverified against the library.

The contract is stated twice: `observe_loop`, a plain sequential loop, observation by observation and record by record, that walks a ray
with bresenham2D's own loop and its error_b; and `observe`, vectorised, with the closed form of the line.  tests/test_obstacle_cpu.py
pins the two to identical results.  All arithmetic is numpy float64 = C double, every operation rounded on its own.

An observation is a dict as gem_amd.Costmap.observe takes it: points (float32 [n, k >= 3]: x, y, z first), origin (x, y, z) and
optionally obstacle_range, raytrace_range, min_obstacle_height, max_obstacle_height, marking, clearing."""
import numpy as np

import costmap_ref as cref
import footprint_ref as fref

MARKING, CLEARING, MAX_OBSERVATIONS = 1, 2, 8
DEFAULTS = {"obstacle_range": 2.5, "raytrace_range": 3.0, "min_obstacle_height": 0.0, "max_obstacle_height": 2.0, "marking": True,
            "clearing": True}
UINT_MAX = 4294967295


def field(o, name):
    return o.get(name, DEFAULTS[name])


def xyz(o):
    """the records' coordinates as float64 arrays (the float32 values widened exactly)"""
    p = np.asarray(o["points"], np.float32)
    p = p.reshape(len(p), -1) if len(p) else np.zeros((0, 3), np.float32)
    return p[:, 0].astype(np.float64), p[:, 1].astype(np.float64), p[:, 2].astype(np.float64)


def std_min(a, b):
    """std::min(a, b): (b < a) ? b : a"""
    return b if b < a else a


def std_max(a, b):
    """std::max(a, b): (a < b) ? b : a"""
    return b if a < b else a


def cell_distance(world_dist, res):
    """cellDistance: (unsigned)max(0.0, ceil(d / resolution)), saturating at UINT_MAX"""
    with np.errstate(all="ignore"):
        c = std_max(np.float64(0.0), np.ceil(np.float64(world_dist) / np.float64(res)))
    return UINT_MAX if c >= float(UINT_MAX) else int(c)


# ---- raytraceLine -----------------------------------------------------------------------------------------------------------------
def ray_end(x0, y0, x1, y1, max_length):
    """how many steps raytraceLine hands to bresenham2D and that clamps: min((unsigned)(scale * da), da)"""
    dx, dy = x1 - x0, y1 - y0
    da = max(abs(dx), abs(dy))
    dist = np.sqrt(np.float64(dx * dx + dy * dy))
    with np.errstate(all="ignore"):
        scale = np.float64(1.0) if dist == 0.0 else std_min(np.float64(1.0), np.float64(max_length) / dist)
    return min(int(scale * np.float64(da)), da)


def raytrace_line(x0, y0, x1, y1, max_length=UINT_MAX):
    """costmap_2d.h raytraceLine + bresenham2D literally, in (x, y) steps instead of offsets into the array: the cells at() visits"""
    dx, dy = x1 - x0, y1 - y0
    abs_dx, abs_dy = abs(dx), abs(dy)
    step_x, step_y = (1 if dx > 0 else -1), (1 if dy > 0 else -1)        # sign(): 0 gives -1, which a zero count never uses
    dist = np.sqrt(np.float64(dx * dx + dy * dy))
    with np.errstate(all="ignore"):
        scale = np.float64(1.0) if dist == 0.0 else std_min(np.float64(1.0), np.float64(max_length) / dist)
    if abs_dx >= abs_dy:
        abs_da, abs_db, error_b, a, b, length = abs_dx, abs_dy, abs_dx // 2, (step_x, 0), (0, step_y), int(scale * np.float64(abs_dx))
    else:
        abs_da, abs_db, error_b, a, b, length = abs_dy, abs_dx, abs_dy // 2, (0, step_y), (step_x, 0), int(scale * np.float64(abs_dy))
    end = min(length, abs_da)
    x, y, out = x0, y0, []
    for _ in range(end):
        out.append((x, y))
        x += a[0]; y += a[1]
        error_b += abs_db
        if error_b >= abs_da:
            x += b[0]; y += b[1]
            error_b -= abs_da
    out.append((x, y))
    return out


# ---- the per-record arithmetic, one record at a time --------------------------------------------------------------------------------
def clip_record(cm, ox, oy, wx, wy):
    """raytraceFreespace's four clips: (wx, wy, number of clips taken)"""
    f = np.float64
    ox, oy, wx, wy = f(ox), f(oy), f(wx), f(wy)
    origin_x, origin_y = f(cm.ox), f(cm.oy)
    map_end_x, map_end_y = origin_x + f(cm.size_x) * f(cm.res), origin_y + f(cm.size_y) * f(cm.res)
    clips = 0
    with np.errstate(all="ignore"):
        a, b = wx - ox, wy - oy
        if wx < origin_x:
            t = (origin_x - ox) / a; wx = origin_x; wy = oy + b * t; clips += 1
        if wy < origin_y:
            t = (origin_y - oy) / b; wx = ox + a * t; wy = origin_y; clips += 1
        if wx > map_end_x:
            t = (map_end_x - ox) / a; wx = map_end_x - f(.001); wy = oy + b * t; clips += 1
        if wy > map_end_y:
            t = (map_end_y - oy) / b; wx = ox + a * t; wy = map_end_y - f(.001); clips += 1
    return wx, wy, clips


def raytrace_bounds(ox, oy, wx, wy, raytrace_range):
    """updateRaytraceBounds: the point it touches"""
    f = np.float64
    with np.errstate(all="ignore"):
        ddx, ddy = f(wx) - f(ox), f(wy) - f(oy)
        full = np.sqrt(ddx * ddx + ddy * ddy)
        s = std_min(f(1.0), f(raytrace_range) / full)
        return float(f(ox) + ddx * s), float(f(oy) + ddy * s)


def check(observations, layer_max_h):
    """the refusals of the contract that a reference can meet (the rest are about pointers)"""
    assert 0 <= len(observations) <= MAX_OBSERVATIONS and not np.isnan(layer_max_h)
    for o in observations:
        assert field(o, "marking") or field(o, "clearing")
        assert all(np.isfinite(v) for v in o["origin"]) and field(o, "obstacle_range") >= 0 and field(o, "raytrace_range") >= 0
        assert field(o, "min_obstacle_height") <= field(o, "max_obstacle_height")


def observe_loop(cm, observations, layer_max_h=2.0, bounds=None):
    """ObstacleLayer::updateBounds, sequentially: every clearing observation, then every marking one"""
    check(observations, layer_max_h)
    flat = cm.grid.reshape(-1)
    for o in observations:                                               # raytraceFreespace
        if not field(o, "clearing"):
            continue
        ox, oy = float(o["origin"][0]), float(o["origin"][1])
        start = cref.world_to_map(cm, ox, oy)
        if start is None:
            continue
        if bounds is not None:
            cref._touch(bounds, ox, oy)
        cell_range = cell_distance(field(o, "raytrace_range"), cm.res)
        for wx, wy, wz in zip(*xyz(o)):
            if not (field(o, "min_obstacle_height") <= wz <= field(o, "max_obstacle_height")):
                continue
            wx, wy, _ = clip_record(cm, ox, oy, wx, wy)
            end = cref.world_to_map(cm, wx, wy)
            if end is None:
                continue
            for x, y in raytrace_line(start[0], start[1], end[0], end[1], cell_range):
                flat[y * cm.size_x + x] = cref.FREE_SPACE
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
                m = cref.world_to_map(cm, px, py)
                if m is None:
                    continue
                flat[m[1] * cm.size_x + m[0]] = cref.LETHAL_OBSTACLE
                if bounds is not None:
                    cref._touch(bounds, float(px), float(py))
    return bounds


# ---- vectorised ---------------------------------------------------------------------------------------------------------------------
def clear_records(cm, o):
    """the clearing arithmetic of one observation over all its records: a dict of arrays [n] -- in_window, clips, ok (worldToMap
    accepted the clipped point), x1, y1, end, da, ex, ey -- and x0, y0, cell_range; None when worldToMap refuses the origin"""
    ox, oy = np.float64(o["origin"][0]), np.float64(o["origin"][1])
    start = cref.world_to_map(cm, ox, oy)
    if start is None:
        return None
    wx, wy, wz = xyz(o)
    origin_x, origin_y = np.float64(cm.ox), np.float64(cm.oy)
    map_end_x, map_end_y = origin_x + np.float64(cm.size_x) * np.float64(cm.res), origin_y + np.float64(cm.size_y) * np.float64(cm.res)
    with np.errstate(all="ignore"):
        in_window = (field(o, "min_obstacle_height") <= wz) & (wz <= field(o, "max_obstacle_height"))
        a, b = wx - ox, wy - oy
        clips = np.zeros(wx.shape, np.int64)
        c = wx < origin_x
        t = (origin_x - ox) / a
        wx, wy = np.where(c, origin_x, wx), np.where(c, oy + b * t, wy)
        clips += c
        c = wy < origin_y
        t = (origin_y - oy) / b
        wx, wy = np.where(c, ox + a * t, wx), np.where(c, origin_y, wy)
        clips += c
        c = wx > map_end_x
        t = (map_end_x - ox) / a
        wx, wy = np.where(c, map_end_x - np.float64(.001), wx), np.where(c, oy + b * t, wy)
        clips += c
        c = wy > map_end_y
        t = (map_end_y - oy) / b
        wx, wy = np.where(c, ox + a * t, wx), np.where(c, map_end_y - np.float64(.001), wy)
        clips += c
        ok, idx = cref.world_to_map_v(cm, wx, wy)
        ok &= in_window
        x1, y1 = np.where(ok, idx % cm.size_x, start[0]), np.where(ok, idx // cm.size_x, start[1])
        dx, dy = x1 - start[0], y1 - start[1]
        da = np.maximum(np.abs(dx), np.abs(dy))
        cell_range = cell_distance(field(o, "raytrace_range"), cm.res)
        dist = np.sqrt((dx * dx + dy * dy).astype(np.float64))
        r = np.float64(cell_range) / dist
        scale = np.where(dist == 0.0, 1.0, np.where(r < 1.0, r, 1.0))
        end = np.minimum((scale * da.astype(np.float64)).astype(np.int64), da)
        ddx, ddy = wx - ox, wy - oy
        full = np.sqrt(ddx * ddx + ddy * ddy)
        r = np.float64(field(o, "raytrace_range")) / full
        s = np.where(r < 1.0, r, 1.0)
        ex, ey = ox + ddx * s, oy + ddy * s
    return {"in_window": in_window, "clips": clips, "ok": ok, "x1": x1, "y1": y1, "end": end, "da": da, "ex": ex, "ey": ey,
            "x0": start[0], "y0": start[1], "cell_range": cell_range}


def mark_records(cm, o, layer_max_h):
    """the marking arithmetic of one observation: in_window, too_high, too_far, ok (marked), idx, px, py"""
    px, py, pz = xyz(o)
    ox, oy, oz = (np.float64(v) for v in o["origin"])
    with np.errstate(all="ignore"):
        in_window = (field(o, "min_obstacle_height") <= pz) & (pz <= field(o, "max_obstacle_height"))
        too_high = in_window & (pz > layer_max_h)
        sq = (px - ox) * (px - ox) + (py - oy) * (py - oy) + (pz - oz) * (pz - oz)
        too_far = in_window & ~too_high & (sq >= np.float64(field(o, "obstacle_range")) * np.float64(field(o, "obstacle_range")))
        on_map, idx = cref.world_to_map_v(cm, px, py)
    return {"in_window": in_window, "too_high": too_high, "too_far": too_far, "ok": in_window & ~too_high & ~too_far & on_map, "idx": idx,
            "px": px, "py": py}


def _fold(bounds, xs, ys):
    """a sequence of touch() calls: the extremes, folded once"""
    if bounds is not None and len(xs):
        bounds[0], bounds[1] = std_min(float(np.min(xs)), bounds[0]), std_min(float(np.min(ys)), bounds[1])
        bounds[2], bounds[3] = std_max(float(np.max(xs)), bounds[2]), std_max(float(np.max(ys)), bounds[3])


def observe(cm, observations, layer_max_h=2.0, bounds=None, chunk=4096):
    """... vectorised: every record's ray by the closed form of the line, cells 0 .. end"""
    check(observations, layer_max_h)
    flat = cm.grid.reshape(-1)
    for o in observations:
        if not field(o, "clearing"):
            continue
        c = clear_records(cm, o)
        if c is None:
            continue
        _fold(bounds, [float(o["origin"][0])], [float(o["origin"][1])])
        sel = np.flatnonzero(c["ok"])
        for at in range(0, sel.size, chunk):
            s = sel[at:at + chunk]
            x0, y0 = np.full(s.size, c["x0"], np.int64), np.full(s.size, c["y0"], np.int64)
            cx, cy, _ = fref.line_closed_v(x0, y0, c["x1"][s], c["y1"][s])
            k = np.arange(cx.shape[1], dtype=np.int64)[None, :]
            take = k <= c["end"][s][:, None]
            flat[(cy * cm.size_x + cx)[take]] = cref.FREE_SPACE
        _fold(bounds, c["ex"][sel], c["ey"][sel])
    for o in observations:
        if not field(o, "marking"):
            continue
        m = mark_records(cm, o, layer_max_h)
        flat[m["idx"][m["ok"]]] = cref.LETHAL_OBSTACLE
        _fold(bounds, m["px"][m["ok"]], m["py"][m["ok"]])
    return bounds


def classes(cm, o, layer_max_h):
    """the share of an observation's records in every class the GPU tests want present: by clips taken and whether the range cut the
    ray (end < da), and by what the marking loop did with the record"""
    n = max(len(o["points"]), 1)
    out = {}
    c = clear_records(cm, o)
    if c is not None:
        cut = c["end"] < c["da"]
        for name, sel in (("no clip, full", (c["clips"] == 0) & ~cut), ("no clip, cut", (c["clips"] == 0) & cut),
                          ("one clip, full", (c["clips"] == 1) & ~cut), ("one clip, cut", (c["clips"] == 1) & cut),
                          ("two clips, full", (c["clips"] == 2) & ~cut), ("two clips, cut", (c["clips"] == 2) & cut)):
            out[name] = float((sel & c["ok"]).sum()) / n
    m = mark_records(cm, o, layer_max_h)
    out["marked"] = float(m["ok"].sum()) / n
    out["too high"] = float(m["too_high"].sum()) / n
    out["too far"] = float(m["too_far"].sum()) / n
    out["outside the window"] = float((~m["in_window"]).sum()) / n
    return out
