"""numpy restatement of the costmap layers (layers/src/pointMap_layer.cpp:45-100, elevationMap_layer.cpp:42-87) and of the pieces of
costmap_2d they call (ROS noetic costmap_2d.cpp / costmap_layer.cpp), the semantics include/gem_hip.h pins for gem_costmap_*.
costmap_2d is not available to these tests: this is a restatement, unverified against the library.

Every operation has two forms: a literal one (`*_loop`: the reference's loop, one record or cell at a time, the definition) and a
vectorised one, fast enough for millions of records; tests/test_costmap_cpu.py pins the two to identical results on small inputs.
All arithmetic is numpy float64 = C double; a grid is uint8 [size_y, size_x], so grid.ravel()[my * size_x + mx] is getIndex."""
import numpy as np

FREE_SPACE, LETHAL_OBSTACLE, NO_INFORMATION = 0, 254, 255
INT_LIMIT = 2147483648.0


class Costmap:
    def __init__(self, size_x, size_y, resolution, origin_x=0.0, origin_y=0.0, default_value=NO_INFORMATION):
        self.size_x, self.size_y = int(size_x), int(size_y)
        self.res, self.ox, self.oy = float(resolution), float(origin_x), float(origin_y)
        self.default = int(default_value)
        self.grid = np.full((self.size_y, self.size_x), self.default, np.uint8)

    def size_in_meters(self):
        return (self.size_x - 1 + 0.5) * self.res, (self.size_y - 1 + 0.5) * self.res

    def reset(self):
        self.grid[:] = self.default


# ---- worldToMap ---------------------------------------------------------------------------------------------------------------
def world_to_map(cm, wx, wy):
    """one point: (mx, my) or None.  Non-finite coordinates and quotients beyond int fail (the contract's deliberate difference)."""
    wx, wy = float(wx), float(wy)
    if not (np.isfinite(wx) and np.isfinite(wy)):
        return None
    if wx < cm.ox or wy < cm.oy:
        return None
    with np.errstate(all="ignore"):
        qx, qy = (np.float64(wx) - cm.ox) / np.float64(cm.res), (np.float64(wy) - cm.oy) / np.float64(cm.res)
    if not (qx < INT_LIMIT and qy < INT_LIMIT):
        return None
    mx, my = int(qx), int(qy)                                            # the (int) cast truncates
    return (mx, my) if mx < cm.size_x and my < cm.size_y else None


def world_to_map_v(cm, wx, wy):
    """arrays: (ok, index) with index = my * size_x + mx where ok"""
    wx, wy = np.asarray(wx, np.float64), np.asarray(wy, np.float64)
    with np.errstate(all="ignore"):
        ok = np.isfinite(wx) & np.isfinite(wy)
        ok &= ~(wx < cm.ox) & ~(wy < cm.oy)
        qx, qy = (wx - cm.ox) / cm.res, (wy - cm.oy) / cm.res
        ok &= (qx < INT_LIMIT) & (qy < INT_LIMIT)
        mx, my = np.where(ok, qx, 0.0).astype(np.int64), np.where(ok, qy, 0.0).astype(np.int64)
    ok &= (mx < cm.size_x) & (my < cm.size_y)
    return ok, my * cm.size_x + mx


# ---- the marking loops --------------------------------------------------------------------------------------------------------
def _std_min(a, b):
    return b if b < a else a                                             # std::min(a, b)


def _std_max(a, b):
    return b if a < b else a                                             # std::max(a, b)


def _touch(bounds, px, py):
    """costmap_layer.cpp touch(): *min_x = std::min(x, *min_x), ..., *max_y = std::max(y, *max_y)"""
    bounds[0], bounds[1] = _std_min(px, bounds[0]), _std_min(py, bounds[1])
    bounds[2], bounds[3] = _std_max(px, bounds[2]), _std_max(py, bounds[3])


def write_loop(cm, px, py, lethal, bounds=None):
    """the body both layers share, input by input: worldToMap, costmap_[index] = verdict, touch"""
    flat = cm.grid.reshape(-1)
    for x, y, l in zip(np.asarray(px, np.float64), np.asarray(py, np.float64), np.asarray(lethal, bool)):
        m = world_to_map(cm, x, y)
        if m is None:
            continue
        flat[m[1] * cm.size_x + m[0]] = LETHAL_OBSTACLE if l else FREE_SPACE
        if bounds is not None:
            _touch(bounds, float(x), float(y))
    return bounds


def write(cm, px, py, lethal, bounds=None):
    """... vectorised: the last accepted input of a cell decides; the bounds take the extremes of the accepted inputs"""
    px, py, lethal = np.asarray(px, np.float64), np.asarray(py, np.float64), np.asarray(lethal, bool)
    ok, idx = world_to_map_v(cm, px, py)
    sel = np.flatnonzero(ok)
    if sel.size == 0:
        return bounds
    cells, first_rev = np.unique(idx[sel][::-1], return_index=True)       # first in reverse = last in order
    last = sel[sel.size - 1 - first_rev]
    cm.grid.reshape(-1)[cells] = np.where(lethal[last], LETHAL_OBSTACLE, FREE_SPACE).astype(np.uint8)
    if bounds is not None:                                               # a sequence of touch() calls: the extremes, folded once
        bounds[0], bounds[1] = _std_min(float(px[sel].min()), bounds[0]), _std_min(float(py[sel].min()), bounds[1])
        bounds[2], bounds[3] = _std_max(float(px[sel].max()), bounds[2]), _std_max(float(py[sel].max()), bounds[3])
    return bounds


def point_inputs(points, thresh):
    """PointMapLayer::updateBounds:57-77: px = (double)x, py = (double)y; travers > thresh is free, anything else (NaN) lethal"""
    with np.errstate(invalid="ignore"):
        lethal = ~(points["travers"].astype(np.float64) > float(thresh))
    return points["x"].astype(np.float64), points["y"].astype(np.float64), lethal


def mark_points(cm, points, thresh, bounds=None, loop=False):
    return (write_loop if loop else write)(cm, *point_inputs(points, thresh), bounds)


class VisualGeom:
    """visualMap_'s geometry as gem_local_capture takes it (the attributes of local_ref.Capture, which serves as well)"""

    def __init__(self, L, map_length, resolution, position, start):
        self.L, self.res = int(L), float(resolution)
        self.off = 0.5 * float(map_length) - 0.5 * self.res
        self.px, self.py = float(position[0]), float(position[1])
        self.sx, self.sy = int(start[0]), int(start[1])


def visual_inputs(traver, g, thresh):
    """ElevationMapLayer::updateBounds:58-67 over visualMap_: all L * L cells in grid_map's iteration order (the linear index of the
    column-major buffer), positions by getPositionFromIndex in double ((p + off) - res * unwrapped index), is_obstacle = traver <
    thresh with NaN for a cell show() did not keep.  traver: the [L * L] plane in that order; g: a VisualGeom."""
    t = np.asarray(traver, np.float32).reshape(-1)
    L = g.L
    lin = np.arange(L * L)
    ux, uy = (lin % L - g.sx) % L, (lin // L - g.sy) % L
    px = (g.px + g.off) + g.res * (-ux).astype(np.float64)
    py = (g.py + g.off) + g.res * (-uy).astype(np.float64)
    with np.errstate(invalid="ignore"):
        lethal = t.astype(np.float64) < float(thresh)
    return px, py, lethal


def mark_visual(cm, traver, g, thresh, bounds=None, loop=False):
    return (write_loop if loop else write)(cm, *visual_inputs(traver, g, thresh), bounds)


def verdict_mix(cm, px, py, lethal):
    """(cells marked, cells that received both verdicts): how much of an input exercises last-writer-wins"""
    ok, idx = world_to_map_v(cm, px, py)
    lethal = np.asarray(lethal, bool)
    got_l = np.zeros(cm.size_x * cm.size_y, bool); got_f = got_l.copy()
    got_l[idx[ok & lethal]] = True
    got_f[idx[ok & ~lethal]] = True
    return int((got_l | got_f).sum()), int((got_l & got_f).sum())


# ---- Costmap2D::updateOrigin ----------------------------------------------------------------------------------------------------
def origin_step(cm, new_ox, new_oy):
    """(cell_ox, cell_oy): int((new_origin - origin) / resolution), truncating toward zero"""
    return int((np.float64(new_ox) - cm.ox) / np.float64(cm.res)), int((np.float64(new_oy) - cm.oy) / np.float64(cm.res))


def update_origin(cm, new_ox, new_oy, loop=False):
    cx, cy = origin_step(cm, new_ox, new_oy)
    if cx == 0 and cy == 0:
        return
    sx, sy = cm.size_x, cm.size_y
    llx, lly = min(max(cx, 0), sx), min(max(cy, 0), sy)
    urx, ury = min(max(cx + sx, 0), sx), min(max(cy + sy, 0), sy)
    new = np.full_like(cm.grid, cm.default)
    if loop:                                                             # copyMapRegion out, resetMaps, copyMapRegion back
        for y in range(lly, ury):
            for x in range(llx, urx):
                new[y - cy, x - cx] = cm.grid[y, x]
    elif urx > llx and ury > lly:
        new[lly - cy:ury - cy, llx - cx:urx - cx] = cm.grid[lly:ury, llx:urx]
    cm.grid = new
    cm.ox, cm.oy = cm.ox + cx * cm.res, cm.oy + cy * cm.res


def roll_to(cm, robot_x, robot_y, loop=False):
    mx, my = cm.size_in_meters()
    update_origin(cm, float(robot_x) - mx / 2, float(robot_y) - my / 2, loop)


# ---- updateCosts ----------------------------------------------------------------------------------------------------------------
OVERWRITE, MAX = 0, 1


def merge(layer, master, window, mode, loop=False):
    """updateWithOverwrite (mode 0; = PointMapLayer::updateCosts) / updateWithMax (mode 1) inside [min_i, max_i) x [min_j, max_j)"""
    min_i, min_j, max_i, max_j = window
    if loop:
        for j in range(min_j, max_j):
            for i in range(min_i, max_i):
                v = layer.grid[j, i]
                if v == NO_INFORMATION:
                    continue
                if mode == OVERWRITE:
                    master.grid[j, i] = v
                else:
                    old = master.grid[j, i]
                    if old == NO_INFORMATION or old < v:
                        master.grid[j, i] = v
        return
    l, m = layer.grid[min_j:max_j, min_i:max_i], master.grid[min_j:max_j, min_i:max_i]
    take = l != NO_INFORMATION
    if mode == MAX:
        take &= (m == NO_INFORMATION) | (m < l)
    m[take] = l[take]
