"""numpy restatement of the footprint contract of include/gem_hip_footprint.h, on top of costmap_ref.Costmap / world_to_map: the pieces
of ROS noetic costmap_2d (footprint.cpp transformFootprint, line_iterator.h, costmap_2d.cpp polygonOutlineCells / convexFillCells /
setConvexPolygonCost, obstacle_layer.cpp updateFootprint) and base_local_planner (costmap_model.cpp footprintCost,
obstacle_cost_function.cpp scoreTrajectory) that gem_costmap_clear_footprint, gem_costmap_footprint_cost and
gem_costmap_score_trajectories stand for.  None of those libraries is available to these tests: this is a restatement, unverified
against them.

Every operation has a sequential form (`*_loop` or the literal iterator: the definition) and a vectorised one;
tests/test_footprint_cpu.py pins the two to identical results.  All arithmetic is numpy float64 = C double, every operation rounded on
its own; poses are (x, y, cos, sin)."""
import math

import numpy as np

import costmap_ref as cref

MAX_VERTICES = 32
INSCRIBED_LETHAL, SUM = 1, 2
# layers/params/costmap_common_params_local.yaml:8
RECTANGLE = [[-0.64, -0.40], [-0.64, 0.40], [0.64, 0.40], [0.64, -0.40]]


def poses_from_yaw(xyt):
    """[n, 3] (x, y, theta) -> [n, 4] (x, y, cos, sin), math.cos / math.sin element by element (the host's libm)"""
    p = np.asarray(xyt, np.float64).reshape(-1, 3)
    out = np.empty((p.shape[0], 4), np.float64)
    out[:, :2] = p[:, :2]
    out[:, 2] = [math.cos(float(t)) for t in p[:, 2]]
    out[:, 3] = [math.sin(float(t)) for t in p[:, 2]]
    return out


def regular_polygon(n, radius):
    return [[radius * math.cos(2 * math.pi * k / n), radius * math.sin(2 * math.pi * k / n)] for k in range(n)]


# ---- transformFootprint -----------------------------------------------------------------------------------------------------------
def transform(pose, spec):
    """one pose: [(wx, wy)] per vertex; x + (sx * cos - sy * sin), y + (sx * sin + sy * cos)"""
    x, y, c, s = (np.float64(v) for v in pose)
    with np.errstate(all="ignore"):
        return [(float(x + (np.float64(sx) * c - np.float64(sy) * s)), float(y + (np.float64(sx) * s + np.float64(sy) * c))) for sx, sy in spec]


def transform_v(poses, spec):
    """[n, 4] poses, [m, 2] spec -> wx [n, m], wy [n, m]"""
    p, v = np.asarray(poses, np.float64).reshape(-1, 4), np.asarray(spec, np.float64).reshape(-1, 2)
    x, y, c, s = (p[:, k:k + 1] for k in range(4))
    sx, sy = v[:, 0][None, :], v[:, 1][None, :]
    with np.errstate(all="ignore"):
        return x + (sx * c - sy * s), y + (sx * s + sy * c)


# ---- LineIterator -----------------------------------------------------------------------------------------------------------------
def line_iter(x0, y0, x1, y1):
    """line_iterator.h literally: the constructor's increments, then isValid / advance"""
    deltax, deltay = abs(x1 - x0), abs(y1 - y0)
    xinc1 = xinc2 = 1 if x1 >= x0 else -1
    yinc1 = yinc2 = 1 if y1 >= y0 else -1
    if deltax >= deltay:
        xinc1, yinc2 = 0, 0
        den, num, numadd, numpixels = deltax, deltax // 2, deltay, deltax
    else:
        xinc2, yinc1 = 0, 0
        den, num, numadd, numpixels = deltay, deltay // 2, deltax, deltay
    x, y, cur, out = x0, y0, 0, []
    while cur <= numpixels:
        out.append((x, y))
        num += numadd
        if num >= den:
            num -= den
            x += xinc1
            y += yinc1
        x += xinc2
        y += yinc2
        cur += 1
    return out


def line_closed(x0, y0, x1, y1):
    """the closed form of the contract: cell k on its own"""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    xi, yi = (1 if x1 >= x0 else -1), (1 if y1 >= y0 else -1)
    if dx >= dy:
        return [(x0 + xi * k, y0 + yi * ((dx // 2 + k * dy) // dx if dx else 0)) for k in range(dx + 1)]
    return [(x0 + xi * ((dy // 2 + k * dx) // dy), y0 + yi * k) for k in range(dy + 1)]


def line_closed_v(x0, y0, x1, y1):
    """arrays [n] of end cells -> (cx [n, K], cy [n, K], valid [n, K]), K = the longest line's cells; int64"""
    x0, y0, x1, y1 = (np.asarray(v, np.int64) for v in (x0, y0, x1, y1))
    dx, dy = np.abs(x1 - x0), np.abs(y1 - y0)
    xi, yi = np.where(x1 >= x0, 1, -1), np.where(y1 >= y0, 1, -1)
    major, minor = np.maximum(dx, dy), np.minimum(dx, dy)
    K = int(major.max()) + 1 if major.size else 1
    k = np.arange(K, dtype=np.int64)[None, :]
    valid = k <= major[:, None]
    m = (major[:, None] // 2 + k * minor[:, None]) // np.maximum(major[:, None], 1)
    xm = (dx >= dy)[:, None]
    cx = x0[:, None] + xi[:, None] * np.where(xm, k, m)
    cy = y0[:, None] + yi[:, None] * np.where(xm, m, k)
    return cx, cy, valid


# ---- pointCost / footprintCost ----------------------------------------------------------------------------------------------------
def point_cost(c, flags=0):
    c = int(c)
    if c == 255:
        return -2
    if c == 254:
        return -1
    if c == 253 and flags & INSCRIBED_LETHAL:
        return -1
    return c


def centre_cost(c):
    c = int(c)
    return -2 if c == 255 else (-1 if c >= 253 else c)


def footprint_cost_loop(cm, pose, spec, flags=0):
    """CostmapModel::footprintCost, sequentially: the first negative event in walk order is the answer"""
    centre = cref.world_to_map(cm, pose[0], pose[1])
    if centre is None:
        return -3
    n = len(spec)
    if n < 3:
        return centre_cost(cm.grid[centre[1], centre[0]])
    world = transform(pose, spec)
    best = 0
    for i in range(n):
        j = (i + 1) % n
        a, b = cref.world_to_map(cm, *world[i]), cref.world_to_map(cm, *world[j])
        if a is None or b is None:
            return -3
        for x, y in line_iter(a[0], a[1], b[0], b[1]):
            pc = point_cost(cm.grid[y, x], flags)
            if pc < 0:
                return pc
            best = max(best, pc)
    return best


def vertex_cells_v(cm, poses, spec):
    """ok [n, m], mx [n, m], my [n, m] (0 where not ok)"""
    wx, wy = transform_v(poses, spec)
    ok, idx = cref.world_to_map_v(cm, wx, wy)
    idx = np.where(ok, idx, 0)
    return ok, idx % cm.size_x, idx // cm.size_x


def footprint_cost(cm, poses, spec, flags=0):
    """... vectorised over the poses, edge by edge: int32 [n]"""
    p = np.asarray(poses, np.float64).reshape(-1, 4)
    n, m = p.shape[0], len(spec)
    res = np.zeros(n, np.int32)
    ok_c, idx_c = cref.world_to_map_v(cm, p[:, 0], p[:, 1])
    res[~ok_c] = -3
    if m < 3:
        c = cm.grid.reshape(-1)[np.where(ok_c, idx_c, 0)].astype(np.int32)
        res[ok_c] = np.where(c == 255, -2, np.where(c >= 253, -1, c))[ok_c]
        return res
    decided = ~ok_c
    best = np.zeros(n, np.int32)
    okv, mx, my = vertex_cells_v(cm, p, spec)
    for i in range(m):
        j = (i + 1) % m
        fail = ~(okv[:, i] & okv[:, j]) & ~decided
        res[fail] = -3
        decided |= fail
        sub = np.flatnonzero(~decided)
        if sub.size == 0:
            break
        cx, cy, valid = line_closed_v(mx[sub, i], my[sub, i], mx[sub, j], my[sub, j])
        c = cm.grid[np.where(valid, cy, 0), np.where(valid, cx, 0)].astype(np.int32)
        pc = np.where(c == 255, -2, np.where((c == 254) | ((c == 253) & bool(flags & INSCRIBED_LETHAL)), -1, c))
        neg = valid & (pc < 0)
        hit = neg.any(axis=1)
        first = neg.argmax(axis=1)
        res[sub[hit]] = pc[hit, first[hit]]
        decided[sub[hit]] = True
        best[sub] = np.maximum(best[sub], np.where(valid & ~neg, pc, 0).max(axis=1))
    res[~decided] = best[~decided]
    return res


# ---- trajectories -----------------------------------------------------------------------------------------------------------------
def score_trajectories_loop(pose_costs, T, flags=0):
    """ObstacleCostFunction::scoreTrajectory's loop shape over trajectories of T consecutive pose costs"""
    r = np.asarray(pose_costs, np.int64).reshape(-1, T)
    out = np.zeros(r.shape[0], np.int32)
    for t in range(r.shape[0]):
        cost = 0
        for f in r[t]:
            if f < 0:
                cost = f
                break
            cost = cost + f if flags & SUM else max(cost, f)
        out[t] = cost
    return out


def score_trajectories(pose_costs, T, flags=0):
    r = np.asarray(pose_costs, np.int64).reshape(-1, T)
    neg = r < 0
    hit = neg.any(axis=1)
    first = neg.argmax(axis=1)
    good = np.where(neg, 0, r)
    out = good.sum(axis=1) if flags & SUM else good.max(axis=1)
    return np.where(hit, r[np.arange(r.shape[0]), first], out).astype(np.int32)


# ---- polygonOutlineCells / convexFillCells / setConvexPolygonCost -------------------------------------------------------------------
def outline(cells):
    """polygonOutlineCells: the lines between consecutive vertex cells and the closing one, in order, duplicates kept"""
    out = []
    n = len(cells)
    for i in range(n):
        a, b = cells[i], cells[(i + 1) % n]
        out += line_iter(a[0], a[1], b[0], b[1])
    return out


def fill_loop(cells):
    """convexFillCells literally: the outline sorted by x (its bubble sort is stable), then the pairwise walk column by column.  Returns
    the list setConvexPolygonCost writes: the outline followed by the columns' cells."""
    if len(cells) < 3:
        return []
    poly = sorted(outline(cells), key=lambda c: c[0])
    out = list(poly)
    i, size = 0, len(poly)
    min_x, max_x = poly[0][0], poly[-1][0]
    for x in range(min_x, max_x + 1):
        if i >= size - 1:
            break
        if poly[i][1] < poly[i + 1][1]:
            min_pt, max_pt = poly[i], poly[i + 1]
        else:
            min_pt, max_pt = poly[i + 1], poly[i]
        i += 2
        while i < size and poly[i][0] == x:
            if poly[i][1] < min_pt[1]:
                min_pt = poly[i]
            elif poly[i][1] > max_pt[1]:
                max_pt = poly[i]
            i += 1
        for y in range(min_pt[1], max_pt[1] + 1):
            out.append((x, y))
    return out


def fill_set(cells):
    """the same as a set, vectorised: (xs, ys) of every cell between the lowest and the highest outline cell of each outline column"""
    if len(cells) < 3:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    c = np.asarray(cells, np.int64)
    cx, cy, valid = line_closed_v(c[:, 0], c[:, 1], np.roll(c[:, 0], -1), np.roll(c[:, 1], -1))
    ox, oy = cx[valid], cy[valid]
    x0 = int(ox.min())
    span = int(ox.max()) - x0 + 1
    lo, hi = np.full(span, np.iinfo(np.int64).max), np.full(span, -1, np.int64)
    np.minimum.at(lo, ox - x0, oy)
    np.maximum.at(hi, ox - x0, oy)
    cols = np.flatnonzero(hi >= 0)
    counts = hi[cols] - lo[cols] + 1
    xs = np.repeat(cols + x0, counts)
    ys = np.concatenate([np.arange(lo[k], hi[k] + 1) for k in cols]) if cols.size else np.zeros(0, np.int64)
    return xs, ys


def clear_footprint(cm, pose, spec, bounds=None, loop=False):
    """updateFootprint (transform, touch every vertex in order) + setConvexPolygonCost(FREE_SPACE).  Returns ok."""
    world = transform(pose, spec)
    if bounds is not None:
        for wx, wy in world:
            cref._touch(bounds, wx, wy)
    if len(spec) < 3:
        return True
    cells = [cref.world_to_map(cm, wx, wy) for wx, wy in world]
    if any(c is None for c in cells):
        return False
    if loop:
        for x, y in fill_loop(cells):
            cm.grid[y, x] = cref.FREE_SPACE
    else:
        xs, ys = fill_set(cells)
        cm.grid[ys, xs] = cref.FREE_SPACE
    return True


# ---- known answers (tests/test_footprint_cpu.py on the restatement, tests/test_footprint_gpu.py on the device) ------------------------
def _edge_cells(cm, pose, spec, e):
    world = transform(pose, spec)
    a, b = cref.world_to_map(cm, *world[e]), cref.world_to_map(cm, *world[(e + 1) % len(spec)])
    return line_closed(a[0], a[1], b[0], b[1])


def known_answers():
    """[(name, Costmap, poses [k, 4], spec, flags, [answers])]: small hand-built cases whose answers follow from the contract's text"""
    out = []
    ox, oy = -3.1, 2.7

    def fresh(value=0):
        cm = cref.Costmap(75, 75, 0.2, ox, oy)
        cm.grid[:] = value
        return cm

    mid = (ox + 7.5, oy + 7.5, 1.0, 0.0)                                   # heading 0: edge 0 left, 1 top, 2 right, 3 bottom

    def on_edge(cm, pose, e, value):
        cells = _edge_cells(cm, pose, RECTANGLE, e)
        x, y = cells[len(cells) // 2]                                     # an inner cell of a side: on no other edge
        cm.grid[y, x] = value

    # the first negative event in walk order decides
    for first, second, want in ((255, 254, -2), (254, 255, -1)):
        cm = fresh()
        on_edge(cm, mid, 0, first); on_edge(cm, mid, 1, second)
        out.append((f"{first} on edge 0, {second} on edge 1", cm, [mid], RECTANGLE, 0, [want]))
    # vertex 2 off the map (heading 45 degrees near the top side: it is the topmost vertex), so edge 1 answers -3 -- unless edge 0 answers first
    r = math.sqrt(0.5)
    top = (ox + 7.5, oy + 75 * 0.2 - 0.5, r, r)
    for e, want in ((0, -1), (None, -3)):
        cm = fresh()
        okv, mx, my = vertex_cells_v(cm, [top], RECTANGLE)
        assert okv[0].tolist() == [True, True, False, True]
        if e == 0:
            on_edge(cm, top, 0, 254)
        else:                                                             # where edge 2 would end (vertex 3's cell): behind the failure
            assert (int(mx[0, 3]), int(my[0, 3])) not in _edge_cells(cm, top, RECTANGLE, 0)
            cm.grid[my[0, 3], mx[0, 3]] = 254
        out.append((f"vertex 2 off the map, 254 on edge {e}", cm, [top], RECTANGLE, 0, [want]))
    # the inscribed cost on an edge, without and with the flag; a plain cost is the answer
    cm = fresh()
    on_edge(cm, mid, 2, 253); on_edge(cm, mid, 3, 100)
    out.append(("253 on an edge", cm, [mid], RECTANGLE, 0, [253]))
    out.append(("253 on an edge, inscribed is lethal", cm, [mid], RECTANGLE, INSCRIBED_LETHAL, [-1]))
    # fewer than three vertices: the centre cell alone, 253 lethal whatever the flag
    for n in (0, 1, 2):
        for value, want in ((0, 0), (100, 100), (253, -1), (254, -1), (255, -2)):
            for flags in (0, INSCRIBED_LETHAL):
                out.append((f"{n} vertices on a centre cell {value}, flags {flags}", fresh(value), [mid], RECTANGLE[:n], flags, [want]))
    # the centre off the map, every vertex on it
    ahead = [[1.0, 0.0], [1.5, 0.0], [1.25, 0.5]]
    out.append(("centre off the map", fresh(), [(ox - 0.5, oy + 3.0, 1.0, 0.0)], ahead, 0, [-3]))
    out.append(("the same spec with the centre on it", fresh(7), [(ox + 0.5, oy + 3.0, 1.0, 0.0)], ahead, 0, [7]))
    # every vertex in one cell; with n >= 3 the centre cell is not read
    cm = fresh()
    cx, cy = cref.world_to_map(cm, mid[0], mid[1])
    cm.grid[cy, cx] = 77
    tiny = [[0.001, 0.001], [0.002, 0.001], [0.001, 0.002]]
    out.append(("every vertex in the centre's cell", cm, [mid], tiny, 0, [77]))
    cm = fresh()
    cm.grid[cy, cx] = 254
    out.append(("the centre cell is not read", cm, [mid], RECTANGLE, 0, [0]))
    # the map's edges, in exact binary fractions: wx == origin_x is cell 0, a cell index of size_x is off the map
    tri = [[-0.5, -0.5], [0.5, -0.5], [0.0, 0.5]]
    cm = cref.Costmap(10, 10, 0.5, -2.0, 1.0)
    cm.grid[:] = 9
    poses = [(-1.5, 3.0, 1.0, 0.0), (2.25, 3.0, 1.0, 0.0), (2.5, 3.0, 1.0, 0.0), (0.0, 1.5, 1.0, 0.0), (0.0, 5.5, 1.0, 0.0),
             (float("nan"), 3.0, 1.0, 0.0), (0.0, 3.0, float("inf"), 0.0)]
    out.append(("on and beyond the map's edges", cm, poses, tri, 0, [9, 9, -3, 9, -3, -3, -3]))
    return out
