"""numpy restatement of the inflation contract of include/gem_hip_inflate.h: the cost table (math.sqrt / math.exp / math.ceil: the same
libm as the library), inflate_exact (the contract: the exact nearest seed, by brute force over the seeds), inflate_brushfire (ROS noetic's
InflationLayer::updateCosts restated literally, for the comparison the header quotes) and Costmap2D::resetMap over a window.  Grids are
uint8 [size_y, size_x]; a window is (min_i, min_j, max_i, max_j), half-open, None for the whole map.  Nothing here is verified against
costmap_2d itself."""
import heapq
import math
from collections import namedtuple

import numpy as np

FREE_SPACE, INSCRIBED, LETHAL, NO_INFORMATION = 0, 253, 254, 255
MAX_CELLS = 127
NONE = np.iinfo(np.int64).max                      # "no seed within R" in a d2 array

Params = namedtuple("Params", "inflation_radius inscribed_radius cost_scaling_factor inflate_unknown")


def cells(p, res):
    """cell_inflation_radius_ = cellDistance(inflation_radius_) = (unsigned)max(0.0, ceil(world_dist / resolution))"""
    return int(max(0.0, math.ceil(p.inflation_radius / res)))


def compute_cost(p, res, distance):
    """InflationLayer::computeCost(distance in cells)"""
    if distance == 0:
        return LETHAL
    if distance * res <= p.inscribed_radius:
        return INSCRIBED
    euclidean_distance = distance * res
    factor = math.exp(-1.0 * p.cost_scaling_factor * (euclidean_distance - p.inscribed_radius))
    return int((INSCRIBED - 1) * factor)           # (unsigned char) of a double in [0, 252]: truncation


def table(p, res):
    """(R, uint8 [R * R + 1]): the cost by squared cell distance"""
    R = cells(p, res)
    return R, np.array([compute_cost(p, res, math.sqrt(float(d2))) for d2 in range(R * R + 1)], np.uint8)


def widened(shape, window, R):
    """the window widened by R and clamped, or None for an empty window"""
    sy, sx = shape
    x0, y0, x1, y1 = (0, 0, sx, sy) if window is None else window
    if x0 == x1 or y0 == y1:
        return None
    return max(0, x0 - R), max(0, y0 - R), min(sx, x1 + R), min(sy, y1 + R)


def seeds(grid, window, R):
    """[(x, y)] of the 254 cells inside the widened window, in the library's scan order (rows, then columns)"""
    w = widened(grid.shape, window, R)
    if w is None:
        return []
    ys, xs = np.nonzero(grid[w[1]:w[3], w[0]:w[2]] == LETHAL)
    return [(int(x) + w[0], int(y) + w[1]) for x, y in zip(xs, ys)]


def nearest_d2(shape, seed_list, R):
    """int64 [size_y, size_x]: min over the seeds of dx^2 + dy^2 where that is <= R^2, NONE elsewhere"""
    sy, sx = shape
    d2 = np.full(shape, NONE, np.int64)
    for x, y in seed_list:
        xa, xb, ya, yb = max(0, x - R), min(sx, x + R + 1), max(0, y - R), min(sy, y + R + 1)
        dx, dy = np.arange(xa, xb, dtype=np.int64) - x, np.arange(ya, yb, dtype=np.int64) - y
        part = d2[ya:yb, xa:xb]
        np.minimum(part, dy[:, None] ** 2 + dx[None, :] ** 2, out=part)
    d2[d2 > R * R] = NONE
    return d2


def apply_costs(grid, d2, tab, inflate_unknown):
    """the rule of updateCosts at every cell that has a seed within R"""
    hit = d2 != NONE
    cost = tab[np.where(hit, d2, 0)]
    take = (grid == NO_INFORMATION) & ((cost > FREE_SPACE) if inflate_unknown else (cost >= INSCRIBED))
    return np.where(hit, np.where(take, cost, np.maximum(grid, cost)), grid).astype(np.uint8)


def inflate_exact(grid, p, res, window=None, with_d2=False):
    """the contract: a new grid (and the squared distances)"""
    R, tab = table(p, res)
    if R == 0:
        d2 = np.full(grid.shape, NONE, np.int64)
        return (grid.copy(), d2) if with_d2 else grid.copy()
    d2 = nearest_d2(grid.shape, seeds(grid, window, R), R)
    out = apply_costs(grid, d2, tab, p.inflate_unknown)
    return (out, d2) if with_d2 else out


def inflate_brushfire(grid, p, res, window=None, with_d2=False):
    """InflationLayer::updateCosts of ROS noetic, literally: inflation_cells_ is a std::map<double, std::vector<CellData>> iterated
    FORWARD only.  enqueue() files a neighbour under its distance to the SOURCE of the cell it was reached from; an entry filed under a
    distance already passed is never visited, one filed under the current distance is (the vector grows while it is walked); seen_
    keeps the first visit.  The neighbours are tried in the order -x, -y, +x, +y."""
    R, tab = table(p, res)
    sy, sx = grid.shape
    out = grid.copy()
    d2_of = np.full(grid.shape, NONE, np.int64)
    if R == 0:
        return (out, d2_of) if with_d2 else out
    seen = np.zeros(grid.shape, bool)
    bins = {0.0: [(x, y, x, y) for x, y in seeds(grid, window, R)]}
    later = []                                      # the keys of `bins` as a heap: std::map's order
    cur = 0.0

    def enqueue(mx, my, srcx, srcy):
        if seen[my, mx]:
            return
        distance = math.hypot(mx - srcx, my - srcy)  # distanceLookup: cached_distances_[|dx|][|dy|] = hypot(dx, dy)
        if distance > R:
            return
        if distance not in bins:
            bins[distance] = []
            heapq.heappush(later, distance)
        bins[distance].append((mx, my, srcx, srcy))

    while True:
        cells_of_bin = bins[cur]
        i = 0
        while i < len(cells_of_bin):
            mx, my, srcx, srcy = cells_of_bin[i]
            i += 1
            if seen[my, mx]:
                continue
            seen[my, mx] = True
            d2 = (mx - srcx) ** 2 + (my - srcy) ** 2
            d2_of[my, mx] = d2
            cost = compute_cost(p, res, math.hypot(mx - srcx, my - srcy))     # costLookup: cached_costs_[|dx|][|dy|]
            old = int(out[my, mx])
            if old == NO_INFORMATION and ((cost > FREE_SPACE) if p.inflate_unknown else (cost >= INSCRIBED)):
                out[my, mx] = cost
            else:
                out[my, mx] = max(old, cost)
            if mx > 0:
                enqueue(mx - 1, my, srcx, srcy)
            if my > 0:
                enqueue(mx, my - 1, srcx, srcy)
            if mx < sx - 1:
                enqueue(mx + 1, my, srcx, srcy)
            if my < sy - 1:
                enqueue(mx, my + 1, srcx, srcy)
        while later and later[0] <= cur:            # keys filed behind the iterator: lost
            heapq.heappop(later)
        if not later:
            break
        cur = heapq.heappop(later)
    return (out, d2_of) if with_d2 else out


def reset_window(grid, x0, y0, xn, yn, default_value=NO_INFORMATION):
    """Costmap2D::resetMap(x0, y0, xn, yn), in place"""
    grid[y0:yn, x0:xn] = default_value


def hypot_is_sqrt(limit=128):
    """what indexing the table by d2 rests on: hypot(i, j) == sqrt(i * i + j * j) for all 0 <= i, j <= limit"""
    return all(math.hypot(i, j) == math.sqrt(float(i * i + j * j)) for i in range(limit + 1) for j in range(limit + 1))
