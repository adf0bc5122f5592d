"""numpy / plain Python restatement of the MapGrid contract of include/gem_hip_mapgrid.h, on top of costmap_ref.Costmap / world_to_map:
base_local_planner's map_grid.cpp (adjustPlanResolution, setTargetCells, setLocalGoal, computeTargetDistance, updatePathCell) and
map_grid_cost_function.cpp (scoreTrajectory).  base_local_planner is not available to these tests: this is a restatement, unverified
against the library.

computeTargetDistance has two forms: the literal FIFO queue in the library's order (`distance_queue`, the definition) and the set form
by levels in numpy (`distance_levels`); tests/test_mapgrid_cpu.py pins the two to identical results.  A grid is uint8 [size_y, size_x];
distances are int32 [size_y, size_x]."""
import math
from collections import deque

import numpy as np

import costmap_ref as cr

PATH, GOAL = 1, 2
STOP_ON_FAILURE, SUM = 1, 2
MAX_POINTS, MAX_WORDS = 1 << 20, 4096


def constants(grid):
    ob = int(grid.shape[0]) * int(grid.shape[1])
    return ob, ob + 1                                                    # obstacleCosts(), unreachableCellCosts()


def blocked(grid):
    return grid >= 253                                                   # INSCRIBED_INFLATED_OBSTACLE, LETHAL_OBSTACLE, NO_INFORMATION


# ---- adjustPlanResolution -----------------------------------------------------------------------------------------------------------
def adjust_plan(plan, resolution):
    """[n, 2] -> [m, 2], python floats = C doubles, every operation rounded on its own"""
    plan = [(float(x), float(y)) for x, y in np.asarray(plan, np.float64).reshape(-1, 2)]
    if not plan:
        return np.zeros((0, 2), np.float64)
    resolution = float(resolution)
    out = [plan[0]]
    last_x, last_y = plan[0]
    min_sq = resolution * resolution
    for x, y in plan[1:]:
        sq = (x - last_x) * (x - last_x) + (y - last_y) * (y - last_y)
        if sq > min_sq:
            steps = int(math.ceil(math.sqrt(sq) / resolution))
            dx, dy = (x - last_x) / steps, (y - last_y) / steps
            for j in range(1, steps):
                out.append((last_x + j * dx, last_y + j * dy))
        out.append((x, y))
        last_x, last_y = x, y
    return np.array(out, np.float64).reshape(-1, 2)


# ---- the run ------------------------------------------------------------------------------------------------------------------------
def plan_cells(cm, adjusted):
    """per point (mx, my) or None"""
    return [cr.world_to_map(cm, x, y) for x, y in adjusted]


def run(grid, cells):
    """(a, b) with a the first accepted index and b the first index above it that is not accepted; None without an accepted point"""
    acc = [c is not None and grid[c[1], c[0]] != 255 for c in cells]
    if True not in acc:
        return None
    a = acc.index(True)
    b = a + 1
    while b < len(acc) and acc[b]:
        b += 1
    return a, b


# ---- computeTargetDistance ----------------------------------------------------------------------------------------------------------
def distance_queue(grid, sources):
    """the literal queue: sources = [(x, y), ...] in order, duplicates allowed"""
    sy, sx = grid.shape
    ob, un = constants(grid)
    blk = blocked(grid)
    dist = np.full((sy, sx), un, np.int32)
    marked = np.zeros((sy, sx), bool)
    q = deque()
    for x, y in sources:                                                 # setTargetCells / setLocalGoal: target_dist = 0, target_mark, push
        dist[y, x] = 0
        marked[y, x] = True
        q.append((x, y))
    while q:
        cx, cy = q.popleft()
        for ok, nx, ny in ((cx > 0, cx - 1, cy), (cx < sx - 1, cx + 1, cy), (cy > 0, cx, cy - 1), (cy < sy - 1, cx, cy + 1)):
            if not ok or marked[ny, nx]:
                continue
            marked[ny, nx] = True                                        # marked on first touch
            if blk[ny, nx]:                                              # updatePathCell: obstacleCosts(), not pushed
                dist[ny, nx] = ob
                continue
            dist[ny, nx] = dist[cy, cx] + 1
            q.append((nx, ny))
    return dist


def _dilate4(m):
    d = np.zeros_like(m)
    d[:, 1:] |= m[:, :-1]
    d[:, :-1] |= m[:, 1:]
    d[1:, :] |= m[:-1, :]
    d[:-1, :] |= m[1:, :]
    return d


def distance_levels(grid, sources):
    """the set form, level by level"""
    ob, un = constants(grid)
    open_ = ~blocked(grid)
    src = np.zeros(grid.shape, bool)
    for x, y in sources:
        src[y, x] = True
    dist = np.full(grid.shape, un, np.int32)
    dist[src] = 0
    reached = src.copy()                                                 # E: the sources and the reached non-blocked cells
    frontier = src
    d = 0
    while frontier.any():
        d += 1
        frontier = _dilate4(frontier) & open_ & ~reached
        dist[frontier] = d
        reached |= frontier
    dist[_dilate4(reached) & ~open_ & ~src] = ob
    return dist


def grids(cm, plan, distance=distance_levels):
    """gem_costmap_mapgrid_prepare(PATH | GOAL) + read: {'path': dist, 'goal': dist, 'started': 0 / 1, 'goal_cell': (x, y)}"""
    cells = plan_cells(cm, adjust_plan(plan, cm.res))
    r = run(cm.grid, cells)
    un = constants(cm.grid)[1]
    if r is None:
        empty = np.full(cm.grid.shape, un, np.int32)
        return {"path": empty, "goal": empty.copy(), "started": 0, "goal_cell": (-1, -1)}
    a, b = r
    return {"path": distance(cm.grid, cells[a:b]), "goal": distance(cm.grid, [cells[b - 1]]), "started": 1, "goal_cell": tuple(cells[b - 1])}


# ---- scoreTrajectory ----------------------------------------------------------------------------------------------------------------
def score(cm, dist, poses, poses_per_traj, xshift=0.0, flags=0):
    """poses [n, 4] (x, y, cos, sin) -> int64 [n / T], the sequential loop"""
    ob, un = constants(cm.grid)
    p = np.asarray(poses, np.float64).reshape(-1, 4)
    T = int(poses_per_traj)
    xshift = float(xshift)
    out = np.zeros(p.shape[0] // T, np.int64)
    for t in range(out.shape[0]):
        cost = 0
        for x, y, c, s in p[t * T:(t + 1) * T].tolist():
            if xshift != 0.0:
                with np.errstate(all="ignore"):
                    px, py = float(np.float64(x) + np.float64(xshift) * np.float64(c)), float(np.float64(y) + np.float64(xshift) * np.float64(s))
            else:
                px, py = x, y
            m = cr.world_to_map(cm, px, py)
            if m is None:
                cost = -4
                break
            d = int(dist[m[1], m[0]])
            if flags & STOP_ON_FAILURE and d == ob:
                cost = -3
                break
            if flags & STOP_ON_FAILURE and d == un:
                cost = -2
                break
            cost = cost + d if flags & SUM else d
        out[t] = cost
    return out
