"""The global-plan contract of include/gem_hip_navplan.h in numpy / plain Python: the weight table, the potential stated twice (a heapq
Dijkstra and an order-free sweep to the fixed point of pot = min(pot, min4(pot) + w)), and GridPath::getPath.  Restated from memory
from the navigation stack's global_planner (use_dijkstra, no quadratic calculator, use_grid_path), unverified against the library.
Grids are uint8 [size_y, size_x]; cells are (x, y); every number is an integer."""
import heapq

import numpy as np

OUTLINE = 1
UNREACHED = 0x7FFFFFFF
# the library's scan order: xd = -1, 0, 1 outer, yd = -1, 0, 1 inner, (0, 0) skipped
NEIGHBOURS = [(xd, yd) for xd in (-1, 0, 1) for yd in (-1, 0, 1) if (xd, yd) != (0, 0)]


def weights(neutral_cost=50, cost_factor=3.0, lethal_cost=253, allow_unknown=True):
    """Expander::getCost as a table by cost byte: int32 [256], 0 = impassable; None when a traversable cost is no whole number"""
    out = np.zeros(256, np.int32)
    f, n = np.float32(cost_factor), np.float32(neutral_cost)
    for c in range(256):
        if not (c < lethal_cost - 1 or (allow_unknown and c == 255)):
            continue
        v = np.float32(np.float32(c) * f) + n                            # float32, each operation rounded on its own
        if v >= np.float32(lethal_cost):
            out[c] = lethal_cost - 1
        else:
            if not v > 0 or float(v) != int(v):
                return None
            out[c] = int(v)
        if out[c] <= 0:
            return None
    return out


def cell_weights(grid, w, flags, start):
    """int64 [size_y, size_x]: the weight of every cell, 0 = impassable; the outline applied.  (The start is a source whatever its weight:
    the two potentials below never relax it.)"""
    cw = np.asarray(w, np.int64)[np.asarray(grid, np.uint8)]
    if flags & OUTLINE:
        cw[0, :] = 0; cw[-1, :] = 0; cw[:, 0] = 0; cw[:, -1] = 0
    return cw


def on_map(grid, cell):
    return cell is not None and 0 <= cell[0] < grid.shape[1] and 0 <= cell[1] < grid.shape[0]


def potential_dijkstra(grid, w, flags, start):
    sy, sx = grid.shape
    pot = np.full((sy, sx), UNREACHED, np.int64)
    if not on_map(grid, start):
        return pot.astype(np.int32)
    cw = cell_weights(grid, w, flags, start)
    pot[start[1], start[0]] = 0
    heap = [(0, start[0], start[1])]
    while heap:
        d, x, y = heapq.heappop(heap)
        if d != pot[y, x]:
            continue
        for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            u, v = x + dx, y + dy
            if not (0 <= u < sx and 0 <= v < sy) or (u, v) == tuple(start) or cw[v, u] <= 0:
                continue
            if d + cw[v, u] < pot[v, u]:
                pot[v, u] = d + cw[v, u]
                heapq.heappush(heap, (int(pot[v, u]), u, v))
    return pot.astype(np.int32)


def potential_sweeps(grid, w, flags, start):
    """the order-free form: every cell at once takes min(pot, min of its four neighbours + its weight), until nothing changes"""
    sy, sx = grid.shape
    big = np.int64(UNREACHED)
    pot = np.full((sy, sx), big, np.int64)
    if not on_map(grid, start):
        return pot.astype(np.int32)
    cw = cell_weights(grid, w, flags, start)
    passable = cw > 0
    passable[start[1], start[0]] = False                                 # the source stays 0
    pot[start[1], start[0]] = 0
    for _ in range(sx * sy + 1):                                         # (bounded by the cell count)
        m = np.full((sy, sx), big, np.int64)
        m[:, 1:] = np.minimum(m[:, 1:], pot[:, :-1])
        m[:, :-1] = np.minimum(m[:, :-1], pot[:, 1:])
        m[1:, :] = np.minimum(m[1:, :], pot[:-1, :])
        m[:-1, :] = np.minimum(m[:-1, :], pot[1:, :])
        cand = np.where(passable & (m < big), m + cw, big)
        new = np.minimum(pot, cand)
        if (new == pot).all():
            break
        pot = new
    return pot.astype(np.int32)


def get_path(pot, start, goal):
    """GridPath::getPath over a converged potential: the cells (x, y) from start to goal, both included; [] without a path"""
    sy, sx = pot.shape
    if not (on_map(pot, start) and on_map(pot, goal)) or pot[goal[1], goal[0]] == UNREACHED:
        return []
    c = (int(goal[0]), int(goal[1]))
    path = [c]
    steps = 0
    while c != (int(start[0]), int(start[1])) and steps < sx * sy:       # (bounded by the cell count)
        best, nxt = None, None
        for xd, yd in NEIGHBOURS:
            x, y = c[0] + xd, c[1] + yd
            if not (0 <= x < sx and 0 <= y < sy):
                continue
            if best is None or pot[y, x] < best:                         # strict <: the first smallest wins
                best, nxt = int(pot[y, x]), (x, y)
        assert nxt is not None and best < pot[c[1], c[0]], "the potential does not fall"
        c = nxt
        path.append(c)
        steps += 1
    return path[::-1]


def plan(grid, w, flags, start, goal):
    """what gem_navplan_host / gem_costmap_navplan answer: the potential, the path's linear cells, found, n_path, goal_potential"""
    grid = np.asarray(grid, np.uint8)
    sx = grid.shape[1]
    pot = potential_dijkstra(grid, w, flags, start)
    path = get_path(pot, start, goal)
    return {"pot": pot, "cells": np.array([y * sx + x for x, y in path], np.int32), "found": int(bool(path)), "n_path": len(path),
            "goal_potential": int(pot[goal[1], goal[0]]) if on_map(grid, goal) else UNREACHED,
            "start_cell": tuple(start) if on_map(grid, start) else (-1, -1), "goal_cell": tuple(goal) if on_map(grid, goal) else (-1, -1)}


def centres(cells, size_x, resolution, origin_x, origin_y):
    """the world points of a path's linear cells: cell centres, in double"""
    c = np.asarray(cells, np.int64)
    return np.stack([origin_x + ((c % size_x).astype(np.float64) + 0.5) * resolution,
                     origin_y + ((c // size_x).astype(np.float64) + 0.5) * resolution], axis=1).reshape(-1, 2)
