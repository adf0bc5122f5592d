"""The quadratic-potential contract of include/gem_hip_navquad.h in numpy / plain Python: the increment as a scalar function, the
potential stated twice (whole-grid Jacobi sweeps; Gauss-Seidel passes in a seeded random cell order) and the plan, whose path is
navplan_ref.get_path on that potential.  The project's own contract, in exact integers.  Grids are uint8 [size_y, size_x]; cells are
(x, y)."""
import functools

import numpy as np

import navplan_ref as lin

OUTLINE = lin.OUTLINE
UNREACHED = lin.UNREACHED
MAX_WEIGHT = 462


def inc(hf, dc):
    """the increment of a cell of weight hf whose two axis minima differ by dc (dc already cut at hf or not: both give hf there)"""
    hf, dc = int(hf), int(dc)
    if dc >= hf:
        return hf
    return max(1, min(hf, (-2301 * dc * dc + 5307 * dc * hf + 7040 * hf * hf) // (10000 * hf)))


def update(hf, left, right, up, down):
    """T(n) of a traversable non-source cell from its four neighbours' potentials (UNREACHED: off the map, impassable or unreached)"""
    h, v = min(left, right), min(up, down)
    ta, tc = min(h, v), max(h, v)
    if ta == UNREACHED:
        return UNREACHED
    dc = hf if tc == UNREACHED else min(tc - ta, hf)
    return ta + inc(hf, dc)


@functools.lru_cache(maxsize=None)
def _inc_table(top):
    """inc as an array [hf, dc] for hf, dc in 0 .. top, filled by the scalar function"""
    t = np.zeros((top + 1, top + 1), np.int64)
    for hf in range(1, top + 1):
        for dc in range(top + 1):
            t[hf, dc] = inc(hf, dc)
    return t


def potential_jacobi(grid, w, flags, start):
    """every cell at once takes min(pot, T) from the grid as it was, until nothing changes"""
    sy, sx = grid.shape
    big = np.int64(UNREACHED)
    pot = np.full((sy, sx), big, np.int64)
    if not lin.on_map(grid, start):
        return pot.astype(np.int32)
    cw = lin.cell_weights(grid, w, flags, start)
    assert cw.max() <= MAX_WEIGHT
    passable = cw > 0
    passable[start[1], start[0]] = False                                 # the source stays 0
    pot[start[1], start[0]] = 0
    table = _inc_table(int(cw.max()) if cw.max() > 0 else 1)
    for _ in range(4 * sx * sy + 4):                                     # (bounded; a sweep that changes nothing ends it)
        p = np.full((sy + 2, sx + 2), big, np.int64)
        p[1:-1, 1:-1] = pot
        h = np.minimum(p[1:-1, :-2], p[1:-1, 2:])
        v = np.minimum(p[:-2, 1:-1], p[2:, 1:-1])
        ta, tc = np.minimum(h, v), np.maximum(h, v)
        dc = np.where(tc == big, cw, np.minimum(tc - ta, cw))
        t = np.where(passable & (ta < big), ta + table[cw, np.clip(dc, 0, table.shape[1] - 1)], big)
        new = np.minimum(pot, t)
        if (new == pot).all():
            break
        pot = new
    else:
        raise AssertionError("the Jacobi sweeps did not converge")
    return pot.astype(np.int32)


def potential_gauss_seidel(grid, w, flags, start, seed):
    """passes over the cells in ONE seeded random order, each cell updated in place from the grid as it is, until a pass changes nothing"""
    sy, sx = grid.shape
    pot = [[UNREACHED] * sx for _ in range(sy)]
    if not lin.on_map(grid, start):
        return np.array(pot, np.int64).astype(np.int32).reshape(sy, sx)
    cw = lin.cell_weights(grid, w, flags, start).tolist()
    pot[start[1]][start[0]] = 0
    order = [(int(c) % sx, int(c) // sx) for c in np.random.default_rng(seed).permutation(sx * sy)]
    order = [(x, y) for x, y in order if cw[y][x] > 0 and (x, y) != (int(start[0]), int(start[1]))]
    for _ in range(4 * sx * sy + 4):                                     # (bounded; a pass that changes nothing ends it)
        changed = False
        for x, y in order:
            t = update(cw[y][x], pot[y][x - 1] if x > 0 else UNREACHED, pot[y][x + 1] if x + 1 < sx else UNREACHED,
                       pot[y - 1][x] if y > 0 else UNREACHED, pot[y + 1][x] if y + 1 < sy else UNREACHED)
            if t < pot[y][x]:
                pot[y][x] = t
                changed = True
        if not changed:
            break
    else:
        raise AssertionError("the Gauss-Seidel passes did not converge")
    return np.array(pot, np.int64).astype(np.int32).reshape(sy, sx)


def plan(grid, w, flags, start, goal):
    """what gem_navquad_host / gem_costmap_navplan_quadratic answer, in the shape of navplan_ref.plan"""
    grid = np.asarray(grid, np.uint8)
    sx = grid.shape[1]
    pot = potential_jacobi(grid, w, flags, start)
    path = lin.get_path(pot, start, goal)
    return {"pot": pot, "cells": np.array([y * sx + x for x, y in path], np.int32), "found": int(bool(path)), "n_path": len(path),
            "goal_potential": int(pot[goal[1], goal[0]]) if lin.on_map(grid, goal) else UNREACHED,
            "start_cell": tuple(start) if lin.on_map(grid, start) else (-1, -1), "goal_cell": tuple(goal) if lin.on_map(grid, goal) else (-1, -1)}
