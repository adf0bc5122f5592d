"""The frontier-search contract of include/gem_hip_frontier.h in numpy / plain Python: the classification of the frontier cells, their
8-connected components stated twice (a flood fill, and order-free sweeps of label = min(label, min8(label)) restricted to the frontier
cells, run to the fixed point), the records, the cost, the pick and the centroid.  In the manner of explore_lite's FrontierSearch,
recalled from memory and unverified against the library; the four deliberate departures are named in the header.
Grids are uint8 [size_y, size_x], potentials int32 of the same shape (navplan_ref), cells are linear (y * size_x + x); every number but
the cost is an integer."""
import numpy as np

UNREACHED = 0x7FFFFFFF
NO_INFORMATION = 255
N4 = ((-1, 0), (1, 0), (0, -1), (0, 1))
N8 = tuple((xd, yd) for yd in (-1, 0, 1) for xd in (-1, 0, 1) if (xd, yd) != (0, 0))


def shifted(a, xd, yd, fill):
    """b[y, x] = a[y + yd, x + xd], `fill` off the map"""
    sy, sx = a.shape
    b = np.full_like(a, fill)
    ys, yt = (slice(yd, sy), slice(0, sy - yd)) if yd >= 0 else (slice(0, sy + yd), slice(-yd, sy))
    xs, xt = (slice(xd, sx), slice(0, sx - xd)) if xd >= 0 else (slice(0, sx + xd), slice(-xd, sx))
    b[yt, xt] = a[ys, xs]
    return b


def classify(grid, pot):
    """(mask bool: the frontier cells, key int64: their access keys (potential << 32) | cell, -1 elsewhere).  A door is a 4-neighbour
    on the map that is known (byte != 255) and reached (pot != UNREACHED); a frontier cell is an unknown cell with a door."""
    grid = np.asarray(grid, np.uint8)
    pot = np.asarray(pot, np.int64)
    sy, sx = grid.shape
    cell = np.arange(sx * sy, dtype=np.int64).reshape(sy, sx)
    door_key = np.where((grid != NO_INFORMATION) & (pot != UNREACHED), (pot << 32) | cell, np.int64(-1))
    big = np.int64(2 ** 63 - 1)
    key = np.full((sy, sx), big, np.int64)
    for xd, yd in N4:
        k = shifted(door_key, xd, yd, np.int64(-1))
        key = np.where(k >= 0, np.minimum(key, k), key)
    mask = (grid == NO_INFORMATION) & (key < big)
    return mask, np.where(mask, key, np.int64(-1))


def labels_flood(mask, neighbours=N8):
    """int32 [size_y, size_x]: the smallest linear cell of the cell's component, -1 for a cell that is no frontier cell"""
    sy, sx = mask.shape
    lab = np.full((sy, sx), -1, np.int32)
    for y0, x0 in zip(*np.nonzero(mask)):                                # ascending linear order: a seed is its component's smallest cell
        if lab[y0, x0] >= 0:
            continue
        root = int(y0) * sx + int(x0)
        lab[y0, x0] = root
        stack = [(int(x0), int(y0))]
        while stack:
            x, y = stack.pop()
            for xd, yd in neighbours:
                u, v = x + xd, y + yd
                if 0 <= u < sx and 0 <= v < sy and mask[v, u] and lab[v, u] < 0:
                    lab[v, u] = root
                    stack.append((u, v))
    return lab


def labels_sweeps(mask):
    """the order-free form: every frontier cell at once takes the minimum of its label and its eight neighbours', until nothing changes"""
    sy, sx = mask.shape
    none = np.int64(UNREACHED)
    lab = np.where(mask, np.arange(sx * sy, dtype=np.int64).reshape(sy, sx), none)
    for _ in range(sx * sy + 1):                                         # (bounded by the cell count)
        m = lab.copy()
        for xd, yd in N8:
            m = np.minimum(m, shifted(lab, xd, yd, none))
        new = np.where(mask, m, none)
        if (new == lab).all():
            break
        lab = new
    return np.where(mask, lab, -1).astype(np.int32)


def records(labels, key):
    """the frontiers in ascending root order: root, size, sum_x, sum_y, access_potential, access_cell"""
    sy, sx = labels.shape
    flat, keys = labels.reshape(-1), key.reshape(-1)
    cells = np.nonzero(flat >= 0)[0]
    out = []
    order = np.argsort(flat[cells], kind="stable")
    cells = cells[order]
    roots, starts = np.unique(flat[cells], return_index=True)
    for root, members in zip(roots.tolist(), np.split(cells, starts[1:])):
        k = int(keys[members].min())
        out.append({"root": int(root), "size": int(members.size), "sum_x": int((members % sx).sum()), "sum_y": int((members // sx).sum()),
                    "access_potential": k >> 32, "access_cell": k & 0xFFFFFFFF})
    return out


def cost(rec, resolution, potential_scale, gain_scale):
    """potential_scale * access_potential - gain_scale * (size * resolution): four double operations, each rounded on its own"""
    gain = np.float64(rec["size"]) * np.float64(resolution)
    return float(np.float64(potential_scale) * np.float64(rec["access_potential"]) - np.float64(gain_scale) * gain)


def search(grid, pot, resolution, min_frontier_size=0.0, potential_scale=1.0, gain_scale=1.0):
    """what gem_frontiers_host / gem_costmap_frontiers answer: labels, the kept list, the counts, the winner"""
    mask, key = classify(grid, pot)
    labels = labels_flood(mask)
    every = records(labels, key)
    kept = []
    best = -1
    for r in every:
        r["cost"] = cost(r, resolution, potential_scale, gain_scale)
        if not float(np.float64(r["size"]) * np.float64(resolution)) >= min_frontier_size:
            continue
        if best < 0 or r["cost"] < kept[best]["cost"]:                   # ascending roots and a strict <: the smaller root wins a tie
            best = len(kept)
        kept.append(r)
    return {"mask": mask, "labels": labels, "all": every, "kept": kept, "n_cells": int(mask.sum()), "n_frontiers": len(every),
            "n_kept": len(kept), "best": best, "best_frontier": kept[best] if best >= 0 else None}


def centroid(rec, resolution, origin_x, origin_y):
    """origin + (sum / size + 0.5) * resolution, in double"""
    return (float(origin_x + (np.float64(rec["sum_x"]) / np.float64(rec["size"]) + 0.5) * resolution),
            float(origin_y + (np.float64(rec["sum_y"]) / np.float64(rec["size"]) + 0.5) * resolution))
