"""numpy / plain Python restatement of the best-trajectory contract of include/gem_hip_critics.h: base_local_planner's
SimpleScoredSamplingPlanner (scoreTrajectory, findBestTrajectory) over the critic scores of tests/footprint_ref.py
(ObstacleCostFunction) and tests/mapgrid_ref.py (MapGridCostFunction), which are used as they are.  base_local_planner is not available
to these tests: this is a restatement, unverified against the library.

A critic is a dict {kind, grid, flags, column, scale, xshift}.  Python floats are C doubles and every operation is rounded on its own.
The combination has two literal forms: `combine` / `find_best` (the contract: no early exit) and `library_find_best` (the library's
loop WITH its early exit against the best cost so far); tests/test_critics_cpu.py pins the two to the same winner."""
import numpy as np

import costmap_ref as cref
import footprint_ref as fref
import mapgrid_ref as mref

OBSTACLE, MAPGRID, EXTERNAL, MAX = 1, 2, 3, 8
GRID_PATH, GRID_GOAL, GRID_FRONT = 1, 2, 4
CENTRE_COST = 4
BAD_LENGTH = -5.0


def obstacle(scale, flags=0):
    return {"kind": OBSTACLE, "grid": 0, "flags": flags, "column": 0, "scale": float(scale), "xshift": 0.0}


def map_grid(scale, grid, xshift=0.0, flags=0):
    return {"kind": MAPGRID, "grid": grid, "flags": flags, "column": 0, "scale": float(scale), "xshift": float(xshift)}


def external(scale, column):
    return {"kind": EXTERNAL, "grid": 0, "flags": 0, "column": column, "scale": float(scale), "xshift": 0.0}


def dwa_list(scales=(1.0, 0.01, 24.0, 32.0, 32.0, 24.0, 0.5), obstacle_flags=0, grid_flags=0, forward=0.325):
    """the order DWAPlanner builds: oscillation (external 0), obstacle, goal_front, alignment, path, goal, twirling (external 1)"""
    stop = mref.STOP_ON_FAILURE
    return [external(scales[0], 0), obstacle(scales[1], obstacle_flags), map_grid(scales[2], GRID_FRONT, forward, grid_flags),
            map_grid(scales[3], GRID_PATH, forward, grid_flags), map_grid(scales[4], GRID_PATH, 0.0, grid_flags | stop),
            map_grid(scales[5], GRID_GOAL, 0.0, grid_flags | stop), external(scales[6], 1)]


def front_plan(plan, forward):
    """DWAPlanner::updatePlanAndLocalCosts: the last point moved by `forward` along the direction from the robot (plan[0]) to it"""
    import math
    p = [(float(x), float(y)) for x, y in plan]
    (x0, y0), (gx, gy) = p[0], p[-1]
    a = math.atan2(gy - y0, gx - x0)
    p[-1] = (gx + forward * math.cos(a), gy + forward * math.sin(a))
    return p


# ---- critic scores ------------------------------------------------------------------------------------------------------------------
def _lengths(n_traj, T, lens):
    return np.full(n_traj, T, np.int64) if lens is None else np.asarray(lens, np.int64).reshape(n_traj)


def obstacle_scores(cm, poses, T, spec, flags, lens=None):
    """float64 [n_traj]: gem_costmap_score_trajectories' trajectory cost over the first lens[t] poses, CENTRE_COST applied to the
    non-negative pose results first"""
    p = np.asarray(poses, np.float64).reshape(-1, 4)
    n_traj = p.shape[0] // T
    pc = fref.footprint_cost(cm, p, spec, flags & fref.INSCRIBED_LETHAL).astype(np.int64)
    if flags & CENTRE_COST:
        ok, idx = cref.world_to_map_v(cm, p[:, 0], p[:, 1])
        byte = cm.grid.reshape(-1)[np.where(ok, idx, 0)].astype(np.int64)
        pc = np.where(pc >= 0, np.maximum(pc, byte), pc)
    ln = _lengths(n_traj, T, lens)
    if lens is None:
        return fref.score_trajectories(pc, T, flags & fref.SUM).astype(np.float64)
    out = np.zeros(n_traj, np.float64)
    for t in range(n_traj):
        L = int(ln[t])
        if 1 <= L <= T:
            out[t] = float(fref.score_trajectories_loop(pc[t * T:t * T + L], L, flags & fref.SUM)[0])
    return out


def map_grid_scores(cm, dist, poses, T, xshift, flags, lens=None):
    p = np.asarray(poses, np.float64).reshape(-1, 4)
    n_traj = p.shape[0] // T
    if lens is None:
        return mref.score(cm, dist, p, T, xshift, flags).astype(np.float64)
    ln = _lengths(n_traj, T, lens)
    out = np.zeros(n_traj, np.float64)
    for t in range(n_traj):
        L = int(ln[t])
        if 1 <= L <= T:
            out[t] = float(mref.score(cm, dist, p[t * T:t * T + L], L, xshift, flags)[0])
    return out


def score_table(cm, grids, critics, poses, T, spec, ext=None, lens=None):
    """float64 [n_critics, n_traj]: every critic's score of every trajectory (whether or not the combination reads it).  grids maps
    GRID_PATH / GRID_GOAL / GRID_FRONT to a distance grid."""
    p = np.asarray(poses, np.float64).reshape(-1, 4)
    n_traj = p.shape[0] // T
    out = np.zeros((len(critics), n_traj), np.float64)
    for k, c in enumerate(critics):
        if c["kind"] == OBSTACLE:
            out[k] = obstacle_scores(cm, p, T, spec, c["flags"], lens)
        elif c["kind"] == MAPGRID:
            out[k] = map_grid_scores(cm, grids[c["grid"]], p, T, c["xshift"], c["flags"], lens)
        else:
            out[k] = np.asarray(ext, np.float64).reshape(-1, n_traj)[c["column"]]
    return out


# ---- the combination ----------------------------------------------------------------------------------------------------------------
def combine_one(critics, column):
    """SimpleScoredSamplingPlanner::scoreTrajectory without the early exit: `column` = the critics' scores of one trajectory"""
    total = 0.0
    for c, s in zip(critics, column):
        if c["scale"] == 0:
            continue
        s = float(s)
        if s < 0:
            total = s
            break
        if s != 0:
            s = s * c["scale"]
        total = total + s
    return total


def combine(critics, scores, lens=None, T=None):
    """float64 [n_traj] totals; a length outside [1, T] answers BAD_LENGTH (the device form's rule)"""
    scores = np.asarray(scores, np.float64).reshape(len(critics), -1)
    out = np.array([combine_one(critics, scores[:, t].tolist()) for t in range(scores.shape[1])], np.float64).reshape(-1)
    if lens is not None:
        ln = np.asarray(lens, np.int64)
        out[(ln < 1) | (ln > T)] = BAD_LENGTH
    return out


def find_best(totals):
    """findBestTrajectory over finished totals: (index, cost, n_valid); strict < in generation order, (-1, -1.0, 0) without a valid one"""
    best, best_cost, n_valid = -1, -1.0, 0
    for t, c in enumerate(np.asarray(totals, np.float64).tolist()):
        if c >= 0:
            n_valid += 1
            if best_cost < 0 or c < best_cost:
                best_cost, best = c, t
    return best, best_cost, n_valid


def library_find_best(critics, scores):
    """the library's two loops literally, WITH scoreTrajectory's early exit against best_traj_cost: (index, cost)"""
    scores = np.asarray(scores, np.float64).reshape(len(critics), -1)

    def score_trajectory(t, best_traj_cost):
        traj_cost = 0.0
        for k, c in enumerate(critics):
            if c["scale"] == 0:
                continue
            cost = float(scores[k, t])
            if cost < 0:
                traj_cost = cost
                break
            if cost != 0:
                cost *= c["scale"]
            traj_cost += cost
            if best_traj_cost > 0:
                if traj_cost > best_traj_cost:                           # "once we are worse than the best, we will stay worse"
                    break
        return traj_cost

    best, best_traj_cost = -1, -1.0
    for t in range(scores.shape[1]):
        loop_traj_cost = score_trajectory(t, best_traj_cost)
        if loop_traj_cost >= 0:
            if best_traj_cost < 0 or loop_traj_cost < best_traj_cost:
                best_traj_cost, best = loop_traj_cost, t
    return best, best_traj_cost
