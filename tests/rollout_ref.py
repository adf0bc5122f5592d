"""Plain-Python / numpy restatement of the rollout contract of include/gem_hip_rollout.h: base_local_planner's
TrajectoryPlanner::createTrajectories and generateTrajectory (ROS noetic trajectory_planner.cpp), on top of costmap_ref, footprint_ref
and trajgen_ref's sine and cosine.  base_local_planner is not available to these tests: this is a restatement from memory, unverified
against the library.

Two forms, which tests/test_rollout_cpu.py pins to the same answers:
  literal       createTrajectories as the library writes it: two trajectories, best and comp, swapped when comp wins; every candidate
                generated where the library calls generateTrajectory, step by step with the sequential footprint loop; the early returns
                after the in-place rotations and after the strafes, so that later candidates are never generated.
  evaluate_all  every candidate of every phase first -- the kinematics of a trajectory on their own, then its footprints, cells and
                grid values as arrays and the first event found among them -- then the pick over the arrays (pick()).

All arithmetic is Python float = C double, every operation rounded on its own.  std::min(a, b) is b if b < a else a, std::max(a, b)
is b if a < b else a."""
import math
import struct

import numpy as np

import costmap_ref as cref
import footprint_ref as fref
from trajgen_ref import M_PI_2, sincos

ESCAPING, STUCK_LEFT, STUCK_RIGHT, STUCK_LEFT_STRAFE, STUCK_RIGHT_STRAFE = 1, 2, 4, 8, 16
MAX_Y_VELS, MAX_LIST, MAX_STEPS = 8, 256, 4096
THETA_BOUND = 64.0 * math.pi - 2.0
NO_AHEAD = -1
DOUBLES = ("sim_time", "sim_granularity", "angular_sim_granularity", "sim_period", "pdist_scale", "gdist_scale", "occdist_scale",
           "heading_lookahead", "max_vel_x", "min_vel_x", "max_vel_th", "min_vel_th", "min_in_place_vel_th", "backup_vel", "acc_lim_x",
           "acc_lim_y", "acc_lim_theta")

# TrajectoryPlannerROS's defaults (meter_scoring off: the scales as they are)
DEFAULTS = dict(sim_time=1.0, sim_granularity=0.025, angular_sim_granularity=0.025, sim_period=0.05, pdist_scale=0.6, gdist_scale=0.8,
                occdist_scale=0.01, heading_lookahead=0.325, max_vel_x=0.5, min_vel_x=0.1, max_vel_th=1.0, min_vel_th=-1.0,
                min_in_place_vel_th=0.4, backup_vel=-0.1, acc_lim_x=2.5, acc_lim_y=2.5, acc_lim_theta=3.2, vx_samples=3, vtheta_samples=20,
                dwa=1, holonomic_robot=1, y_vels=(-0.3, -0.1, 0.1, 0.3), final_goal=None)


def std_min(a, b):
    return b if b < a else a


def std_max(a, b):
    return b if a < b else a


# ---- the window and the candidates ------------------------------------------------------------------------------------------------------
def window(cfg, pos, vel):
    mx = float(cfg["max_vel_x"])
    if cfg.get("final_goal") is not None:
        dx, dy = float(cfg["final_goal"][0]) - float(pos[0]), float(cfg["final_goal"][1]) - float(pos[1])
        mx = std_min(mx, math.sqrt(dx * dx + dy * dy) / float(cfg["sim_time"]))
    T = float(cfg["sim_period"]) if cfg["dwa"] else float(cfg["sim_time"])
    w = {}
    w["max_x"] = std_max(std_min(mx, float(vel[0]) + float(cfg["acc_lim_x"]) * T), float(cfg["min_vel_x"]))
    w["min_x"] = std_max(float(cfg["min_vel_x"]), float(vel[0]) - float(cfg["acc_lim_x"]) * T)
    w["max_th"] = std_min(float(cfg["max_vel_th"]), float(vel[2]) + float(cfg["acc_lim_theta"]) * T)
    w["min_th"] = std_max(float(cfg["min_vel_th"]), float(vel[2]) - float(cfg["acc_lim_theta"]) * T)
    w["dvx"] = (w["max_x"] - w["min_x"]) / float(int(cfg["vx_samples"]) - 1)
    w["dvth"] = (w["max_th"] - w["min_th"]) / float(int(cfg["vtheta_samples"]) - 1)
    return w


def limited(vth, min_in_place):
    return std_max(vth, min_in_place) if vth > 0 else std_min(vth, -1.0 * min_in_place)


def candidates(cfg, pos, vel, state):
    """[(phase, (sx, sy, sth), unlimited vth or None)] in the library's call order, the values by its running additions"""
    w = window(cfg, pos, vel)
    out = []
    if not state & ESCAPING:
        vx_samp = w["min_x"]
        for _ in range(int(cfg["vx_samples"])):
            out.append(("A", (vx_samp, 0.0, 0.0), None))
            vth_samp = w["min_th"]
            for _ in range(int(cfg["vtheta_samples"]) - 1):
                out.append(("A", (vx_samp, 0.0, vth_samp), None))
                vth_samp += w["dvth"]
            vx_samp += w["dvx"]
        if cfg["holonomic_robot"]:
            out.append(("A", (0.1, 0.1, 0.0), None))
            out.append(("A", (0.1, -0.1, 0.0), None))
    vth_samp = w["min_th"]
    for _ in range(int(cfg["vtheta_samples"])):
        out.append(("B", (0.0, 0.0, limited(vth_samp, float(cfg["min_in_place_vel_th"]))), vth_samp))
        vth_samp += w["dvth"]
    if cfg["holonomic_robot"]:
        for v in cfg["y_vels"]:
            out.append(("C", (0.0, float(v), 0.0), None))
    out.append(("D", (float(cfg["backup_vel"]), 0.0, 0.0), None))
    return out


def num_steps(cfg, s):
    vmag = math.sqrt(s[0] * s[0] + s[1] * s[1])
    n = int(std_max(vmag * float(cfg["sim_time"]) / float(cfg["sim_granularity"]), math.fabs(s[2]) / float(cfg["angular_sim_granularity"])) + 0.5)
    return 1 if n == 0 else n


def new_velocity(target, v, acc, dt):
    if target - v >= 0:
        return std_min(target, v + acc * dt)
    return std_max(target, v - acc * dt)


def ahead_of(cm, goal, cfg, end):
    """`ahead` of an end pose (x, y, cos, sin): GOAL of the cell heading_lookahead in front of it, NO_AHEAD off the map"""
    la = float(cfg["heading_lookahead"])
    c = cref.world_to_map(cm, end[0] + la * end[2], end[1] + la * end[3])
    return NO_AHEAD if c is None else int(goal[c[1], c[0]])


# ---- generateTrajectory, literally ------------------------------------------------------------------------------------------------------
def generate(cm, path, goal, cfg, pos, vel, s, spec, flags=0):
    """one candidate step by step: {'cost', 'poses': [(x, y, cos, sin)] recorded, 'ahead', 'num_steps', 'first': what stopped it}"""
    n = num_steps(cfg, s)
    dt = float(cfg["sim_time"]) / float(n)
    OB = cm.size_x * cm.size_y
    acc = (float(cfg["acc_lim_x"]), float(cfg["acc_lim_y"]), float(cfg["acc_lim_theta"]))
    x, y, th = (float(v) for v in pos)
    vx, vy, vth = (float(v) for v in vel)
    occ = pd = gd = 0
    poses = []
    res = {"num_steps": n, "first": None}
    for _ in range(n):
        cell = cref.world_to_map(cm, x, y)
        if cell is None:
            res.update(cost=-1.0, first="off")
            break
        sn, cs = sincos(th)
        sn2, cs2 = sincos(M_PI_2 + th)
        f = fref.footprint_cost_loop(cm, (x, y, cs, sn), spec, flags)
        if f < 0:
            res.update(cost=-1.0, first="footprint")
            break
        occ = max(max(occ, f), int(cm.grid[cell[1], cell[0]]))
        pd, gd = int(path[cell[1], cell[0]]), int(goal[cell[1], cell[0]])
        if OB <= gd or OB <= pd:
            res.update(cost=-2.0, first="UN" if max(gd, pd) > OB else "OB")
            break
        poses.append((x, y, cs, sn))
        vx, vy, vth = new_velocity(s[0], vx, acc[0], dt), new_velocity(s[1], vy, acc[1], dt), new_velocity(s[2], vth, acc[2], dt)
        x = x + (vx * cs + vy * cs2) * dt
        y = y + (vx * sn + vy * sn2) * dt
        th = th + vth * dt
    else:
        res["cost"] = (float(cfg["pdist_scale"]) * float(pd) + float(gd) * float(cfg["gdist_scale"])) + float(cfg["occdist_scale"]) * float(occ)
    res["poses"] = poses
    res["ahead"] = ahead_of(cm, goal, cfg, poses[-1]) if res["cost"] >= 0 else NO_AHEAD
    return res


# ---- createTrajectories, literally ------------------------------------------------------------------------------------------------------
def answer(index, stage, cost, raw, v):
    return {"index": index, "stage": stage, "cost": cost, "raw_cost": raw, "velocity": tuple(v),
            "bytes": struct.pack("<qiidddddq", index, stage, 0, cost, raw, v[0], v[1], v[2], 0)}


def create_trajectories_literal(cm, path, goal, cfg, pos, vel, state, spec, flags=0):
    """(answer, the trajectories generated on the way, in call order)"""
    w = window(cfg, pos, vel)
    made = []

    def gen(s):
        t = generate(cm, path, goal, cfg, pos, vel, s, spec, flags)
        t["index"], t["xv"], t["yv"], t["thetav"] = len(made), s[0], s[1], s[2]
        made.append(t)
        return t

    best, comp = {"cost": -1.0, "yv": 0.0, "index": -1}, None
    if not state & ESCAPING:
        vx_samp = w["min_x"]
        for _ in range(int(cfg["vx_samples"])):
            comp = gen((vx_samp, 0.0, 0.0))
            if comp["cost"] >= 0 and (comp["cost"] < best["cost"] or best["cost"] < 0):
                best, comp = comp, best
            vth_samp = w["min_th"]
            for _ in range(int(cfg["vtheta_samples"]) - 1):
                comp = gen((vx_samp, 0.0, vth_samp))
                if comp["cost"] >= 0 and (comp["cost"] < best["cost"] or best["cost"] < 0):
                    best, comp = comp, best
                vth_samp += w["dvth"]
            vx_samp += w["dvx"]
        if cfg["holonomic_robot"]:
            for vy_samp in (0.1, -0.1):
                comp = gen((0.1, vy_samp, 0.0))
                if comp["cost"] >= 0 and (comp["cost"] < best["cost"] or best["cost"] < 0):
                    best, comp = comp, best
    vth_samp = w["min_th"]
    heading_dist = float("inf")                                           # DBL_MAX
    for _ in range(int(cfg["vtheta_samples"])):
        comp = gen((0.0, 0.0, limited(vth_samp, float(cfg["min_in_place_vel_th"]))))
        if comp["cost"] >= 0 and (comp["cost"] <= best["cost"] or best["cost"] < 0 or best["yv"] != 0.0) and \
                (vth_samp > w["dvth"] or vth_samp < -1 * w["dvth"]):
            a = comp["ahead"]                                             # the end point's cell heading_lookahead ahead, when worldToMap gives one
            if a != NO_AHEAD and a < heading_dist:
                if vth_samp < 0 and not state & STUCK_LEFT:
                    best, comp = comp, best
                    heading_dist = a
                elif vth_samp > 0 and not state & STUCK_RIGHT:
                    best, comp = comp, best
                    heading_dist = a
        vth_samp += w["dvth"]
    if best["cost"] >= 0:
        return answer(best["index"], 1, best["cost"], best["cost"], (best["xv"], best["yv"], best["thetav"])), made
    if cfg["holonomic_robot"]:
        for v in cfg["y_vels"]:
            vy_samp = float(v)
            comp = gen((0.0, vy_samp, 0.0))
            if comp["cost"] >= 0 and (comp["cost"] <= best["cost"] or best["cost"] < 0):
                a = comp["ahead"]
                if a != NO_AHEAD and a < heading_dist:
                    if vy_samp > 0 and not state & STUCK_LEFT_STRAFE:
                        best, comp = comp, best
                        heading_dist = a
                    elif vy_samp < 0 and not state & STUCK_RIGHT_STRAFE:
                        best, comp = comp, best
                        heading_dist = a
    if best["cost"] >= 0:
        return answer(best["index"], 2, best["cost"], best["cost"], (best["xv"], best["yv"], best["thetav"])), made
    comp = gen((float(cfg["backup_vel"]), 0.0, 0.0))
    best, comp = comp, best                                               # whatever its cost
    raw = best["cost"]
    cost = 1.0 if raw == -1.0 else raw
    return answer(best["index"], 3, cost, raw, (best["xv"], best["yv"], best["thetav"])), made


# ---- evaluate all, then pick --------------------------------------------------------------------------------------------------------------
def kinematics(cfg, pos, vel, s):
    """the poses of all num_steps steps, whatever the map says: float64 [n, 4] (x, y, cos, sin)"""
    n = num_steps(cfg, s)
    dt = float(cfg["sim_time"]) / float(n)
    acc = (float(cfg["acc_lim_x"]), float(cfg["acc_lim_y"]), float(cfg["acc_lim_theta"]))
    x, y, th = (float(v) for v in pos)
    vx, vy, vth = (float(v) for v in vel)
    out = np.zeros((n, 4), np.float64)
    for i in range(n):
        sn, cs = sincos(th)
        sn2, cs2 = sincos(M_PI_2 + th)
        out[i] = (x, y, cs, sn)
        vx, vy, vth = new_velocity(s[0], vx, acc[0], dt), new_velocity(s[1], vy, acc[1], dt), new_velocity(s[2], vth, acc[2], dt)
        x = x + (vx * cs + vy * cs2) * dt
        y = y + (vx * sn + vy * sn2) * dt
        th = th + vth * dt
    return out


OFF, FOOTPRINT, OB_CELL, UN_CELL = 1, 2, 3, 4                                # why a step stops a trajectory (0: it does not)


def evaluate(cm, path, goal, cfg, pos, vel, s, spec, flags=0):
    """(cost, ahead, recorded steps, poses [n, 4], per step why it would stop the trajectory): the events found among arrays"""
    poses = kinematics(cfg, pos, vel, s)
    OB = cm.size_x * cm.size_y
    ok, idx = cref.world_to_map_v(cm, poses[:, 0], poses[:, 1])
    idx = np.where(ok, idx, 0)
    f = fref.footprint_cost(cm, poses, spec, flags)
    pd, gd = path.reshape(-1)[idx].astype(np.int64), goal.reshape(-1)[idx].astype(np.int64)
    why = np.where(~ok, OFF, np.where(f < 0, FOOTPRINT, np.where((OB <= gd) | (OB <= pd), np.where(np.maximum(gd, pd) > OB, UN_CELL, OB_CELL), 0)))
    bad = np.flatnonzero(why)
    if bad.size:
        return (-1.0 if why[bad[0]] in (OFF, FOOTPRINT) else -2.0), NO_AHEAD, int(bad[0]), poses, why
    occ = int(max(int(f.max()), int(cm.grid.reshape(-1)[idx].max())))
    cost = (float(cfg["pdist_scale"]) * float(pd[-1]) + float(gd[-1]) * float(cfg["gdist_scale"])) + float(cfg["occdist_scale"]) * float(occ)
    return cost, ahead_of(cm, goal, cfg, poses[-1]), poses.shape[0], poses, why


def pick(cfg, pos, vel, state, cands, cost, ahead):
    """the pick over arrays: phases by the candidates' tags"""
    w = window(cfg, pos, vel)
    best, best_cost, best_yv = -1, -1.0, 0.0
    heading = None
    for c, (phase, s, _) in enumerate(cands):
        if phase == "A" and cost[c] >= 0 and (cost[c] < best_cost or best_cost < 0):
            best, best_cost, best_yv = c, float(cost[c]), s[1]
    for c, (phase, s, vth) in enumerate(cands):
        if phase != "B":
            continue
        if not (cost[c] >= 0 and (cost[c] <= best_cost or best_cost < 0 or best_yv != 0.0)):
            continue
        if not (vth > w["dvth"] or vth < -w["dvth"]):
            continue
        if ahead[c] == NO_AHEAD or (heading is not None and not ahead[c] < heading):
            continue
        if (vth < 0 and not state & STUCK_LEFT) or (vth > 0 and not state & STUCK_RIGHT):
            best, best_cost, best_yv, heading = c, float(cost[c]), 0.0, int(ahead[c])
    stage = 1
    if best_cost < 0:
        stage = 2
        for c, (phase, s, _) in enumerate(cands):
            if phase != "C":
                continue
            if not (cost[c] >= 0 and (cost[c] <= best_cost or best_cost < 0)):
                continue
            if ahead[c] == NO_AHEAD or (heading is not None and not ahead[c] < heading):
                continue
            if (s[1] > 0 and not state & STUCK_LEFT_STRAFE) or (s[1] < 0 and not state & STUCK_RIGHT_STRAFE):
                best, best_cost, best_yv, heading = c, float(cost[c]), s[1], int(ahead[c])
    raw = best_cost
    if best_cost < 0:
        stage, best = 3, len(cands) - 1
        raw = float(cost[best])
        best_cost = 1.0 if raw == -1.0 else raw
    return answer(best, stage, best_cost, raw, cands[best][1])


def evaluate_all(cm, path, goal, cfg, pos, vel, state, spec, flags=0, fill=0.0):
    """what gem_rollout_host leaves: {'answer', 'cost' float64 [n], 'ahead' int32 [n], 'steps' int32 [n], 'poses' float64 [n, T, 4] with
    `fill` past the steps, 'num_steps' [n], 'why': per candidate the per-step reasons, 'cands', 'max_steps'}"""
    cands = candidates(cfg, pos, vel, state)
    n = len(cands)
    T = max(num_steps(cfg, s) for _, s, _ in cands)
    cost, ahead, steps = np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros(n, np.int32)
    poses = np.full((n, T, 4), fill, np.float64)
    codes, ns = [], np.zeros(n, np.int32)
    for c, (_, s, _) in enumerate(cands):
        cost[c], ahead[c], steps[c], p, why = evaluate(cm, path, goal, cfg, pos, vel, s, spec, flags)
        poses[c, :steps[c]] = p[:steps[c]]
        codes.append(why)
        ns[c] = p.shape[0]
    return {"answer": pick(cfg, pos, vel, state, cands, cost, ahead), "cost": cost, "ahead": ahead, "steps": steps, "poses": poses,
            "num_steps": ns, "why": codes, "cands": cands, "max_steps": T}
