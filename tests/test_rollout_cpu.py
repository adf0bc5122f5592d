"""Trajectory rollout (include/gem_hip_rollout.h) without a device: the two forms of tests/rollout_ref.py against each other, and the
host twin gem_rollout_host / gem_rollout_pick / gem_rollout_plan against them.  Every comparison is exact: arrays by tobytes(),
indices and stages as integers, costs and the 64-byte answer by their bytes.

  1. every scene: the literal createTrajectories and evaluate-all-then-pick give the same answer, and the literal form's trajectories
     are a prefix of the other's;
  2. every scene: the twin's poses, step counts, costs, `ahead` and answer equal the reference's; the plan's window and lists too;
  3. the scenes' coverage, asserted from rollout_ref alone: a scene that stops exercising a branch fails here;
  4. (int)(x + 0.5) on both sides of a half; 5. every refusal, outputs untouched; 6. the header, the bindings, the stand-alone twin."""
import ctypes as C
import functools
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import gem_amd
from gem_amd import _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import footprint_ref as fref  # noqa: E402
import mapgrid_ref as mref  # noqa: E402
import rollout_ref as ref  # noqa: E402
from test_critics_gpu import CLEARED, SMALL, parity_case  # noqa: E402
from test_mapgrid_gpu import centre, ref_map  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
INV = _lib.GEM_OK - 1
SENTINEL = -77.0
E, SL, SR, SLS, SRS = ref.ESCAPING, ref.STUCK_LEFT, ref.STUCK_RIGHT, ref.STUCK_LEFT_STRAFE, ref.STUCK_RIGHT_STRAFE
TRIANGLE = [[0.3, 0.0], [-0.2, 0.2], [-0.2, -0.2]]
ROUND32 = fref.regular_polygon(32, 0.35)
DEFAULTS = ref.DEFAULTS                                                   # 3 x 20, holonomic, four y_vels, dwa
TWO = dict(DEFAULTS, vx_samples=2, vtheta_samples=2, dwa=0, holonomic_robot=0, y_vels=(), min_vel_x=0.0)     # 2 x 2 without dwa
UTURN = dict(TWO, sim_time=3.0, sim_granularity=0.1, angular_sim_granularity=0.1, min_vel_x=0.1)


# ---- the maps (computed once, never changed) ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def world(name):
    """(Costmap, PATH, GOAL): the reference's local costmap geometry (75 x 75 at 0.2) over the seeded noise and cleared block of
    test_critics_gpu.parity_case, and its 130 x 90 map at 0.05 as it is"""
    if name == "75":
        cm = ref_map(np.array(parity_case("75x75")["cm"].grid), res=0.2)
        want = mref.grids(cm, [centre(cm, 1, 1), centre(cm, 37, 37), centre(cm, 63, 63)])
    else:
        c = parity_case("130x90")
        cm, want = c["cm"], c["want"]
    for a in (cm.grid, want["path"], want["goal"]):
        a.setflags(write=False)
    return cm, want["path"], want["goal"]


def world_plan(name):
    """the global plan the grids of world(name) were prepared from"""
    cm = world(name)[0]
    return [centre(cm, 1, 1), centre(cm, 37, 37), centre(cm, 63, 63)] if name == "75" else parity_case("130x90")["plan"]


def block(name):
    rows, cols = CLEARED["75x75" if name == "75" else "130x90"]
    return cols.start, rows.start


def at(name, dx, dy, yaw):
    """a pose at the centre of the cell (dx, dy) of the cleared block"""
    cm = world(name)[0]
    x0, y0 = block(name)
    return (*centre(cm, x0 + dx, y0 + dy), yaw)


# name: (map, pose, vel, config, state flags, spec, footprint flags)
SCENES = {
    "75 open": ("75", at("75", 25, 25, 0.7), (0.2, 0.0, 0.1), DEFAULTS, 0, fref.RECTANGLE, 0),
    "75 open escaping": ("75", at("75", 25, 25, 0.7), (0.2, 0.0, 0.1), DEFAULTS, E, fref.RECTANGLE, 0),
    "75 open escaping, no rotation": ("75", at("75", 25, 25, 0.7), (0.2, 0.0, 0.1), DEFAULTS, E | SL | SR, fref.RECTANGLE, 0),
    "75 open all stuck": ("75", at("75", 25, 25, 0.7), (0.2, 0.0, 0.1), DEFAULTS, E | SL | SR | SLS | SRS, fref.RECTANGLE, 0),
    "75 rotation wins": ("75", at("75", 20, 30, -2.5), (0.2, 0.0, 0.1), DEFAULTS, 0, fref.RECTANGLE, 0),
    "75 rotation wins, stuck left": ("75", at("75", 20, 30, -2.5), (0.2, 0.0, 0.1), DEFAULTS, SL, fref.RECTANGLE, 0),
    "75 final goal": ("75", at("75", 30, 8, 2.0), (0.3, 0.0, -0.2), dict(DEFAULTS, final_goal=at("75", 31, 9, 0.0)[:2]), 0, SMALL, 1),
    "75 over the lethal patch": ("75", at("75", 16, 11, 0.3), (0.1, 0.0, 0.0), DEFAULTS, 0, fref.RECTANGLE, 0),
    "75 on the inscribed patch": ("75", at("75", 10, 22, 0.0), (0.1, 0.0, 0.0), DEFAULTS, 0, fref.RECTANGLE, 0),
    "75 towards the lethal patch": ("75", at("75", 11, 11, 0.0), (0.5, 0.0, 0.0), dict(DEFAULTS, sim_time=2.0), 0, TRIANGLE, 0),
    "75 towards the inscribed patch": ("75", at("75", 4, 22, 0.0), (0.5, 0.0, 0.0), dict(DEFAULTS, sim_time=2.5), 0, [], 0),
    "75 u-turn over the edge": ("75", (*centre(world("75")[0], 2, 14), math.pi + 0.1), (0.5, 0.0, -1.0), UTURN, 0, [], 0),
    "75 u-turn over the edge, up": ("75", (*centre(world("75")[0], 30, 73), math.pi / 2 + 0.1), (0.5, 0.0, -1.0), UTURN, 0, [], 0),
    "75 two by two": ("75", at("75", 25, 25, -1.0), (0.0, 0.0, 0.0), TWO, 0, ROUND32, 0),
    "75 yaw near pi": ("75", at("75", 22, 14, 3.1415925), (0.2, 0.0, 0.3), DEFAULTS, 0, fref.RECTANGLE, 0),
    "75 yaw near -pi": ("75", at("75", 22, 14, -3.1415925), (0.2, 0.0, -0.3), DEFAULTS, 0, SMALL, 0),
    "130 open": ("130", at("130", 25, 12, 0.4), (0.2, 0.0, 0.0), DEFAULTS, 0, SMALL, 0),
    "130 rectangle": ("130", at("130", 30, 8, 1.2), (0.3, 0.0, 0.2), DEFAULTS, 0, fref.RECTANGLE, 0),
    "130 strafe": ("130", at("130", 25, 12, 0.4), (0.0, 0.0, 0.0), DEFAULTS, E | SL | SR, TRIANGLE, 1),
    "130 two by two, final goal": ("130", at("130", 20, 15, 2.0), (0.1, 0.0, 0.0), dict(TWO, final_goal=at("130", 22, 15, 0.0)[:2]), 0, [], 0),
    "130 inscribed patch, then the lethal one": ("130", at("130", 8, 27, math.atan2(-11.0, 6.0)), (0.5, 0.0, 0.0), dict(DEFAULTS, sim_time=2.5), 0, SMALL, 0),
    "130 lethal patch, then the inscribed one": ("130", at("130", 19, 9, math.atan2(11.0, -6.0)), (0.5, 0.0, 0.0), dict(DEFAULTS, sim_time=2.5), 0, SMALL, 0),
    "130 round": ("130", at("130", 35, 20, -0.6), (0.25, 0.0, -0.1), dict(DEFAULTS, holonomic_robot=0), 0, ROUND32, 1),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(evaluate_all's arrays with the sentinel in unused pose slots, the literal form's answer and trajectories)"""
    which, pos, vel, cfg, state, spec, flags = SCENES[name]
    cm, path, goal = world(which)
    r = ref.evaluate_all(cm, path, goal, cfg, pos, vel, state, spec, flags, fill=SENTINEL)
    lit = ref.create_trajectories_literal(cm, path, goal, cfg, pos, vel, state, spec, flags)
    for a in (r["cost"], r["ahead"], r["steps"], r["poses"]):
        a.setflags(write=False)
    return r, lit


def twin(name):
    which, pos, vel, cfg, state, spec, flags = SCENES[name]
    cm, path, goal = world(which)
    plan = gem_amd.rollout_plan(cfg, pos, vel, state)
    return plan, gem_amd.rollout_host(plan, pos, vel, cm.grid, cm.res, (cm.ox, cm.oy), path, goal, spec, flags, poses=True, fill=SENTINEL)


# ---- 1. the two forms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_the_two_forms_agree(name):
    r, (lit, made) = reference(name)
    assert lit["bytes"] == r["answer"]["bytes"], (lit, r["answer"])
    assert len(made) <= len(r["cands"]) and lit["index"] in {t["index"] for t in made}
    for t in made:                                                        # what the literal form generated on its way, in call order
        c = t["index"]
        assert (t["xv"], t["yv"], t["thetav"]) == r["cands"][c][1]
        assert np.float64(t["cost"]).tobytes() == r["cost"][c].tobytes() and t["ahead"] == r["ahead"][c] and len(t["poses"]) == r["steps"][c]
        assert np.array(t["poses"], np.float64).reshape(-1, 4).tobytes() == r["poses"][c, :r["steps"][c]].tobytes()
        assert t["num_steps"] == r["num_steps"][c]
    stage = lit["stage"]                                                  # the early returns: nothing behind the deciding phase was generated
    phases = {r["cands"][t["index"]][0] for t in made}
    assert phases <= {1: {"A", "B"}, 2: {"A", "B", "C"}, 3: {"A", "B", "C", "D"}}[stage] and ("D" in phases) == (stage == 3)


# ---- 2. the twin -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_the_twin_equals_the_reference(name):
    which, pos, vel, cfg, state, spec, flags = SCENES[name]
    r, _ = reference(name)
    plan, (ans, cost, ahead, steps, poses) = twin(name)
    w = ref.window(cfg, pos, vel)
    assert [plan.max_x, plan.min_x, plan.max_th, plan.min_th, plan.dvx, plan.dvth] == [w[k] for k in ("max_x", "min_x", "max_th", "min_th", "dvx", "dvth")]
    assert plan.n_cand == len(r["cands"]) and plan.max_steps == r["max_steps"] and plan.state_flags == state
    phases = [p for p, _, _ in r["cands"]]
    assert (plan.off_b, plan.off_c, plan.off_d) == (phases.count("A"), phases.count("A") + phases.count("B"), len(phases) - 1)
    assert steps.tobytes() == r["steps"].tobytes(), f"{int((steps != r['steps']).sum())} step counts differ"
    assert poses.tobytes() == r["poses"].tobytes(), f"{int((poses != r['poses']).any(axis=(1, 2)).sum())} trajectories differ"
    assert cost.tobytes() == r["cost"].tobytes() and ahead.tobytes() == r["ahead"].tobytes()
    assert ans["bytes"] == r["answer"]["bytes"], (ans, r["answer"])
    assert gem_amd.rollout_pick(plan, state, cost, ahead)["bytes"] == ans["bytes"]


# ---- 3. what the scenes cover, from the reference alone ---------------------------------------------------------------------------------------
def repick(name, state):
    """the scene's pick under other stuck flags (the ESCAPING bit is the scene's: it decides the candidates)"""
    which, pos, vel, cfg, own, spec, flags = SCENES[name]
    r, _ = reference(name)
    assert (state & E) == (own & E)
    return ref.pick(cfg, pos, vel, state, r["cands"], r["cost"], r["ahead"])


def test_the_scenes_cover_the_contract():
    seen = set()
    for name, (which, pos, vel, cfg, state, spec, flags) in SCENES.items():
        r, _ = reference(name)
        a, cands, cost, ahead = r["answer"], r["cands"], r["cost"], r["ahead"]
        w = ref.window(cfg, pos, vel)
        seen.add(f"stage {a['stage']}")
        if a["stage"] == 3:
            seen.add(f"stage 3 raw {a['raw_cost']:g}" if a["raw_cost"] < 0 else "stage 3 legal")
        in_a = [c for c, (p, _, _) in enumerate(cands) if p == "A"]
        legal_a = [c for c in in_a if cost[c] >= 0]
        if state & E:
            assert not in_a
            seen.add("escaping removes phase A")
        if legal_a:
            low = min(cost[c] for c in legal_a)
            first = [c for c in legal_a if cost[c] == low]
            if len(first) > 1:
                seen.add("a tie in phase A")
                assert ref.pick(cfg, pos, vel, state | SL | SR, cands, cost, ahead)["index"] == first[0]      # (no rotation may displace it)
            winner_a = first[0]
            if cands[a["index"]][0] == "B" and a["stage"] == 1:
                if cost[a["index"]] <= cost[winner_a] and cands[winner_a][1][1] == 0.0:
                    seen.add("B displaces a cheaper-or-equal A winner")
                if cands[winner_a][1][1] != 0.0 and cost[a["index"]] > cost[winner_a]:
                    seen.add("B of higher cost displaces a strafing A winner")
        for c, (p, s, vth) in enumerate(cands):
            if p == "B":
                seen.add("eligible" if vth > w["dvth"] or vth < -w["dvth"] else "ineligible")
            if s[1] != 0.0 and r["steps"][c] > 1:
                seen.add("vy != 0")
            if r["num_steps"][c] == 1 and max(abs(v) for v in s) < 0.02:
                seen.add("the num_steps floor of 1")
            if cost[c] >= 0 and ahead[c] == ref.NO_AHEAD:
                seen.add("ahead is none")
            why = r["why"][c]
            bad = np.flatnonzero(why)
            if bad.size:
                k, later = int(why[bad[0]]), set(why[bad[1:]].tolist())
                other = {ref.OB_CELL, ref.UN_CELL} if k in (ref.OFF, ref.FOOTPRINT) else {ref.OFF, ref.FOOTPRINT}
                seen.add(f"first event {k}")
                if later & other:
                    seen.add(f"first event {k}, the other code behind it")
            if "yaw" in name and r["steps"][c] > 2 and r["poses"][c, 0, 3] * r["poses"][c, r["steps"][c] - 1, 3] < 0 and r["poses"][c, 0, 2] < -0.9:
                seen.add("yaw crosses pi " + name[-3:].strip())
        for bit, what in ((SL, "STUCK_LEFT"), (SR, "STUCK_RIGHT"), (SLS, "STUCK_LEFT_STRAFE"), (SRS, "STUCK_RIGHT_STRAFE")):
            if repick(name, state ^ bit)["bytes"] != a["bytes"]:
                seen.add(what + " changes the answer")
    want = {"stage 1", "stage 2", "stage 3", "stage 3 raw -1", "stage 3 raw -2", "stage 3 legal", "escaping removes phase A", "a tie in phase A",
            "B displaces a cheaper-or-equal A winner", "B of higher cost displaces a strafing A winner", "eligible", "ineligible", "vy != 0",
            "the num_steps floor of 1", "ahead is none", "yaw crosses pi pi", "yaw crosses pi -pi",
            "STUCK_LEFT changes the answer", "STUCK_RIGHT changes the answer", "STUCK_LEFT_STRAFE changes the answer", "STUCK_RIGHT_STRAFE changes the answer"}
    want |= {f"first event {k}, the other code behind it" for k in (ref.OFF, ref.FOOTPRINT, ref.OB_CELL, ref.UN_CELL)}
    assert not want - seen, sorted(want - seen)
    specs = {len(s[5]) for s in SCENES.values()}
    assert specs == {0, 3, 4, 32} and {s[0] for s in SCENES.values()} == {"75", "130"}
    assert any(s[3].get("final_goal") is not None for s in SCENES.values()) and any(s[3].get("final_goal") is None for s in SCENES.values())
    assert any((s[3]["vx_samples"], s[3]["vtheta_samples"], s[3]["dwa"]) == (2, 2, 0) for s in SCENES.values())
    assert any((s[3]["vx_samples"], s[3]["vtheta_samples"], len(s[3]["y_vels"]), s[3]["holonomic_robot"]) == (3, 20, 4, 1) for s in SCENES.values())


# ---- 4. (int)(x + 0.5) ---------------------------------------------------------------------------------------------------------------------------
def test_num_steps_on_both_sides_of_a_half():
    """sim_time 1 and a granularity of 1/8 (exact): a backward speed of 0.3125 is 2.5 steps -> 3; one ulp below it -> 2.  The angular
    term has no sim_time: with sim_time 2, 0.3125 / 0.125 is still 2.5.  The zero sample takes one step."""
    cm, path, goal = world("75")
    pos, vel = at("75", 25, 25, 0.7), (0.0, 0.0, 0.0)
    half = 0.3125
    for backup, sim_time, want in ((-half, 1.0, 3), (-math.nextafter(half, 0.0), 1.0, 2), (-math.nextafter(half, 1.0), 1.0, 3), (-0.125 * 3.5, 1.0, 4),
                                   (-math.nextafter(0.125 * 3.5, 0.0), 1.0, 3)):
        cfg = dict(TWO, sim_time=sim_time, sim_granularity=0.125, angular_sim_granularity=0.125, backup_vel=backup, min_vel_x=0.0, max_vel_x=0.0,
                   max_vel_th=0.0, min_vel_th=0.0, min_in_place_vel_th=0.0)
        assert ref.num_steps(cfg, (backup, 0.0, 0.0)) == want
        plan = gem_amd.rollout_plan(cfg, pos, vel, 0)
        ans, cost, ahead, steps = gem_amd.rollout_host(plan, pos, vel, cm.grid, cm.res, (cm.ox, cm.oy), path, goal, [], 0)
        r = ref.evaluate_all(cm, path, goal, cfg, pos, vel, 0, [], 0)
        assert plan.max_steps == want and steps.tolist() == r["steps"].tolist() and steps[-1] == want and cost[-1] >= 0
        assert steps[:-1].tolist() == [1] * (plan.n_cand - 1)                                  # every other sample is the zero sample: the floor of 1
    for th, sim_time, want in ((half, 2.0, 3), (math.nextafter(half, 0.0), 2.0, 2)):        # the angular term: in-place candidates, no sim_time in it
        cfg = dict(TWO, sim_time=sim_time, sim_granularity=0.125, angular_sim_granularity=0.125, min_in_place_vel_th=th, min_vel_x=0.0, max_vel_x=0.0,
                   max_vel_th=0.01, min_vel_th=-0.01, backup_vel=0.0)
        plan = gem_amd.rollout_plan(cfg, pos, vel, E)
        ans, cost, ahead, steps = gem_amd.rollout_host(plan, pos, vel, cm.grid, cm.res, (cm.ox, cm.oy), path, goal, [], 0)
        assert steps.tolist() == [want, want, 1] == ref.evaluate_all(cm, path, goal, cfg, pos, vel, E, [], 0)["steps"].tolist()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_outputs_untouched():
    lib = _lib.load()
    which, pos, vel, cfg, state, spec, flags = SCENES["75 open"]
    cm, path, goal = world(which)
    nan, inf = float("nan"), float("inf")
    d3 = lambda v: None if v is None else (C.c_double * 3)(*v)
    good = gem_amd.rollout_plan(cfg, pos, vel, state)

    def plan_rc(pos_=pos, vel_=vel, state_=state, out=True, **kw):
        c = gem_amd.rollout_config(dict(cfg, **{k: v for k, v in kw.items() if k != "n_y_vels"}))
        if "n_y_vels" in kw:
            c.n_y_vels = kw["n_y_vels"]
        p = _lib.RolloutPlan()
        p.n_cand = -9
        rc = lib.gem_rollout_plan(C.byref(c), d3(pos_), d3(vel_), state_, C.byref(p) if out else None)
        assert rc == 0 or p.n_cand == -9
        return rc

    assert plan_rc() == 0
    for k in ref.DOUBLES:
        assert plan_rc(**{k: nan}) == INV and plan_rc(**{k: inf}) == INV, k
    for k in ("sim_time", "sim_granularity", "angular_sim_granularity", "sim_period"):
        assert plan_rc(**{k: 0.0}) == INV and plan_rc(**{k: -1.0}) == INV, k
    assert plan_rc(dwa=0, sim_period=0.0) == 0                           # (sim_period is read with dwa only)
    assert plan_rc(vx_samples=1) == INV and plan_rc(vtheta_samples=1) == INV and plan_rc(vx_samples=0) == INV      # the library divides by zero there
    assert plan_rc(vx_samples=128, vtheta_samples=128) == 0 and plan_rc(vx_samples=129, vtheta_samples=128) == INV and plan_rc(vx_samples=257) == INV
    for k in ("pdist_scale", "gdist_scale", "occdist_scale"):
        assert plan_rc(**{k: -0.5}) == INV and plan_rc(**{k: -0.0}) == INV and plan_rc(**{k: 0.0}) == 0, k
    assert plan_rc(n_y_vels=9) == INV and plan_rc(n_y_vels=-1) == INV and plan_rc(y_vels=(0.1, 0.0, 0.2)) == INV and plan_rc(y_vels=(0.1, nan)) == INV
    assert plan_rc(state_=32) == INV and plan_rc(state_=-1) == INV and plan_rc(out=False) == INV and plan_rc(pos_=None) == INV and plan_rc(vel_=None) == INV
    assert plan_rc(pos_=(pos[0], nan, 0.0)) == INV and plan_rc(vel_=(inf, 0.0, 0.0)) == INV
    assert plan_rc(pos_=(pos[0], pos[1], 64 * math.pi)) == INV and plan_rc(vel_=(0.1, 0.0, 200.0), max_vel_th=300.0, acc_lim_theta=0.0) == INV     # the 64 pi bound
    assert plan_rc(sim_granularity=1e-5) == INV                          # more than GEM_ROLLOUT_MAX_STEPS steps
    assert plan_rc(final_goal=(nan, 0.0)) == INV
    assert lib.gem_rollout_plan(None, d3(pos), d3(vel), 0, C.byref(_lib.RolloutPlan())) == INV

    nc, T = good.n_cand, good.max_steps
    cost, ahead, steps = np.full(nc, -99.0), np.full(nc, -7, np.int32), np.full(nc, -7, np.int32)
    poses = np.full((nc, T, 4), SENTINEL)
    best = _lib.RolloutBest(-9, -9, -9, -9.0, -9.0, -9.0, -9.0, -9.0, -9)
    geom = _lib.CostmapConfig(cm.size_x, cm.size_y, cm.res, cm.ox, cm.oy, 0)
    sp = np.ascontiguousarray(spec, np.float64)
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def tampered(**kw):
        q = _lib.RolloutPlan.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def host_rc(p=good, pos_=pos, vel_=vel, g=geom, bytes_=cm.grid, path_=path, goal_=goal, sp_=sp, nv=4, fl=0, c=cost, a=ahead, s=steps, b=True):
        return lib.gem_rollout_host(C.byref(p) if p is not None else None, d3(pos_), d3(vel_), C.byref(g) if g is not None else None, P(bytes_), P(path_),
                                    P(goal_), sp_.ctypes.data_as(C.POINTER(C.c_double)) if sp_ is not None else None, nv, fl, P(c), P(a), P(s), P(poses),
                                    C.byref(best) if b else None)

    bad_plans = [tampered(n_cand=nc + 1), tampered(max_steps=T - 1), tampered(off_b=good.off_b + 1), tampered(n_vx=2), tampered(dvth=0.0),
                 tampered(state_flags=E), tampered(min_x=good.min_x + 0.01)]
    q = tampered()
    q.lists[1] = nan
    bad_plans.append(q)
    q = tampered()
    q.config.sim_time = 0.0
    bad_plans.append(q)
    q = tampered()
    q.config.occdist_scale = -1.0
    bad_plans.append(q)
    for q in bad_plans:
        assert host_rc(p=q) == INV
    small = _lib.CostmapConfig(0, cm.size_y, cm.res, cm.ox, cm.oy, 0)
    coarse = _lib.CostmapConfig(cm.size_x, cm.size_y, 0.0, cm.ox, cm.oy, 0)
    for kw in (dict(p=None), dict(pos_=None), dict(vel_=None), dict(g=None), dict(g=small), dict(g=coarse), dict(bytes_=None), dict(path_=None),
               dict(goal_=None), dict(sp_=None), dict(nv=33), dict(nv=-1), dict(fl=2), dict(fl=4), dict(c=None), dict(a=None), dict(s=None), dict(b=False),
               dict(vel_=(vel[0] + 0.1, vel[1], vel[2])), dict(vel_=(vel[0], vel[1], vel[2] + 0.1)), dict(pos_=(nan, pos[1], pos[2]))):     # (a plan made for another velocity: its window differs)
        assert host_rc(**kw) == INV, kw
    bad_spec = sp.copy()
    bad_spec[2, 1] = inf
    assert host_rc(sp_=bad_spec) == INV
    pick_best = _lib.RolloutBest(-9, -9, -9, -9.0, -9.0, -9.0, -9.0, -9.0, -9)
    want = reference("75 open")[0]
    pc, pa = np.array(want["cost"]), np.array(want["ahead"])
    pick_rc = lambda p=good, st=state, c=pc, a=pa, b=True: lib.gem_rollout_pick(C.byref(p) if p is not None else None, st, P(c), P(a), C.byref(pick_best) if b else None)
    assert pick_rc(p=None) == INV and pick_rc(st=E) == INV and pick_rc(st=32) == INV and pick_rc(c=None) == INV and pick_rc(a=None) == INV and pick_rc(b=False) == INV
    for q in [bad_plans[k] for k in (0, 2, 3, 7, 8, 9)]:                 # what the pick indexes by and reads (it has no state to make the window from)
        assert pick_rc(p=q) == INV
    # nothing was written by any refusal
    assert (cost == -99.0).all() and (ahead == -7).all() and (steps == -7).all() and (poses == SENTINEL).all()
    assert (best.index, best.stage, best.cost, best.reserved1) == (-9, -9, -9.0, -9) and (pick_best.index, pick_best.stage) == (-9, -9)
    # ... and the same calls, unbroken, answer
    assert host_rc() == 0 and pick_rc() == 0 and pick_rc(st=SL | SRS) == 0
    assert cost.tobytes() == want["cost"].tobytes() and ahead.tobytes() == want["ahead"].tobytes() and steps.tobytes() == want["steps"].tobytes()
    assert bytes(best) == want["answer"]["bytes"] and poses.tobytes() == want["poses"].tobytes()


# ---- 6. the header, the bindings, the stand-alone twin -----------------------------------------------------------------------------------------
def test_header_and_bindings():
    import re
    lib = _lib.load()
    hdr = (ROOT / "include" / "gem_hip_rollout.h").read_text()
    names = sorted(set(re.findall(r"\b(gem_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert names == sorted(_lib.ROLLOUT_SIGNATURES) == ["gem_costmap_rollout_best", "gem_costmap_rollout_best_device", "gem_rollout_host", "gem_rollout_pick",
                                                        "gem_rollout_plan"]
    for n in names:
        assert getattr(lib, n).argtypes == _lib.ROLLOUT_SIGNATURES[n][1]
    text = (ROOT / "include" / "gem_hip.h").read_text()
    assert text.index('#include "gem_hip_trajgen.h"') < text.index('#include "gem_hip_rollout.h"') and lib.gem_abi_version() == 9
    for word in ("RESTATED FROM MEMORY", "UNVERIFIED", "meter_scoring", "hypot", "stuck_left", "heading_scoring", "simple_attractor", "checkTrajectory",
                 "divides by zero", "stop-and-rotate", "int(... + 0.5)"):
        assert word in hdr, word
    assert (C.sizeof(_lib.RolloutConfig), C.sizeof(_lib.RolloutPlan), C.sizeof(_lib.RolloutBest)) == (240, 2368, 64)
    assert (_lib.RolloutBest.cost.offset, _lib.RolloutBest.thetav.offset, _lib.RolloutPlan.lists.offset, _lib.RolloutConfig.y_vels.offset) == (16, 48, 320, 176)
    from gem_amd import build
    assert any(p.name == "gem_rollout.hip" for p in build.SOURCES) and any(p.name == "gem_capi_rollout.cpp" for p in build.SOURCES)
    assert {"gem_rollout.hpp", "gem_hip_rollout.h"} <= {p.name for p in build.HEADERS}


def test_the_header_is_c(tmp_path):
    """the plan's struct shares its name with the call that makes it: a C compiler takes the header as it is"""
    src = tmp_path / "c_header.c"
    src.write_text('#include "gem_hip.h"\n#include <stdio.h>\nint main(void){struct gem_rollout_plan p; gem_rollout_best b;'
                   'printf("%zu %zu %zu\\n", sizeof(gem_rollout_config), sizeof p, sizeof b);return 0;}\n')
    exe = tmp_path / "c_header"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["240", "2368", "64"]


def build_rollout_host(exe, extra=()):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *extra, str(ROOT / "tests" / "cpp" / "rollout_host.cpp"), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_the_stand_alone_twin(tmp_path):
    """gem_amd/csrc/gem_rollout.hpp by a plain C++ compiler, without HIP and without the library (tests/cpp/rollout_host.cpp)"""
    exe = build_rollout_host(tmp_path / "rollout_host")
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr


def build_rollout_check(exe):
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-I", str(ROOT / "tests" / "cpp" / "fake_eigen"),
           str(ROOT / "tests" / "cpp" / "rollout_check.cpp"), "-o", str(exe), f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_cpp_rollout_facade_host_part(tmp_path):
    """tests/cpp/rollout_check.cpp without a device: the plan, the host twin and the pick through gem.hpp"""
    _lib.load()
    exe = build_rollout_check(tmp_path / "rollout_check")
    res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.startswith("OK"), res.stdout + res.stderr
