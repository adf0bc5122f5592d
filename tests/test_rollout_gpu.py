"""Trajectory rollout on the device costmap (gem_costmap_rollout_best / _device) against the host twin (gem_rollout_host, itself pinned to
tests/rollout_ref.py by tests/test_rollout_cpu.py) and the restatement's answer.  Every comparison is exact: arrays by tobytes(), the
64-byte answer by its bytes.

  1. the device against the twin on every scene of the CPU test, both map sizes, with costs, host form and device form;
  2. group widths and raggedness: step counts 1 .. T for T = 1 .. 65 in one batch, 0 .. 32 vertices, 2 x 2 candidates and one count
     above a stride of the grid, output buffers pre-filled with a sentinel;
  3. early stops: a robot standing on a blocked cell (every candidate -1 at step 0), nothing reachable (every candidate -2);
  4. the enqueued cycle with no host wait before the 64 bytes, and no allocation in a second identical cycle;
  5. a stale grid after roll_to, and every refusal with nothing enqueued;
  6. the C++ facade (tests/cpp/rollout_check.cpp) as a child process."""
import ctypes as C
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import gem_amd
from gem_amd import ElevationMap, _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import footprint_ref as fref  # noqa: E402
import mapgrid_ref as mref  # noqa: E402
import rollout_ref as ref  # noqa: E402
from test_mapgrid_gpu import centre, device_copy  # noqa: E402
from test_rollout_cpu import DEFAULTS, ROUND32, SCENES, SENTINEL, TWO, at, build_rollout_check, reference, twin, world, world_plan  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
INV = _lib.GEM_OK - 1
MAX_BLOCKS, THREADS = 256, 256                                           # kRolloutMaxBlocks, kRolloutThreads of the kernel as built


@pytest.fixture(scope="module")
def emap():
    m = ElevationMap(32, 0.05)
    yield m
    m.close()


@pytest.fixture(scope="module")
def devices(emap):
    """the two maps on the device, their grids prepared: shared by the tests that change nothing"""
    out = {}
    for name in ("75", "130"):
        dev = device_copy(emap, world(name)[0])
        dev.prepare_map_grid(world_plan(name))
        out[name] = dev
    yield out
    for dev in out.values():
        dev.close()


def sentinel_form(emap, dev, plan, pos, vel, state, spec, flags, pad=8):
    """the _device entry into buffers pre-filled with a sentinel and `pad` entries too long: (answer bytes, costs, ahead) and the pads"""
    import torch
    nc = int(plan.n_cand)
    cost = torch.full((nc + pad,), SENTINEL, dtype=torch.float64, device="cuda:0")
    ahead = torch.full((nc + pad,), -7, dtype=torch.int32, device="cuda:0")
    best = torch.full((64 + pad,), 0xEE, dtype=torch.uint8, device="cuda:0")
    sp = np.ascontiguousarray(spec, np.float64).reshape(-1, 2)
    d3 = lambda v: (C.c_double * 3)(*[float(x) for x in v])
    rc = emap._lib.gem_costmap_rollout_best_device(emap._h, dev.id, C.byref(plan), d3(pos), d3(vel), state,
                                                   sp.ctypes.data_as(C.POINTER(C.c_double)) if sp.size else None, sp.shape[0], flags,
                                                   C.c_void_p(cost.data_ptr()), C.c_void_p(ahead.data_ptr()), C.c_void_p(best.data_ptr()))
    assert rc == 0
    emap.synchronize()
    cost, ahead, best = cost.cpu().numpy(), ahead.cpu().numpy(), best.cpu().numpy()
    assert (cost[nc:] == SENTINEL).all() and (ahead[nc:] == -7).all() and (best[64:] == 0xEE).all()
    return best[:64].tobytes(), cost[:nc], ahead[:nc]


def both_forms_equal(emap, dev, plan, pos, vel, state, spec, flags, want, what):
    """want = (answer bytes, costs, ahead) of the twin"""
    ans, cost, ahead = dev.rollout_best(plan, pos, vel, state, spec, flags, costs=True)                    # the host form
    assert cost.tobytes() == want[1].tobytes(), f"{what}: {int((cost.view(np.uint64) != want[1].view(np.uint64)).sum())} costs differ"
    assert ahead.tobytes() == want[2].tobytes(), f"{what}: {int((ahead != want[2]).sum())} ahead values differ"
    assert ans["bytes"] == want[0], (what, ans)
    assert dev.rollout_best(plan, pos, vel, state, spec, flags)["bytes"] == want[0]
    b, c, a = sentinel_form(emap, dev, plan, pos, vel, state, spec, flags)                                 # the device form
    assert c.tobytes() == want[1].tobytes() and a.tobytes() == want[2].tobytes() and b == want[0], what


# ---- 1. the device against the twin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_device_against_twin(emap, devices, name):
    which, pos, vel, cfg, state, spec, flags = SCENES[name]
    plan, (ans, cost, ahead, steps, poses) = twin(name)
    assert ans["bytes"] == reference(name)[0]["answer"]["bytes"]
    both_forms_equal(emap, devices[which], plan, pos, vel, state, spec, flags, (ans["bytes"], cost, ahead), name)
    import torch
    d_best = devices[which].rollout_best(plan, pos, vel, state, spec, flags, device=True)                 # the API's device form
    emap.synchronize()
    assert gem_amd.rollout_answer(d_best.cpu().numpy())["bytes"] == ans["bytes"] and d_best.dtype == torch.uint8


# ---- 2. group widths and raggedness ----------------------------------------------------------------------------------------------------------
def width_inputs(T):
    """T + 1 forward speeds whose num_steps are 1, 1, 2 .. T (sim_time 1, the granularity a hair above vmax / T, as
    test_trajgen_gpu.width_inputs), rotations of at most one step"""
    vmax = 0.5
    cfg = dict(TWO, sim_time=1.0, sim_granularity=vmax / T * 1.0005, angular_sim_granularity=1.5, max_vel_x=vmax, min_vel_x=0.0, acc_lim_x=100.0,
               vx_samples=T + 1 if T > 1 else 2, vtheta_samples=2, max_vel_th=0.6, min_vel_th=-0.6, min_in_place_vel_th=0.4, backup_vel=-0.1)
    return cfg, at("75", 22, 26, 1.0), (0.1, 0.0, 0.0)


@pytest.mark.parametrize("T", [1, 2, 7, 8, 9, 31, 32, 33, 64, 65])
def test_group_widths_and_raggedness(emap, devices, T):
    cm, path, goal = world("75")
    cfg, pos, vel = width_inputs(T)
    plan = gem_amd.rollout_plan(cfg, pos, vel, 0)
    assert plan.max_steps == T
    seen = set()
    for nv in (0, 3, 7, 8, 31, 32):
        spec = fref.regular_polygon(nv, 0.3) if nv else []
        ans, cost, ahead, steps = gem_amd.rollout_host(plan, pos, vel, cm.grid, cm.res, (cm.ox, cm.oy), path, goal, spec, 0)
        assert sorted(set(steps[cost >= 0].tolist())) == list(range(1, T + 1)) and (cost >= 0).all()        # every step count, every candidate to its end
        both_forms_equal(emap, devices["75"], plan, pos, vel, 0, spec, 0, (ans["bytes"], cost, ahead), f"T {T}, {nv} vertices")
        seen.add(cost.tobytes())
    assert len(seen) > 1 or T < 3                                                                         # (the footprint is part of the cost)


COUNTS = {7: (2, 2), 8254: (130, 63)}


@pytest.mark.parametrize("count", list(COUNTS))
def test_candidate_counts(emap, devices, count):
    """2 x 2, and 130 x 63 + 63 + 1 candidates of at most 8 steps and 4 vertices: more than one stride of the grid (256 workgroups of 32
    groups); the last candidates, beyond the first stride, among them"""
    cm, path, goal = world("75")
    nx, nth = COUNTS[count]
    cfg = dict(TWO, sim_time=1.0, sim_granularity=0.07, angular_sim_granularity=0.2, vx_samples=nx, vtheta_samples=nth, acc_lim_x=100.0, acc_lim_theta=100.0)
    pos, vel = at("75", 22, 26, -2.0), (0.2, 0.0, 0.0)
    plan = gem_amd.rollout_plan(cfg, pos, vel, 0)
    assert plan.n_cand == count and plan.max_steps <= 8
    if count > 1000:
        assert count > MAX_BLOCKS * (THREADS // 8)
    spec = fref.RECTANGLE
    ans, cost, ahead, steps = gem_amd.rollout_host(plan, pos, vel, cm.grid, cm.res, (cm.ox, cm.oy), path, goal, spec, 0)
    assert len(set(steps.tolist())) > 1 and (cost >= 0).any()
    both_forms_equal(emap, devices["75"], plan, pos, vel, 0, spec, 0, (ans["bytes"], cost, ahead), f"count {count}")


# ---- 3. early stops ------------------------------------------------------------------------------------------------------------------------------
def test_every_candidate_stops_at_step_zero(emap, devices):
    cm, path, goal = world("75")
    pos, vel = at("75", 16, 11, 0.3), (0.1, 0.0, 0.0)                     # the lethal patch's centre cell, a point robot
    assert cm.grid[int((pos[1] - cm.oy) / cm.res), int((pos[0] - cm.ox) / cm.res)] == 254
    plan = gem_amd.rollout_plan(DEFAULTS, pos, vel, 0)
    ans, cost, ahead, steps = gem_amd.rollout_host(plan, pos, vel, cm.grid, cm.res, (cm.ox, cm.oy), path, goal, [], 0)
    assert (cost == -1.0).all() and (steps == 0).all() and (ahead == -1).all() and (ans["stage"], ans["cost"], ans["raw_cost"]) == (3, 1.0, -1.0)
    both_forms_equal(emap, devices["75"], plan, pos, vel, 0, [], 0, (ans["bytes"], cost, ahead), "on a blocked cell")


def test_nothing_reachable(emap):
    cm, _, _ = world("75")
    off = [(cm.ox - 5.0, cm.oy - 5.0)]                                    # a plan off the map: nothing starts, both grids stay UN
    want = mref.grids(cm, off)
    assert want["started"] == 0 and (want["path"] == cm.size_x * cm.size_y + 1).all()
    pos, vel = at("75", 25, 25, 0.7), (0.2, 0.0, 0.1)
    plan = gem_amd.rollout_plan(DEFAULTS, pos, vel, 0)
    ans, cost, ahead, steps = gem_amd.rollout_host(plan, pos, vel, cm.grid, cm.res, (cm.ox, cm.oy), want["path"], want["goal"], fref.RECTANGLE, 0)
    assert (cost == -2.0).all() and (steps == 0).all() and (ans["stage"], ans["cost"], ans["raw_cost"]) == (3, -2.0, -2.0)
    dev = device_copy(emap, cm)
    try:
        dev.prepare_map_grid(off)
        both_forms_equal(emap, dev, plan, pos, vel, 0, fref.RECTANGLE, 0, (ans["bytes"], cost, ahead), "nothing reachable")
    finally:
        dev.close()


# ---- 4. no wait, no allocation ------------------------------------------------------------------------------------------------------------------
def test_the_enqueued_cycle_and_a_second_cycle_allocates_nothing(emap):
    which, pos, vel, cfg, state, spec, flags = SCENES["75 open"]
    want = reference("75 open")[0]["answer"]["bytes"]
    plan = gem_amd.rollout_plan(cfg, pos, vel, state)
    dev = device_copy(emap, world(which)[0])

    def cycle():
        dev.prepare_map_grid(world_plan(which))                           # only enqueued, like everything up to the answer
        d_best = dev.rollout_best(plan, pos, vel, state, spec, flags, device=True)
        emap.synchronize()                                                # the first host wait
        assert d_best.cpu().numpy().tobytes() == want

    try:
        cycle()
        a1 = emap.debug_get("arena_allocations")
        cycle()
        assert emap.debug_get("arena_allocations") == a1
        host = dev.rollout_best(plan, pos, vel, state, spec, flags, costs=True)                           # the host form: its staging once, then nothing
        a2 = emap.debug_get("arena_allocations")
        again = dev.rollout_best(plan, pos, vel, state, spec, flags, costs=True)
        assert again[0]["bytes"] == host[0]["bytes"] == want and again[1].tobytes() == host[1].tobytes() and emap.debug_get("arena_allocations") == a2
    finally:
        dev.close()


# ---- 5. stale grids and refusals ------------------------------------------------------------------------------------------------------------------
def test_stale_grids_and_every_refusal():
    import torch
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    which, pos, vel, cfg, state, spec, flags = SCENES["75 open"]
    cm, path, goal = world(which)
    want = reference("75 open")[0]
    plan = gem_amd.rollout_plan(cfg, pos, vel, state)
    nc = int(plan.n_cand)
    nan = float("nan")
    d3 = lambda v: None if v is None else (C.c_double * 3)(*v)
    sp = np.ascontiguousarray(spec, np.float64)
    d_cost = torch.full((nc,), SENTINEL, dtype=torch.float64, device="cuda:0")
    d_ahead = torch.full((nc,), -7, dtype=torch.int32, device="cuda:0")
    d_best = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda:0")
    cost, ahead = np.full(nc, SENTINEL), np.full(nc, -7, np.int32)
    hbest = _lib.RolloutBest(-9, -9, -9, -9.0, -9.0, -9.0, -9.0, -9.0, -9)
    P = lambda t: C.c_void_p(t.data_ptr())
    dev = device_copy(m, cm)

    def tampered(**kw):
        q = _lib.RolloutPlan.from_buffer_copy(plan)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def call(p=plan, id_=None, pos_=pos, vel_=vel, st=state, sp_=sp, nv=4, fl=flags, device=False, handle=h, library=lib, b=True):
        fn = library.gem_costmap_rollout_best_device if device else library.gem_costmap_rollout_best
        out_b = (P(d_best) if device else C.byref(hbest)) if b else None
        return fn(handle, dev.id if id_ is None else id_, C.byref(p) if p is not None else None, d3(pos_), d3(vel_), st,
                  sp_.ctypes.data_as(C.POINTER(C.c_double)) if sp_ is not None else None, nv, fl,
                  P(d_cost) if device else cost.ctypes.data_as(C.c_void_p), P(d_ahead) if device else ahead.ctypes.data_as(C.c_void_p), out_b)

    def both(**kw):
        return call(**kw) == INV and call(device=True, **kw) == INV

    try:
        assert both()                                                     # the grids were never prepared
        dev.prepare_map_grid(world_plan(which), _lib.MAPGRID_PATH)
        assert both()                                                     # ... GOAL still was not
        dev.prepare_map_grid(world_plan(which))
        bad_plans = [tampered(n_cand=nc + 1), tampered(max_steps=plan.max_steps + 1), tampered(off_b=plan.off_b - 1), tampered(n_vth=2), tampered(dvth=0.0),
                     tampered(state_flags=ref.ESCAPING), tampered(max_th=plan.max_th + 0.5)]
        q = tampered()
        q.lists[3] = nan
        bad_plans.append(q)
        for key, v in (("sim_time", 0.0), ("sim_granularity", -1.0), ("angular_sim_granularity", 0.0), ("sim_period", 0.0), ("sim_time", nan),
                       ("pdist_scale", -1.0), ("gdist_scale", nan), ("occdist_scale", -0.0), ("vx_samples", 1), ("vtheta_samples", 1), ("n_y_vels", 9)):
            q = tampered()
            setattr(q.config, key, v)
            bad_plans.append(q)
        q = tampered()
        q.config.y_vels[1] = 0.0
        bad_plans.append(q)
        for q in bad_plans:
            assert both(p=q)
        for kw in (dict(p=None), dict(pos_=None), dict(vel_=None), dict(b=False), dict(pos_=(pos[0], nan, 0.0)), dict(vel_=(float("inf"), 0.0, 0.0)),
                   dict(vel_=(vel[0], vel[1], vel[2] + 0.25)), dict(st=state | ref.STUCK_LEFT), dict(st=32), dict(st=ref.ESCAPING),
                   dict(pos_=(pos[0], pos[1], 64 * math.pi)), dict(sp_=None), dict(nv=33), dict(nv=-1), dict(fl=2), dict(fl=8),
                   dict(id_=-1), dict(id_=5), dict(id_=8)):
            assert both(**kw), kw
        bad_spec = sp.copy()
        bad_spec[1, 0] = nan
        assert both(sp_=bad_spec)
        fresh = m.costmap(75, 75, 0.2, cm.ox, cm.oy, 0)                    # a costmap whose grids were never prepared
        try:
            assert both(id_=fresh.id)
        finally:
            fresh.close()
        w2 = ElevationMap(32, 0.05)                                       # a handle with a communicator
        w2.comm_init_loopback(9547, 1, 0, tile_strips=False)
        assert both(handle=w2._h, library=w2._lib, id_=0)
        w2.close()
        # nothing was enqueued or written by any refusal
        m.synchronize()
        assert (d_cost.cpu() == SENTINEL).all() and (d_ahead.cpu() == -7).all() and (d_best.cpu() == 0xEE).all()
        assert (cost == SENTINEL).all() and (ahead == -7).all() and (hbest.index, hbest.stage, hbest.cost, hbest.reserved1) == (-9, -9, -9.0, -9)
        # ... and the same calls, unbroken, answer
        assert call() == 0 and call(device=True) == 0
        m.synchronize()
        assert cost.tobytes() == want["cost"].tobytes() and ahead.tobytes() == want["ahead"].tobytes() and bytes(hbest) == want["answer"]["bytes"]
        assert d_cost.cpu().numpy().tobytes() == want["cost"].tobytes() and d_best.cpu().numpy().tobytes() == want["answer"]["bytes"]
        # a roll that moves the map makes both grids stale until they are prepared again
        sizes = cm.size_in_meters()
        dev.roll_to(cm.ox + sizes[0] / 2 + 7 * cm.res, cm.oy + sizes[1] / 2 - 4 * cm.res)
        assert both()
        dev.prepare_map_grid(world_plan(which), _lib.MAPGRID_GOAL)
        assert both()                                                     # PATH is still the old one
        dev.prepare_map_grid(world_plan(which), _lib.MAPGRID_PATH)
        assert call() == 0
    finally:
        dev.close()
        m.close()


# ---- 6. the C++ facade ---------------------------------------------------------------------------------------------------------------------------
def test_cpp_rollout_facade(tmp_path):
    exe = build_rollout_check(tmp_path / "rollout_check")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
