"""DWA's sampled trajectories on the device (gem_trajgen_generate_device, gem_costmap_dwa_best / _device) against the host twin
(gem_trajgen_generate, itself pinned to tests/trajgen_ref.py by tests/test_trajgen_cpu.py) and against the restatements.  Every
comparison is exact: arrays by tobytes(), the winner's index and the valid count as integers, its cost by its bytes.

  1. the kernel against the twin with every sample generated: use_dwa and continued acceleration, by time and by distance, a vy list,
     lists 3 x 1 x 5 and 7 x 3 x 11 with an inserted zero, a start yaw near +-pi;
  2. group widths and slots: poses_per_traj 1 .. 65 with num_steps 0 .. T, sample counts 1, 63, 64, 65 and one above a stride of the
     grid, buffers pre-filled with a sentinel;
  3. the six oscillation bits, each alone, against samples of both signs and zero; twirling of -0.0;
  4. dwa_best on the 75 x 75 noise map against critics_ref over trajgen_ref's trajectories, and the winner's velocity;
  5. the enqueued cycle with no host wait before the answer, and no allocation in a second identical cycle;
  6. every refusal, with the outputs untouched;
  7. the C++ facade (tests/cpp/trajgen_check.cpp) as a child process."""
import ctypes as C
import functools
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import gem_amd
from gem_amd import ElevationMap, _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import critics_ref as cref  # noqa: E402
import trajgen_ref as ref  # noqa: E402
from test_critics_cpu import as_c  # noqa: E402
from test_critics_gpu import CLEARED, SMALL, centre, parity_case, prepared, rejected_by  # noqa: E402
from test_trajgen_cpu import CONFIG, GOAL, LIMITS, build_trajgen_check  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
INV = _lib.GEM_OK - 1
FREE = dict(LIMITS, min_vel_trans=-1.0, max_vel_trans=-1.0)              # no sample is dropped
SENTINEL = -77.0
MAX_BLOCKS, THREADS = 1024, 256                                          # kTrajgenMaxBlocks, kTrajgenThreads of the kernel as built


@pytest.fixture(scope="module")
def emap():
    m = ElevationMap(32, 0.05)
    yield m
    m.close()


def on_device(m, plan, pos, vel, T, fill=SENTINEL):
    out = gem_amd.generate_trajectories(plan, pos, vel, T, elevation_map=m, fill=fill)       # only enqueued
    m.synchronize()
    return [t.cpu().numpy() for t in out]


def same_as_twin(m, limits, config, pos, vel, T=None, what=""):
    """the kernel's four arrays equal the twin's, both written over the sentinel: (plan, the twin's arrays)"""
    plan = gem_amd.trajgen_plan(limits, config, pos, vel, GOAL)
    T = max(plan.max_steps, 1) if T is None else T
    want = gem_amd.generate_trajectories(plan, pos, vel, T, fill=SENTINEL)
    got = on_device(m, plan, pos, vel, T)
    for g, w, name in zip(got, want, ("poses", "lengths", "external columns", "velocities")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert g.tobytes() == w.tobytes(), f"{what}: {name} differ in {int((g != w).sum())} places"
    return plan, want


# ---- 1. the kernel against the twin -------------------------------------------------------------------------------------------------------
PARITY = {
    "dwa by distance 3x1x5": (dict(FREE, max_vel_y=0.0, min_vel_y=0.0), dict(CONFIG, vsamples=(3, 1, 4)), (1.0, 2.0, 0.3), (0.2, 0.0, 0.1), (3, 1, 5)),
    "dwa by time 7x3x11": (FREE, dict(CONFIG, vsamples=(7, 3, 10), discretize_by_time=True), (-4.0, 7.5, -1.2), (0.3, 0.02, 0.1), (7, 3, 11)),
    "continued by distance": (dict(FREE, min_vel_x=0.05), dict(CONFIG, use_dwa=False, continued_acceleration=True, vsamples=(7, 3, 10)), (1.0, 2.0, 0.3), (0.3, 0.05, -0.3), (7, 3, 11)),
    "continued by time": (FREE, dict(CONFIG, use_dwa=False, continued_acceleration=True, discretize_by_time=True, vsamples=(3, 3, 4)), (1.0, 2.0, 2.5), (0.1, -0.05, 0.4), (3, 3, 5)),
    "yaw near -pi": (FREE, dict(CONFIG, vsamples=(3, 3, 4)), (-4.0, 7.5, -3.1415925), (0.3, 0.0, -0.1), (3, 3, 5)),
    "yaw near +pi": (dict(FREE, min_vel_x=0.05), dict(CONFIG, vsamples=(7, 3, 10)), (120.5, -80.25, 3.1415925), (0.1, 0.02, 0.1), (7, 3, 11)),
}


@pytest.mark.parametrize("name", list(PARITY))
def test_device_against_twin(emap, name):
    limits, config, pos, vel, counts = PARITY[name]
    plan, (poses, lens, ext, vels) = same_as_twin(emap, limits, config, pos, vel, what=name)
    assert (plan.n_x, plan.n_y, plan.n_th) == counts and (lens > 0).all()                       # every sample is active
    x, y, th = gem_amd.plan_lists(plan)
    assert int((th == 0).sum()) == 1 and th.min() < 0 < th.max()                                # the inserted zero
    if counts[1] > 1:
        assert (y != 0).any()
    if "yaw" in name:                                                                          # the heading crosses +-pi on the way
        s = poses.reshape(int(plan.n_traj), -1, 4)[:, :, 3]
        assert (s[lens > 2, 0] * np.array([s[t, lens[t] - 1] for t in range(len(lens)) if lens[t] > 2]) < 0).any()
    if config["continued_acceleration"]:
        assert (vels != np.array([[a, b, c] for a in x for b in y for c in th], np.float32)).any()      # (xv, yv, thetav) is not the sample


# ---- 2. group widths and slot handling ---------------------------------------------------------------------------------------------------
def width_inputs(T):
    """T + 1 forward speeds whose num_steps are 0 .. T (by distance, sim_time 1, the granularity a hair above vmax / T), three rotations
    of which the outer two give the standing sample one step: lengths 0 .. T all occur"""
    vmax = 0.5
    limits = dict(FREE, max_vel_x=vmax, min_vel_x=0.0, max_vel_y=0.0, min_vel_y=0.0, acc_lim_x=100.0, acc_lim_theta=2.0, max_vel_theta=1.0)
    config = dict(CONFIG, sim_time=1.0, sim_granularity=vmax / T * 1.0005, angular_sim_granularity=1.0, vsamples=(T + 1, 1, 3))
    return limits, config, (0.5, -0.25, 1.0), (0.1, 0.0, 0.0)


@pytest.mark.parametrize("T", [1, 2, 7, 8, 9, 31, 32, 33, 64, 65])
def test_group_widths_and_slots(emap, T):
    limits, config, pos, vel = width_inputs(T)
    plan, (poses, lens, ext, vels) = same_as_twin(emap, limits, config, pos, vel, T=T, what=f"T {T}")
    assert plan.max_steps == T and plan.n_traj == (T + 1 if T > 1 else 2) * 3
    assert sorted(set(lens.tolist())) == list(range(T + 1))                                     # num_steps 0 (not generated) and 1 .. T
    p = poses.reshape(int(plan.n_traj), T, 4)
    for t, n in enumerate(lens.tolist()):
        assert (p[t, n:] == SENTINEL).all() and (p[t, :n] != SENTINEL).any(axis=1).all()        # slots past the length keep the sentinel
    assert (ext != SENTINEL).all() and (vels != SENTINEL).all()                                 # ... the scores of a sample not generated are written
    # more slots than any sample needs
    same_as_twin(emap, limits, config, pos, vel, T=T + 3, what=f"T {T} + 3")


COUNTS = {1: (1, 1, 1), 63: (7, 3, 3), 64: (8, 8, 1), 65: (13, 5, 1), 33792: (33, 32, 32)}


@pytest.mark.parametrize("count", list(COUNTS))
def test_sample_counts(emap, count):
    """lists on the positive side (nothing inserted), so the counts are exact; 33 792 trajectories of up to 4 poses are more than one
    stride of the grid (1024 workgroups of 32 groups)"""
    nx, ny, nth = COUNTS[count]
    limits = dict(FREE, max_vel_x=0.5, min_vel_x=0.1 if nx > 1 else 0.5, max_vel_y=0.05, min_vel_y=0.01 if ny > 1 else 0.05, acc_lim_x=100.0, acc_lim_y=100.0,
                  acc_lim_theta=2.0 if nth > 1 else 0.0)
    config = dict(CONFIG, sim_time=1.0, sim_granularity=0.13, angular_sim_granularity=0.1, vsamples=(nx, ny, nth))
    pos, vel = (2.0, 3.0, -0.7), (0.3, 0.03, 0.2)
    plan, (poses, lens, ext, vels) = same_as_twin(emap, limits, config, pos, vel, what=f"count {count}")
    assert plan.n_traj == count and (plan.n_x, plan.n_y, plan.n_th) == (nx, ny, nth) and 1 <= plan.max_steps <= 8 and (lens > 0).all()
    if count > 1000:
        assert count > MAX_BLOCKS * (THREADS // 8) and len(set(lens.tolist())) > 1
        last = poses.reshape(count, -1, 4)[-1]
        assert (last[:lens[-1]] != SENTINEL).all()                                              # the last sample, beyond the first stride


# ---- 3. the velocity-only critics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit", [1, 2, 4, 8, 16, 32])
def test_oscillation_flags(emap, bit):
    limits = dict(FREE, max_vel_x=0.2, min_vel_x=-0.2, max_vel_y=0.1, min_vel_y=-0.1, acc_lim_x=100.0, acc_lim_y=100.0, acc_lim_theta=4.0)
    config = dict(CONFIG, discretize_by_time=True, sim_granularity=0.5, vsamples=(3, 3, 3), oscillation_flags=bit)
    pos, vel = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
    plan, (poses, lens, ext, vels) = same_as_twin(emap, limits, config, pos, vel, what=f"bit {bit}")
    assert plan.n_traj == 27 and {np.sign(v) for v in vels[:, 0]} == {np.sign(v) for v in vels[:, 2]} == {-1.0, 0.0, 1.0}
    axis, negative = {1: (0, True), 2: (0, False), 4: (1, True), 8: (1, False), 16: (2, True), 32: (2, False)}[bit]
    fires = vels[:, axis] < 0 if negative else vels[:, axis] > 0
    assert ext[0].tolist() == np.where(fires, -5.0, 0.0).tolist() and int(fires.sum()) == 9
    want = ref.generate(limits, config, pos, vel, GOAL, plan.max_steps, fill=SENTINEL)
    assert ext.tobytes() == want[2].tobytes() and vels.tobytes() == want[3].tobytes()


def test_twirling_of_minus_zero(emap):
    limits = dict(FREE, max_vel_x=0.2, min_vel_x=0.2, max_vel_y=0.0, min_vel_y=0.0, acc_lim_theta=0.0)
    config = dict(CONFIG, vsamples=(1, 1, 1), oscillation_flags=16 | 32)
    pos, vel = (0.0, 0.0, 0.0), (0.2, 0.0, -0.0)
    plan, (poses, lens, ext, vels) = same_as_twin(emap, limits, config, pos, vel, what="-0.0")
    assert plan.n_traj == 1 and vels[0, 2] == 0 and np.signbit(vels[0, 2])                      # the only rotation sample is -0.0
    assert ext[:, 0].tobytes() == np.array([0.0, 0.0]).tobytes()                                # no bit fires on it, and fabs gives +0.0
    assert ext.tobytes() == ref.generate(limits, config, pos, vel, GOAL, plan.max_steps)[2].tobytes()


# ---- 4. dwa_best against the restatements ---------------------------------------------------------------------------------------------------
DWA_CONFIG = dict(CONFIG, oscillation_flags=16, vsamples=(6, 3, 9))
DWA_VEL = (0.1, 0.0, 0.1)


@functools.lru_cache(maxsize=None)
def dwa_case():
    """the 75 x 75 noise map with the cleared region of test_critics_gpu.parity_case, the robot nine cells in front of its lethal patch and
    heading for it: (pos, T, trajgen_ref's arrays, totals, (index, cost, n_valid), per trajectory the rejecting critic)"""
    c = parity_case("75x75")
    rows, cols = CLEARED["75x75"]
    x, y = centre(c["cm"], cols.start + 9, rows.start + 11)
    pos = (x, y, 0.0)
    T = ref.max_steps(LIMITS, DWA_CONFIG, ref.lists(LIMITS, DWA_CONFIG, pos, DWA_VEL, GOAL))
    poses, lens, ext, vels = ref.generate(LIMITS, DWA_CONFIG, pos, DWA_VEL, GOAL, T)
    critics = cref.dwa_list()
    table = cref.score_table(c["cm"], c["grids"], critics, poses, T, SMALL, ext, lens)
    totals = cref.combine(critics, table, lens, T)
    for a in (poses, lens, ext, vels, totals):
        a.setflags(write=False)
    return pos, T, (poses, lens, ext, vels), totals, cref.find_best(totals), rejected_by(critics, table)


def test_dwa_best_against_the_restatements(emap):
    import torch
    c = parity_case("75x75")
    pos, T, (poses, lens, ext, vels), totals, best, by = dwa_case()
    # the case cannot pass empty: asserted on the restatements' output alone
    generated = lens > 0
    assert int((~generated).sum()) >= 1 and best[2] >= 1 and int(((by == 1) & generated).sum()) >= 1 and int(((by == 0) & generated).sum()) >= 1
    assert best[0] > 0 and (totals[~generated] == -5.0).all() and best[2] == int((totals >= 0).sum()) < int(generated.sum())
    critics = cref.dwa_list()
    cs = as_c(critics)[:len(critics)]
    plan = gem_amd.trajgen_plan(LIMITS, DWA_CONFIG, pos, DWA_VEL, GOAL)
    assert plan.max_steps == T and plan.n_traj == lens.size
    dev = prepared(emap, c)
    try:
        i, cost, n_valid, tot = dev.dwa_best(cs, plan, pos, DWA_VEL, T, SMALL, totals=True)                  # the host form
        assert tot.tobytes() == totals.tobytes(), f"{int((tot.view(np.uint64) != totals.view(np.uint64)).sum())} totals differ"
        assert (i, np.float64(cost).tobytes(), n_valid) == (best[0], np.float64(best[1]).tobytes(), best[2])
        assert dev.dwa_best(cs, plan, pos, DWA_VEL, T, SMALL) == (i, cost, n_valid)
        d_best, d_tot = dev.dwa_best(cs, plan, pos, DWA_VEL, T + 2, SMALL, totals=True, device=True)        # only enqueued; two spare slots
        emap.synchronize()
        b = d_best.cpu()
        assert d_tot.cpu().numpy().tobytes() == totals.tobytes()
        assert (int(b[0]), np.float64(float(b.view(torch.float64)[2])).tobytes(), int(b[1]), int(b[3])) == (best[0], np.float64(best[1]).tobytes(), best[2], 0)
        # the winner's velocity from the twin, by the index alone
        assert np.array(gem_amd.trajectory_velocity(plan, DWA_VEL, int(b[0])), np.float32).tobytes() == vels[best[0]].tobytes()
        # an external critic's column 0 / 1 is the generated column
        only = [cref.external(1.0, 1)]
        got = dev.dwa_best(as_c(only)[:1], plan, pos, DWA_VEL, T, SMALL, totals=True)
        want = cref.combine(only, ext[1:2], lens, T)
        assert got[3].tobytes() == want.tobytes() and got[:3] == cref.find_best(want)
    finally:
        dev.close()


# ---- 5. no wait, no allocation ---------------------------------------------------------------------------------------------------------------
def test_the_enqueued_cycle_and_a_second_cycle_allocates_nothing(emap):
    import torch
    c = parity_case("75x75")
    pos, T, _, totals, best, _ = dwa_case()
    critics = cref.dwa_list()
    cs = as_c(critics)[:len(critics)]
    plan = gem_amd.trajgen_plan(LIMITS, DWA_CONFIG, pos, DWA_VEL, GOAL)
    dev = prepared(emap, c)

    def cycle():
        dev.prepare_map_grid(c["plan"])                                    # only enqueued, like everything up to the answer
        dev.prepare_map_grid_front(c["front"])
        d_best = dev.dwa_best(cs, plan, pos, DWA_VEL, T, SMALL, device=True)
        emap.synchronize()                                                 # the first host wait
        b = d_best.cpu()
        assert (int(b[0]), np.float64(float(b.view(torch.float64)[2])).tobytes(), int(b[1])) == (best[0], np.float64(best[1]).tobytes(), best[2])

    try:
        cycle()
        a1 = emap.debug_get("arena_allocations")
        cycle()
        assert emap.debug_get("arena_allocations") == a1
        host = dev.dwa_best(cs, plan, pos, DWA_VEL, T, SMALL)              # the host form: its staging once, then nothing
        a2 = emap.debug_get("arena_allocations")
        assert dev.dwa_best(cs, plan, pos, DWA_VEL, T, SMALL) == host and emap.debug_get("arena_allocations") == a2
    finally:
        dev.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_outputs_untouched():
    import torch
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    c = parity_case("75x75")
    pos, T, _, totals, best, _ = dwa_case()
    dev = prepared(m, c)
    dwa = cref.dwa_list()
    plan = gem_amd.trajgen_plan(LIMITS, DWA_CONFIG, pos, DWA_VEL, GOAL)
    nt = int(plan.n_traj)
    nan = float("nan")
    f3 = lambda v: (C.c_float * 3)(*v)
    spec = np.ascontiguousarray(SMALL, np.float64)
    d_poses = torch.full((nt * T, 4), SENTINEL, dtype=torch.float64, device="cuda:0")
    d_lens = torch.full((nt,), -7, dtype=torch.int32, device="cuda:0")
    d_ext = torch.full((2, nt), SENTINEL, dtype=torch.float64, device="cuda:0")
    d_vel = torch.full((nt, 3), SENTINEL, dtype=torch.float32, device="cuda:0")
    d_tot = torch.full((nt,), -99.0, dtype=torch.float64, device="cuda:0")
    d_best = torch.full((4,), -9, dtype=torch.int64, device="cuda:0")
    tot = np.full(nt, -99.0)
    hbest = _lib.BestTrajectory(-9, -9, -9.0, -9)
    P = lambda t: C.c_void_p(t.data_ptr())

    def tampered(**kw):
        q = _lib.DwaPlan.from_buffer_copy(plan)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def gen(p=plan, pos_=pos, vel_=DWA_VEL, T_=T, poses=d_poses, lens=d_lens, ext=d_ext, handle=h, library=lib):
        return library.gem_trajgen_generate_device(handle, C.byref(p) if p is not None else None, f3(pos_) if pos_ is not None else None,
                                                   f3(vel_) if vel_ is not None else None, P(poses) if poses is not None else None,
                                                   P(lens) if lens is not None else None, P(ext) if ext is not None else None, P(d_vel), T_)

    def dwa_best(critics=dwa, id_=None, n_critics=None, p=plan, pos_=pos, vel_=DWA_VEL, T_=T, sp=spec, nv=4, device=False, handle=h, library=lib, b=True):
        cs = as_c(critics) if critics is not None else None
        fn = library.gem_costmap_dwa_best_device if device else library.gem_costmap_dwa_best
        out_b = (P(d_best) if device else C.byref(hbest)) if b else None
        return fn(handle, dev.id if id_ is None else id_, cs, (len(critics) if critics is not None else 1) if n_critics is None else n_critics,
                  C.byref(p) if p is not None else None, f3(pos_) if pos_ is not None else None, f3(vel_) if vel_ is not None else None, T_,
                  sp.ctypes.data_as(C.POINTER(C.c_double)) if sp is not None else None, nv,
                  P(d_tot) if device else tot.ctypes.data_as(C.c_void_p), out_b)

    def with_(k, **kw):
        cs = [dict(x) for x in dwa]
        cs[k].update(kw)
        return cs

    try:
        bad_plans = [tampered(n_traj=nt + 1), tampered(max_steps=T - 1), tampered(n_th=plan.n_th + 1), tampered(n_x=-1)]
        q = tampered()
        q.samples[1] = nan
        bad_plans.append(q)
        for key, v in (("sim_time", 0.0), ("sim_granularity", -1.0), ("angular_sim_granularity", 0.0), ("sim_period", 0.0), ("sim_time", nan)):
            q = tampered()
            setattr(q.config, key, v)
            bad_plans.append(q)
        q = tampered()
        q.limits.acc_lim_x = float("inf")
        bad_plans.append(q)
        q = tampered()
        q.config.oscillation_flags = 64
        bad_plans.append(q)
        for q in bad_plans:
            assert gen(p=q) == INV and dwa_best(p=q) == INV and dwa_best(p=q, device=True) == INV
        for kw in (dict(p=None), dict(pos_=None), dict(vel_=None), dict(T_=T - 1), dict(T_=0), dict(T_=(1 << 20) + 1),
                   dict(pos_=(pos[0], nan, 0.0)), dict(vel_=(float("inf"), 0.0, 0.0)),
                   dict(pos_=(pos[0], pos[1], 64 * math.pi)), dict(pos_=(pos[0], pos[1], -199.5)), dict(vel_=(0.1, 0.0, 118.0))):      # ... the 64 pi bound
            assert gen(**kw) == INV and dwa_best(**kw) == INV and dwa_best(device=True, **kw) == INV, kw
        assert gen(poses=None) == INV and gen(lens=None) == INV and gen(ext=None) == INV
        big = gem_amd.trajgen_plan(FREE, dict(CONFIG, vsamples=(80, 80, 80), discretize_by_time=True), pos, DWA_VEL, GOAL)
        assert big.n_traj * (1 << 20) > 2 ** 31 - 2 and gen(p=big, T_=1 << 20) == INV and dwa_best(p=big, T_=1 << 20) == INV      # more than 2^31 - 2 pose slots
        # the cases of best_trajectory that apply
        for bad in (-1, 5, 8):
            assert dwa_best(id_=bad) == INV
        assert dwa_best(critics=None) == INV and dwa_best(n_critics=0) == INV and dwa_best(critics=[dwa[0]] * 9) == INV and dwa_best(b=False) == INV
        assert dwa_best(with_(1, kind=0)) == INV and dwa_best(with_(1, kind=4)) == INV and dwa_best(with_(2, grid=3)) == INV
        assert dwa_best(with_(1, flags=8)) == INV and dwa_best(with_(0, flags=1)) == INV and dwa_best(with_(1, scale=-1.0)) == INV and dwa_best(with_(2, xshift=nan)) == INV
        assert dwa_best(with_(6, column=2)) == INV and dwa_best(with_(0, column=-1)) == INV            # two generated columns, no more
        assert dwa_best(critics=[dwa[1], dwa[1]]) == INV and dwa_best(nv=33) == INV and dwa_best(sp=None) == INV
        assert dwa_best(with_(1, scale=-1.0), device=True) == INV and dwa_best(with_(2, grid=3), device=True) == INV
        fresh = m.costmap(75, 75, 0.05, 0.0, 0.0, 0)                                                    # a costmap whose grids were never prepared
        try:
            assert dwa_best(id_=fresh.id) == INV
        finally:
            fresh.close()
        w2 = ElevationMap(32, 0.05)                                                                    # a handle with a communicator
        w2.comm_init_loopback(9546, 1, 0, tile_strips=False)
        assert gen(handle=w2._h, library=w2._lib) == INV
        assert dwa_best(handle=w2._h, library=w2._lib, id_=0) == INV and dwa_best(handle=w2._h, library=w2._lib, id_=0, device=True) == INV
        w2.close()
        # nothing was enqueued or written by any refusal
        m.synchronize()
        assert (d_poses.cpu() == SENTINEL).all() and (d_lens.cpu() == -7).all() and (d_ext.cpu() == SENTINEL).all() and (d_vel.cpu() == SENTINEL).all()
        assert d_tot.cpu().tolist() == [-99.0] * nt and d_best.cpu().tolist() == [-9] * 4
        assert tot.tolist() == [-99.0] * nt and (hbest.index, hbest.n_valid, hbest.cost, hbest.reserved) == (-9, -9, -9.0, -9)
        # ... and the same calls, unbroken, answer
        assert gen() == 0 and dwa_best() == 0 and dwa_best(device=True) == 0
        m.synchronize()
        assert tot.tobytes() == totals.tobytes() and d_tot.cpu().numpy().tobytes() == totals.tobytes()
        assert (hbest.index, hbest.n_valid) == (best[0], best[2]) and d_best.cpu().tolist()[:2] == [best[0], best[2]]
        assert (d_lens.cpu().numpy() == dwa_case()[2][1]).all()
        empty = gem_amd.trajgen_plan(LIMITS, dict(DWA_CONFIG, vsamples=(0, 3, 3)), pos, DWA_VEL, GOAL)       # no samples: valid, no winner
        assert dwa_best(p=empty) == 0 and (hbest.index, hbest.cost, hbest.n_valid) == (-1, -1.0, 0)
    finally:
        dev.close()
        m.close()


# ---- 7. the C++ facade ---------------------------------------------------------------------------------------------------------------------
def test_cpp_trajgen_facade(tmp_path):
    exe = build_trajgen_check(tmp_path / "trajgen_check")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
