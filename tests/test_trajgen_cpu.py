"""CPU tests of the trajectory-generation contract of include/gem_hip_trajgen.h: the restatement (tests/trajgen_ref.py) on cases with
known answers, the host twin of the kernel (gem_trajgen_plan / _generate / _velocity / _sincos) against the restatement bit for bit,
the contract's cosine against libm, the recurrence against its libm form, every refusal, and the ABI.  No GPU."""
import ctypes as C
import math
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import trajgen_ref as ref  # noqa: E402

EPS = 1e-4
LIMITS = dict(max_vel_x=0.55, min_vel_x=0.0, max_vel_y=0.1, min_vel_y=-0.1, max_vel_theta=1.0, min_vel_theta=0.4, max_vel_trans=0.55,
              min_vel_trans=0.1, acc_lim_x=2.5, acc_lim_y=2.5, acc_lim_theta=3.2)
CONFIG = dict(sim_time=1.7, sim_granularity=0.025, angular_sim_granularity=0.1, sim_period=0.05, use_dwa=True, discretize_by_time=False,
              continued_acceleration=False, oscillation_flags=0, vsamples=(6, 3, 20))
POS, VEL, GOAL = (1.0, 2.0, 0.3), (0.2, 0.0, 0.1), (3.0, 3.5)


def f32(x):
    return ref.f32(x)


@pytest.fixture(scope="module")
def lib():
    from gem_amd import _lib
    return _lib.load()


def twin(limits, config, pos, vel, goal=GOAL, T=None, fill=0.0):
    """(plan, poses, lens, ext, vels) of the host twin"""
    import gem_amd
    plan = gem_amd.trajgen_plan(limits, config, pos, vel, goal)
    return (plan,) + gem_amd.generate_trajectories(plan, pos, vel, max(plan.max_steps, 1) if T is None else T, fill=fill)


def both(limits, config, pos=POS, vel=VEL, goal=GOAL, T=None):
    """the twin's output, after it has been found equal to the restatement's byte for byte (the lists and max_steps too)"""
    import gem_amd
    plan, poses, lens, ext, vels = twin(limits, config, pos, vel, goal, T)
    ls = ref.lists(limits, config, pos, vel, goal)
    got = gem_amd.plan_lists(plan)
    assert [len(v) for v in ls] == [plan.n_x, plan.n_y, plan.n_th] and plan.n_traj == len(ls[0]) * len(ls[1]) * len(ls[2])
    for a, b in zip(got, ls):
        assert a.tobytes() == np.array(b, np.float32).tobytes()
    assert plan.max_steps == ref.max_steps(limits, config, ls)
    want = ref.generate(limits, config, pos, vel, goal, max(plan.max_steps if T is None else T, 1))
    if plan.n_traj:
        for g, w, name in zip((poses, lens, ext, vels), want, ("poses", "lengths", "external columns", "velocities")):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
    return plan, poses, lens, ext, vels


def single(sample, limits=None, config=None, **kw):
    """limits / config whose lists are the one sample (x, y, theta), float32 values: windows with min == max"""
    L = dict(LIMITS if limits is None else limits)
    L.update(max_vel_x=sample[0], min_vel_x=sample[0], max_vel_y=sample[1], min_vel_y=sample[1], max_vel_theta=100.0, acc_lim_theta=0.0)
    c = dict(CONFIG if config is None else config, vsamples=(1, 1, 1))
    L.update({k: v for k, v in kw.items() if k in L})
    c.update({k: v for k, v in kw.items() if k in c})
    return L, c, tuple(sample)                    # the velocity: inside every window, and theta's collapses onto vel[2] with acc_lim_theta = 0


# ---- the cosine -----------------------------------------------------------------------------------------------------------------------
def test_the_contracts_cosine_against_libm():
    import gem_amd
    rng = np.random.default_rng(20261019)
    special = [0.0, -0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi]
    special += [float(np.float32(v)) for v in special] + [float(np.nextafter(np.float32(v), np.float32(s))) for v in special[2:] for s in (-10, 10)]
    angles = np.concatenate([rng.uniform(-64 * math.pi, 64 * math.pi, 200000), rng.uniform(-math.pi, math.pi, 100000), np.array(special),
                             rng.uniform(-64 * math.pi, 64 * math.pi, 20000).astype(np.float32).astype(np.float64)])
    s, c = gem_amd.contract_sincos(angles)
    rs, rc = ref.sincos_array(angles)
    assert s.tobytes() == rs.tobytes() and c.tobytes() == rc.tobytes()              # twin and restatement: to the bit
    for i in list(range(0, angles.size, 997)) + list(range(300000, 300000 + len(special))):       # ... and the scalar form of the restatement
        assert ref.sincos(float(angles[i])) == (float(s[i]), float(c[i]))
    ms = np.array([math.sin(float(a)) for a in angles])
    mc = np.array([math.cos(float(a)) for a in angles])
    worst = max(float(np.abs(s - ms).max()), float(np.abs(c - mc).max()))
    print(f"largest difference to libm: {worst / 2.0 ** -53:.2f} * 2^-53 over {angles.size} angles")
    assert worst <= 2.0 ** -52
    assert ref.sincos(0.0) == (0.0, 1.0)
    # every quadrant occurs, for positive and negative angles
    k = np.rint(angles * ref.INV).astype(np.int64)
    assert {int(v) for v in np.unique(k & 3)} == {0, 1, 2, 3} and (k < 0).any() and (k > 0).any()


# ---- the iterator and the window --------------------------------------------------------------------------------------------------------
def test_velocity_iterator_cases():
    assert ref.velocity_iterator(0.3, 0.3, 5) == [0.3]                                             # min == max
    assert ref.velocity_iterator(0.0, 1.0, 1) == [0.0, 1.0]                                        # n = 1 becomes 2
    assert ref.velocity_iterator(-1.0, 1.0, 3) == [-1.0, 0.0, 1.0]                                 # 0 is a sample: nothing inserted
    assert ref.velocity_iterator(-1.0, 2.0, 3) == [-1.0, 0.0, 0.5, 2.0]                            # straddling without 0: inserted
    assert ref.velocity_iterator(-1.0, 2.0, 2) == [-1.0, 0.0, 2.0]
    assert ref.velocity_iterator(0.0, 1.0, 5) == [0.0, 0.25, 0.5, 0.75, 1.0] and ref.velocity_iterator(-2.0, -1.0, 3) == [-2.0, -1.5, -1.0]
    # through the plan: theta straddles 0 without hitting it (an inserted 0.0), y hits it (none inserted)
    plan, *_ = both(LIMITS, CONFIG)
    import gem_amd
    x, y, th = gem_amd.plan_lists(plan)
    assert (plan.n_x, plan.n_y, plan.n_th) == (6, 3, 21) and y.tolist() == [np.float32(-0.1), 0.0, np.float32(0.1)]
    assert int((th == 0).sum()) == 1 and th[3] < 0 < th[5] and th[4] == 0.0
    plan, *_ = both(LIMITS, dict(CONFIG, vsamples=(1, 1, 1)))
    assert (plan.n_x, plan.n_y, plan.n_th) == (2, 3, 3)                                            # n = 1 becomes 2; y and theta gain their 0.0
    for vs in ((0, 3, 3), (3, 0, 3), (3, 3, 0), (-2, 3, 3)):                                       # a product <= 0: no samples
        plan, poses, lens, ext, vels = both(LIMITS, dict(CONFIG, vsamples=vs))
        assert plan.n_traj == 0 and plan.max_steps == 0 and (plan.n_x, plan.n_y, plan.n_th) == (0, 0, 0) and lens.size == 0
    plan, *_ = both(LIMITS, dict(CONFIG, vsamples=(-2, -3, 4)))                                    # a positive product of negative counts: n = max(2, n)
    assert (plan.n_x, plan.n_y) == (2, 3)


def test_both_branches_of_the_velocity_window():
    lo, hi = ref.window(LIMITS, CONFIG, POS, VEL, GOAL)                                            # use_dwa: vel +- acc * sim_period
    assert hi == [f32(f32(0.2) + 2.5 * 0.05), f32(0.1), f32(f32(0.1) + f32(3.2) * 0.05)]
    assert lo == [f32(f32(0.2) - 2.5 * 0.05), f32(-0.1), f32(f32(0.1) - f32(3.2) * 0.05)]
    far = dict(CONFIG, use_dwa=False, continued_acceleration=True)
    lo, hi = ref.window(LIMITS, far, POS, VEL, GOAL)                                               # not: vel +- acc * sim_time, dist / sim_time above the limit
    dist = math.sqrt(2.0 * 2.0 + 1.5 * 1.5)
    assert dist / 1.7 > 0.55 and hi == [f32(0.55), f32(0.1), f32(1.0)] and lo == [f32(0.0), f32(-0.1), f32(-1.0)]
    near = (POS[0] + 0.3, POS[1] + 0.4)                                                            # dist / sim_time limits x; y's limit is lower still
    lo, hi = ref.window(LIMITS, far, POS, VEL, near)
    d = math.sqrt(f32(f32(near[0]) - 1.0) ** 2 + f32(f32(near[1]) - 2.0) ** 2)
    assert 0.0 < d / 1.7 < 0.55 and hi[0] == f32(d / 1.7) and hi[1] == f32(0.1)
    slow = dict(LIMITS, min_vel_x=0.4)                                                             # dist / sim_time clamps below min_vel_x: max = min
    lo, hi = ref.window(slow, far, POS, VEL, near)
    assert d / 1.7 < 0.4 and hi[0] == lo[0] == f32(0.4)
    for L, c, goal in ((LIMITS, far, GOAL), (LIMITS, far, near), (slow, far, near)):
        plan, *_ = both(L, c, goal=goal)
        assert plan.n_traj > 0
    plan, *_ = both(slow, far, goal=near)
    assert plan.n_x == 1                                                                          # ... and the x list is the single value


# ---- generateTrajectory -----------------------------------------------------------------------------------------------------------------
def test_both_rejection_rules_at_eps():
    v, w = f32(0.25), f32(0.125)
    up = lambda x: math.nextafter(x, math.inf)
    for min_trans, min_theta, generated in ((v + EPS, up(w + EPS), True), (up(v + EPS), w + EPS, True),      # one half alone does not reject
                                            (up(v + EPS), up(w + EPS), False), (v + EPS, w + EPS, True),
                                            (-1.0, up(w + EPS), True), (up(v + EPS), -1.0, True)):          # a negative limit switches its half off
        L, c, vel = single((v, 0.0, w), min_vel_trans=min_trans, min_vel_theta=min_theta, max_vel_trans=-1.0)
        assert (ref.num_steps(L, c, (v, 0.0, w)) > 0) == generated
        assert (both(L, c, vel=vel)[2][0] > 0) == generated
    vmag = math.sqrt(v * v + w * w)
    for max_trans, generated in ((vmag - EPS, True), (math.nextafter(vmag - EPS, -math.inf), False), (-1.0, True), (0.0, False)):
        L, c, vel = single((v, w, 0.5), max_vel_trans=max_trans, min_vel_trans=0.0)
        assert (ref.num_steps(L, c, (v, w, 0.5)) > 0) == generated
        plan, poses, lens, ext, vels = both(L, c, vel=vel)
        assert (lens[0] > 0) == generated and ext[1, 0] == 0.5 and vels[0].tolist() == [v, w, 0.5]        # the external scores are written all the same


def test_num_steps():
    free = dict(min_vel_trans=-1.0, max_vel_trans=-1.0)
    L, c, vel = single((f32(0.5), 0.0, f32(0.25)), discretize_by_time=True, **free)
    assert ref.num_steps(L, c, (f32(0.5), 0.0, f32(0.25))) == math.ceil(1.7 / 0.025) == 68 and both(L, c, vel=vel)[2].tolist() == [68]
    L, c, vel = single((f32(0.5), 0.0, f32(0.25)), **free)                                       # by distance: 0.5 * 1.7 / 0.025 = 34
    assert both(L, c, vel=vel)[2].tolist() == [34]
    L, c, vel = single((f32(0.125), f32(0.125), f32(1.5)), **free)                                 # by angle: 1.5 * 1.7 / 0.1 = 25.5 -> 26
    assert math.sqrt(2 * 0.125 ** 2) * 1.7 / 0.025 < 25.5 and both(L, c, vel=vel)[2].tolist() == [26]
    L, c, vel = single((0.0, 0.0, 0.0), **free)                                                    # the zero sample: no steps, not generated
    plan, poses, lens, ext, vels = both(L, c, vel=vel)
    assert plan.max_steps == 0 and lens.tolist() == [0] and ext[:, 0].tolist() == [0.0, 0.0]
    L, c, vel = single((0.0, 0.0, 0.0), discretize_by_time=True, **free)                           # ... by time it is generated: 68 equal poses
    plan, poses, lens, ext, vels = both(L, c, vel=vel)
    assert lens.tolist() == [68] and (poses == poses[0]).all()


def test_continued_acceleration_reaches_its_target_mid_trajectory():
    free = dict(min_vel_trans=-1.0, max_vel_trans=-1.0)
    target = (f32(0.5), 0.0, 0.0)
    L, c, _ = single(target, use_dwa=False, continued_acceleration=True, discretize_by_time=True, sim_time=2.0, sim_granularity=0.1,
                     acc_lim_x=1.0, **free)
    L.update(min_vel_x=0.0, max_vel_x=0.5)
    c.update(vsamples=(2, 1, 1))
    vel = (0.0, 0.0, 0.0)
    n, pts, v = ref.trajectory(L, c, POS, vel, target)
    assert n == 20 and v[0] == f32(0.0 + f32(1.0) * 0.1)
    xs = [p[0] for p in pts]
    steps = np.diff(np.array(xs))
    # the velocity climbs by acc * dt a step, reaches 0.5 at the fifth update and stays: the steps grow, then are equal
    assert steps[0] < steps[1] < steps[2] < steps[3] and abs(steps[3] - 0.5 * 0.1 * math.cos(0.3)) < 1e-6 and np.ptp(steps[4:]) < 1e-6
    plan, poses, lens, ext, vels = both(L, c, vel=vel, goal=(POS[0] + 5.0, POS[1]))
    assert plan.n_x == 2 and lens.tolist() == [20, 20] and vels[1, 0] == np.float32(v[0]) and vels[0, 0] == 0.0
    # decelerating towards a target below the velocity
    n, pts, v = ref.trajectory(L, c, POS, (1.0, 0.0, 0.0), target)
    assert v[0] == f32(1.0 - f32(1.0) * 0.1)


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------
CASES = {"dwa": (LIMITS, CONFIG, POS, VEL),
         "by time": (LIMITS, dict(CONFIG, discretize_by_time=True, oscillation_flags=1 | 8 | 16), POS, VEL),
         "continued": (LIMITS, dict(CONFIG, use_dwa=False, continued_acceleration=True, vsamples=(4, 3, 7), oscillation_flags=2 | 4 | 32), POS, (0.2, 0.05, -0.3)),
         "near -pi": (LIMITS, dict(CONFIG, vsamples=(3, 1, 5)), (-4.0, 7.5, -3.1415925), (0.3, 0.0, -0.2)),
         "near +pi": (dict(LIMITS, min_vel_trans=-1.0), dict(CONFIG, vsamples=(7, 3, 11)), (120.5, -80.25, 3.1415925), (0.1, 0.02, 0.3))}


@pytest.mark.parametrize("name", list(CASES))
def test_host_twin_equals_the_restatement_bit_for_bit(name):
    L, c, pos, vel = CASES[name]
    plan, poses, lens, ext, vels = both(L, c, pos, vel)
    assert plan.n_traj > 30 and (lens > 0).sum() > 10
    if name in ("dwa", "by time", "continued"):
        assert (lens == 0).any()                                                                  # the slow, straight samples are not generated
    if c["oscillation_flags"]:
        assert (ext[0] == -5.0).any() and (ext[0] == 0.0).any()
    # the winner's velocity from the index alone
    import gem_amd
    for t in (0, int(plan.n_traj) // 2, int(plan.n_traj) - 1):
        assert np.array(gem_amd.trajectory_velocity(plan, vel, t), np.float32).tobytes() == vels[t].tobytes()
    # slots beyond a length, and those of a sample that is not generated, keep what they held
    T = plan.max_steps + 3
    _, poses2, lens2, _, _ = twin(L, c, pos, vel, T=T, fill=-77.0)
    assert lens2.tobytes() == lens.tobytes()
    p2 = poses2.reshape(-1, T, 4)
    p1 = poses.reshape(-1, plan.max_steps, 4)
    for t in range(int(plan.n_traj)):
        assert (p2[t, lens[t]:] == -77.0).all() and p2[t, :lens[t]].tobytes() == p1[t, :lens[t]].tobytes()


def test_twin_against_the_libm_form():
    """the same recurrence with math.cos / math.sin: theta has no cosine in it and is bit-equal; each step's rounding of x, y can flip
    one float32 ulp and a carried difference passes through an addition without growing by more than one, so after i steps x and y
    differ by at most i ulps of the largest magnitude on the trajectory (the bound used is T = num_steps)"""
    differing = total = 0
    worst = 0.0
    for name, (L, c, pos, vel) in CASES.items():
        ls = ref.lists(L, c, pos, vel, GOAL)
        for s in ref.samples(ls):
            n, pts, _ = ref.trajectory(L, c, pos, vel, s)
            n2, pts2, _ = ref.trajectory(L, c, pos, vel, s, trig=ref.libm_trig)
            assert n == n2
            if not n:
                continue
            a, b = np.array(pts, np.float32), np.array(pts2, np.float32)
            assert a[:, 2].tobytes() == b[:, 2].tobytes()
            for k in (0, 1):
                ulp = float(np.spacing(np.float32(max(np.abs(a[:, k]).max(), np.abs(b[:, k]).max()))))
                d = float(np.abs(a[:, k].astype(np.float64) - b[:, k].astype(np.float64)).max()) / ulp
                worst = max(worst, d)
                assert d <= n, (name, s, d)
            differing += int((a != b).any(axis=1).sum())
            total += n
    print(f"poses differing from the libm form: {differing} of {total}, at most {worst:.0f} ulp")
    assert total > 10000


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal(lib):
    from gem_amd import _lib
    import gem_amd
    INV = _lib.GEM_OK - 1
    nan, inf = float("nan"), float("inf")
    f3 = lambda v: (C.c_float * len(v))(*v)

    def plan_rc(limits=LIMITS, config=CONFIG, pos=POS, vel=VEL, goal=GOAL, out=True, null=None):
        L = _lib.TrajgenLimits(*[float(limits[k]) for k in gem_amd.api.TRAJGEN_LIMITS])
        c = _lib.TrajgenConfig(config["sim_time"], config["sim_granularity"], config["angular_sim_granularity"], config["sim_period"], int(config["use_dwa"]),
                               int(config["discretize_by_time"]), int(config["continued_acceleration"]), config["oscillation_flags"],
                               (C.c_int * 3)(*config["vsamples"]), 0)
        plan = _lib.DwaPlan()
        plan.n_traj = -9
        args = [C.byref(L), C.byref(c), f3(pos), f3(vel), f3(goal), C.byref(plan)]
        if null is not None:
            args[null] = None
        return lib.gem_trajgen_plan(*args), plan

    assert plan_rc()[0] == 0
    for k in LIMITS:
        for bad in (nan, inf, -inf):
            rc, plan = plan_rc(limits=dict(LIMITS, **{k: bad}))
            assert rc == INV and plan.n_traj == -9, (k, bad)
    for k in ("sim_time", "sim_granularity", "angular_sim_granularity", "sim_period"):
        for bad in (nan, inf, 0.0, -1.0):
            assert plan_rc(config=dict(CONFIG, **{k: bad}))[0] == INV, (k, bad)
    assert plan_rc(config=dict(CONFIG, discretize_by_time=True, angular_sim_granularity=0.0))[0] == 0      # not in use: not checked for its sign
    assert plan_rc(config=dict(CONFIG, discretize_by_time=True, angular_sim_granularity=nan))[0] == INV    # ... but finite
    assert plan_rc(config=dict(CONFIG, oscillation_flags=64))[0] == INV and plan_rc(config=dict(CONFIG, oscillation_flags=-1))[0] == INV
    for i in range(3):
        for bad in (nan, inf):
            assert plan_rc(pos=[bad if j == i else v for j, v in enumerate(POS)])[0] == INV
            assert plan_rc(vel=[bad if j == i else v for j, v in enumerate(VEL)])[0] == INV
    assert plan_rc(goal=(nan, 0.0))[0] == INV and plan_rc(goal=(0.0, inf))[0] == INV
    for i in range(6):
        assert plan_rc(null=i)[0] == INV
    assert plan_rc(config=dict(CONFIG, vsamples=(100, 100, 56)))[0] == INV                                # 256 + the inserted zeros
    assert plan_rc(config=dict(CONFIG, vsamples=(100, 100, 50)))[0] == 0
    assert plan_rc(config=dict(CONFIG, vsamples=(300, 1, 1)))[0] == INV

    # generate / velocity
    plan = gem_amd.trajgen_plan(LIMITS, CONFIG, POS, VEL, GOAL)
    T, nt = plan.max_steps, int(plan.n_traj)
    poses, lens, ext, vels = np.full((nt * (T + 1), 4), -77.0), np.full(nt, -7, np.int32), np.full((2, nt), -77.0), np.full((nt, 3), -77.0, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def gen_rc(p=plan, pos=POS, vel=VEL, T_=T, arrays=(poses, lens, ext, vels), null_plan=False, null_pos=False, null_vel=False):
        return lib.gem_trajgen_generate(None if null_plan else C.byref(p), None if null_pos else f3(pos), None if null_vel else f3(vel),
                                        *[ptr(a) if a is not None else None for a in arrays], T_)

    def tampered(**kw):
        q = _lib.DwaPlan.from_buffer_copy(plan)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    assert gen_rc(T_=T - 1) == INV and gen_rc(T_=0) == INV and gen_rc(T_=(1 << 20) + 1) == INV and gen_rc(T_=-3) == INV
    assert gen_rc(null_plan=True) == INV and gen_rc(null_pos=True) == INV and gen_rc(null_vel=True) == INV
    for i in range(3):
        arrays = [poses, lens, ext, vels]
        arrays[i] = None
        assert gen_rc(arrays=arrays) == INV
    assert gen_rc(pos=(0.0, 0.0, nan)) == INV and gen_rc(vel=(inf, 0.0, 0.0)) == INV
    assert gen_rc(pos=(0.0, 0.0, 64 * math.pi)) == INV and gen_rc(pos=(0.0, 0.0, -199.5)) == INV       # the 64 pi bound: |theta| + sim_time * |w| <= 64 pi - 2
    assert gen_rc(vel=(0.2, 0.0, 120.0)) == INV                                                      # ... the velocity's share of it
    for q in (tampered(n_traj=nt + 1), tampered(max_steps=T - 1), tampered(n_x=plan.n_x + 1), tampered(n_th=-1), tampered(n_x=200, n_y=57, n_th=1, n_traj=200 * 57)):
        assert gen_rc(p=q) == INV
        assert lib.gem_trajgen_velocity(C.byref(q), f3(VEL), 0, f3((0, 0, 0))) == INV
    q = tampered()
    q.samples[2] = nan
    assert gen_rc(p=q) == INV
    q = tampered()
    q.config.sim_time = -1.0
    assert gen_rc(p=q) == INV
    big = gem_amd.trajgen_plan(dict(LIMITS, min_vel_trans=-1.0), dict(CONFIG, vsamples=(80, 80, 80), discretize_by_time=True), POS, VEL, GOAL)
    assert big.n_traj * (1 << 20) > 2 ** 31 - 2
    assert lib.gem_trajgen_generate(C.byref(big), f3(POS), f3(VEL), ptr(poses), ptr(lens), ptr(ext), None, 1 << 20) == INV     # more than 2^31 - 2 pose slots
    out = f3((-7.0, -7.0, -7.0))
    for bad in (-1, nt, 1 << 40):
        assert lib.gem_trajgen_velocity(C.byref(plan), f3(VEL), bad, out) == INV
    assert lib.gem_trajgen_velocity(None, f3(VEL), 0, out) == INV and lib.gem_trajgen_velocity(C.byref(plan), None, 0, out) == INV
    assert lib.gem_trajgen_velocity(C.byref(plan), f3(VEL), 0, None) == INV and lib.gem_trajgen_velocity(C.byref(plan), f3((nan, 0, 0)), 0, out) == INV
    assert list(out) == [-7.0] * 3
    assert lib.gem_trajgen_sincos(None, 3, ptr(ext), ptr(ext)) == INV and lib.gem_trajgen_sincos(ptr(ext), -1, ptr(ext), ptr(ext)) == INV
    # nothing was written by any refusal
    assert (poses == -77.0).all() and (lens == -7).all() and (ext == -77.0).all() and (vels == -77.0).all()
    assert gen_rc(arrays=(poses, lens, ext, None)) == 0 and (lens >= 0).all() and (vels == -77.0).all()      # out_vel may be NULL
    with pytest.raises(ValueError):
        gem_amd.trajgen_plan(dict(LIMITS, max_vel_x=nan), CONFIG, POS, VEL)
    with pytest.raises(ValueError):
        gem_amd.generate_trajectories(plan, POS, VEL, T - 1)
    with pytest.raises(ValueError):
        gem_amd.trajectory_velocity(plan, VEL, nt)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def declared(header):
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(gem_[a-z_0-9]+)\s*\(", text)))


def test_trajgen_symbols_are_declared_exported_and_bound(lib):
    from gem_amd import _lib
    names = declared(ROOT / "include" / "gem_hip_trajgen.h")
    assert names == sorted(_lib.TRAJGEN_SIGNATURES) == ["gem_costmap_dwa_best", "gem_costmap_dwa_best_device", "gem_trajgen_generate",
                                                        "gem_trajgen_generate_device", "gem_trajgen_plan", "gem_trajgen_sincos", "gem_trajgen_velocity"]
    for n in names:
        assert getattr(lib, n).argtypes == _lib.TRAJGEN_SIGNATURES[n][1]
    text = (ROOT / "include" / "gem_hip.h").read_text()
    assert text.index('#include "gem_hip_critics.h"') < text.index('#include "gem_hip_trajgen.h"')
    hdr = (ROOT / "include" / "gem_hip_trajgen.h").read_text()
    assert "NOT verified" in hdr and "UNVERIFIED" in hdr and "hypot" in hdr
    assert "unverified" in (ROOT / "tests" / "trajgen_ref.py").read_text()
    assert lib.gem_abi_version() == 9


def test_constants_and_sizes_match_the_header(tmp_path):
    from gem_amd import _lib
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "gem_hip.h"\nint main(void) { printf("%d %d %d %d %d %d %d %d %d %d\\n", GEM_TRAJGEN_MAX_LIST, '
                   "GEM_OSC_FORWARD_POS_ONLY, GEM_OSC_FORWARD_NEG_ONLY, GEM_OSC_STRAFE_POS_ONLY, GEM_OSC_STRAFE_NEG_ONLY, GEM_OSC_ROT_POS_ONLY, "
                   "GEM_OSC_ROT_NEG_ONLY, (int)sizeof(gem_trajgen_limits), (int)sizeof(gem_trajgen_config), (int)sizeof(gem_dwa_plan)); return 0; }\n")
    exe = tmp_path / "consts"
    res = subprocess.run(["cc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [_lib.TRAJGEN_MAX_LIST, _lib.OSC_FORWARD_POS_ONLY, _lib.OSC_FORWARD_NEG_ONLY, _lib.OSC_STRAFE_POS_ONLY, _lib.OSC_STRAFE_NEG_ONLY,
                   _lib.OSC_ROT_POS_ONLY, _lib.OSC_ROT_NEG_ONLY, C.sizeof(_lib.TrajgenLimits), C.sizeof(_lib.TrajgenConfig), C.sizeof(_lib.DwaPlan)]
    assert got == [256, 1, 2, 4, 8, 16, 32, 88, 64, 1200]


def test_python_facade_has_the_trajgen_calls():
    import gem_amd
    assert callable(gem_amd.Costmap.dwa_best)
    for name in ("trajgen_plan", "generate_trajectories", "trajectory_velocity", "plan_lists", "contract_sincos"):
        assert callable(getattr(gem_amd, name))


def build_trajgen_check(out: Path) -> Path:
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc", "-std=c++17", "-O2", "-Wall", "-Werror",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "trajgen_check.cpp"), "-o", str(out),
           f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_host_restatement_on_its_own(tmp_path):
    """gem_amd/csrc/gem_trajgen.hpp and gem_sincos.hpp compiled by a plain C++ compiler, without HIP and without the library
    (tests/cpp/trajgen_host.cpp): plans of every shape through plan, generate and velocity with buffers of exactly the stated sizes.
    The same program is what a sanitizer build (-fsanitize=address,undefined) runs."""
    exe = tmp_path / "trajgen_host"
    res = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "trajgen_host.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


def test_trajgen_facade_builds():
    """gem::TrajectoryLimits, gem::TrajectoryConfig, gem::generateTrajectories and gem::Costmap::dwaBest compile with hipcc -Wall -Werror
    against the headers and the library; the host twin is checked, and without a GPU the check exits early."""
    from gem_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as td:
        exe = build_trajgen_check(Path(td) / "trajgen_check")
        res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: built)"), res.stdout + res.stderr
