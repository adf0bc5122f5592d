"""numpy / plain Python restatement of the trajectory-generation contract of include/gem_hip_trajgen.h: base_local_planner's
SimpleTrajectoryGenerator (initialise, generateTrajectory, computeNewVelocities), VelocityIterator and the oscillation and twirling
cost functions.  base_local_planner is not available to these tests: this is a restatement, unverified against the library.

Every cast is explicit.  A float32 quantity is held as a Python float (a C double) whose value is float32-representable, made by f32();
all arithmetic is then Python double arithmetic, every operation rounded on its own, and nothing depends on numpy's promotion rules
(under numpy 2 a Python float is "weak": np.float32(x) + 0.1 would stay float32 where the contract wants double)."""
import math

import numpy as np

OSC_BITS = 63
M_PI_2 = 1.5707963267948966
THETA_BOUND = 64.0 * math.pi - 2.0
LIMITS = ("max_vel_x", "min_vel_x", "max_vel_y", "min_vel_y", "max_vel_theta", "min_vel_theta", "max_vel_trans", "min_vel_trans",
          "acc_lim_x", "acc_lim_y", "acc_lim_theta")


def f32(x):
    """(float)x: round to nearest float32, held as a double"""
    with np.errstate(over="ignore"):
        return float(np.float32(x))


# ---- the contract's sine and cosine ---------------------------------------------------------------------------------------------------
INV = float.fromhex("0x1.45F306DC9C883p-1")          # 0x3FE45F306DC9C883
P1 = float.fromhex("0x1.921FB544p+0")                # 0x3FF921FB54400000
P2 = float.fromhex("0x1.0B4611A6p-34")               # 0x3DD0B4611A600000
P3 = float.fromhex("0x1.3198A2E037073p-69")          # 0x3BA3198A2E037073
BIG = 6755399441055744.0
SIN_COEFF = [(-1.0) ** i / math.factorial(2 * i + 1) for i in range(8, 0, -1)]      # quotients of exact integers: correctly rounded
COS_COEFF = [(-1.0) ** i / math.factorial(2 * i) for i in range(8, 0, -1)]


def sincos(t):
    """(sin t, cos t) of a Python float, in plain double + - *"""
    t = float(t)
    k = (t * INV + BIG) - BIG
    r = ((t - k * P1) - k * P2) - k * P3
    z = r * r
    p = SIN_COEFF[0]
    for c in SIN_COEFF[1:]:
        p = p * z + c
    sr = r + r * (z * p)
    q = COS_COEFF[0]
    for c in COS_COEFF[1:]:
        q = q * z + c
    cr = 1.0 + z * q
    quad = int(k) & 3
    return ((sr, cr), (cr, -sr), (-sr, -cr), (-cr, sr))[quad]


def sincos_array(t):
    """the same over a float64 array (numpy's elementwise float64 + - * are the IEEE operations)"""
    t = np.asarray(t, np.float64)
    k = (t * INV + BIG) - BIG
    r = ((t - k * P1) - k * P2) - k * P3
    z = r * r
    p = np.full_like(t, SIN_COEFF[0])
    for c in SIN_COEFF[1:]:
        p = p * z + c
    sr = r + r * (z * p)
    q = np.full_like(t, COS_COEFF[0])
    for c in COS_COEFF[1:]:
        q = q * z + c
    cr = 1.0 + z * q
    quad = k.astype(np.int64) & 3
    return np.choose(quad, [sr, cr, -sr, -cr]), np.choose(quad, [cr, -sr, -cr, sr])


# ---- the window and the lists ---------------------------------------------------------------------------------------------------------
def velocity_iterator(vmin, vmax, n):
    """VelocityIterator(min, max, n): the doubles it yields"""
    vmin, vmax = float(vmin), float(vmax)
    if vmin == vmax:
        return [vmin]
    n = max(2, int(n))
    step = (vmax - vmin) / float(max(1, n - 1))
    out = []
    nxt = vmin
    for _ in range(n - 1):
        current = nxt
        nxt += step
        out.append(current)
        if current < 0 and nxt > 0:
            out.append(0.0)
    out.append(vmax)
    return out


def window(limits, config, pos, vel, goal):
    """initialise's (min_vel[3], max_vel[3]) as float32 values"""
    pos, vel, goal = [f32(v) for v in pos], [f32(v) for v in vel], [f32(v) for v in goal]
    acc = [f32(limits["acc_lim_x"]), f32(limits["acc_lim_y"]), f32(limits["acc_lim_theta"])]
    max_vel_x, max_vel_y = float(limits["max_vel_x"]), float(limits["max_vel_y"])
    max_vel_th = float(limits["max_vel_theta"])
    min_vel_th = -1.0 * max_vel_th
    horizon = float(config["sim_period"])
    if not config.get("use_dwa", True):
        dx, dy = f32(goal[0] - pos[0]), f32(goal[1] - pos[1])
        dist = math.sqrt(dx * dx + dy * dy)
        max_vel_x = max(min(max_vel_x, dist / float(config["sim_time"])), float(limits["min_vel_x"]))
        max_vel_y = max(min(max_vel_y, dist / float(config["sim_time"])), float(limits["min_vel_y"]))
        horizon = float(config["sim_time"])
    hi = [max_vel_x, max_vel_y, max_vel_th]
    lo = [float(limits["min_vel_x"]), float(limits["min_vel_y"]), min_vel_th]
    max_vel = [f32(min(hi[i], vel[i] + acc[i] * horizon)) for i in range(3)]
    min_vel = [f32(max(lo[i], vel[i] - acc[i] * horizon)) for i in range(3)]
    return min_vel, max_vel


def lists(limits, config, pos, vel, goal=(0.0, 0.0)):
    """the three lists as float32 values (empty when the product of vsamples is not positive)"""
    vs = config["vsamples"]
    if float(vs[0]) * float(vs[1]) * float(vs[2]) <= 0:
        return [], [], []
    min_vel, max_vel = window(limits, config, pos, vel, goal)
    return tuple([f32(v) for v in velocity_iterator(min_vel[i], max_vel[i], vs[i])] for i in range(3))


def samples(ls):
    """the product, x outermost and theta innermost"""
    return [(x, y, th) for x in ls[0] for y in ls[1] for th in ls[2]]


# ---- a trajectory ---------------------------------------------------------------------------------------------------------------------
def num_steps(limits, config, s):
    """0: not generated"""
    s0, s1, s2 = s
    vmag = math.sqrt(s0 * s0 + s1 * s1)
    eps = 1e-4
    min_trans, max_trans, min_theta = float(limits["min_vel_trans"]), float(limits["max_vel_trans"]), float(limits["min_vel_theta"])
    if (min_trans >= 0 and vmag + eps < min_trans) and (min_theta >= 0 and math.fabs(s2) + eps < min_theta):
        return 0
    if max_trans >= 0 and vmag - eps > max_trans:
        return 0
    sim_time = float(config["sim_time"])
    if config.get("discretize_by_time", False):
        return int(math.ceil(sim_time / float(config["sim_granularity"])))
    return int(math.ceil(max(vmag * sim_time / float(config["sim_granularity"]),
                             math.fabs(s2) * sim_time / float(config["angular_sim_granularity"]))))


def new_velocities(target, vel, acc, dt):
    out = []
    for i in range(3):
        if vel[i] < target[i]:
            out.append(f32(min(target[i], vel[i] + acc[i] * dt)))
        else:
            out.append(f32(max(target[i], vel[i] - acc[i] * dt)))
    return out


def oscillation(bits, v):
    xv, yv, thetav = v
    fires = ((bits & 1) and xv < 0) or ((bits & 2) and xv > 0) or ((bits & 4) and yv < 0) or ((bits & 8) and yv > 0) or \
        ((bits & 16) and thetav < 0) or ((bits & 32) and thetav > 0)
    return -5.0 if fires else 0.0


def trajectory(limits, config, pos, vel, s, trig=sincos):
    """(num_steps, [(x, y, theta)] float32 values, (xv, yv, thetav)); trig: the (sin, cos) of a double"""
    pos, vel = [f32(v) for v in pos], [f32(v) for v in vel]
    acc = [f32(limits["acc_lim_x"]), f32(limits["acc_lim_y"]), f32(limits["acc_lim_theta"])]
    n = num_steps(limits, config, s)
    if n == 0:
        return 0, [], tuple(s)
    dt = float(config["sim_time"]) / float(n)
    cont = bool(config.get("continued_acceleration", False))
    loop_vel = new_velocities(s, vel, acc, dt) if cont else list(s)
    v = tuple(loop_vel)
    out = []
    for _ in range(n):
        out.append(tuple(pos))
        if cont:
            loop_vel = new_velocities(s, loop_vel, acc, dt)
        sn, cs = trig(pos[2])
        sn2, cs2 = trig(M_PI_2 + pos[2])
        pos = [f32(pos[0] + (loop_vel[0] * cs + loop_vel[1] * cs2) * dt),
               f32(pos[1] + (loop_vel[0] * sn + loop_vel[1] * sn2) * dt),
               f32(pos[2] + loop_vel[2] * dt)]
    return n, out, v


def libm_trig(t):
    return math.sin(t), math.cos(t)


def generate(limits, config, pos, vel, goal, T, fill=0.0):
    """what gem_trajgen_generate leaves: (poses float64 [n_traj * T, 4], traj_len int32, ext float64 [2, n_traj], vel float32 [n_traj, 3])"""
    sm = samples(lists(limits, config, pos, vel, goal))
    nt = len(sm)
    poses = np.full((nt * T, 4), fill, np.float64)
    lens = np.zeros(nt, np.int32)
    ext = np.zeros((2, nt), np.float64)
    vels = np.zeros((nt, 3), np.float32)
    for t, s in enumerate(sm):
        n, pts, v = trajectory(limits, config, pos, vel, s)
        assert n <= T
        lens[t] = n
        for i, (x, y, th) in enumerate(pts):
            sn, cs = sincos(th)
            poses[t * T + i] = (x, y, cs, sn)
        ext[0, t] = oscillation(int(config.get("oscillation_flags", 0)), v)
        ext[1, t] = math.fabs(v[2])
        vels[t] = v
    return poses, lens, ext, vels


def max_steps(limits, config, ls):
    """the largest num_steps over the samples, rejected ones included (what the plan reports)"""
    if not ls[0] or not ls[1] or not ls[2]:
        return 0
    free = dict(limits, min_vel_trans=-1.0, max_vel_trans=-1.0)
    return max(num_steps(free, config, s) for s in samples(ls))
