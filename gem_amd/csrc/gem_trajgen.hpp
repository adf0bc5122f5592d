// gem_trajgen.hpp -- DWA's sampled trajectories (internal header): the arithmetic of the contract of include/gem_hip_trajgen.h that
// the kernel (gem_trajgen.hip) and its host twin share, the host twin itself (plan, generate, velocity: plain C++, no device), the
// kernel's argument block and its launcher.  Compiles without HIP too: the host twin is run on its own under the sanitizers.
#pragma once

#include "../../include/gem_hip.h"
#include "gem_sincos.hpp"

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GEM_TG_HD __host__ __device__ __forceinline__
#else
#define GEM_TG_HD inline
#endif

namespace gem {

constexpr int kTrajgenThreads = 256;
constexpr int kTrajgenMaxBlocks = 1024;                            // the groups stride over the rest
constexpr int kTrajgenMaxList = 256;                               // GEM_TRAJGEN_MAX_LIST
constexpr int kTrajgenMaxPosesPerTraj = 1 << 20;
constexpr long long kTrajgenMaxPoses = 2147483646ll;               // 2^31 - 2, as gem_costmap_best_trajectory
constexpr int kTrajgenOscBits = 63;
constexpr double kTrajgenPi2 = 1.57079632679489661923;             // M_PI_2
constexpr double kTrajgenThetaBound = 64.0 * 3.14159265358979323846 - 2.0;

// what a trajectory needs beside its sample, as the kernel reads it
struct TrajgenParams {
    double sim_time, gran, ang_gran, min_vel_trans, max_vel_trans, min_vel_theta;
    float pos[3], vel[3], acc[3];
    int by_time, cont, osc;
    int n_x, n_y, n_th;
};

GEM_TG_HD double tg_min(double a, double b) { return b < a ? b : a; }       // std::min / std::max
GEM_TG_HD double tg_max(double a, double b) { return a < b ? b : a; }

// num_steps of the sample, 0: not generated (steps above 2^30 answer 2^30: the host refuses them all the same)
GEM_TG_HD int trajgen_steps(const TrajgenParams& p, float s0, float s1, float s2)
{
    const double vmag = sqrt((double)s0 * (double)s0 + (double)s1 * (double)s1), eps = 1e-4;
    if ((p.min_vel_trans >= 0 && vmag + eps < p.min_vel_trans) && (p.min_vel_theta >= 0 && fabs((double)s2) + eps < p.min_vel_theta)) return 0;
    if (p.max_vel_trans >= 0 && vmag - eps > p.max_vel_trans) return 0;
    double n;
    if (p.by_time) n = ceil(p.sim_time / p.gran);
    else n = ceil(tg_max(vmag * p.sim_time / p.gran, fabs((double)s2) * p.sim_time / p.ang_gran));
    return n > 1073741824.0 ? 1073741824 : (int)n;
}

// computeNewVelocities, one component
GEM_TG_HD float trajgen_new_velocity(float target, float v, float acc, double dt)
{
    if (v < target) return (float)tg_min((double)target, (double)v + (double)acc * dt);
    return (float)tg_max((double)target, (double)v - (double)acc * dt);
}

GEM_TG_HD double trajgen_oscillation(int bits, float xv, float yv, float thetav)
{
    const bool fires = ((bits & 1) && xv < 0.f) || ((bits & 2) && xv > 0.f) || ((bits & 4) && yv < 0.f) || ((bits & 8) && yv > 0.f) ||
                       ((bits & 16) && thetav < 0.f) || ((bits & 32) && thetav > 0.f);
    return fires ? -5.0 : 0.0;
}

// sample t of the lists: x outermost, theta innermost
GEM_TG_HD void trajgen_sample(const TrajgenParams& p, const float* lists, unsigned t, float& s0, float& s1, float& s2)
{
    const unsigned ith = t % (unsigned)p.n_th, r = t / (unsigned)p.n_th, iy = r % (unsigned)p.n_y, ix = r / (unsigned)p.n_y;
    s0 = lists[ix]; s1 = lists[(unsigned)p.n_x + iy]; s2 = lists[(unsigned)(p.n_x + p.n_y) + ith];
}

// num_steps, dt and the trajectory's (xv, yv, thetav) of a sample
GEM_TG_HD int trajgen_start(const TrajgenParams& p, float s0, float s1, float s2, double& dt, float& v0, float& v1, float& v2)
{
    const int n = trajgen_steps(p, s0, s1, s2);
    v0 = s0; v1 = s1; v2 = s2; dt = 0.0;
    if (n > 0) {
        dt = p.sim_time / (double)n;
        if (p.cont) {
            v0 = trajgen_new_velocity(s0, p.vel[0], p.acc[0], dt);
            v1 = trajgen_new_velocity(s1, p.vel[1], p.acc[1], dt);
            v2 = trajgen_new_velocity(s2, p.vel[2], p.acc[2], dt);
        }
    }
    return n;
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------
inline bool tg_finite(double v) { return std::isfinite(v); }

// VelocityIterator(min, max, n): the values, each rounded to float as it enters a sample.  Returns the count, -1 beyond `room`.
inline int trajgen_list(double vmin, double vmax, int n, float* out, int room)
{
    int m = 0;
    auto push = [&](double v) { if (m < room) out[m] = (float)v; ++m; };
    if (vmin == vmax) push(vmin);
    else {
        n = n > 2 ? n : 2;
        const double step = (vmax - vmin) / (double)(n - 1 > 1 ? n - 1 : 1);
        double next = vmin;
        for (int j = 0; j < n - 1; ++j) {
            const double current = next;
            next += step;
            push(current);
            if (current < 0 && next > 0) push(0.0);
        }
        push(vmax);
    }
    return m <= room ? m : -1;
}

inline bool trajgen_inputs_ok(const gem_trajgen_limits& L, const gem_trajgen_config& c)
{
    const double v[] = {L.max_vel_x, L.min_vel_x, L.max_vel_y, L.min_vel_y, L.max_vel_theta, L.min_vel_theta, L.max_vel_trans, L.min_vel_trans,
                        L.acc_lim_x, L.acc_lim_y, L.acc_lim_theta, c.sim_time, c.sim_granularity, c.angular_sim_granularity, c.sim_period};
    for (double x : v) if (!tg_finite(x)) return false;
    if (!tg_finite((double)(float)L.acc_lim_x) || !tg_finite((double)(float)L.acc_lim_y) || !tg_finite((double)(float)L.acc_lim_theta)) return false;
    if (!(c.sim_time > 0) || !(c.sim_period > 0) || !(c.sim_granularity > 0)) return false;
    if (!c.discretize_by_time && !(c.angular_sim_granularity > 0)) return false;
    if (c.oscillation_flags & ~kTrajgenOscBits) return false;
    return true;
}

inline TrajgenParams trajgen_params(const gem_dwa_plan& pl, const float pos[3], const float vel[3])
{
    TrajgenParams p{};
    p.sim_time = pl.config.sim_time; p.gran = pl.config.sim_granularity; p.ang_gran = pl.config.angular_sim_granularity;
    p.min_vel_trans = pl.limits.min_vel_trans; p.max_vel_trans = pl.limits.max_vel_trans; p.min_vel_theta = pl.limits.min_vel_theta;
    for (int i = 0; i < 3; ++i) { p.pos[i] = pos ? pos[i] : 0.f; p.vel[i] = vel[i]; }
    p.acc[0] = (float)pl.limits.acc_lim_x; p.acc[1] = (float)pl.limits.acc_lim_y; p.acc[2] = (float)pl.limits.acc_lim_theta;
    p.by_time = pl.config.discretize_by_time != 0; p.cont = pl.config.continued_acceleration != 0; p.osc = pl.config.oscillation_flags;
    p.n_x = pl.n_x; p.n_y = pl.n_y; p.n_th = pl.n_th;
    return p;
}

// the largest num_steps of the plan's samples: ceil, the maxima, the products and the square root are monotone in |s0|, |s1|, |s2|
inline int trajgen_max_steps(const gem_dwa_plan& pl)
{
    if (pl.n_traj == 0) return 0;
    float m[3] = {0.f, 0.f, 0.f};
    const int at[4] = {0, pl.n_x, pl.n_x + pl.n_y, pl.n_x + pl.n_y + pl.n_th};
    for (int a = 0; a < 3; ++a)
        for (int i = at[a]; i < at[a + 1]; ++i) { const float v = std::fabs(pl.samples[i]); m[a] = v > m[a] ? v : m[a]; }
    const float zero[3] = {0.f, 0.f, 0.f};
    TrajgenParams p = trajgen_params(pl, zero, zero);
    p.min_vel_trans = -1.0; p.max_vel_trans = -1.0;                 // (no sample is dropped from the bound)
    return trajgen_steps(p, m[0], m[1], m[2]);
}

inline int trajgen_plan_host(const gem_trajgen_limits* L, const gem_trajgen_config* c, const float pos[3], const float vel[3], const float goal[2],
                             gem_dwa_plan* out)
{
    if (!L || !c || !pos || !vel || !goal || !out || !trajgen_inputs_ok(*L, *c)) return GEM_ERR_INVALID;
    for (int i = 0; i < 3; ++i) if (!tg_finite(pos[i]) || !tg_finite(vel[i])) return GEM_ERR_INVALID;
    if (!tg_finite(goal[0]) || !tg_finite(goal[1])) return GEM_ERR_INVALID;
    gem_dwa_plan pl{};
    pl.limits = *L; pl.config = *c;
    pl.config.reserved = 0;
    if ((double)c->vsamples[0] * (double)c->vsamples[1] * (double)c->vsamples[2] > 0) {
        const float acc[3] = {(float)L->acc_lim_x, (float)L->acc_lim_y, (float)L->acc_lim_theta};
        double max_vel_x = L->max_vel_x, max_vel_y = L->max_vel_y;
        const double max_vel_th = L->max_vel_theta, min_vel_th = -1.0 * L->max_vel_theta;
        double horizon = c->sim_period;
        if (!c->use_dwa) {
            const float dx = goal[0] - pos[0], dy = goal[1] - pos[1];
            const double dist = sqrt((double)dx * (double)dx + (double)dy * (double)dy);
            max_vel_x = tg_max(tg_min(max_vel_x, dist / c->sim_time), L->min_vel_x);
            max_vel_y = tg_max(tg_min(max_vel_y, dist / c->sim_time), L->min_vel_y);
            horizon = c->sim_time;
        }
        const double hi[3] = {max_vel_x, max_vel_y, max_vel_th}, lo[3] = {L->min_vel_x, L->min_vel_y, min_vel_th};
        int n[3], at = 0;
        for (int i = 0; i < 3; ++i) {
            const float vmax = (float)tg_min(hi[i], (double)vel[i] + (double)acc[i] * horizon);
            const float vmin = (float)tg_max(lo[i], (double)vel[i] - (double)acc[i] * horizon);
            if (c->vsamples[i] > kTrajgenMaxList) return GEM_ERR_INVALID;
            n[i] = trajgen_list((double)vmin, (double)vmax, c->vsamples[i], pl.samples + at, kTrajgenMaxList - at);
            if (n[i] < 0) return GEM_ERR_INVALID;
            at += n[i];
        }
        for (int i = 0; i < at; ++i) if (!tg_finite(pl.samples[i])) return GEM_ERR_INVALID;
        pl.n_x = n[0]; pl.n_y = n[1]; pl.n_th = n[2];
        pl.n_traj = (long long)n[0] * n[1] * n[2];
    }
    pl.max_steps = trajgen_max_steps(pl);
    *out = pl;
    return GEM_OK;
}

// a plan as gem_trajgen_plan leaves it (it is caller memory: everything the kernel trusts is checked again)
inline bool trajgen_plan_ok(const gem_dwa_plan& pl)
{
    if (!trajgen_inputs_ok(pl.limits, pl.config)) return false;
    if (pl.n_x < 0 || pl.n_y < 0 || pl.n_th < 0 || pl.n_x > kTrajgenMaxList || pl.n_y > kTrajgenMaxList || pl.n_th > kTrajgenMaxList) return false;
    if (pl.n_x + pl.n_y + pl.n_th > kTrajgenMaxList || pl.n_traj != (long long)pl.n_x * pl.n_y * pl.n_th) return false;
    if (pl.n_traj == 0 && (pl.n_x || pl.n_y || pl.n_th)) return false;
    for (int i = 0; i < pl.n_x + pl.n_y + pl.n_th; ++i) if (!tg_finite(pl.samples[i])) return false;
    return pl.max_steps == trajgen_max_steps(pl);
}

// what every generating call checks: the plan, the start state, the slots, the 64 pi bound
inline bool trajgen_call_ok(const gem_dwa_plan* pl, const float pos[3], const float vel[3], int T)
{
    if (!pl || !pos || !vel || !trajgen_plan_ok(*pl)) return false;
    for (int i = 0; i < 3; ++i) if (!tg_finite(pos[i]) || !tg_finite(vel[i])) return false;
    if (T < 1 || T > kTrajgenMaxPosesPerTraj || pl->n_traj > kTrajgenMaxPoses / T || pl->max_steps > T) return false;
    double w = std::fabs((double)vel[2]);
    for (int i = pl->n_x + pl->n_y; i < pl->n_x + pl->n_y + pl->n_th; ++i) w = tg_max(w, std::fabs((double)pl->samples[i]));
    return std::fabs((double)pos[2]) + pl->config.sim_time * w <= kTrajgenThetaBound;
}

// the twin of k_trajgen for one sample; poses: the sample's T slots
inline void trajgen_one(const TrajgenParams& p, const float* lists, long long t, long long n_traj, gem_footprint_pose* poses, int* traj_len,
                        double* ext, float* out_vel)
{
    float s0, s1, s2, v0, v1, v2;
    double dt;
    trajgen_sample(p, lists, (unsigned)t, s0, s1, s2);
    const int n = trajgen_start(p, s0, s1, s2, dt, v0, v1, v2);
    if (traj_len) traj_len[t] = n;
    if (ext) { ext[t] = trajgen_oscillation(p.osc, v0, v1, v2); ext[n_traj + t] = fabs((double)v2); }
    if (out_vel) { out_vel[3 * t] = v0; out_vel[3 * t + 1] = v1; out_vel[3 * t + 2] = v2; }
    if (!poses) return;
    float x = p.pos[0], y = p.pos[1], th = p.pos[2];
    for (int i = 0; i < n; ++i) {
        double sn, cs, sn2, cs2;
        gem_sincos((double)th, sn, cs);
        gem_sincos(kTrajgenPi2 + (double)th, sn2, cs2);
        poses[i] = gem_footprint_pose{(double)x, (double)y, cs, sn};
        if (p.cont) {
            v0 = trajgen_new_velocity(s0, v0, p.acc[0], dt);
            v1 = trajgen_new_velocity(s1, v1, p.acc[1], dt);
            v2 = trajgen_new_velocity(s2, v2, p.acc[2], dt);
        }
        const float nx = (float)((double)x + ((double)v0 * cs + (double)v1 * cs2) * dt);
        const float ny = (float)((double)y + ((double)v0 * sn + (double)v1 * sn2) * dt);
        th = (float)((double)th + (double)v2 * dt);
        x = nx; y = ny;
    }
}

inline int trajgen_generate_host(const gem_dwa_plan* pl, const float pos[3], const float vel[3], gem_footprint_pose* poses, int* traj_len,
                                 double* ext, float* out_vel, int T)
{
    if (!trajgen_call_ok(pl, pos, vel, T)) return GEM_ERR_INVALID;
    if (pl->n_traj > 0 && (!poses || !traj_len || !ext)) return GEM_ERR_INVALID;
    const TrajgenParams p = trajgen_params(*pl, pos, vel);
    for (long long t = 0; t < pl->n_traj; ++t) trajgen_one(p, pl->samples, t, pl->n_traj, poses + t * T, traj_len, ext, out_vel);
    return GEM_OK;
}

inline int trajgen_velocity_host(const gem_dwa_plan* pl, const float vel[3], long long index, float out[3])
{
    if (!pl || !vel || !out || !trajgen_plan_ok(*pl) || index < 0 || index >= pl->n_traj) return GEM_ERR_INVALID;
    for (int i = 0; i < 3; ++i) if (!tg_finite(vel[i])) return GEM_ERR_INVALID;
    const TrajgenParams p = trajgen_params(*pl, nullptr, vel);
    float s0, s1, s2;
    double dt;
    trajgen_sample(p, pl->samples, (unsigned)index, s0, s1, s2);
    trajgen_start(p, s0, s1, s2, dt, out[0], out[1], out[2]);
    return GEM_OK;
}

#if defined(__HIPCC__)
struct TrajgenArgs {
    gem_footprint_pose* poses;          // [n_traj * T]
    int* traj_len;                      // [n_traj]
    double* ext;                        // [2 * n_traj]: oscillation | twirling
    float* vel_out;                     // [3 * n_traj] or NULL
    long long n_traj;
    int T;
    TrajgenParams p;
    float lists[kTrajgenMaxList];
};

// the lane-group width for T pose slots a trajectory: 8 / 16 / 32
int trajgen_group_width(int T);

hipError_t launch_trajgen(hipStream_t st, const TrajgenArgs& a);
#endif

} // namespace gem
