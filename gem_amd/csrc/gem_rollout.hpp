// gem_rollout.hpp -- trajectory rollout on the device costmap (internal header): the arithmetic of the contract of
// include/gem_hip_rollout.h that the kernels (gem_rollout.hip) and their host twin share, the host twin itself (plan, trajectories,
// pick: plain C++, no device), the kernels' argument block and their launcher.  Compiles without HIP too: the host twin is run on its
// own under the sanitizers (tests/cpp/rollout_host.cpp).
#pragma once

#include "../../include/gem_hip.h"
#include "gem_sincos.hpp"

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GEM_RO_HD __host__ __device__ __forceinline__
#else
#define GEM_RO_HD inline
#endif

namespace gem {

using RolloutPlan = struct ::gem_rollout_plan;                      // (the call of the same name hides the bare one)

constexpr int kRolloutThreads = 256;
constexpr int kRolloutMaxBlocks = 256;                             // a workgroup per CU; the groups stride over the rest
constexpr int kRolloutMaxList = 256;                               // GEM_ROLLOUT_MAX_LIST
constexpr int kRolloutMaxYVels = 8;                                // GEM_ROLLOUT_MAX_Y_VELS
constexpr int kRolloutMaxSteps = 4096;                             // GEM_ROLLOUT_MAX_STEPS
constexpr int kRolloutStateBits = 31;
constexpr int kRolloutEscaping = 1, kRolloutStuckLeft = 2, kRolloutStuckRight = 4, kRolloutStuckLeftStrafe = 8, kRolloutStuckRightStrafe = 16;
constexpr int kRolloutMaxVertices = 32;                            // GEM_FOOTPRINT_MAX_VERTICES
constexpr double kRolloutPi2 = 1.57079632679489661923;             // M_PI_2
constexpr double kRolloutThetaBound = 64.0 * 3.14159265358979323846 - 2.0;
constexpr int kRolloutNoAhead = -1;

// the map as worldToMap needs it (= CostGeom of gem_costmap.hpp, which needs HIP)
struct RolloutGeom {
    double ox, oy, res;
    uint32_t sx, sy;
};

// what a candidate needs beside its index, as the kernels read it
struct RolloutParams {
    double sim_time, gran, ang_gran, pdist, gdist, occdist, lookahead, min_in_place, backup_vel, dvth;
    double pos[3], vel[3], acc[3];
    double y_vels[kRolloutMaxYVels];
    int n_vx, n_vth, holonomic, n_y;
    int off_b, off_c, off_d, n_cand;
    int inscribed_lethal, state;
};

// = gem_rollout_best
struct RolloutBest {
    long long index;
    int stage, reserved;
    double cost, raw_cost, xv, yv, thetav;
    long long reserved1;
};

GEM_RO_HD double ro_min(double a, double b) { return b < a ? b : a; }       // std::min / std::max
GEM_RO_HD double ro_max(double a, double b) { return a < b ? b : a; }

// Costmap2D::worldToMap with the contract's stricter failure (cost_cell_xy of gem_costmap.hpp, for a compiler without HIP)
GEM_RO_HD bool ro_cell_xy(const RolloutGeom& g, double wx, double wy, uint32_t& mx, uint32_t& my)
{
    if (!(__builtin_fabs(wx) <= DBL_MAX && __builtin_fabs(wy) <= DBL_MAX)) return false;
    if (wx < g.ox || wy < g.oy) return false;
    const double qx = (wx - g.ox) / g.res, qy = (wy - g.oy) / g.res;
    if (!(qx < 2147483648.0 && qy < 2147483648.0)) return false;
    mx = (uint32_t)(int)qx; my = (uint32_t)(int)qy;
    return mx < g.sx && my < g.sy;
}

// the in-place candidate's simulated value
GEM_RO_HD double rollout_limited(double vth, double min_in_place) { return vth > 0 ? ro_max(vth, min_in_place) : ro_min(vth, -min_in_place); }

// candidate c of the plan: its sample
GEM_RO_HD void rollout_candidate(const RolloutParams& p, const double* lists, int c, double& sx, double& sy, double& sth)
{
    sx = 0.0; sy = 0.0; sth = 0.0;
    if (c < p.off_b) {
        const int grid = p.n_vx * p.n_vth;
        if (c < grid) {
            const int i = c / p.n_vth, j = c - i * p.n_vth;
            sx = lists[i];
            if (j > 0) sth = lists[p.n_vx + j - 1];
        } else {
            sx = 0.1; sy = c == grid ? 0.1 : -0.1;
        }
    } else if (c < p.off_c) {
        sth = rollout_limited(lists[p.n_vx + (c - p.off_b)], p.min_in_place);
    } else if (c < p.off_d) {
        sy = p.y_vels[c - p.off_c];
    } else {
        sx = p.backup_vel;
    }
}

// num_steps of a sample (a count beyond 2^30 answers 2^30: the host refuses it all the same)
GEM_RO_HD int rollout_steps(const RolloutParams& p, double sx, double sy, double sth)
{
    const double vmag = sqrt(sx * sx + sy * sy);
    const double m = ro_max(vmag * p.sim_time / p.gran, fabs(sth) / p.ang_gran) + 0.5;
    if (!(m < 1073741824.0)) return 1073741824;
    const int n = (int)m;
    return n == 0 ? 1 : n;
}

// step 6, one component
GEM_RO_HD double rollout_new_velocity(double target, double v, double acc, double dt)
{
    if (target - v >= 0) return ro_min(target, v + acc * dt);
    return ro_max(target, v - acc * dt);
}

// the cost of a trajectory that ran to its end
GEM_RO_HD double rollout_cost(const RolloutParams& p, int path, int goal, int occ)
{
    return (p.pdist * (double)path + (double)goal * p.gdist) + p.occdist * (double)occ;
}

// the point `ahead` is read at
GEM_RO_HD void rollout_ahead_point(const RolloutParams& p, double xe, double ye, double cs, double sn, double& ax, double& ay)
{
    ax = xe + p.lookahead * cs;
    ay = ye + p.lookahead * sn;
}

// phases B, C and D of the pick, in order, from phase A's winner (a_index -1 with a_cost -1.0: none): what one lane of k_rollout_pick
// and the host run.  cost / ahead: the candidates' arrays.
GEM_RO_HD RolloutBest rollout_pick_tail(const RolloutParams& p, const double* lists, const double* cost, const int* ahead, long long a_index, double a_cost)
{
    long long best = a_index;
    double best_cost = a_cost, best_yv = 0.0;
    if (best >= 0) { double sx, sth; rollout_candidate(p, lists, (int)best, sx, best_yv, sth); }
    bool bounded = false;                                                // heading_dist: unbounded until the first take
    int heading_dist = 0;
    int stage = 3;
    for (int c = p.off_b; c < p.off_c; ++c) {                            // B
        const double cc = cost[c], vth = lists[p.n_vx + (c - p.off_b)];
        if (!(cc >= 0 && (cc <= best_cost || best_cost < 0 || best_yv != 0.0))) continue;
        if (!(vth > p.dvth || vth < -p.dvth)) continue;
        const int a = ahead[c];
        if (a < 0 || (bounded && !(a < heading_dist))) continue;
        if ((vth < 0 && !(p.state & kRolloutStuckLeft)) || (!(vth < 0) && vth > 0 && !(p.state & kRolloutStuckRight))) {
            best = c; best_cost = cc; best_yv = 0.0; heading_dist = a; bounded = true;
        }
    }
    if (best_cost >= 0) stage = 1;
    else {
        for (int c = p.off_c; c < p.off_d; ++c) {                        // C
            const double cc = cost[c], vy = p.y_vels[c - p.off_c];
            if (!(cc >= 0 && (cc <= best_cost || best_cost < 0))) continue;
            const int a = ahead[c];
            if (a < 0 || (bounded && !(a < heading_dist))) continue;
            if ((vy > 0 && !(p.state & kRolloutStuckLeftStrafe)) || (!(vy > 0) && vy < 0 && !(p.state & kRolloutStuckRightStrafe))) {
                best = c; best_cost = cc; best_yv = vy; heading_dist = a; bounded = true;
            }
        }
        if (best_cost >= 0) stage = 2;
    }
    RolloutBest out{};
    double raw = best_cost;
    if (stage == 3) {                                                    // D
        best = p.off_d;
        raw = cost[p.off_d];
        best_cost = raw == -1.0 ? 1.0 : raw;
    }
    out.index = best; out.stage = stage; out.cost = best_cost; out.raw_cost = raw;
    rollout_candidate(p, lists, (int)best, out.xv, out.yv, out.thetav);
    return out;
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------
inline bool ro_finite(double v) { return std::isfinite(v); }
inline bool ro_scale_ok(double v) { return std::isfinite(v) && !std::signbit(v); }

inline bool rollout_config_ok(const gem_rollout_config& c)
{
    const double v[] = {c.sim_time, c.sim_granularity, c.angular_sim_granularity, c.sim_period, c.pdist_scale, c.gdist_scale, c.occdist_scale,
                        c.heading_lookahead, c.max_vel_x, c.min_vel_x, c.max_vel_th, c.min_vel_th, c.min_in_place_vel_th, c.backup_vel,
                        c.acc_lim_x, c.acc_lim_y, c.acc_lim_theta, c.final_goal_x, c.final_goal_y};
    for (double x : v) if (!ro_finite(x)) return false;
    if (!(c.sim_time > 0) || !(c.sim_granularity > 0) || !(c.angular_sim_granularity > 0)) return false;
    if (c.dwa && !(c.sim_period > 0)) return false;
    if (c.vx_samples < 2 || c.vtheta_samples < 2) return false;         // (the library divides by samples - 1)
    if (c.vx_samples > kRolloutMaxList || c.vtheta_samples > kRolloutMaxList || c.vx_samples + c.vtheta_samples > kRolloutMaxList) return false;
    if (!ro_scale_ok(c.pdist_scale) || !ro_scale_ok(c.gdist_scale) || !ro_scale_ok(c.occdist_scale)) return false;
    if (c.n_y_vels < 0 || c.n_y_vels > kRolloutMaxYVels) return false;
    for (int i = 0; i < kRolloutMaxYVels; ++i) {
        if (!ro_finite(c.y_vels[i])) return false;
        if (i < c.n_y_vels && c.y_vels[i] == 0.0) return false;
    }
    return true;
}

inline RolloutParams rollout_params(const RolloutPlan& pl, const double pos[3], const double vel[3], int state, int flags)
{
    RolloutParams p{};
    const gem_rollout_config& c = pl.config;
    p.sim_time = c.sim_time; p.gran = c.sim_granularity; p.ang_gran = c.angular_sim_granularity;
    p.pdist = c.pdist_scale; p.gdist = c.gdist_scale; p.occdist = c.occdist_scale; p.lookahead = c.heading_lookahead;
    p.min_in_place = c.min_in_place_vel_th; p.backup_vel = c.backup_vel; p.dvth = pl.dvth;
    for (int i = 0; i < 3; ++i) { p.pos[i] = pos[i]; p.vel[i] = vel[i]; }
    p.acc[0] = c.acc_lim_x; p.acc[1] = c.acc_lim_y; p.acc[2] = c.acc_lim_theta;
    for (int i = 0; i < kRolloutMaxYVels; ++i) p.y_vels[i] = c.y_vels[i];
    p.n_vx = pl.n_vx; p.n_vth = pl.n_vth; p.holonomic = c.holonomic_robot != 0; p.n_y = p.holonomic ? c.n_y_vels : 0;
    p.off_b = pl.off_b; p.off_c = pl.off_c; p.off_d = pl.off_d; p.n_cand = pl.n_cand;
    p.inscribed_lethal = (flags & GEM_FOOTPRINT_INSCRIBED_LETHAL) != 0; p.state = state;
    return p;
}

inline int rollout_plan_host(const gem_rollout_config* cfg, const double pos[3], const double vel[3], int state, RolloutPlan* out)
{
    if (!cfg || !pos || !vel || !out || !rollout_config_ok(*cfg) || (state & ~kRolloutStateBits)) return GEM_ERR_INVALID;
    for (int i = 0; i < 3; ++i) if (!ro_finite(pos[i]) || !ro_finite(vel[i])) return GEM_ERR_INVALID;
    const gem_rollout_config& c = *cfg;
    RolloutPlan pl;
    std::memset(&pl, 0, sizeof pl);
    pl.config = c;
    pl.config.dwa = c.dwa != 0; pl.config.holonomic_robot = c.holonomic_robot != 0; pl.config.final_goal_valid = c.final_goal_valid != 0;
    double mx = c.max_vel_x;
    if (c.final_goal_valid) {
        const double dx = c.final_goal_x - pos[0], dy = c.final_goal_y - pos[1];
        mx = ro_min(mx, sqrt(dx * dx + dy * dy) / c.sim_time);
    }
    const double T = c.dwa ? c.sim_period : c.sim_time;
    pl.max_x = ro_max(ro_min(mx, vel[0] + c.acc_lim_x * T), c.min_vel_x);
    pl.min_x = ro_max(c.min_vel_x, vel[0] - c.acc_lim_x * T);
    pl.max_th = ro_min(c.max_vel_th, vel[2] + c.acc_lim_theta * T);
    pl.min_th = ro_max(c.min_vel_th, vel[2] - c.acc_lim_theta * T);
    pl.dvx = (pl.max_x - pl.min_x) / (double)(c.vx_samples - 1);
    pl.dvth = (pl.max_th - pl.min_th) / (double)(c.vtheta_samples - 1);
    pl.n_vx = c.vx_samples; pl.n_vth = c.vtheta_samples;
    double v = pl.min_x;
    for (int i = 0; i < pl.n_vx; ++i) { pl.lists[i] = v; v += pl.dvx; }
    v = pl.min_th;
    for (int j = 0; j < pl.n_vth; ++j) { pl.lists[pl.n_vx + j] = v; v += pl.dvth; }
    for (int i = 0; i < pl.n_vx + pl.n_vth; ++i) if (!ro_finite(pl.lists[i])) return GEM_ERR_INVALID;
    if (!ro_finite(pl.dvx) || !ro_finite(pl.dvth)) return GEM_ERR_INVALID;
    pl.state_flags = state;
    pl.off_b = (state & kRolloutEscaping) ? 0 : pl.n_vx * pl.n_vth + (c.holonomic_robot ? 2 : 0);
    pl.off_c = pl.off_b + pl.n_vth;
    pl.off_d = pl.off_c + (c.holonomic_robot ? c.n_y_vels : 0);
    pl.n_cand = pl.off_d + 1;
    const RolloutParams p = rollout_params(pl, pos, vel, state, 0);
    int most = 0;
    double w = std::fabs(vel[2]);
    for (int k = 0; k < pl.n_cand; ++k) {
        double sx, sy, sth;
        rollout_candidate(p, pl.lists, k, sx, sy, sth);
        const int n = rollout_steps(p, sx, sy, sth);
        most = n > most ? n : most;
        w = ro_max(w, std::fabs(sth));
    }
    if (most > kRolloutMaxSteps) return GEM_ERR_INVALID;
    if (!(std::fabs(pos[2]) + c.sim_time * w <= kRolloutThetaBound)) return GEM_ERR_INVALID;
    pl.max_steps = most;
    *out = pl;
    return GEM_OK;
}

// what every call checks: the plan is the one gem_rollout_plan makes from these arguments, byte for byte (it is caller memory:
// everything the kernels trust is made again)
inline bool rollout_call_ok(const RolloutPlan* pl, const double pos[3], const double vel[3], int state)
{
    if (!pl || !pos || !vel) return false;
    RolloutPlan again;
    if (rollout_plan_host(&pl->config, pos, vel, state, &again) != GEM_OK) return false;
    return std::memcmp(&again, pl, sizeof again) == 0;
}

inline bool rollout_spec_ok(const double* spec_xy, int n_vertices, int flags)
{
    if (flags & ~GEM_FOOTPRINT_INSCRIBED_LETHAL) return false;
    if (n_vertices < 0 || n_vertices > kRolloutMaxVertices || (n_vertices > 0 && !spec_xy)) return false;
    for (int i = 0; i < 2 * n_vertices; ++i) if (!ro_finite(spec_xy[i])) return false;
    return true;
}

// cell k of line(x0, y0, x1, y1): the closed form of gem_hip_footprint.h
inline void ro_line_cell(int x0, int y0, int x1, int y1, uint32_t k, uint32_t& cx, uint32_t& cy)
{
    const uint32_t dx = (uint32_t)(x1 >= x0 ? x1 - x0 : x0 - x1), dy = (uint32_t)(y1 >= y0 ? y1 - y0 : y0 - y1);
    const int xi = x1 >= x0 ? 1 : -1, yi = y1 >= y0 ? 1 : -1;
    const bool x_major = dx >= dy;
    const uint32_t major = x_major ? dx : dy, minor = x_major ? dy : dx;
    const uint32_t m = major ? (uint32_t)(((unsigned long long)(major / 2u) + (unsigned long long)k * minor) / major) : 0u;
    cx = (uint32_t)(x0 + xi * (int)(x_major ? k : m));
    cy = (uint32_t)(y0 + yi * (int)(x_major ? m : k));
}

// footprintCost of gem_hip_footprint.h as the sequential loop it is stated as (the kernel's is foot_pose_cost of gem_score_device.hpp)
inline int rollout_foot_cost_host(const RolloutGeom& g, const unsigned char* grid, const double* spec_xy, int n, double x, double y, double cs,
                                  double sn, bool inscribed_lethal)
{
    uint32_t mx, my;
    if (!ro_cell_xy(g, x, y, mx, my)) return -3;
    if (n < 3) {
        const unsigned char c = grid[(size_t)my * g.sx + mx];
        return c == 255 ? -2 : (c >= 253 ? -1 : (int)c);
    }
    int vx[kRolloutMaxVertices], vy[kRolloutMaxVertices];
    for (int i = 0; i < n; ++i) {
        const double wx = x + (spec_xy[2 * i] * cs - spec_xy[2 * i + 1] * sn), wy = y + (spec_xy[2 * i] * sn + spec_xy[2 * i + 1] * cs);
        uint32_t ax, ay;
        if (ro_cell_xy(g, wx, wy, ax, ay)) { vx[i] = (int)ax; vy[i] = (int)ay; } else { vx[i] = -1; vy[i] = 0; }
    }
    int best = 0;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 == n ? 0 : i + 1;
        if (vx[i] < 0 || vx[j] < 0) return -3;
        const uint32_t dx = (uint32_t)std::abs(vx[j] - vx[i]), dy = (uint32_t)std::abs(vy[j] - vy[i]), len = (dx > dy ? dx : dy) + 1u;
        for (uint32_t k = 0; k < len; ++k) {
            uint32_t cx, cy;
            ro_line_cell(vx[i], vy[i], vx[j], vy[j], k, cx, cy);
            const unsigned char c = grid[(size_t)cy * g.sx + cx];
            if (c == 255) return -2;
            if (c == 254 || (c == 253 && inscribed_lethal)) return -1;
            best = (int)c > best ? (int)c : best;
        }
    }
    return best;
}

// the twin of k_rollout for one candidate; poses: the candidate's max_steps slots or NULL.  Returns the cost.
inline double rollout_one_host(const RolloutParams& p, const double* lists, int c, const RolloutGeom& g, const unsigned char* grid, const int* path,
                               const int* goal, const double* spec_xy, int n_vertices, int* out_ahead, int* out_steps, gem_footprint_pose* poses)
{
    double sx, sy, sth;
    rollout_candidate(p, lists, c, sx, sy, sth);
    const int n = rollout_steps(p, sx, sy, sth);
    const double dt = p.sim_time / (double)n;
    const long long OB = (long long)g.sx * g.sy;
    double x = p.pos[0], y = p.pos[1], th = p.pos[2], vx = p.vel[0], vy = p.vel[1], vth = p.vel[2];
    int occ = 0, pd = 0, gd = 0, recorded = 0;
    double cost = 0.0, xe = 0, ye = 0, ce = 1, se = 0;
    bool failed = false;
    for (int i = 0; i < n; ++i) {
        uint32_t mx, my;
        if (!ro_cell_xy(g, x, y, mx, my)) { cost = -1.0; failed = true; break; }
        double sn, cs, sn2, cs2;
        gem_sincos(th, sn, cs);
        gem_sincos(kRolloutPi2 + th, sn2, cs2);
        const int f = rollout_foot_cost_host(g, grid, spec_xy, n_vertices, x, y, cs, sn, p.inscribed_lethal != 0);
        if (f < 0) { cost = -1.0; failed = true; break; }
        const size_t cell = (size_t)my * g.sx + mx;
        const int b = (int)grid[cell];
        occ = occ > f ? occ : f;
        occ = occ > b ? occ : b;
        pd = path[cell]; gd = goal[cell];
        if (OB <= (long long)gd || OB <= (long long)pd) { cost = -2.0; failed = true; break; }
        if (poses) poses[i] = gem_footprint_pose{x, y, cs, sn};
        xe = x; ye = y; ce = cs; se = sn;
        ++recorded;
        vx = rollout_new_velocity(sx, vx, p.acc[0], dt);
        vy = rollout_new_velocity(sy, vy, p.acc[1], dt);
        vth = rollout_new_velocity(sth, vth, p.acc[2], dt);
        x = x + (vx * cs + vy * cs2) * dt;
        y = y + (vx * sn + vy * sn2) * dt;
        th = th + vth * dt;
    }
    int ahead = kRolloutNoAhead;
    if (!failed) {
        cost = rollout_cost(p, pd, gd, occ);
        double ax, ay;
        rollout_ahead_point(p, xe, ye, ce, se, ax, ay);
        uint32_t mx, my;
        if (ro_cell_xy(g, ax, ay, mx, my)) ahead = goal[(size_t)my * g.sx + mx];
    }
    if (out_ahead) *out_ahead = ahead;
    if (out_steps) *out_steps = recorded;
    return cost;
}

inline RolloutBest rollout_pick_host(const RolloutParams& p, const double* lists, const double* cost, const int* ahead)
{
    long long best = -1;
    double best_cost = -1.0;
    for (int c = 0; c < p.off_b; ++c)                                    // A: strict <, in order
        if (cost[c] >= 0 && (cost[c] < best_cost || best_cost < 0)) { best = c; best_cost = cost[c]; }
    return rollout_pick_tail(p, lists, cost, ahead, best, best_cost);
}

inline int rollout_pick_checked(const RolloutPlan* pl, int state, const double* cost, const int* ahead, gem_rollout_best* out_best)
{
    if (!pl || !cost || !ahead || !out_best || (state & ~kRolloutStateBits)) return GEM_ERR_INVALID;
    // (the pick needs no state: the plan's own fields are checked for what the loops index by)
    if (!rollout_config_ok(pl->config) || pl->n_vx != pl->config.vx_samples || pl->n_vth != pl->config.vtheta_samples) return GEM_ERR_INVALID;
    const int escaping = (state & kRolloutEscaping) != 0;
    const int off_b = escaping ? 0 : pl->n_vx * pl->n_vth + (pl->config.holonomic_robot ? 2 : 0);
    const int off_c = off_b + pl->n_vth, off_d = off_c + (pl->config.holonomic_robot ? pl->config.n_y_vels : 0);
    if (((pl->state_flags & kRolloutEscaping) != 0) != (escaping != 0) || (pl->state_flags & ~kRolloutStateBits) || pl->off_b != off_b || pl->off_c != off_c || pl->off_d != off_d || pl->n_cand != off_d + 1) return GEM_ERR_INVALID;
    for (int i = 0; i < pl->n_vx + pl->n_vth; ++i) if (!ro_finite(pl->lists[i])) return GEM_ERR_INVALID;
    if (!ro_finite(pl->dvth)) return GEM_ERR_INVALID;
    const double zero[3] = {0.0, 0.0, 0.0};
    const RolloutParams p = rollout_params(*pl, zero, zero, state, 0);
    const RolloutBest b = rollout_pick_host(p, pl->lists, cost, ahead);
    std::memcpy(out_best, &b, sizeof b);
    return GEM_OK;
}

inline int rollout_host(const RolloutPlan* pl, const double pos[3], const double vel[3], const gem_costmap_config* geometry, const unsigned char* bytes,
                        const int* path, const int* goal, const double* spec_xy, int n_vertices, int flags, double* out_cost, int* out_ahead,
                        int* out_steps, gem_footprint_pose* out_poses, gem_rollout_best* out_best)
{
    if (!geometry || !bytes || !path || !goal || !out_cost || !out_ahead || !out_steps || !out_best) return GEM_ERR_INVALID;
    if (geometry->size_x < 1u || geometry->size_y < 1u || (unsigned long long)geometry->size_x * geometry->size_y > 2147483646ull) return GEM_ERR_INVALID;
    if (!ro_finite(geometry->resolution) || !(geometry->resolution > 0) || !ro_finite(geometry->origin_x) || !ro_finite(geometry->origin_y)) return GEM_ERR_INVALID;
    if (!pl || !rollout_spec_ok(spec_xy, n_vertices, flags) || !rollout_call_ok(pl, pos, vel, pl->state_flags)) return GEM_ERR_INVALID;
    const int state = pl->state_flags;
    const RolloutGeom g{geometry->origin_x, geometry->origin_y, geometry->resolution, geometry->size_x, geometry->size_y};
    const RolloutParams p = rollout_params(*pl, pos, vel, state, flags);
    for (int c = 0; c < pl->n_cand; ++c)
        out_cost[c] = rollout_one_host(p, pl->lists, c, g, bytes, path, goal, spec_xy, n_vertices, out_ahead + c, out_steps + c,
                                       out_poses ? out_poses + (size_t)c * (size_t)pl->max_steps : nullptr);
    const RolloutBest b = rollout_pick_host(p, pl->lists, out_cost, out_ahead);
    std::memcpy(out_best, &b, sizeof b);
    return GEM_OK;
}

#if defined(__HIPCC__)
struct RolloutArgs {
    const unsigned char* grid;
    const int* path;
    const int* goal;
    double* cost;                       // [n_cand]
    int* ahead;                         // [n_cand]
    RolloutBest* out_best;
    RolloutParams p;
    double lists[kRolloutMaxList];
};

// the lane-group width: the smallest of 8 / 16 / 32 / 64 with a lane beyond the vertices and no smaller than the step count asks for
int rollout_group_width(int n_vertices, int max_steps);

struct CostGeom;
struct FootSpec;
// both launches: k_rollout over the candidates, then k_rollout_pick
hipError_t launch_rollout(hipStream_t st, const CostGeom& g, const FootSpec& spec, const RolloutArgs& a, int max_steps);
#endif

} // namespace gem
