// gem_trajgen.hip -- DWA's sampled trajectories on the device, gfx950: SimpleTrajectoryGenerator's poses, the per-sample lengths and the
// two velocity-only critics' columns, written where gem_costmap_best_trajectory_device reads them.  The contract is restated in
// include/gem_hip_trajgen.h; the arithmetic is gem_trajgen.hpp's, shared with the host twin, and the cosine is gem_sincos.hpp's: no
// transcendental of anybody's library, every operation rounded on its own (-ffp-contract=off).
//
// k_trajgen.  The lane-group scheme of k_critics: a group of G lanes owns a trajectory and strides over the samples.  The recurrences are
// serial but cheap -- a double add rounded to float for theta, the same for x and y, and with continued acceleration three clamped
// velocity updates -- while the two cosine evaluations of a step are the arithmetic, and they are independent once the thetas exist.
// So, G steps at a time:
//   1. every lane runs the theta (and velocity) chain of the G steps redundantly and keeps the theta and velocities of step base + l;
//   2. lane l evaluates sin / cos of its theta and of M_PI_2 + theta and the step's two increments;
//   3. the x / y chain runs uniformly in the group, the increments broadcast by shuffle; lane l keeps the position before its step;
//   4. lane l stores pose base + l: a group writes G consecutive 32-byte poses.
// Lane 0 writes the length, the two external scores and, when asked, (xv, yv, thetav).  A sample that is not generated writes length
// 0 and no pose; slots past the length are not touched.  No global atomic, no spin-wait, no waiting on another workgroup; every loop is
// bounded by a count in its own condition; only vector loads and stores touch memory.
#include "gem_trajgen.hpp"

namespace gem {

template <int G>
__global__ __launch_bounds__(kTrajgenThreads) void k_trajgen(TrajgenArgs a)
{
    constexpr int kGroups = kTrajgenThreads / G;
    const int l = (int)threadIdx.x & (G - 1);
    const TrajgenParams& p = a.p;
    const long long stride = (long long)gridDim.x * kGroups;
    for (long long t = (long long)blockIdx.x * kGroups + (long long)(threadIdx.x / G); t < a.n_traj; t += stride) {
        float s0, s1, s2, v0, v1, v2;
        double dt;
        trajgen_sample(p, a.lists, (unsigned)t, s0, s1, s2);
        int n = trajgen_start(p, s0, s1, s2, dt, v0, v1, v2);
        if (n > a.T) n = 0;                                             // (the host refused it: max_steps <= T.  No slot beyond T is ever written.)
        if (l == 0) {
            a.traj_len[t] = n;
            a.ext[t] = trajgen_oscillation(p.osc, v0, v1, v2);
            a.ext[a.n_traj + t] = fabs((double)v2);
            if (a.vel_out) { a.vel_out[3 * t] = v0; a.vel_out[3 * t + 1] = v1; a.vel_out[3 * t + 2] = v2; }
        }
        float x = p.pos[0], y = p.pos[1], th = p.pos[2];
        gem_footprint_pose* __restrict__ out = a.poses + t * a.T;
        for (int base = 0; base < n; base += G) {
            const bool mine = base + l < n;
            float my_th = 0.f, my_v0 = 0.f, my_v1 = 0.f;
#pragma nounroll
            for (int j = 0; j < G; ++j) {                               // 1. the theta chain: the pose records theta before the step
                if (j == l && mine) my_th = th;
                if (p.cont) {
                    v0 = trajgen_new_velocity(s0, v0, p.acc[0], dt);
                    v1 = trajgen_new_velocity(s1, v1, p.acc[1], dt);
                    v2 = trajgen_new_velocity(s2, v2, p.acc[2], dt);
                }
                if (j == l) { my_v0 = v0; my_v1 = v1; }
                th = (float)((double)th + (double)v2 * dt);
            }
            double sn, cs, sn2, cs2;                                    // 2. (a lane beyond the end works on theta = 0 and stores nothing)
            gem_sincos((double)my_th, sn, cs);
            gem_sincos(kTrajgenPi2 + (double)my_th, sn2, cs2);
            const double inc_x = ((double)my_v0 * cs + (double)my_v1 * cs2) * dt;
            const double inc_y = ((double)my_v0 * sn + (double)my_v1 * sn2) * dt;
            float my_x = x, my_y = y;
#pragma nounroll
            for (int j = 0; j < G; ++j) {                               // 3. the x / y chain
                const double dx = __shfl(inc_x, j, G), dy = __shfl(inc_y, j, G);
                if (j == l) { my_x = x; my_y = y; }
                x = (float)((double)x + dx);
                y = (float)((double)y + dy);
            }
            if (mine) out[base + l] = gem_footprint_pose{(double)my_x, (double)my_y, cs, sn};      // 4.
        }
    }
}

int trajgen_group_width(int T) { return T <= 8 ? 8 : (T <= 16 ? 16 : 32); }

hipError_t launch_trajgen(hipStream_t st, const TrajgenArgs& a)
{
    if (a.n_traj <= 0) return hipSuccess;
    const int G = trajgen_group_width(a.T);
    const long long groups = kTrajgenThreads / G;
    const long long nb = (a.n_traj + groups - 1) / groups;
    const unsigned blocks = (unsigned)(nb > kTrajgenMaxBlocks ? kTrajgenMaxBlocks : nb);
    switch (G) {
    case 8: hipLaunchKernelGGL(k_trajgen<8>, dim3(blocks), dim3(kTrajgenThreads), 0, st, a); break;
    case 16: hipLaunchKernelGGL(k_trajgen<16>, dim3(blocks), dim3(kTrajgenThreads), 0, st, a); break;
    default: hipLaunchKernelGGL(k_trajgen<32>, dim3(blocks), dim3(kTrajgenThreads), 0, st, a); break;
    }
    return hipGetLastError();
}

} // namespace gem
