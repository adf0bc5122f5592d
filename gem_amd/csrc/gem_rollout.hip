// gem_rollout.hip -- trajectory rollout on the device costmap, gfx950, wave64: TrajectoryPlanner::generateTrajectory for every
// candidate of createTrajectories and its pick, 64 bytes out.  The contract is restated in include/gem_hip_rollout.h; the arithmetic
// is gem_rollout.hpp's, shared with the host twin, the sine and cosine are gem_sincos.hpp's and footprintCost is foot_pose_cost of
// gem_score_device.hpp: no transcendental of anybody's library, every operation rounded on its own (-ffp-contract=off).
//
// k_rollout.  The lane-group scheme of k_trajgen / k_critics: a group of G lanes owns a candidate and strides over the plan.  G steps
// at a time:
//   1. every lane runs the velocity and theta chain of the G steps redundantly (three clamped updates and an add a step) and keeps the
//      theta before and the velocities after step base + l;
//   2. lane l evaluates its two gem_sincos and the step's two increments;
//   3. the x / y chain runs uniformly in the group, the increments broadcast by shuffle; lane l keeps the position before its step.
// The poses then stay in registers: no pose reaches memory.
//   4. lane l does worldToMap, the centre byte and the two grid loads of its own step and forms the event key step << 2 | code
//      (0: off the map, cost -1 | 1: a PATH or GOAL distance of OB or more, cost -2); the group's minimum is the first such event;
//   5. the footprints of the batch are walked pose by pose with all G lanes on a pose (the pose broadcast by shuffle), up to and
//      including the step of that event -- the footprint's -1 comes before the same step's -2 -- and the walk stops at the first
//      negative footprint.  The smaller key decides between -1 and -2.
// occ is a running max (the centre bytes joined by one shuffle reduction at the end), path / goal are those of step num_steps - 1,
// and the end pose is that step's: its lane forms `ahead`.  Lane 0 writes cost[c] and ahead[c].
//
// k_rollout_pick.  One workgroup.  Phase A is a min-reduction over (bits of cost, index): a legal cost is >= +0.0, so its bit pattern
// orders as an unsigned integer and the index breaks ties to the first, which is the strict < of the sequential loop.  Phases B - D
// run in one lane over the few dozen remaining candidates, in order (rollout_pick_tail, shared with the host).  It is a second launch
// on purpose, as k_critics_pick is: the kernel boundary is what makes the costs visible, where a "last workgroup done" ticket would need
// release / acquire across the XCDs' L2s.
//
// No global atomic, no spin-wait, no waiting on another workgroup; every loop is bounded by a count in its own condition; only vector
// loads and stores touch memory.
#include "gem_rollout.hpp"

#include "gem_score_device.hpp"

namespace gem {

static_assert(sizeof(RolloutGeom) == sizeof(CostGeom), "RolloutGeom is CostGeom");
static_assert(kRolloutMaxVertices == kFootMaxVertices, "the spec's limit");

template <int G, class Wide>
__global__ __launch_bounds__(kRolloutThreads) void k_rollout(CostGeom g, FootSpec spec, RolloutArgs a)
{
    constexpr int kGroups = kRolloutThreads / G;
    const int l = (int)threadIdx.x & (G - 1), nv = spec.n;
    const RolloutParams& p = a.p;
    double vsx = 0.0, vsy = 0.0;
    if (l < nv) { vsx = spec.xy[2 * l]; vsy = spec.xy[2 * l + 1]; }
    const long long OB = (long long)g.sx * g.sy;
    const int stride = (int)gridDim.x * kGroups;
    for (int c = (int)blockIdx.x * kGroups + (int)(threadIdx.x / G); c < p.n_cand; c += stride) {
        double sx, sy, sth;
        rollout_candidate(p, a.lists, c, sx, sy, sth);
        int n = rollout_steps(p, sx, sy, sth);
        if (n > kRolloutMaxSteps) n = kRolloutMaxSteps;                    // (the host refused it)
        const double dt = p.sim_time / (double)n;
        double x = p.pos[0], y = p.pos[1], th = p.pos[2], vx = p.vel[0], vy = p.vel[1], vth = p.vel[2];
        int occ = 0, centre = 0, pd = 0, gd = 0, ahead = kRolloutNoAhead;
        unsigned long long key = ~0ull;                                   // the first event of the trajectory
        for (int base = 0; base < n && key == ~0ull; base += G) {
            const bool mine = base + l < n;
            double my_th = 0.0, my_vx = 0.0, my_vy = 0.0;
#pragma nounroll
            for (int j = 0; j < G; ++j) {                                 // 1.
                if (j == l) my_th = th;
                vx = rollout_new_velocity(sx, vx, p.acc[0], dt);
                vy = rollout_new_velocity(sy, vy, p.acc[1], dt);
                vth = rollout_new_velocity(sth, vth, p.acc[2], dt);
                if (j == l) { my_vx = vx; my_vy = vy; }
                th = th + vth * dt;
            }
            if (!mine) my_th = 0.0;                                       // (a lane beyond the end works on theta = 0 and decides nothing)
            double sn, cs, sn2, cs2;                                      // 2.
            gem_sincos(my_th, sn, cs);
            gem_sincos(kRolloutPi2 + my_th, sn2, cs2);
            const double inc_x = (my_vx * cs + my_vy * cs2) * dt;
            const double inc_y = (my_vx * sn + my_vy * sn2) * dt;
            double my_x = x, my_y = y;
#pragma nounroll
            for (int j = 0; j < G; ++j) {                                 // 3.
                const double dx = __shfl(inc_x, j, G), dy = __shfl(inc_y, j, G);
                if (j == l) { my_x = x; my_y = y; }
                x = x + dx;
                y = y + dy;
            }
            unsigned long long ev = ~0ull;                                // 4.
            int my_pd = 0, my_gd = 0;
            if (mine) {
                uint32_t cell = 0u;
                if (!cost_cell(g, my_x, my_y, cell)) ev = (unsigned long long)(base + l) << 2;
                else {
                    const int b = (int)a.grid[cell];
                    my_pd = a.path[cell]; my_gd = a.goal[cell];
                    if (OB <= (long long)my_gd || OB <= (long long)my_pd) ev = (unsigned long long)(base + l) << 2 | 1ull;
                    else centre = b > centre ? b : centre;
                }
            }
#pragma unroll
            for (int off = G / 2; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(ev, off, G);
                ev = o < ev ? o : ev;
            }
            const int stop = ev == ~0ull ? n : (int)(ev >> 2) + (int)(ev & 1ull);       // steps whose footprint is walked: below `stop`
            const int last = base + G < stop ? base + G : stop;
            for (int s = base; s < last; ++s) {                           // 5.
                const int j = s - base;
                const FootPose P{__shfl(my_x, j, G), __shfl(my_y, j, G), __shfl(cs, j, G), __shfl(sn, j, G)};
                const int f = foot_pose_cost<G, Wide>(g, a.grid, nv, l, vsx, vsy, P, p.inscribed_lethal != 0);
                if (f < 0) { key = (unsigned long long)s << 2; break; }
                occ = f > occ ? f : occ;
            }
            key = ev < key ? ev : key;
            if (key == ~0ull && base + G >= n) {                          // the last batch of a trajectory that ran to its end
                const int e = n - 1 - base;                               // the lane of step n - 1
                double ax, ay;
                rollout_ahead_point(p, my_x, my_y, cs, sn, ax, ay);
                uint32_t cell = 0u;
                int my_ahead = kRolloutNoAhead;
                if (l == e && cost_cell(g, ax, ay, cell)) my_ahead = a.goal[cell];
                pd = __shfl(my_pd, e, G); gd = __shfl(my_gd, e, G); ahead = __shfl(my_ahead, e, G);
            }
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {
            const int o = __shfl_xor(centre, off, G);
            centre = o > centre ? o : centre;
        }
        if (l == 0) {
            double cost;
            if (key != ~0ull) { cost = (key & 3ull) ? -2.0 : -1.0; ahead = kRolloutNoAhead; }
            else cost = rollout_cost(p, pd, gd, occ > centre ? occ : centre);
            a.cost[c] = cost;
            a.ahead[c] = ahead;
        }
    }
}

__global__ __launch_bounds__(kRolloutThreads) void k_rollout_pick(RolloutArgs a)
{
    constexpr int kWaves = kRolloutThreads / 64;
    __shared__ unsigned long long s_key[kWaves];
    __shared__ long long s_index[kWaves];
    const RolloutParams& p = a.p;
    unsigned long long key = ~0ull;
    long long index = 0x7fffffffffffffffll;
    for (int c = (int)threadIdx.x; c < p.off_b; c += kRolloutThreads) {   // A
        const double v = a.cost[c];
        if (v >= 0.0) {
            const unsigned long long k = (unsigned long long)__double_as_longlong(v);
            if (k < key || (k == key && c < index)) { key = k; index = c; }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long ok = __shfl_xor(key, off, 64);
        const long long oi = __shfl_xor(index, off, 64);
        if (ok < key || (ok == key && oi < index)) { key = ok; index = oi; }
    }
    const int wave = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) { s_key[wave] = key; s_index[wave] = index; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (int w = 1; w < kWaves; ++w)
            if (s_key[w] < key || (s_key[w] == key && s_index[w] < index)) { key = s_key[w]; index = s_index[w]; }
        const bool any = key != ~0ull;
        *a.out_best = rollout_pick_tail(p, a.lists, a.cost, a.ahead, any ? index : -1ll, any ? __longlong_as_double((long long)key) : -1.0);
    }
}

int rollout_group_width(int n_vertices, int max_steps)
{
    int g = max_steps <= 8 ? 8 : (max_steps <= 16 ? 16 : 32);
    while (g < 64 && g < n_vertices + 1) g *= 2;
    return g;
}

template <int G>
static hipError_t launch_rollout_pass(hipStream_t st, const CostGeom& g, const FootSpec& spec, const RolloutArgs& a, int blocks)
{
    if (g.sx <= kFootNarrow && g.sy <= kFootNarrow)
        hipLaunchKernelGGL((k_rollout<G, uint32_t>), dim3((unsigned)blocks), dim3(kRolloutThreads), 0, st, g, spec, a);
    else
        hipLaunchKernelGGL((k_rollout<G, unsigned long long>), dim3((unsigned)blocks), dim3(kRolloutThreads), 0, st, g, spec, a);
    return hipGetLastError();
}

hipError_t launch_rollout(hipStream_t st, const CostGeom& g, const FootSpec& spec, const RolloutArgs& a, int max_steps)
{
    const int G = rollout_group_width(spec.n, max_steps);
    const int groups = kRolloutThreads / G;
    const int nb = (a.p.n_cand + groups - 1) / groups;
    const int blocks = nb > kRolloutMaxBlocks ? kRolloutMaxBlocks : nb;
    hipError_t e;
    switch (G) {
    case 8: e = launch_rollout_pass<8>(st, g, spec, a, blocks); break;
    case 16: e = launch_rollout_pass<16>(st, g, spec, a, blocks); break;
    case 32: e = launch_rollout_pass<32>(st, g, spec, a, blocks); break;
    default: e = launch_rollout_pass<64>(st, g, spec, a, blocks); break;
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rollout_pick, dim3(1), dim3(kRolloutThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace gem
