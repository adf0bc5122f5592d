// gem_critics.hip -- the best trajectory on the device costmap, gfx950: every critic of every trajectory in one pass over the poses,
// combined as SimpleScoredSamplingPlanner::scoreTrajectory does, and findBestTrajectory's winner.  The contract is restated in
// include/gem_hip_critics.h.  Double arithmetic only where the contract has it (a score's conversion, the scale's product, the sum);
// no transcendental; grids and bytes through plain loads.
//
// Pass 1, k_critics.  The lane-group scheme of gem_footprint.hip / gem_mapgrid.hip: a group of G lanes owns whole trajectories and
// strides over the batch.  The critics of a trajectory run in list order; a rejection skips the rest, and so does a zero scale.
//   obstacle  the poses one after the other with all G lanes on a pose (foot_pose_cost), stopping at the first negative pose;
//   grid      the poses dealt to the lanes, p = l, l + G, ..., the MIN of the event keys pose << 2 | code for "the first negative event
//             decides" and 64-bit shuffle sums (k_mapgrid_score's loop, mapgrid_pose_code);
//   external  one load, the same address in every lane of the group.
// Every lane of a group holds the same total, so the walk is uniform in the group; lane 0 writes out_total[t] when asked and keeps the
// group's best (key, index) and valid count, key = the bits of the total: a valid total is >= +0.0 (never -0.0: it starts at +0.0 and
// only non-negative terms are added), so its bit pattern orders as an unsigned 64-bit integer, +inf included, and the index breaks
// ties.  The workgroup then reduces over its groups, by shuffles in a wave and through LDS across the waves, and writes ONE candidate.
//
// Pass 2, k_critics_pick.  One workgroup reduces the candidates and writes the 32 bytes.  It is a second launch on purpose: the kernel
// boundary is what makes the candidates visible, where a "last workgroup done" ticket would need release / acquire across the XCDs'
// L2s.  So there is nothing to wait on and nothing can hang: no spin-wait, no atomic on global memory, no waiting on another
// workgroup, and every loop is bounded by a count in its own condition.  Only vector loads and stores touch memory.
#include "gem_critics.hpp"

#include "gem_score_device.hpp"

namespace gem {

constexpr long long kNoIndex = 0x7fffffffffffffffll;

// (key, index) <- the smaller of it and (ok, oi): the smaller key, then the smaller index
__device__ __forceinline__ void critics_take(unsigned long long& key, long long& index, unsigned long long ok, long long oi)
{
    if (ok < key || (ok == key && oi < index)) { key = ok; index = oi; }
}

// the workgroup's (key, index, count) from every thread's; thread 0 returns it
__device__ __forceinline__ void critics_reduce_block(unsigned long long& key, long long& index, long long& count)
{
    constexpr int kWaves = kCriticsThreads / 64;
    __shared__ unsigned long long s_key[kWaves];
    __shared__ long long s_index[kWaves], s_count[kWaves];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long ok = __shfl_xor(key, off, 64);
        const long long oi = __shfl_xor(index, off, 64);
        count += __shfl_xor(count, off, 64);
        critics_take(key, index, ok, oi);
    }
    const int wave = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) { s_key[wave] = key; s_index[wave] = index; s_count[wave] = count; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (int w = 1; w < kWaves; ++w) {
            critics_take(key, index, s_key[w], s_index[w]);
            count += s_count[w];
        }
    }
}

template <int G, class Wide>
__global__ __launch_bounds__(kCriticsThreads) void k_critics(CostGeom g, FootSpec spec, CriticsArgs a)
{
    constexpr int kGroups = kCriticsThreads / G;
    const int l = (int)threadIdx.x & (G - 1), n = spec.n;
    double sx = 0.0, sy = 0.0;
    if (l < n) { sx = spec.xy[2 * l]; sy = spec.xy[2 * l + 1]; }
    const long long OB = (long long)g.sx * g.sy, UN = OB + 1;
    unsigned long long best_key = ~0ull;
    long long best_index = kNoIndex, n_valid = 0;
    const long long stride = (long long)gridDim.x * kGroups;
    for (long long t = (long long)blockIdx.x * kGroups + (long long)(threadIdx.x / G); t < a.n_traj; t += stride) {
        const int len = a.traj_len ? a.traj_len[t] : a.T;
        const FootPose* __restrict__ poses = a.poses + t * a.T;
        double total = 0.0;
        if (len < 1 || len > a.T) total = -5.0;                         // a length nobody could refuse: rejected, no pose is read
        else for (int k = 0; k < a.n_critics; ++k) {
            const double scale = a.c[k].scale;
            if (scale == 0.0) continue;
            const int kind = a.c[k].kind, flags = a.c[k].flags;
            double s;
            if (kind == kCriticExternal) {
                s = a.ext[(long long)a.c[k].column * a.n_traj + t];
            } else if (kind == kCriticObstacle) {
                int first_neg = 0, acc = 0;
                for (int p = 0; p < len; ++p) {
                    const FootPose P = poses[p];
                    int r = foot_pose_cost<G, Wide>(g, a.grid, n, l, sx, sy, P, (flags & 1) != 0);
                    if (r < 0) { first_neg = r; break; }                // nothing behind it can change the score
                    if (flags & kCriticCentreCost) {                    // (r >= 0: the centre is on the map)
                        uint32_t cell = 0u;
                        if (cost_cell(g, P.x, P.y, cell)) {
                            const int b = (int)a.grid[cell];
                            r = b > r ? b : r;
                        }
                    }
                    acc = (flags & 2) ? acc + r : (r > acc ? r : acc);
                }
                s = (double)(first_neg ? first_neg : acc);
            } else {
                const int* __restrict__ dist = a.dist[a.c[k].grid];
                const double xshift = a.c[k].xshift;
                unsigned long long key = ~0ull;                         // the earliest negative event of this lane
                long long sum = 0, last = 0;
                for (int p = l; p < len; p += G) {
                    const FootPose P = poses[p];
                    long long dd;
                    const int code = mapgrid_pose_code(g, dist, P, xshift, (flags & 1) != 0, OB, UN, dd);
                    if (code >= 0) {
                        const unsigned long long e = (unsigned long long)p << 2 | (unsigned long long)code;
                        key = e < key ? e : key;
                        break;                                          // this lane's later poses come later in the walk
                    }
                    sum += dd;
                    if (p == len - 1) last = dd;
                }
#pragma unroll
                for (int off = G / 2; off > 0; off >>= 1) {
                    const unsigned long long o = __shfl_xor(key, off, G);
                    key = o < key ? o : key;
                    sum += __shfl_xor(sum, off, G);
                    last += __shfl_xor(last, off, G);
                }
                s = (double)(key != ~0ull ? (long long)(key & 3ull) - 4 : ((flags & 2) ? sum : last));
            }
            if (s < 0.0) { total = s; break; }
            if (s != 0.0) s = s * scale;
            total = total + s;
        }
        if (l == 0) {
            if (a.out_total) a.out_total[t] = total;
            if (total >= 0.0) {                                         // (false for a NaN)
                ++n_valid;
                critics_take(best_key, best_index, (unsigned long long)__double_as_longlong(total), t);
            }
        }
    }
    critics_reduce_block(best_key, best_index, n_valid);
    if (threadIdx.x == 0u) a.cand[blockIdx.x] = CriticsCandidate{best_key, best_index, n_valid};
}

__global__ __launch_bounds__(kCriticsThreads) void k_critics_pick(const CriticsCandidate* __restrict__ cand, int n_cand, CriticsBest* __restrict__ out)
{
    unsigned long long key = ~0ull;
    long long index = kNoIndex, n_valid = 0;
    for (int i = (int)threadIdx.x; i < n_cand; i += kCriticsThreads) {
        const CriticsCandidate c = cand[i];
        critics_take(key, index, c.key, c.index);
        n_valid += c.n_valid;
    }
    critics_reduce_block(key, index, n_valid);
    if (threadIdx.x == 0u) {
        const bool any = key != ~0ull;                                  // (all-ones is a NaN's pattern: never a valid total)
        *out = CriticsBest{any ? index : -1ll, n_valid, any ? __longlong_as_double((long long)key) : -1.0, 0ll};
    }
}

int critics_group_width(int n_vertices, int T)
{
    int g = T <= 8 ? 8 : (T <= 16 ? 16 : 32);
    while (g < 64 && g < n_vertices + 1) g *= 2;
    return g;
}

template <int G>
static hipError_t launch_pass1(hipStream_t st, const CostGeom& g, const FootSpec& spec, const CriticsArgs& a, int blocks)
{
    if (g.sx <= kFootNarrow && g.sy <= kFootNarrow)
        hipLaunchKernelGGL((k_critics<G, uint32_t>), dim3((unsigned)blocks), dim3(kCriticsThreads), 0, st, g, spec, a);
    else
        hipLaunchKernelGGL((k_critics<G, unsigned long long>), dim3((unsigned)blocks), dim3(kCriticsThreads), 0, st, g, spec, a);
    return hipGetLastError();
}

hipError_t launch_critics(hipStream_t st, const CostGeom& g, const FootSpec& spec, const CriticsArgs& a)
{
    int blocks = 0;
    if (a.n_traj > 0) {
        const int G = critics_group_width(spec.n, a.T);
        const long long groups = kCriticsThreads / G;
        const long long nb = (a.n_traj + groups - 1) / groups;
        blocks = (int)(nb > kCriticsMaxBlocks ? kCriticsMaxBlocks : nb);
        hipError_t e;
        switch (G) {
        case 8: e = launch_pass1<8>(st, g, spec, a, blocks); break;
        case 16: e = launch_pass1<16>(st, g, spec, a, blocks); break;
        case 32: e = launch_pass1<32>(st, g, spec, a, blocks); break;
        default: e = launch_pass1<64>(st, g, spec, a, blocks); break;
        }
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_critics_pick, dim3(1), dim3(kCriticsThreads), 0, st, a.cand, blocks, a.out_best);
    return hipGetLastError();
}

} // namespace gem
