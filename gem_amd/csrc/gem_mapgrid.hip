// gem_mapgrid.hip -- base_local_planner's MapGrid on the device costmap, gfx950: the path and goal distance grids
// (computeTargetDistance through the non-blocked cells of the grid where it lies) and MapGridCostFunction::scoreTrajectory for batches
// of trajectories.  The contract is restated in include/gem_hip_mapgrid.h.  Integer code except the two shift products of scoring.
//
// Distance.  k_mapgrid_distance: ONE workgroup per requested grid (PATH | GOAL is one launch of two).  The search runs on bit planes,
// a 64-bit word holding 64 cells of a row, rows padded to whole words: at most kMapGridMaxWords words a plane.  A thread OWNS up to
// kMapGridWordsPerThread words (w = thread + k * blockDim); its open, unvisited and source words stay in registers for the whole
// search, so the LDS holds three planes of at most 32 KB: `open` while it is built, and the two frontiers.
//   prologue  a wave's ballot over 64 bytes of a row is that row's `open` word (1: not blocked; the pad bits are 0 and act as the wall),
//             the way k_inflate_seeds makes its seed words.  The run of the plan (first accepted point a, first point above it that
//             is not accepted b) comes from two workgroup-wide integer min-reductions in LDS (ds_min) over the accepted flags; the
//             cells of a .. b-1 (the goal grid: of b-1 alone) are set in frontier 0 (ds_or) and store distance 0.
//   level d   next = (F << 1 | carry of the left word | F >> 1 | carry of the right word | word above | word below) & unvisited;
//             unvisited &= ~next; every set bit of next stores d.  A word with nothing unvisited reads nothing and has next = 0.
//             The frontier is double-buffered.  ONE barrier per level separates the levels; a flag word in LDS, set by whoever
//             found a new cell, ends the loop when next is empty everywhere.  The barrier is the bare instruction behind a wait
//             for the LDS counter only (mapgrid_lds_barrier says why).
//   epilogue  E = sources | (open & ~unvisited) goes to a frontier plane; the cells of dilate4(E) & ~open & ~sources store OB.
// No hang by construction: every level but the last reaches at least one new cell, so the loop is bounded by the cell count (and
// stated so in its condition); there is no spin-wait, no waiting on another workgroup and no atomic on global memory.  Every cell's
// distance is stored by the one thread that owns its word (sources: by whoever marks them, always 0), after the fill launch that
// made the grid UN.  Only vector loads and stores touch memory.
//
// Scoring.  k_mapgrid_score: the lane-group scheme of gem_footprint.hip.  A group of G lanes owns whole trajectories; lane l takes
// poses l, l + G, ...; a negative event carries its place in the sequential walk, pose << 2 | (answer + 4), and the group takes the
// integer MIN of these keys: "the first negative event decides", whatever the timing.  Last is the last pose's d, Sum a 64-bit sum;
// both are reduced by shuffles.  A pose's own part (shift, worldToMap, the cell's distance, its event) is mapgrid_pose_code of
// gem_score_device.hpp, which k_critics (gem_critics.hip) shares.
#include "gem_score_device.hpp"

#include <mutex>

namespace gem {

static_assert(kMapGridMaxWords == (uint32_t)(kMapGridMaxThreads * kMapGridWordsPerThread), "a thread owns a fixed number of words");

__global__ __launch_bounds__(256) void k_mapgrid_fill(int* __restrict__ d0, int* __restrict__ d1, uint32_t cells, int value)
{
    int* d = blockIdx.y ? d1 : d0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < cells; i += gridDim.x * 256u) d[i] = value;
}

// every set bit of `bits` (cells base .. base + 63 of a row) stores v
__device__ __forceinline__ void mapgrid_store_bits(int* __restrict__ row, unsigned long long bits, int v)
{
    while (bits) {
        row[__builtin_ctzll(bits)] = v;
        bits &= bits - 1ull;
    }
}

// The barrier between two levels.  __syncthreads() would also wait for every distance store still on its way to memory
// (vmcnt(0): the stores of a level are about a microsecond away), level after level; the levels hand each other LDS words only,
// so the LDS counter is waited for and the barrier is the bare instruction.  Nobody reads a distance before the kernel ends.
__device__ __forceinline__ void mapgrid_lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

__global__ __launch_bounds__(kMapGridMaxThreads) void k_mapgrid_distance(MapGridArgs a)
{
    extern __shared__ unsigned long long s_planes[];
    __shared__ int s_run[2];
    __shared__ int s_any[3];
    const uint32_t W = a.nw * a.sy, nt = blockDim.x, tid = threadIdx.x;
    unsigned long long* s_open = s_planes;
    unsigned long long* const s_f0 = s_planes + W;                      // frontier p: s_f0 + p * W
    int* __restrict__ dist = a.dist[blockIdx.x];
    int* __restrict__ status = a.status[blockIdx.x];
    const bool goal = a.goal[blockIdx.x] != 0;
    const int OB = (int)(a.sx * a.sy);

    // ---- prologue: the open plane (eight words' loads in flight per wave), frontier 0 cleared
    {
        const uint32_t lane = tid & 63u, wave = tid >> 6, waves = nt >> 6;
        for (uint32_t w0 = wave * 8u; w0 < W; w0 += waves * 8u) {       // (w0 is the same in the whole wave)
            unsigned char byte[8];
            bool in[8];
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j) {                         // (no branch around a load: the eight go out together)
                const uint32_t w = w0 + j, y = w / a.nw, x = (w - y * a.nw) * 64u + lane;
                in[j] = w < W && x < a.sx;
                byte[j] = a.grid[in[j] ? (size_t)y * a.sx + x : (size_t)0];
            }
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j) {
                const unsigned long long word = __ballot(in[j] && byte[j] < kMapGridBlocked);
                if (lane == 0u && w0 + j < W) s_open[w0 + j] = word;
            }
        }
        for (uint32_t w = tid; w < W; w += nt) s_f0[w] = 0ull;
        if (tid == 0u) { s_run[0] = a.n; s_run[1] = a.n; s_any[0] = s_any[1] = s_any[2] = 0; }
    }
    __syncthreads();
    // the run: a = the first accepted point
    for (int i = (int)tid; i < a.n; i += (int)nt) {
        const int c = a.cells[i];
        if (c >= 0 && a.grid[c] != kCostNoInfo) { atomicMin(&s_run[0], i); break; }     // (i only grows in a thread)
    }
    __syncthreads();
    const int ra = s_run[0];
    if (ra >= a.n) {                                                    // no accepted point: the grid stays UN (uniform exit)
        if (tid == 0u) { status[kMapGridStarted] = 0; status[kMapGridGoalX] = -1; status[kMapGridGoalY] = -1; status[kMapGridLevels] = 0; }
        return;
    }
    // b = the first point above a that is not accepted
    for (int i = ra + 1 + (int)tid; i < a.n; i += (int)nt) {
        const int c = a.cells[i];
        if (!(c >= 0 && a.grid[c] != kCostNoInfo)) { atomicMin(&s_run[1], i); break; }
    }
    __syncthreads();
    const int rb = s_run[1];
    // the sources: into frontier 0, distance 0
    for (int i = (goal ? rb - 1 : ra) + (int)tid; i < rb; i += (int)nt) {
        const uint32_t c = (uint32_t)a.cells[i], y = c / a.sx, x = c - y * a.sx;
        atomicOr(&s_f0[y * a.nw + (x >> 6)], 1ull << (x & 63u));
        dist[c] = 0;
    }
    if (tid == 0u) {
        const uint32_t c = (uint32_t)a.cells[rb - 1];
        status[kMapGridStarted] = 1; status[kMapGridGoalX] = (int)(c % a.sx); status[kMapGridGoalY] = (int)(c / a.sx);
    }
    __syncthreads();

    // a thread's own words: open, sources, unvisited in registers; where the word lies
    unsigned long long open[kMapGridWordsPerThread], src[kMapGridWordsPerThread], unv[kMapGridWordsPerThread];
    uint32_t at[kMapGridWordsPerThread];                                // 1: a word to the left | 2: right | 4: above | 8: below | 16: mine
#pragma unroll
    for (int k = 0; k < kMapGridWordsPerThread; ++k) {
        const uint32_t w = tid + (uint32_t)k * nt;
        open[k] = src[k] = unv[k] = 0ull; at[k] = 0u;
        if (w < W) {
            const uint32_t y = w / a.nw, c = w - y * a.nw;
            open[k] = s_open[w]; src[k] = s_f0[w]; unv[k] = open[k] & ~src[k];
            at[k] = 16u | (c > 0u ? 1u : 0u) | (c + 1u < a.nw ? 2u : 0u) | (y > 0u ? 4u : 0u) | (y + 1u < a.sy ? 8u : 0u);
        }
    }

    // ---- the levels.  s_any[d % 3] says whether level d found a cell: set before the barrier, read behind it, and cleared one
    // level ahead, when everybody has read it a barrier ago
    int cur = 0, d = 1;
    uint32_t r0 = 1u, r1 = 2u, r2 = 0u;                                 // d % 3, (d + 1) % 3, (d + 2) % 3
    for (; d <= OB; ++d) {                                              // (ends at an empty level long before)
        const unsigned long long* F = s_f0 + (cur ? W : 0u);
        unsigned long long* N = s_f0 + (cur ? 0u : W);
        if (tid == 0u) s_any[r1] = 0;
        bool any = false;
#pragma unroll
        for (int k = 0; k < kMapGridWordsPerThread; ++k) {
            if (!(at[k] & 16u)) continue;
            const uint32_t w = tid + (uint32_t)k * nt;
            unsigned long long next = 0ull;
            if (unv[k]) {
                const unsigned long long f = F[w];
                const unsigned long long l = (at[k] & 1u) ? F[w - 1u] : 0ull, r = (at[k] & 2u) ? F[w + 1u] : 0ull;
                const unsigned long long u = (at[k] & 4u) ? F[w - a.nw] : 0ull, b = (at[k] & 8u) ? F[w + a.nw] : 0ull;
                next = (f << 1 | l >> 63 | f >> 1 | r << 63 | u | b) & unv[k];
                if (next) {
                    unv[k] &= ~next;
                    const uint32_t y = w / a.nw, c = w - y * a.nw;
                    mapgrid_store_bits(dist + (size_t)y * a.sx + c * 64u, next, d);
                    any = true;
                }
            }
            N[w] = next;
        }
        if (any) s_any[r0] = 1;
        cur ^= 1;
        mapgrid_lds_barrier();
        if (!s_any[r0]) break;                                          // (the same word for everybody: a uniform exit)
        const uint32_t t = r0; r0 = r1; r1 = r2; r2 = t;
    }
    __syncthreads();                                                    // (s_any read by all before anybody goes on)

    // ---- epilogue: E into a frontier plane (nobody reads the frontiers any more), then the blocked rim
    unsigned long long* E = s_f0 + (cur ? 0u : W);
#pragma unroll
    for (int k = 0; k < kMapGridWordsPerThread; ++k)
        if (at[k] & 16u) E[tid + (uint32_t)k * nt] = src[k] | (open[k] & ~unv[k]);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kMapGridWordsPerThread; ++k) {
        if (!(at[k] & 16u)) continue;
        const uint32_t w = tid + (uint32_t)k * nt, y = w / a.nw, c = w - y * a.nw;
        const uint32_t left = a.sx - c * 64u;                           // cells of the row from this word on
        const unsigned long long in_row = left >= 64u ? ~0ull : (1ull << left) - 1ull;
        const unsigned long long e = E[w];
        const unsigned long long l = (at[k] & 1u) ? E[w - 1u] : 0ull, r = (at[k] & 2u) ? E[w + 1u] : 0ull;
        const unsigned long long u = (at[k] & 4u) ? E[w - a.nw] : 0ull, b = (at[k] & 8u) ? E[w + a.nw] : 0ull;
        const unsigned long long rim = (e << 1 | l >> 63 | e >> 1 | r << 63 | u | b) & ~open[k] & ~src[k] & in_row;
        mapgrid_store_bits(dist + (size_t)y * a.sx + c * 64u, rim, OB);
    }
    if (tid == 0u) status[kMapGridLevels] = d;
}

template <int G>
__global__ __launch_bounds__(kMapGridScoreThreads) void k_mapgrid_score(CostGeom g, MapGridScoreArgs a)
{
    constexpr int kGroups = kMapGridScoreThreads / G;
    const int l = (int)threadIdx.x & (G - 1);
    const long long OB = (long long)g.sx * g.sy, UN = OB + 1;
    const long long stride = (long long)gridDim.x * kGroups;
    for (long long t = (long long)blockIdx.x * kGroups + (long long)(threadIdx.x / G); t < a.n_traj; t += stride) {
        unsigned long long key = ~0ull;                                 // the earliest negative event of this lane
        long long sum = 0, last = 0;
        for (int p = l; p < a.T; p += G) {
            const FootPose P = a.poses[t * a.T + p];
            long long dd;
            const int code = mapgrid_pose_code(g, a.dist, P, a.xshift, a.stop_on_failure != 0, OB, UN, dd);
            if (code >= 0) {
                const unsigned long long e = (unsigned long long)p << 2 | (unsigned long long)code;
                key = e < key ? e : key;
                break;                                                  // this lane's later poses come later in the walk
            }
            sum += dd;
            if (p == a.T - 1) last = dd;
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(key, off, G);
            key = o < key ? o : key;
            sum += __shfl_xor(sum, off, G);
            last += __shfl_xor(last, off, G);
        }
        if (l == 0) a.out[t] = key != ~0ull ? (long long)(key & 3ull) - 4 : (a.sum ? sum : last);
    }
}

hipError_t launch_mapgrid_fill(hipStream_t st, int* d0, int* d1, uint32_t cells, int value)
{
    if (!cells || !d0) return hipSuccess;
    const uint32_t blocks = std::min<uint32_t>((cells + 1023u) / 1024u, 1024u);
    hipLaunchKernelGGL(k_mapgrid_fill, dim3(blocks, d1 ? 2u : 1u), dim3(256), 0, st, d0, d1, cells, value);
    return hipGetLastError();
}

// more than 64 KB of dynamic LDS has to be asked for once per device (as gem_sort.hip does for its kernels)
static hipError_t mapgrid_allow_lds(size_t lds)
{
    constexpr int kMaxDev = 64;
    static std::mutex mu;
    static size_t configured[kMaxDev] = {};
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(mu);
    if (dev < 0 || dev >= kMaxDev || lds > configured[dev]) {
        e = hipFuncSetAttribute((const void*)k_mapgrid_distance, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < kMaxDev) configured[dev] = lds;
    }
    return hipSuccess;
}

hipError_t launch_mapgrid_distance(hipStream_t st, const MapGridArgs& a, int n_grids)
{
    const uint32_t W = a.nw * a.sy;
    if (n_grids < 1 || n_grids > 2 || W == 0u || W > kMapGridMaxWords) return hipErrorInvalidValue;
    const size_t lds = mapgrid_lds_bytes(W);
    if (lds > (48u << 10)) {
        const hipError_t e = mapgrid_allow_lds(lds);
        if (e != hipSuccess) return e;
    }
    // a thread owns at most kMapGridWordsPerThread words, and as few as the workgroup's size allows: a level's cost is a wave's walk
    // through its own words, one after the other, so a word per thread where that fits (measured: profiles/mapgrid_c2.txt)
    const int threads = (int)std::min<uint32_t>((W + 63u) & ~63u, kMapGridMaxThreads);
    hipLaunchKernelGGL(k_mapgrid_distance, dim3((unsigned)n_grids), dim3(threads), lds, st, a);
    return hipGetLastError();
}

template <int G>
static hipError_t launch_score(hipStream_t st, const CostGeom& g, const MapGridScoreArgs& a)
{
    constexpr long long kGroups = kMapGridScoreThreads / G;
    long long nb = (a.n_traj + kGroups - 1) / kGroups;
    if (nb > 8192) nb = 8192;                                           // the groups stride over the rest
    hipLaunchKernelGGL((k_mapgrid_score<G>), dim3((unsigned)nb), dim3(kMapGridScoreThreads), 0, st, g, a);
    return hipGetLastError();
}

hipError_t launch_mapgrid_score(hipStream_t st, const CostGeom& g, const MapGridScoreArgs& a)
{
    if (a.n_traj <= 0) return hipSuccess;
    if (a.T <= 8) return launch_score<8>(st, g, a);
    if (a.T <= 16) return launch_score<16>(st, g, a);
    return launch_score<32>(st, g, a);
}

} // namespace gem
