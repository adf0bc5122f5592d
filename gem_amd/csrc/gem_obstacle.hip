// gem_obstacle.hip -- costmap_2d::ObstacleLayer::updateBounds on the device costmap, gfx950: ray-traced clearing, then marking.  The
// contract is restated in include/gem_hip_obstacle.h; its per-record and per-ray arithmetic is in gem_obstacle.hpp, shared with the
// host twin.
//
// The result is a set function of the call (254 where an accepted marking record lies, else 0 where a ray crosses, else unchanged), so
// nothing here keeps an order: every clear of the call runs before the one launch that applies the marks, and that is all.
//
// pass   ONE pass over an observation's cloud, sixteen records per thread as the mark kernels: the double arithmetic of a record is
//        done once and leaves a bit for its END cell (x1, y1) in one bitmap, a bit for its MARKED cell in a second, and the touched
//        points in the four bounds keys of CostAccum.  A lane whose successor holds the same cell stays silent (a sweep puts runs of
//        returns into one cell), and in global memory an END bit that already reads as set is not set again; a costmap of at most kCostLdsCells cells keeps both bitmaps of the workgroup in LDS (ds_or_b32) and
//        each non-zero word leaves with one global atomic OR; a larger one sends the lanes' bits straight to global memory.
// walk   ONE walk per DISTINCT end cell, not per record.  This is exact, not an approximation: the cells raytraceLine visits are the
//        cells 0 .. end of line(x0, y0, x1, y1) with end a function of (x1 - x0, y1 - y0, cell_range) -- integers all, and (x0, y0)
//        and cell_range belong to the observation.  Two records with the same end cell therefore clear the same set of cells, and the
//        set a walk writes is the union over the end cells whichever record brought them.  (The world coordinates of the clipped
//        point only enter the bounds, which the pass has taken per record.)  The set bits are compacted into a list (gem_compact.hpp,
//        the bitmap cleared as it is read), and a group of G lanes (8 .. 64, by the longest possible ray) takes a ray: lane l computes
//        the cells l, l + G, ... by the closed form and stores the byte 0.  Racing stores of the same byte need no atomic.  (Walking
//        the bitmap itself, a wave per 64 cells and its ballot as the compaction, saves the three launches of the compaction and was
//        measured slower: the rays that leave the map fill whole words of the rim, and their waves walk 64 long rays one after the
//        other -- profiles/obstacle_c2.txt.)
// apply  behind every walk of the call: 254 where a mark bit is set, the mark bitmap cleared as it is read, the bounds keys published
//        and reset as k_cost_resolve does.
// The DIRECT form (gem_debug_set "obstacle_direct" 1) skips the end bitmap and the compaction: the pass writes every record's end cell
// (or none) to a list of n words and the same walk takes a group per record.  Measured (tools/bench_obstacle.py, profiles/
// obstacle_c2.txt) it is the faster one on every workload tried -- the end-cell form halves the walk but pays three launches of
// compaction and an end bitmap whose rim words every workgroup hits -- so it is the DEFAULT, and the end-cell form is the second path.
// The reduction of the bounds, their publication and the choice of the walk's group width, line arithmetic and grid are
// gem_cost_pass.hpp's, shared with the mark kernels and VoxelLayer.
// Integer and double arithmetic only (division and square root IEEE); only vector stores and atomics write memory.
#include "gem_compact.hpp"
#include "gem_cost_pass.hpp"

namespace gem {

// the bit of `cell` (kObsNoCell: none) into a bitmap, the run of lanes on one cell reduced to its last lane
template <bool LDS, bool TEST>
__device__ __forceinline__ void obs_set_bit(uint32_t cell, uint32_t* bits)
{
    const uint32_t next = (uint32_t)__shfl_down((int)cell, 1);
    if (cell == kObsNoCell || (lane_id() < 63 && next == cell)) return;
    const uint32_t bit = 1u << (cell & 31u);
    if (LDS) { atomicOr(&bits[cell >> 5], bit); return; }
    // TEST (the end bitmap): a bit only goes from 0 to 1 while the pass runs, so one that reads as set needs no atomic and a stale 0 only
    // costs one.  The rays that leave the map all end on its rim, thousands of records on a few words: the test takes them off the
    // atomic unit (k_obs_pass on 600 x 600: 99 us without it, 44 with it).  The marks are spread and go without.
    if (TEST && (__hip_atomic_load(bits + (cell >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) return;
    __hip_atomic_fetch_or(bits + (cell >> 5), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS, bool DIRECT>
__global__ __launch_bounds__(kCostThreads) void k_obs_pass(CostGeom g, ObsParams p, ObsScratch s)
{
    extern __shared__ uint32_t s_bits[];                                // LDS form: [2 * words], end cells | marked cells
    __shared__ unsigned long long s_acc[4];
    const uint32_t words = (g.sx * g.sy + 31u) / 32u;
    if (LDS)
        for (uint32_t w = threadIdx.x; w < 2u * words; w += kCostThreads) s_bits[w] = 0u;
    if (threadIdx.x < 4) s_acc[threadIdx.x] = ~0ull;
    __syncthreads();

    const size_t n = p.n, base = (size_t)blockIdx.x * kCostChunk;
    double lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
    constexpr int kBatch = 4;                                           // loads in flight per lane
    for (int k0 = 0; k0 < kCostItems; k0 += kBatch) {                   // workgroup-uniform trip count
        if (base + (size_t)k0 * kCostThreads >= n) break;
        float vx[kBatch], vy[kBatch], vz[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const size_t i = base + (size_t)(k0 + k) * kCostThreads + threadIdx.x;
            if (i < n) {
                const float* r = reinterpret_cast<const float*>(p.points + i * p.step);
                vx[k] = r[0]; vy[k] = r[1]; vz[k] = r[2];
            }
        }
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const size_t i = base + (size_t)(k0 + k) * kCostThreads + threadIdx.x;
            uint32_t end_cell = kObsNoCell, mark_cell = kObsNoCell;
            if (i < n) {
                const double wx = (double)vx[k], wy = (double)vy[k], wz = (double)vz[k];
                if (obs_in_window(p, wz)) {
                    if (p.clearing) {
                        uint32_t x1, y1;
                        double ex, ey;
                        if (obs_clear_record(g, p, wx, wy, x1, y1, ex, ey)) {
                            end_cell = y1 * g.sx + x1;
                            lo_x = fmin(lo_x, ex); hi_x = fmax(hi_x, ex);
                            lo_y = fmin(lo_y, ey); hi_y = fmax(hi_y, ey);
                        }
                    }
                    if (p.marking) {
                        uint32_t c;
                        if (obs_mark_record(g, p, wx, wy, wz, c)) {
                            mark_cell = c;
                            lo_x = fmin(lo_x, wx); hi_x = fmax(hi_x, wx);
                            lo_y = fmin(lo_y, wy); hi_y = fmax(hi_y, wy);
                        }
                    }
                }
                if (DIRECT && p.clearing) s.rays[i] = end_cell;
            }
            if (!DIRECT) obs_set_bit<LDS, true>(end_cell, LDS ? s_bits : s.end_bits);
            obs_set_bit<LDS, false>(mark_cell, LDS ? s_bits + words : s.mark_bits);
        }
    }

    cost_bounds_out(lo_x, lo_y, hi_x, hi_y, s_acc, s.acc);
    if (LDS)
        for (uint32_t w = threadIdx.x; w < 2u * words; w += kCostThreads) {
            const uint32_t b = s_bits[w];
            if (b) __hip_atomic_fetch_or((w < words ? s.end_bits + w : s.mark_bits + (w - words)), b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
}

// the ray from (x0, y0) to `cell` by the G lanes of a group: lane l stores the cells l, l + G, ... of 0 .. end
template <int G, class Wide>
__device__ __forceinline__ void obs_walk_ray(const CostGeom& g, int x0, int y0, uint32_t cell, uint32_t cell_range, uint32_t l,
                                             unsigned char* __restrict__ grid)
{
    const int x1 = (int)(cell % g.sx), y1 = (int)(cell / g.sx);
    const uint32_t end = obs_ray_end(x0, y0, x1, y1, cell_range);
    for (uint32_t k = l; k <= end; k += G) {
        uint32_t cx, cy;
        obs_line_cell<Wide>(x0, y0, x1, y1, k, cx, cy);
        if (cx < g.sx && cy < g.sy) grid[(size_t)cy * g.sx + (size_t)cx] = kCostFree;       // (a line between two cells of the map stays on it)
    }
}

// a group of G lanes takes a ray of rays[0 .. count): an end cell, or kObsNoCell for a record of the direct form that has none.
// count is n, or with `total` (the end-cell form's list) min(*total, n)
template <int G, class Wide>
__global__ __launch_bounds__(kObsWalkThreads) void k_obs_walk(CostGeom g, int x0, int y0, uint32_t cell_range, const uint32_t* __restrict__ rays,
                                                              const uint32_t* __restrict__ total, uint32_t n, unsigned char* __restrict__ grid)
{
    constexpr uint32_t kGroups = kObsWalkThreads / G;
    const uint32_t l = threadIdx.x & (G - 1), cells = g.sx * g.sy;
    const uint32_t count = total ? min(*total, n) : n;
    for (uint32_t r = blockIdx.x * kGroups + threadIdx.x / G; r < count; r += gridDim.x * kGroups) {
        const uint32_t cell = rays[r];
        if (!(cell < cells)) continue;                                  // kObsNoCell: the record has no ray
        obs_walk_ray<G, Wide>(g, x0, y0, cell, cell_range, l, grid);
    }
}

// end-cell form: the set bits of the end bitmap as a list of cells (gem_compact.hpp).  An item is a cell, its word is held from the
// load to the write, and the write clears the word -- a wave's 64 consecutive cells are two whole words that no other wave of the
// launch reads.  k_obs_walk then walks the list: min(*total, cap) rays.
struct ObsEndSrc : CompactSrc {
    uint32_t* bits;
    uint32_t* rays;
    uint32_t cells, cap;                // cap: the list's room (the set bits of one observation never exceed it)
    struct Item { uint32_t w; };
    __device__ size_t size() const { return cells; }
    __device__ Item load(size_t i) const { return {bits[i >> 5]}; }
    __device__ int cls(size_t i, const Item& v) const { return ((v.w >> (i & 31u)) & 1u) ? 0 : -1; }
    __device__ bool emit(int, size_t i, const Item&, size_t o) const
    {
        if (o < cap) rays[o] = (uint32_t)i;
        bits[i >> 5] = 0u;
        return false;
    }
};

// a word of the mark bitmap per thread; workgroup 0 publishes the bounds words and resets them for the next call
__global__ __launch_bounds__(256) void k_obs_apply(uint32_t cells, uint32_t* __restrict__ mark_bits, unsigned char* __restrict__ grid,
                                                   unsigned long long* __restrict__ acc, unsigned long long* __restrict__ published)
{
    if (blockIdx.x == 0) cost_publish(acc, published);
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= (cells + 31u) / 32u) return;
    uint32_t b = mark_bits[w];
    if (!b) return;
    mark_bits[w] = 0u;
    while (b) {
        const uint32_t c = w * 32u + (uint32_t)(__ffs((int)b) - 1);
        b &= b - 1u;
        if (c < cells) grid[c] = kCostLethal;
    }
}

hipError_t launch_obs_pass(hipStream_t st, const CostGeom& g, const ObsParams& p, const ObsScratch& s, bool direct)
{
    const long long nb = cost_mark_blocks((long long)p.n);
    if (nb <= 0) return hipSuccess;
    if (nb > INT_MAX) return hipErrorInvalidValue;
    const uint32_t cells = g.sx * g.sy;
    const dim3 grid((unsigned)nb), block(kCostThreads);
    if (cells <= kCostLdsCells) {
        const size_t lds = 2 * (size_t)obs_words(cells) * sizeof(uint32_t);
        if (direct) hipLaunchKernelGGL((k_obs_pass<true, true>), grid, block, lds, st, g, p, s);
        else hipLaunchKernelGGL((k_obs_pass<true, false>), grid, block, lds, st, g, p, s);
    } else {
        if (direct) hipLaunchKernelGGL((k_obs_pass<false, true>), grid, block, 0, st, g, p, s);
        else hipLaunchKernelGGL((k_obs_pass<false, false>), grid, block, 0, st, g, p, s);
    }
    return hipGetLastError();
}

// k_obs_walk over rays[0 .. bound) for launch_walk_groups
struct ObsWalk {
    hipStream_t st;
    const CostGeom& g;
    const ObsParams& p;
    const uint32_t *rays, *total;
    uint32_t bound;
    unsigned char* grid;
    template <int G, class Wide>
    void launch(uint32_t nb) const
    {
        hipLaunchKernelGGL((k_obs_walk<G, Wide>), dim3(nb), dim3(kObsWalkThreads), 0, st, g, (int)p.x0, (int)p.y0, p.cell_range, rays, total, bound, grid);
    }
};

hipError_t launch_obs_walk_cells(hipStream_t st, const CostGeom& g, const ObsParams& p, const ObsScratch& s, unsigned char* grid)
{
    const uint32_t cells = g.sx * g.sy, bound = cells < p.n ? cells : p.n;   // no more distinct end cells than cells or records
    ObsEndSrc src;
    src.bits = s.end_bits; src.rays = s.rays; src.cells = cells; src.cap = bound;
    const hipError_t e = compact(st, src, (long long)cells, s.block_cnt, s.total);
    if (e != hipSuccess) return e;
    return launch_walk_groups(g, p.cell_range, bound, ObsWalk{st, g, p, s.rays, s.total, bound, grid});
}

hipError_t launch_obs_walk_records(hipStream_t st, const CostGeom& g, const ObsParams& p, const ObsScratch& s, unsigned char* grid)
{
    return launch_walk_groups(g, p.cell_range, p.n, ObsWalk{st, g, p, s.rays, nullptr, p.n, grid});
}

hipError_t launch_obs_apply(hipStream_t st, uint32_t cells, uint32_t* mark_bits, unsigned char* grid, unsigned long long* acc,
                            unsigned long long* published)
{
    hipLaunchKernelGGL(k_obs_apply, dim3(cost_blocks(obs_words(cells))), dim3(256), 0, st, cells, mark_bits, grid, acc, published);
    return hipGetLastError();
}

} // namespace gem
