// gem_cost_pass.hpp -- what the costmap layers' kernels share (internal header, device side): gem_costmap.hip (PointMapLayer,
// ElevationMapLayer), gem_obstacle.hip (ObstacleLayer) and gem_voxlayer.hip (VoxelLayer) each take a stream of inputs and write a grid.
//   cost_bounds_out    a lane's bounds -> wave -> workgroup (LDS) -> the four words of CostAccum::acc
//   cost_publish       the four words published and reset for the next call
//   launch_walk_groups the lane-group width, the narrow / wide line arithmetic and the block cap of a ray walk
// The record loop itself (4096 inputs per workgroup, sixteen per thread in batches of four loads) is written out in each layer's pass
// kernel: with the per-record work behind a function of a shared loop template the optimiser unrolls the batches differently, and
// k_obs_pass and k_vox_pass come out with other register counts and, measured, a slower first voxel observe
// (profiles/cost_pass_c2.txt).
#pragma once

#include "gem_obstacle.hpp"
#include "gem_wave.hpp"

namespace gem {

// the wave's bounds into the workgroup's four keys (s_acc, all-ones before the first wave arrives), the workgroup's into the call's.
// Every thread of the workgroup calls it; behind its barrier every input of the workgroup is done.
__device__ __forceinline__ void cost_bounds_out(double lo_x, double lo_y, double hi_x, double hi_y, unsigned long long* s_acc,
                                                unsigned long long* acc)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo_x = fmin(lo_x, __shfl_xor(lo_x, off)); hi_x = fmax(hi_x, __shfl_xor(hi_x, off));
        lo_y = fmin(lo_y, __shfl_xor(lo_y, off)); hi_y = fmax(hi_y, __shfl_xor(hi_y, off));
    }
    if (lane_id() == 0 && lo_x <= hi_x) {                               // the wave touched a point
        atomicMin(&s_acc[0], cost_key(lo_x)); atomicMin(&s_acc[1], cost_key(lo_y));
        atomicMin(&s_acc[2], ~cost_key(hi_x)); atomicMin(&s_acc[3], ~cost_key(hi_y));
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_acc[threadIdx.x] != ~0ull)
        __hip_atomic_fetch_min(acc + threadIdx.x, s_acc[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// acc -> published[4] (the words as they are), acc reset to all-ones; the first four threads of ONE workgroup of the call's last launch
__device__ __forceinline__ void cost_publish(unsigned long long* acc, unsigned long long* published)
{
    if (threadIdx.x < 4) {
        published[threadIdx.x] = acc[threadIdx.x];
        acc[threadIdx.x] = ~0ull;
    }
}

// the lane-group width of a walk: a power of two in 8 .. 64 near half the longest ray's cell count (a ray is a pass or two)
inline int obs_group_width(const CostGeom& g, uint32_t cell_range)
{
    const uint32_t side = g.sx > g.sy ? g.sx : g.sy, longest = cell_range < side ? cell_range : side;
    int w = 8;
    while (w < 64 && (uint32_t)w < (longest + 1u) / 2u) w *= 2;
    return w;
}

// A walk over `rays` rays, a group of G lanes per ray: walk.launch<G, Wide>(blocks) enqueues the layer's kernel with kObsWalkThreads
// threads per block, Wide the integer its lines are computed in.  At most 8192 blocks: the groups stride over the rest.
template <int G, class Walk>
hipError_t launch_walk_width(const CostGeom& g, uint32_t rays, const Walk& walk)
{
    constexpr uint32_t kGroups = kObsWalkThreads / G;
    uint32_t nb = (rays + kGroups - 1) / kGroups;
    if (nb > 8192u) nb = 8192u;
    if (nb == 0u) return hipSuccess;
    if (g.sx <= kObsNarrow && g.sy <= kObsNarrow) walk.template launch<G, uint32_t>(nb);
    else walk.template launch<G, unsigned long long>(nb);
    return hipGetLastError();
}

template <class Walk>
hipError_t launch_walk_groups(const CostGeom& g, uint32_t cell_range, uint32_t rays, const Walk& walk)
{
    switch (obs_group_width(g, cell_range)) {
    case 8: return launch_walk_width<8>(g, rays, walk);
    case 16: return launch_walk_width<16>(g, rays, walk);
    case 32: return launch_walk_width<32>(g, rays, walk);
    default: return launch_walk_width<64>(g, rays, walk);
    }
}

} // namespace gem
