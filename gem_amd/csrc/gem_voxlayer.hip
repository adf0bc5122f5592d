// gem_voxlayer.hip -- costmap_2d::VoxelLayer::updateBounds on the device costmap, gfx950: 3-D ray-traced clearing, then marking, on a
// 32-bit voxel column per cell.  The contract is restated in include/gem_hip_voxlayer.h; its per-record and per-ray arithmetic is in
// gem_voxlayer.hpp, shared with the host twin.  The shape is gem_obstacle.hip's direct form.
//
// The result is a set function of the call (the header states the argument): clearing only removes bits, marking only adds them and
// every clear precedes every mark, so a cell's byte follows from the column after all clears (col_c), whether a ray crossed the cell,
// and the OR of its accepted marks.  Nothing here keeps an order beyond "every walk before the apply".
//
// pass   ONE pass over an observation's cloud, sixteen records per thread as the mark kernels: the double arithmetic of a record is
//        done once.  An accepted mark goes by atomic OR into the NEW-MARKS word of its cell (scratch, all-zero between calls) -- the
//        column itself must stay col_c until the apply --, a clearing record leaves its packed ray (end cell, end z, last step) or
//        kVoxNoRay, and the touched points go to the four bounds keys of CostAccum.
// walk   a group of G lanes (8 .. 64, by the longest possible ray) takes a ray: lane l computes the voxels l, l + G, ... by the closed
//        form of bresenham3D and clears both bits with an atomic AND; the cell's TOUCHED byte is a plain store of 1 (racing stores of
//        one value need no atomic and no answer, as the 2-D walk's).  Hundreds of rays share the cells next to the sensor, so the
//        column is LOADED first, by a plain load that the CU's cache may serve, and the atomic is skipped when both bits already read
//        as clear: bits move one way within the phase, so a stale read only costs a redundant atomic.  (Agent-scope loads of the
//        column and an atomic OR into a touched BITMAP behind a load of its word were the first form: every voxel of every ray then
//        went to the few L2 lines of the cells round the sensor, and the walk took 340 .. 950 us -- profiles/voxlayer_c2.txt.)
// apply  behind every walk of the call, a cell per thread: the byte rule (vox_cell_byte), the column with the marks OR-ed in, the
//        new-marks word and the touched byte zeroed, the bounds keys published and reset as k_cost_resolve does.
// With mark_threshold above 0 only the accepted records of a cell that ended LETHAL touch the bounds, which is known behind the apply:
// k_vox_mark_bounds then reads the marking clouds once more (only when the caller asked for bounds) and k_vox_publish ends the call.
// The reduction of the bounds, their publication and the walk's dispatch are gem_cost_pass.hpp's; the columns are filled,
// rolled and read through the element-wise kernels of gem_costmap.hip (launch_cost_fill / _roll / _window with 4-byte elements).
// Integer and double arithmetic only (division and square root IEEE); only vector stores and atomics write memory.
#include "gem_cost_pass.hpp"
#include "gem_voxlayer.hpp"

namespace gem {

// BOUNDS_ONLY: the second reading of a marking cloud behind the apply (mark_threshold above 0)
template <bool BOUNDS_ONLY>
__global__ __launch_bounds__(kCostThreads) void k_vox_pass(CostGeom g, VoxGeom v, VoxParams p, VoxScratch s)
{
    __shared__ unsigned long long s_acc[4];
    if (threadIdx.x < 4) s_acc[threadIdx.x] = ~0ull;
    __syncthreads();

    const ObsParams& o = p.o;
    const size_t n = o.n, base = (size_t)blockIdx.x * kCostChunk;
    const uint32_t cells = g.sx * g.sy;
    double lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
    constexpr int kBatch = 4;                                           // loads in flight per lane
    for (int k0 = 0; k0 < kCostItems; k0 += kBatch) {                   // workgroup-uniform trip count
        if (base + (size_t)k0 * kCostThreads >= n) break;
        float vx[kBatch], vy[kBatch], vz[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const size_t i = base + (size_t)(k0 + k) * kCostThreads + threadIdx.x;
            if (i < n) {
                const float* r = reinterpret_cast<const float*>(o.points + i * o.step);
                vx[k] = r[0]; vy[k] = r[1]; vz[k] = r[2];
            }
        }
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const size_t i = base + (size_t)(k0 + k) * kCostThreads + threadIdx.x;
            if (i >= n) continue;
            const double wx = (double)vx[k], wy = (double)vy[k], wz = (double)vz[k];
            const bool in = obs_in_window(o, wz);
            if (!BOUNDS_ONLY && o.clearing) {
                unsigned long long ray = kVoxNoRay;
                double ex, ey;
                if (in && vox_clear_record(g, v, p, wx, wy, wz, ray, ex, ey)) {
                    lo_x = fmin(lo_x, ex); hi_x = fmax(hi_x, ex);
                    lo_y = fmin(lo_y, ey); hi_y = fmax(hi_y, ey);
                }
                s.rays[i] = ray;
            }
            if (in && o.marking) {
                uint32_t cell, z;
                if (vox_mark_record(g, v, p, wx, wy, wz, cell, z) && cell < cells) {
                    bool touches = p.mark_touches != 0;
                    if (BOUNDS_ONLY) {
                        touches = !vox_below(vox_marked(s.columns[cell]), v.mark_thr);      // the column is col_f behind the apply
                    } else {
                        const uint32_t m = vox_mask(z);
                        if ((__hip_atomic_load(s.marks + cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m) != m)
                            __hip_atomic_fetch_or(s.marks + cell, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    if (touches) {
                        lo_x = fmin(lo_x, wx); hi_x = fmax(hi_x, wx);
                        lo_y = fmin(lo_y, wy); hi_y = fmax(hi_y, wy);
                    }
                }
            }
        }
    }
    cost_bounds_out(lo_x, lo_y, hi_x, hi_y, s_acc, s.acc);
}

// a group of G lanes takes a ray of rays[0 .. n): lane l clears the voxels l, l + G, ... of 0 .. end and touches their cells
template <int G, class Wide>
__global__ __launch_bounds__(kObsWalkThreads) void k_vox_walk(CostGeom g, uint32_t sz, int x0, int y0, int z0,
                                                              const unsigned long long* __restrict__ rays, uint32_t n,
                                                              uint32_t* __restrict__ columns, unsigned char* __restrict__ touched)
{
    constexpr uint32_t kGroups = kObsWalkThreads / G;
    const uint32_t l = threadIdx.x & (G - 1), cells = g.sx * g.sy;
    for (uint32_t r = blockIdx.x * kGroups + threadIdx.x / G; r < n; r += gridDim.x * kGroups) {
        const unsigned long long ray = rays[r];
        if (ray == kVoxNoRay) continue;
        const uint32_t cell = (uint32_t)ray & 0x3FFFFFFFu, z1 = (uint32_t)(ray >> 30) & 15u, end = (uint32_t)(ray >> 34);
        if (!(cell < cells)) continue;
        const VoxLine line = vox_line(x0, y0, z0, (int)(cell % g.sx), (int)(cell / g.sx), (int)z1);
        for (uint32_t k = l; k <= end; k += G) {
            uint32_t cx, cy, cz;
            vox_line_voxel<Wide>(line, k, cx, cy, cz);
            if (!(cx < g.sx && cy < g.sy && cz < sz)) continue;          // (a line between two voxels of the grid stays in it)
            const uint32_t c = cy * g.sx + cx, m = vox_mask(cz);
            if (columns[c] & m) __hip_atomic_fetch_and(columns + c, ~m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            touched[c] = 1;
        }
    }
}

// a cell per thread
__global__ __launch_bounds__(256) void k_vox_apply(uint32_t cells, VoxGeom v, uint32_t* __restrict__ columns, uint32_t* __restrict__ marks,
                                                   unsigned char* __restrict__ touched, unsigned char* __restrict__ grid, int publish,
                                                   unsigned long long* __restrict__ acc, unsigned long long* __restrict__ published)
{
    if (publish && blockIdx.x == 0) cost_publish(acc, published);
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= cells) return;
    const uint32_t nm = marks[c];
    const bool t = touched[c] != 0;
    if (nm || t) {
        const uint32_t col_c = columns[c];
        unsigned char byte;
        if (vox_cell_byte(v, col_c, nm, t, &byte)) grid[c] = byte;
        if (nm) {
            columns[c] = col_c | nm;
            marks[c] = 0u;
        }
        if (t) touched[c] = 0;
    }
}

__global__ __launch_bounds__(64) void k_vox_publish(unsigned long long* __restrict__ acc, unsigned long long* __restrict__ published)
{
    cost_publish(acc, published);
}

hipError_t launch_vox_pass(hipStream_t st, const CostGeom& g, const VoxGeom& v, const VoxParams& p, const VoxScratch& s)
{
    const long long nb = cost_mark_blocks((long long)p.o.n);
    if (nb <= 0) return hipSuccess;
    if (nb > INT_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_vox_pass<false>), dim3((unsigned)nb), dim3(kCostThreads), 0, st, g, v, p, s);
    return hipGetLastError();
}

hipError_t launch_vox_mark_bounds(hipStream_t st, const CostGeom& g, const VoxGeom& v, const VoxParams& p, const VoxScratch& s)
{
    const long long nb = cost_mark_blocks((long long)p.o.n);
    if (nb <= 0) return hipSuccess;
    if (nb > INT_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_vox_pass<true>), dim3((unsigned)nb), dim3(kCostThreads), 0, st, g, v, p, s);
    return hipGetLastError();
}

// k_vox_walk over the rays of an observation for launch_walk_groups
struct VoxWalk {
    hipStream_t st;
    const CostGeom& g;
    const VoxGeom& v;
    const VoxParams& p;
    const VoxScratch& s;
    template <int G, class Wide>
    void launch(uint32_t nb) const
    {
        hipLaunchKernelGGL((k_vox_walk<G, Wide>), dim3(nb), dim3(kObsWalkThreads), 0, st, g, v.sz, (int)p.fx0, (int)p.fy0, (int)p.fz0, s.rays, p.o.n,
                           s.columns, s.touched);
    }
};

hipError_t launch_vox_walk(hipStream_t st, const CostGeom& g, const VoxGeom& v, const VoxParams& p, const VoxScratch& s)
{
    return launch_walk_groups(g, p.o.cell_range, p.o.n, VoxWalk{st, g, v, p, s});   // the dominant axis is x or y for every ray longer than 16 voxels
}

hipError_t launch_vox_apply(hipStream_t st, const CostGeom& g, const VoxGeom& v, const VoxScratch& s, unsigned char* grid, bool publish,
                            unsigned long long* published)
{
    const uint32_t cells = g.sx * g.sy;
    hipLaunchKernelGGL(k_vox_apply, dim3(cost_blocks(cells)), dim3(256), 0, st, cells, v, s.columns, s.marks, s.touched, grid, publish ? 1 : 0, s.acc,
                       published);
    return hipGetLastError();
}

hipError_t launch_vox_publish(hipStream_t st, unsigned long long* acc, unsigned long long* published)
{
    hipLaunchKernelGGL(k_vox_publish, dim3(1), dim3(64), 0, st, acc, published);
    return hipGetLastError();
}

} // namespace gem
