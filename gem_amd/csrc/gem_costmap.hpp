// gem_costmap.hpp -- the costmap layers on the device (internal header): argument blocks and host launchers of gem_costmap.hip.
//   mark     the updateBounds bodies of PointMapLayer (layers/src/pointMap_layer.cpp:55-81) and ElevationMapLayer
//            (layers/src/elevationMap_layer.cpp:58-81): every input's costmap cell in double, its verdict carried by a stamp
//   resolve  the stamps into the byte grid (FREE_SPACE / LETHAL_OBSTACLE), the stamps cleared, the touched bounds published
//   fill / roll / window   element-wise over the bytes or the voxel columns: a reset, Costmap2D::updateOrigin through a second grid,
//            a window packed for the read-back and unpacked for the write
//   merge    updateWithOverwrite / updateWithMax over a window
#pragma once

#include "gem_local.hpp"

#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

namespace gem {

constexpr unsigned char kCostFree = 0, kCostLethal = 254, kCostNoInfo = 255;
// The one size-dependent switch: a costmap of at most this many cells keeps a stamp grid per workgroup in LDS (32 KB), a larger one
// sends its wave-reduced stamps straight to global memory.
constexpr uint32_t kCostLdsCells = 8192;
constexpr int kCostThreads = 256, kCostItems = 16;                  // inputs per thread: a workgroup takes 4096 consecutive inputs
constexpr int kCostChunk = kCostThreads * kCostItems;

struct CostGeom {
    double ox, oy, res;
    uint32_t sx, sy;
};

// Costmap2D::worldToMap with the contract's stricter failure: non-finite coordinates and quotients beyond int fail.  Shared by the
// mark kernels, the footprint kernels (gem_footprint.hip) and the host side of gem_costmap_clear_footprint.
__host__ __device__ __forceinline__ bool cost_cell_xy(const CostGeom& g, double wx, double wy, uint32_t& mx, uint32_t& my)
{
    if (!(__builtin_fabs(wx) <= DBL_MAX && __builtin_fabs(wy) <= DBL_MAX)) return false;
    if (wx < g.ox || wy < g.oy) return false;
    const double qx = (wx - g.ox) / g.res, qy = (wy - g.oy) / g.res;
    if (!(qx < 2147483648.0 && qy < 2147483648.0)) return false;
    mx = (uint32_t)(int)qx; my = (uint32_t)(int)qy;
    return mx < g.sx && my < g.sy;
}

__host__ __device__ __forceinline__ bool cost_cell(const CostGeom& g, double wx, double wy, uint32_t& cell)
{
    uint32_t mx, my;
    if (!cost_cell_xy(g, wx, wy, mx, my)) return false;
    cell = my * g.sx + mx;
    return true;
}

// what a mark launch accumulates into: a stamp per cell, 2 * (input index + 1) + lethal, 0 = untouched, resolved by integer max; and
// four 64-bit words, the order-preserving keys of min px, min py, ~max px, ~max py over the accepted inputs, all reduced by integer
// min (all-ones: no input accepted)
struct CostAccum {
    uint32_t* stamps;
    unsigned long long* acc;
};

struct CostPointsArgs {
    const LocalRecord* rec;
    const uint32_t* count;              // the record count on the device (a capture's), or NULL: n
    uint32_t n;                         // records (an upper bound with `count`)
    uint32_t base;                      // index of rec[0] in the whole input (the submaps of one call follow each other)
    double thresh;
};

struct CostVisualArgs {
    const LocalRecord* rec; const int* lin; const uint32_t* count;   // the capture
    LocalGeom g;
    double thresh;
};

// doubles as unsigned integers in the same order (-0 below +0): the keys of CostAccum::acc (the mark kernels, gem_obstacle.hip)
__device__ __forceinline__ unsigned long long cost_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}

// the host side of CostAccum::acc (cost_key): false when the word is all-ones
inline bool cost_key_decode(unsigned long long k, bool inverted, double* out)
{
    if (k == ~0ull) return false;
    if (inverted) k = ~k;
    const unsigned long long b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
    __builtin_memcpy(out, &b, 8);
    return true;
}

inline long long cost_mark_blocks(long long items) { return (items + kCostChunk - 1) / kCostChunk; }

// whether the culling rule of k_cost_mark_history is exact for this geometry: the far limits ox + (sx + 1) res are fine enough
// in double that the extra cell covers the roundings of worldToMap (the argument is next to the rule in gem_costmap.hip)
inline bool cost_cull_exact(const CostGeom& g)
{
    const double lim_x = g.ox + (double)(g.sx + 1u) * g.res, lim_y = g.oy + (double)(g.sy + 1u) * g.res, span = g.res * 2251799813685248.0;   // 2^51
    return __builtin_fabs(lim_x) <= span && __builtin_fabs(lim_y) <= span;
}

hipError_t launch_cost_mark_points(hipStream_t st, const CostGeom& g, const CostPointsArgs& a, CostAccum out);
hipError_t launch_cost_mark_visual(hipStream_t st, const CostGeom& g, const CostVisualArgs& a, CostAccum out);
// launch_cost_mark_points (count NULL, base 0) with a box {min_x, min_y, max_x, max_y} per workgroup: a workgroup whose box lies off
// the map leaves at once and adds one to *culled (gem_costmap.hip states the rule).  box NULL: nothing is culled.
hipError_t launch_cost_mark_history(hipStream_t st, const CostGeom& g, const CostPointsArgs& a, CostAccum out, const float4* box,
                                    uint32_t* culled);
// stamps -> grid; acc -> published[4] (the words as they are), acc reset to all-ones
hipError_t launch_cost_resolve(hipStream_t st, uint32_t cells, uint32_t* stamps, unsigned char* grid, unsigned long long* acc,
                               unsigned long long* published);
struct CostWindow { int min_i, min_j, max_i, max_j; };
inline uint64_t cost_window_cells(CostWindow w) { return (uint64_t)(w.max_i - w.min_i) * (uint64_t)(w.max_j - w.min_j); }
inline unsigned cost_blocks(uint64_t threads) { return (unsigned)((threads + 255) / 256); }        // workgroups of 256 threads
hipError_t launch_cost_merge(hipStream_t st, const unsigned char* layer, unsigned char* master, uint32_t sx, CostWindow w, int mode);
// The element-wise kernels of a grid of `elem`-byte elements: 1, the costmap's bytes, or 4, its voxel columns (gem_voxlayer.hpp).
//   fill    every element `value`
//   roll    dst(x, y) = src(x + cell_ox, y + cell_oy) where that lies in the map, `value` elsewhere
//   window  pack: the window's elements into `packed`, row after row; else the reverse.  An empty window launches nothing.
hipError_t launch_cost_fill(hipStream_t st, void* grid, size_t elem, uint32_t cells, uint32_t value);
hipError_t launch_cost_roll(hipStream_t st, const void* src, void* dst, size_t elem, uint32_t sx, uint32_t sy, long long cell_ox,
                            long long cell_oy, uint32_t value);
hipError_t launch_cost_window(hipStream_t st, void* grid, size_t elem, uint32_t sx, CostWindow w, void* packed, bool pack);

} // namespace gem
