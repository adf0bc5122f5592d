// gem_obstacle.hpp -- ObstacleLayer on the device costmap (internal header): the per-record and per-ray arithmetic of the contract of
// include/gem_hip_obstacle.h, written once for the kernels (gem_obstacle.hip) and the host twin (gem_capi_obstacle.cpp), and the
// argument blocks and host launchers of the kernels.
//   pass    one pass over an observation's cloud: a bit per end cell, a bit per marked cell, the touched bounds
//   walk    one group of lanes per ray: the cells 0 .. end of the closed-form line become FREE_SPACE
//   apply   LETHAL_OBSTACLE where a mark bit is set, behind every walk; the bounds words published
#pragma once

#include "gem_costmap.hpp"

#include <math.h>

namespace gem {

constexpr int kObsMax = 8;                                         // GEM_OBS_MAX
constexpr unsigned kObsMarking = 1u, kObsClearing = 2u;            // GEM_OBS_MARKING, GEM_OBS_CLEARING
constexpr int kObsWalkThreads = 256;
constexpr uint32_t kObsNarrow = 32768;                             // maps up to this wide and high walk their lines in 32-bit integers
constexpr uint32_t kObsNoCell = ~0u;

// one observation as the kernels see it: the header's gem_observation with the host's part of the contract done
struct ObsParams {
    const unsigned char* points;
    uint32_t n, step;
    double ox, oy, oz;
    double sq_obstacle_range, raytrace_range;                       // obstacle_range * obstacle_range
    double min_h, max_h, layer_max_h;
    double end_x, end_y;                                            // map_end_x, map_end_y
    uint32_t x0, y0;                                                // the origin's cell (clearing only)
    uint32_t cell_range;                                            // cellDistance(raytrace_range)
    int marking, clearing;                                          // clearing: the flag AND worldToMap(origin) succeeded
};

// std::min / std::max as the library's calls resolve: a NaN second argument leaves the first
__host__ __device__ __forceinline__ double obs_std_min(double a, double b) { return b < a ? b : a; }
__host__ __device__ __forceinline__ double obs_std_max(double a, double b) { return a < b ? b : a; }

// cellDistance: saturating where the library's cast is undefined
__host__ __device__ __forceinline__ uint32_t obs_cell_distance(double range, double res)
{
    const double c = obs_std_max(0.0, ceil(range / res));
    return c >= 4294967295.0 ? 4294967295u : (uint32_t)c;
}

// ObservationBuffer's height window
__host__ __device__ __forceinline__ bool obs_in_window(const ObsParams& p, double wz) { return p.min_h <= wz && wz <= p.max_h; }

// raytraceFreespace's body for one record of the window: false when worldToMap refuses the clipped point; else its cell and the
// point updateRaytraceBounds touches
__host__ __device__ __forceinline__ bool obs_clear_record(const CostGeom& g, const ObsParams& p, double wx, double wy, uint32_t& x1,
                                                          uint32_t& y1, double& ex, double& ey)
{
    const double a = wx - p.ox, b = wy - p.oy;
    if (wx < g.ox) { const double t = (g.ox - p.ox) / a; wx = g.ox; wy = p.oy + b * t; }
    if (wy < g.oy) { const double t = (g.oy - p.oy) / b; wx = p.ox + a * t; wy = g.oy; }
    if (wx > p.end_x) { const double t = (p.end_x - p.ox) / a; wx = p.end_x - .001; wy = p.oy + b * t; }
    if (wy > p.end_y) { const double t = (p.end_y - p.oy) / b; wx = p.ox + a * t; wy = p.end_y - .001; }
    if (!cost_cell_xy(g, wx, wy, x1, y1)) return false;
    const double ddx = wx - p.ox, ddy = wy - p.oy;
    const double full = sqrt(ddx * ddx + ddy * ddy);
    const double s = obs_std_min(1.0, p.raytrace_range / full);
    ex = p.ox + ddx * s; ey = p.oy + ddy * s;
    return true;
}

// updateBounds' marking body for one record of the window
__host__ __device__ __forceinline__ bool obs_mark_record(const CostGeom& g, const ObsParams& p, double px, double py, double pz, uint32_t& cell)
{
    if (pz > p.layer_max_h) return false;
    const double sq = (px - p.ox) * (px - p.ox) + (py - p.oy) * (py - p.oy) + (pz - p.oz) * (pz - p.oz);
    if (sq >= p.sq_obstacle_range) return false;
    return cost_cell(g, px, py, cell);
}

// raytraceLine's length: the ray (x0, y0) -> (x1, y1) visits the cells 0 .. end of line()
__host__ __device__ __forceinline__ uint32_t obs_ray_end(int x0, int y0, int x1, int y1, uint32_t cell_range)
{
    const long long dx = (long long)x1 - x0, dy = (long long)y1 - y0;
    const uint32_t adx = (uint32_t)(dx < 0 ? -dx : dx), ady = (uint32_t)(dy < 0 ? -dy : dy), da = adx > ady ? adx : ady;
    const double dist = sqrt((double)(dx * dx + dy * dy));
    const double scale = dist == 0.0 ? 1.0 : obs_std_min(1.0, (double)cell_range / dist);
    const uint32_t len = (uint32_t)(scale * (double)da);
    return len < da ? len : da;
}

// cell k of line(x0, y0, x1, y1): the closed form of gem_hip_footprint.h (foot_line_cell of gem_score_device.hpp, for host and device)
template <class Wide>
__host__ __device__ __forceinline__ void obs_line_cell(int x0, int y0, int x1, int y1, uint32_t k, uint32_t& cx, uint32_t& cy)
{
    const uint32_t dx = (uint32_t)(x1 >= x0 ? x1 - x0 : x0 - x1), dy = (uint32_t)(y1 >= y0 ? y1 - y0 : y0 - y1);
    const int xi = x1 >= x0 ? 1 : -1, yi = y1 >= y0 ? 1 : -1;
    const bool x_major = dx >= dy;
    const uint32_t major = x_major ? dx : dy, minor = x_major ? dy : dx;
    const uint32_t m = major ? (uint32_t)(((Wide)(major / 2u) + (Wide)k * (Wide)minor) / (Wide)major) : 0u;
    cx = (uint32_t)(x0 + xi * (int)(x_major ? k : m));
    cy = (uint32_t)(y0 + yi * (int)(x_major ? m : k));
}

// what a call's kernels share: the two bitmaps (a bit per cell, all-zero between calls), the ray list, the bounds words
struct ObsScratch {
    uint32_t* end_bits;                 // [words]: the end cells of the observation in flight (end-cell form)
    uint32_t* mark_bits;                // [words]: the marked cells of the whole call
    uint32_t* rays;                     // the rays to walk: distinct end cells (end-cell form) or an end cell / kObsNoCell per record (direct form)
    uint32_t* block_cnt;                // the compaction's per-workgroup counts (gem_compact.hpp)
    uint32_t* total;                    // ... and its total: the rays of the end-cell form
    unsigned long long* acc;            // CostAccum::acc
};

inline uint32_t obs_words(uint32_t cells) { return (cells + 31u) / 32u; }

// the pass over one observation's cloud; direct: every record's end cell goes to s.rays[record] instead of the end bitmap
hipError_t launch_obs_pass(hipStream_t st, const CostGeom& g, const ObsParams& p, const ObsScratch& s, bool direct);
// end-cell form: the set bits of s.end_bits compacted into s.rays (the bits cleared), then one walk per ray
hipError_t launch_obs_walk_cells(hipStream_t st, const CostGeom& g, const ObsParams& p, const ObsScratch& s, unsigned char* grid);
// direct form: one walk per record of s.rays[0 .. p.n)
hipError_t launch_obs_walk_records(hipStream_t st, const CostGeom& g, const ObsParams& p, const ObsScratch& s, unsigned char* grid);
// 254 where a mark bit is set, the bits cleared; acc -> published[4], acc reset to all-ones
hipError_t launch_obs_apply(hipStream_t st, uint32_t cells, uint32_t* mark_bits, unsigned char* grid, unsigned long long* acc,
                            unsigned long long* published);

} // namespace gem
