// gem_voxlayer.hpp -- VoxelLayer on the device costmap (internal header): the per-record and per-ray arithmetic of the contract of
// include/gem_hip_voxlayer.h, written once for the kernels (gem_voxlayer.hip) and the host twin (gem_capi_voxlayer.cpp), and the
// argument blocks and host launchers of the kernels.  It stands on gem_obstacle.hpp: the observation block, std::min / std::max,
// cellDistance and the height window are ObstacleLayer's.
//   pass    one pass over an observation's cloud: the accepted marks OR-ed into the new-marks word of their cell, a packed ray (or
//           none) per clearing record, the touched bounds
//   walk    one group of lanes per ray: both bits of the voxels 0 .. end of the closed-form 3-D line cleared, their cells touched
//   apply   behind every walk: the byte rule per cell from the cleared column, the touched byte and the new marks; the scratch zeroed
// The columns themselves are reset, rolled and windowed by gem_costmap.hpp's element-wise launchers.
#pragma once

#include "gem_obstacle.hpp"

namespace gem {

constexpr uint32_t kVoxUnknown = 0x0000FFFFu;                      // a column after reset: every voxel unknown
constexpr unsigned long long kVoxNoRay = ~0ull;

// the third axis of a costmap with voxels attached (gem_voxel_config)
struct VoxGeom {
    double oz, zres;
    uint32_t sz, unknown_thr, mark_thr;
};

// one observation as the kernels see it: ObstacleLayer's block (end_x / end_y are getSizeInMeters' map ends here, x0 / y0 unused)
// and the sensor's voxel coordinates (clearing only)
struct VoxParams {
    ObsParams o;
    double fx0, fy0, fz0;
    int mark_touches;                                               // the pass touches every accepted record (mark_threshold 0)
};

__host__ __device__ __forceinline__ uint32_t vox_mask(uint32_t z) { return 0x00010001u << z; }
__host__ __device__ __forceinline__ uint32_t vox_popcount(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(v);
#else
    return (uint32_t)__builtin_popcount(v);
#endif
}
__host__ __device__ __forceinline__ bool vox_below(uint32_t bits, uint32_t thr) { return vox_popcount(bits) <= thr; }
__host__ __device__ __forceinline__ uint32_t vox_marked(uint32_t col) { return col >> 16; }
__host__ __device__ __forceinline__ uint32_t vox_unknown(uint32_t col) { return ((col >> 16) ^ col) & 0xFFFFu; }

// the byte rule of the contract: col_c the column after every clear, marks the accepted marks of the call, touched the walks' byte.
// Returns whether *byte is written.
__host__ __device__ __forceinline__ bool vox_cell_byte(const VoxGeom& v, uint32_t col_c, uint32_t marks, bool touched, unsigned char* byte)
{
    if (marks && !vox_below(vox_marked(col_c | marks), v.mark_thr)) { *byte = kCostLethal; return true; }
    if (touched && vox_below(vox_marked(col_c), v.mark_thr)) {
        *byte = vox_below(vox_unknown(col_c), v.unknown_thr) ? kCostFree : kCostNoInfo;
        return true;
    }
    return false;
}

// worldToMap3DFloat, with the family's failure on non-finite input
__host__ __device__ __forceinline__ bool vox_cell_float(const CostGeom& g, const VoxGeom& v, double wx, double wy, double wz, double& fx,
                                                        double& fy, double& fz)
{
    if (!(__builtin_fabs(wx) <= DBL_MAX && __builtin_fabs(wy) <= DBL_MAX && __builtin_fabs(wz) <= DBL_MAX)) return false;
    if (wx < g.ox || wy < g.oy || wz < v.oz) return false;
    fx = (wx - g.ox) / g.res; fy = (wy - g.oy) / g.res; fz = (wz - v.oz) / v.zres;
    return fx < (double)g.sx && fy < (double)g.sy && fz < (double)v.sz;
}

// worldToMap3D: the quotients truncated to int before the tests (a quotient beyond int fails)
__host__ __device__ __forceinline__ bool vox_cell_int(const CostGeom& g, const VoxGeom& v, double wx, double wy, double wz, uint32_t& mx,
                                                      uint32_t& my, uint32_t& mz)
{
    if (!(__builtin_fabs(wx) <= DBL_MAX && __builtin_fabs(wy) <= DBL_MAX && __builtin_fabs(wz) <= DBL_MAX)) return false;
    if (wx < g.ox || wy < g.oy || wz < v.oz) return false;
    const double qx = (wx - g.ox) / g.res, qy = (wy - g.oy) / g.res, qz = (wz - v.oz) / v.zres;
    if (!(qx < 2147483648.0 && qy < 2147483648.0 && qz < 2147483648.0)) return false;
    mx = (uint32_t)(int)qx; my = (uint32_t)(int)qy; mz = (uint32_t)(int)qz;
    return mx < g.sx && my < g.sy && mz < v.sz;
}

// a ray: the end voxel's cell (30 bits), its z (4 bits) and the last step `end` of raytraceLine (30 bits)
__host__ __device__ __forceinline__ unsigned long long vox_pack_ray(uint32_t cell, uint32_t z, uint32_t end)
{
    return (unsigned long long)cell | ((unsigned long long)z << 30) | ((unsigned long long)end << 34);
}

// raytraceLine's length on double voxel coordinates: the voxels 0 .. end of the line (int)(x0, y0, z0) -> (int)(x1, y1, z1)
__host__ __device__ __forceinline__ uint32_t vox_ray_end(double x0, double y0, double z0, double x1, double y1, double z1, uint32_t max_length)
{
    const int dx = (int)x1 - (int)x0, dy = (int)y1 - (int)y0, dz = (int)z1 - (int)z0;
    const uint32_t adx = (uint32_t)(dx < 0 ? -dx : dx), ady = (uint32_t)(dy < 0 ? -dy : dy), adz = (uint32_t)(dz < 0 ? -dz : dz);
    const uint32_t myz = ady > adz ? ady : adz, da = adx >= myz ? adx : myz;
    const double dist = sqrt((x0 - x1) * (x0 - x1) + (y0 - y1) * (y0 - y1) + (z0 - z1) * (z0 - z1));
    const double scale = obs_std_min(1.0, (double)max_length / dist);
    const uint32_t len = (uint32_t)(scale * (double)da);
    return len < da ? len : da;
}

// raytraceFreespace's body for one record of the window: false when worldToMap3DFloat refuses the clipped point; else its ray and the
// point updateRaytraceBounds touches
__host__ __device__ __forceinline__ bool vox_clear_record(const CostGeom& g, const VoxGeom& v, const VoxParams& p, double wx, double wy,
                                                          double wz, unsigned long long& ray, double& ex, double& ey)
{
    const ObsParams& o = p.o;
    const double d = sqrt((wx - o.ox) * (wx - o.ox) + (wy - o.oy) * (wy - o.oy) + (wz - o.oz) * (wz - o.oz));
    const double f = obs_std_max(obs_std_min(1.0, (d - 2 * g.res) / d), 0.0);
    wx = f * (wx - o.ox) + o.ox; wy = f * (wy - o.oy) + o.oy; wz = f * (wz - o.oz) + o.oz;
    const double a = wx - o.ox, b = wy - o.oy, c = wz - o.oz;
    double t = 1.0;
    if (wz > o.layer_max_h) t = obs_std_max(0.0, obs_std_min(t, (o.layer_max_h - 0.01 - o.oz) / c));
    else if (wz < v.oz) t = obs_std_min(t, (v.oz - o.oz) / c);
    if (wx < g.ox) t = obs_std_min(t, (g.ox - o.ox) / a);
    if (wy < g.oy) t = obs_std_min(t, (g.oy - o.oy) / b);
    if (wx > o.end_x) t = obs_std_min(t, (o.end_x - o.ox) / a);
    if (wy > o.end_y) t = obs_std_min(t, (o.end_y - o.oy) / b);
    wx = o.ox + a * t; wy = o.oy + b * t; wz = o.oz + c * t;
    double fx, fy, fz;
    if (!vox_cell_float(g, v, wx, wy, wz, fx, fy, fz)) return false;
    const uint32_t end = vox_ray_end(p.fx0, p.fy0, p.fz0, fx, fy, fz, o.cell_range);
    ray = vox_pack_ray((uint32_t)(int)fy * g.sx + (uint32_t)(int)fx, (uint32_t)(int)fz, end);
    const double ddx = wx - o.ox, ddy = wy - o.oy;
    const double full = sqrt(ddx * ddx + ddy * ddy);
    const double s = obs_std_min(1.0, o.raytrace_range / full);
    ex = o.ox + ddx * s; ey = o.oy + ddy * s;
    return true;
}

// updateBounds' marking body for one record of the window: its cell and z-voxel
__host__ __device__ __forceinline__ bool vox_mark_record(const CostGeom& g, const VoxGeom& v, const VoxParams& p, double px, double py,
                                                         double pz, uint32_t& cell, uint32_t& z)
{
    const ObsParams& o = p.o;
    if (pz > o.layer_max_h) return false;
    const double sq = (px - o.ox) * (px - o.ox) + (py - o.oy) * (py - o.oy) + (pz - o.oz) * (pz - o.oz);
    if (sq >= o.sq_obstacle_range) return false;
    uint32_t mx, my;
    if (!vox_cell_int(g, v, px, py, pz < v.oz ? v.oz : pz, mx, my, z)) return false;
    cell = my * g.sx + mx;
    return true;
}

// the line (x0, y0, z0) -> (x1, y1, z1) as bresenham3D walks it, in closed form: what does not depend on the step
struct VoxLine {
    int x0, y0, z0, xi, yi, zi;
    uint32_t adx, ady, adz, da;
    int axis;                                                       // the dominant one: 0 x, 1 y, 2 z
};

__host__ __device__ __forceinline__ VoxLine vox_line(int x0, int y0, int z0, int x1, int y1, int z1)
{
    VoxLine l;
    l.x0 = x0; l.y0 = y0; l.z0 = z0;
    l.xi = x1 >= x0 ? 1 : -1; l.yi = y1 >= y0 ? 1 : -1; l.zi = z1 >= z0 ? 1 : -1;
    l.adx = (uint32_t)(x1 >= x0 ? x1 - x0 : x0 - x1); l.ady = (uint32_t)(y1 >= y0 ? y1 - y0 : y0 - y1);
    l.adz = (uint32_t)(z1 >= z0 ? z1 - z0 : z0 - z1);
    const uint32_t myz = l.ady > l.adz ? l.ady : l.adz;
    l.axis = l.adx >= myz ? 0 : (l.ady >= l.adz ? 1 : 2);
    l.da = l.axis == 0 ? l.adx : (l.axis == 1 ? l.ady : l.adz);
    return l;
}

// voxel k of the line: k steps along the dominant axis, (da / 2 + k * db) / da along each of the other two
template <class Wide>
__host__ __device__ __forceinline__ void vox_line_voxel(const VoxLine& l, uint32_t k, uint32_t& cx, uint32_t& cy, uint32_t& cz)
{
    const Wide half = (Wide)(l.da / 2u);
    const uint32_t mx = l.axis == 0 ? k : (l.da ? (uint32_t)((half + (Wide)k * (Wide)l.adx) / (Wide)l.da) : 0u);
    const uint32_t my = l.axis == 1 ? k : (l.da ? (uint32_t)((half + (Wide)k * (Wide)l.ady) / (Wide)l.da) : 0u);
    const uint32_t mz = l.axis == 2 ? k : (l.da ? (uint32_t)((half + (Wide)k * (Wide)l.adz) / (Wide)l.da) : 0u);
    cx = (uint32_t)(l.x0 + l.xi * (int)mx); cy = (uint32_t)(l.y0 + l.yi * (int)my); cz = (uint32_t)(l.z0 + l.zi * (int)mz);
}

// what a call's kernels share
struct VoxScratch {
    uint32_t* columns;                  // [cells]: the costmap's voxel columns
    uint32_t* marks;                    // [cells]: the accepted marks of the call, all-zero between calls
    unsigned char* touched;             // [cells]: 1 where a ray crossed the cell, all-zero between calls
    unsigned long long* rays;           // a packed ray / kVoxNoRay per record of the observation in flight
    unsigned long long* acc;            // CostAccum::acc
};

// the pass over one observation's cloud
hipError_t launch_vox_pass(hipStream_t st, const CostGeom& g, const VoxGeom& v, const VoxParams& p, const VoxScratch& s);
// one walk per record of s.rays[0 .. p.o.n)
hipError_t launch_vox_walk(hipStream_t st, const CostGeom& g, const VoxGeom& v, const VoxParams& p, const VoxScratch& s);
// the byte rule per cell, the columns with the marks OR-ed in, marks and touched zeroed; publish: acc -> published[4], acc reset
hipError_t launch_vox_apply(hipStream_t st, const CostGeom& g, const VoxGeom& v, const VoxScratch& s, unsigned char* grid, bool publish,
                            unsigned long long* published);
// mark_threshold above 0: the accepted records of a marking observation whose cell ended LETHAL touch the bounds (behind the apply)
hipError_t launch_vox_mark_bounds(hipStream_t st, const CostGeom& g, const VoxGeom& v, const VoxParams& p, const VoxScratch& s);
// acc -> published[4], acc reset to all-ones
hipError_t launch_vox_publish(hipStream_t st, unsigned long long* acc, unsigned long long* published);

} // namespace gem
