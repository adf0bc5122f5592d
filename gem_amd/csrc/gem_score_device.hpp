// gem_score_device.hpp -- the device functions the trajectory scoring kernels share (internal header, device code only): the closed form
// of the line iterator and footprintCost of one pose by a group of lanes (k_foot_score of gem_footprint.hip, k_critics of
// gem_critics.hip), and one pose of MapGridCostFunction::scoreTrajectory (k_mapgrid_score of gem_mapgrid.hip, k_critics).  The
// contracts are in include/gem_hip_footprint.h and include/gem_hip_mapgrid.h; the lane-group scheme is described in gem_footprint.hip.
#pragma once

#include "gem_mapgrid.hpp"

namespace gem {

// cell k of line(x0, y0, x1, y1): LineIterator / bresenham2D in closed form
template <class Wide>
__device__ __forceinline__ void foot_line_cell(int x0, int y0, int x1, int y1, uint32_t k, uint32_t& cx, uint32_t& cy)
{
    const uint32_t dx = (uint32_t)abs(x1 - x0), dy = (uint32_t)abs(y1 - y0);
    const int xi = x1 >= x0 ? 1 : -1, yi = y1 >= y0 ? 1 : -1;
    const bool x_major = dx >= dy;
    const uint32_t major = x_major ? dx : dy, minor = x_major ? dy : dx;
    const uint32_t m = major ? (uint32_t)(((Wide)(major / 2u) + (Wide)k * (Wide)minor) / (Wide)major) : 0u;
    cx = (uint32_t)(x0 + xi * (int)(x_major ? k : m));
    cy = (uint32_t)(y0 + yi * (int)(x_major ? m : k));
}

// footprintCost of one pose by the G lanes of a group; every lane returns the answer
template <int G, class Wide>
__device__ __forceinline__ int foot_pose_cost(const CostGeom& g, const unsigned char* __restrict__ grid, int n, int l, double sx, double sy,
                                              const FootPose& P, bool inscribed_lethal)
{
    double wx = P.x, wy = P.y;                                          // lanes beyond the vertices: the centre
    if (l < n) foot_vertex(P, sx, sy, wx, wy);
    uint32_t mx = 0u, my = 0u;
    const bool ok = cost_cell_xy(g, wx, wy, mx, my);
    const int vx = ok ? (int)mx : -1, vy = (int)my;                     // -1: worldToMap refused it
    const int ccx = __shfl(vx, G - 1, G), ccy = __shfl(vy, G - 1, G);
    if (ccx < 0) return -3;                                             // (the same in every lane of the group)
    if (n < 3) {
        const unsigned char c = grid[(size_t)ccy * g.sx + (size_t)ccx];
        return c == 255 ? -2 : (c >= 253 ? -1 : (int)c);
    }
    unsigned long long key = ~0ull;                                     // the earliest negative event of this lane
    int best = 0;
    bool dead = false;                                                  // an edge before this one failed worldToMap
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 == n ? 0 : i + 1;
        const int x0 = __shfl(vx, i, G), y0 = __shfl(vy, i, G), x1 = __shfl(vx, j, G), y1 = __shfl(vy, j, G);
        if (dead) continue;
        if (x0 < 0 || x1 < 0) {
            const unsigned long long e = (unsigned long long)i << 34;  // position 0, code 0 = -3
            key = e < key ? e : key;
            dead = true;
            continue;
        }
        const uint32_t dx = (uint32_t)abs(x1 - x0), dy = (uint32_t)abs(y1 - y0), len = (dx > dy ? dx : dy) + 1u;
        for (uint32_t k = (uint32_t)l; k < len; k += G) {
            uint32_t cx, cy;
            foot_line_cell<Wide>(x0, y0, x1, y1, k, cx, cy);
            if (!(cx < g.sx && cy < g.sy)) continue;                    // (a line between two cells of the map stays on it)
            const unsigned char c = grid[(size_t)cy * g.sx + (size_t)cx];
            const bool neg = c >= 254 || (c == 253 && inscribed_lethal);
            if (neg) {
                const unsigned long long e = (unsigned long long)i << 34 | (unsigned long long)(k + 1u) << 2 | (c == 255 ? 1u : 2u);
                key = e < key ? e : key;
            } else {
                best = (int)c > best ? (int)c : best;
            }
        }
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off, G);
        key = o < key ? o : key;
        const int b = __shfl_xor(best, off, G);
        best = b > best ? b : best;
    }
    return key != ~0ull ? (int)(key & 3ull) - 3 : best;
}

// one pose of MapGridCostFunction::scoreTrajectory: the code of its negative event (0: -4 off the map | 1: -3 on an obstacle cell |
// 2: -2 on an unreachable one, the last two with stop_on_failure only), or -1 with dd = the cell's distance
__device__ __forceinline__ int mapgrid_pose_code(const CostGeom& g, const int* __restrict__ dist, const FootPose& P, double xshift,
                                                 bool stop_on_failure, long long OB, long long UN, long long& dd)
{
    double px = P.x, py = P.y;
    if (xshift != 0.0) { px = P.x + xshift * P.c; py = P.y + xshift * P.s; }                   // (-ffp-contract=off: no fma)
    uint32_t cell = 0u;
    dd = 0;
    if (!cost_cell(g, px, py, cell)) return 0;                          // -4
    dd = dist[cell];
    if (stop_on_failure) return dd == OB ? 1 : (dd == UN ? 2 : -1);     // -3 | -2
    return -1;
}

} // namespace gem
