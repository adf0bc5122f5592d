// gem_footprint.hip -- footprints on the device costmap, gfx950: CostmapModel::footprintCost for batches of poses and whole
// trajectories, and Costmap2D::setConvexPolygonCost(FREE_SPACE).  The contract is restated in include/gem_hip_footprint.h.
//
// Scoring.  The closed form of the line iterator makes every cell of every edge computable on its own, so a pose is walked by a GROUP
// of G lanes (8, 16, 32 or 64; the host picks G from the spec, foot_group_width):
//   lane l < n transforms vertex l and takes its cell, the group's last lane takes the centre's (G > n always), all in double;
//   the edges are taken in order (the loop is uniform: every pose has the same n); the two end cells of edge i come from lanes i and
//   i + 1 by shuffles, and lane l reads cells l, l + G, ... of its line from the byte grid;
//   every event carries its place in the sequential walk, edge << 34 | (position + 1) << 2 | code with position 0 for the edge's
//   worldToMap test and code = answer + 3; the group takes the integer MIN of these keys over the negative events and the MAX of the
//   other costs by shuffles.  That is "the first negative event decides", whatever the timing; no memory is written in between.
// A group owns whole trajectories, one after the other, so a trajectory's first-negative / max / sum lives in registers; without a
// per-pose output it stops at its first negative pose, as ObstacleCostFunction::scoreTrajectory does.
// The grid is read through the caches where it lies (a 75 x 75 window is 5.6 KB, a 1000 x 1000 one 1 MB: both stay in L2).
// Lines on maps of at most kFootNarrow cells a side are walked in 32-bit integers (k * minor + major / 2 < 2^31), larger ones in 64-bit.
//
// Clearing.  The host has the vertex cells (it knows the geometry after rolling).  A workgroup takes kFootClearColumns columns of the
// outline's box: the outline's cells that fall into them go to per-column min / max words in LDS (ds_min / ds_max), then the columns
// are filled row by row.  Only vector loads and stores touch memory.
// foot_line_cell and foot_pose_cost are in gem_score_device.hpp: k_critics (gem_critics.hip) walks poses with them too.
#include "gem_score_device.hpp"

namespace gem {

template <int G, class Wide>
__global__ __launch_bounds__(kFootThreads) void k_foot_score(CostGeom g, const unsigned char* __restrict__ grid, FootSpec spec, FootScoreArgs a)
{
    constexpr int kGroups = kFootThreads / G;
    const int l = (int)threadIdx.x & (G - 1), n = spec.n;
    double sx = 0.0, sy = 0.0;
    if (l < n) { sx = spec.xy[2 * l]; sy = spec.xy[2 * l + 1]; }
    const long long stride = (long long)gridDim.x * kGroups;
    for (long long t = (long long)blockIdx.x * kGroups + (long long)(threadIdx.x / G); t < a.n_traj; t += stride) {
        int first_neg = 0, acc = 0;
        for (int p = 0; p < a.T; ++p) {
            const long long at = t * a.T + p;
            const FootPose P = a.poses[at];
            const int r = foot_pose_cost<G, Wide>(g, grid, n, l, sx, sy, P, a.inscribed_lethal != 0);
            if (a.pose_cost && l == 0) a.pose_cost[at] = r;
            if (!first_neg) {
                if (r < 0) first_neg = r;
                else acc = a.sum ? acc + r : (r > acc ? r : acc);
            }
            if (first_neg && !a.pose_cost) break;                       // nothing behind it can change the score
        }
        if (l == 0) a.traj_cost[t] = first_neg ? first_neg : acc;
    }
}

__global__ __launch_bounds__(kFootThreads) void k_foot_clear(unsigned char* __restrict__ grid, uint32_t sx, uint32_t sy, FootCells c)
{
    static_assert(kFootClearColumns == (uint32_t)kFootThreads, "a thread per column");
    __shared__ uint32_t s_lo[kFootClearColumns], s_hi[kFootClearColumns];
    const uint32_t c0 = c.min_x + blockIdx.x * kFootClearColumns;
    s_lo[threadIdx.x] = ~0u;
    s_hi[threadIdx.x] = 0u;
    __syncthreads();
    for (int i = 0; i < c.n; ++i) {
        const int j = i + 1 == c.n ? 0 : i + 1;
        const int x0 = (int)c.x[i], y0 = (int)c.y[i], x1 = (int)c.x[j], y1 = (int)c.y[j];
        const uint32_t dx = (uint32_t)abs(x1 - x0), dy = (uint32_t)abs(y1 - y0), len = (dx > dy ? dx : dy) + 1u;
        for (uint32_t k = threadIdx.x; k < len; k += kFootThreads) {
            uint32_t cx, cy;
            foot_line_cell<unsigned long long>(x0, y0, x1, y1, k, cx, cy);
            const uint32_t col = cx - c0;
            if (col < kFootClearColumns) {                              // (also false for cx < c0: the difference wraps)
                atomicMin(&s_lo[col], cy);
                atomicMax(&s_hi[col], cy);
            }
        }
    }
    __syncthreads();
    const uint32_t x = c0 + threadIdx.x, lo = s_lo[threadIdx.x], hi = s_hi[threadIdx.x];
    if (!(x < sx) || lo > hi) return;                                   // beyond the map (never: the box is on it), or not a column of the outline
    for (uint32_t y = c.min_y; y <= c.max_y && y < sy; ++y)             // rows in step across the workgroup: a row's bytes lie together
        if (lo <= y && y <= hi) grid[(size_t)y * sx + (size_t)x] = kCostFree;
}

int foot_group_width(const FootSpec& spec, double res)
{
    double longest = 0.0;
    for (int i = 0; i < spec.n; ++i) {
        const int j = i + 1 == spec.n ? 0 : i + 1;
        const double ex = spec.xy[2 * j] - spec.xy[2 * i], ey = spec.xy[2 * j + 1] - spec.xy[2 * i + 1];
        const double e = __builtin_sqrt(ex * ex + ey * ey) / res;
        if (e > longest) longest = e;                                   // (a NaN never is: the width only steers the speed)
    }
    int g = 8;
    while (g < 64 && (g < spec.n + 1 || (double)g < 0.5 * (longest + 1.0))) g *= 2;
    return g;
}

template <int G>
static hipError_t launch_score(hipStream_t st, const CostGeom& g, const unsigned char* grid, const FootSpec& spec, const FootScoreArgs& a)
{
    constexpr long long kGroups = kFootThreads / G;
    long long nb = (a.n_traj + kGroups - 1) / kGroups;
    if (nb > 8192) nb = 8192;                                           // the groups stride over the rest
    if (g.sx <= kFootNarrow && g.sy <= kFootNarrow)
        hipLaunchKernelGGL((k_foot_score<G, uint32_t>), dim3((unsigned)nb), dim3(kFootThreads), 0, st, g, grid, spec, a);
    else
        hipLaunchKernelGGL((k_foot_score<G, unsigned long long>), dim3((unsigned)nb), dim3(kFootThreads), 0, st, g, grid, spec, a);
    return hipGetLastError();
}

hipError_t launch_foot_score(hipStream_t st, const CostGeom& g, const unsigned char* grid, const FootSpec& spec, const FootScoreArgs& a)
{
    if (a.n_traj <= 0) return hipSuccess;
    switch (foot_group_width(spec, g.res)) {
    case 8: return launch_score<8>(st, g, grid, spec, a);
    case 16: return launch_score<16>(st, g, grid, spec, a);
    case 32: return launch_score<32>(st, g, grid, spec, a);
    default: return launch_score<64>(st, g, grid, spec, a);
    }
}

hipError_t launch_foot_clear(hipStream_t st, unsigned char* grid, uint32_t sx, uint32_t sy, const FootCells& c)
{
    const uint32_t chunks = (c.max_x - c.min_x) / kFootClearColumns + 1u;
    hipLaunchKernelGGL(k_foot_clear, dim3(chunks), dim3(kFootThreads), 0, st, grid, sx, sy, c);
    return hipGetLastError();
}

} // namespace gem
