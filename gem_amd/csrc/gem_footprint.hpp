// gem_footprint.hpp -- footprints on the device costmap (internal header): argument blocks and host launchers of gem_footprint.hip,
// and the pieces of the contract of include/gem_hip_footprint.h that the host side (gem_capi_footprint.cpp) computes itself.
//   score   footprintCost of base_local_planner's CostmapModel for batches of poses and whole trajectories
//   clear   setConvexPolygonCost(FREE_SPACE) of an outline whose vertex cells the host has computed
#pragma once

#include "gem_costmap.hpp"

namespace gem {

constexpr int kFootMaxVertices = 32;                               // GEM_FOOTPRINT_MAX_VERTICES
constexpr int kFootThreads = 256;
constexpr uint32_t kFootClearColumns = 256;                        // columns of the polygon a clearing workgroup takes
constexpr uint32_t kFootNarrow = 32768;                            // maps up to this wide and high walk their lines in 32-bit integers

// the footprint specification, by value in the kernel arguments: a lane reads its own vertex from there
struct FootSpec {
    double xy[2 * kFootMaxVertices];
    int n;
};

struct FootPose { double x, y, c, s; };                            // = gem_footprint_pose

// trajectory t owns poses [t * T, (t + 1) * T); gem_costmap_footprint_cost is T = 1 with traj_cost as its output
struct FootScoreArgs {
    const FootPose* poses;
    int* pose_cost;                     // [n_traj * T] or NULL
    int* traj_cost;                     // [n_traj]
    long long n_traj;
    int T;
    int inscribed_lethal, sum;          // the two flags
};

// transformFootprint of one vertex, every operation rounded on its own (the library is built with -ffp-contract=off)
__host__ __device__ __forceinline__ void foot_vertex(const FootPose& p, double sx, double sy, double& wx, double& wy)
{
    wx = p.x + (sx * p.c - sy * p.s);
    wy = p.y + (sx * p.s + sy * p.c);
}

// the lane-group width of the scoring kernel for a spec on a map of this resolution: a power of two in 8 .. 64 with a lane beyond
// the vertices (it takes the centre), near half the longest edge's cell count so that an edge is a pass or two of the group
int foot_group_width(const FootSpec& spec, double res);

hipError_t launch_foot_score(hipStream_t st, const CostGeom& g, const unsigned char* grid, const FootSpec& spec, const FootScoreArgs& a);

// the outline's vertex cells (all on the map, n >= 3) and their box
struct FootCells {
    uint32_t x[kFootMaxVertices], y[kFootMaxVertices];
    int n;
    uint32_t min_x, max_x, min_y, max_y;
};
hipError_t launch_foot_clear(hipStream_t st, unsigned char* grid, uint32_t sx, uint32_t sy, const FootCells& c);

} // namespace gem
