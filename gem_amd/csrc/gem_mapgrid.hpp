// gem_mapgrid.hpp -- path and goal distance grids on the device costmap (internal header): argument blocks and host launchers of
// gem_mapgrid.hip.
//   fill      the requested grids become UN
//   distance  MapGrid::computeTargetDistance from the accepted run of the plan's cells, one workgroup per grid, the search in LDS
//   score     MapGridCostFunction::scoreTrajectory for batches of trajectories
// The contract is in include/gem_hip_mapgrid.h.
#pragma once

#include "gem_footprint.hpp"

namespace gem {

constexpr uint32_t kMapGridMaxWords = 4096;                        // GEM_MAPGRID_MAX_WORDS: a bit plane is at most 32 KB of LDS
constexpr int kMapGridMaxThreads = 1024;
constexpr int kMapGridWordsPerThread = 4;                          // kMapGridMaxWords / kMapGridMaxThreads: a thread's words live in registers
constexpr int kMapGridScoreThreads = 256;
constexpr unsigned char kMapGridBlocked = 253;                     // a byte from here on is blocked: 253, 254, 255
constexpr int kMapGridPlanes = 3;                                  // LDS planes: open (prologue) | two frontiers

// status words of a grid on the device.  kMapGridLevels: the levels k_mapgrid_distance walked; of a grid made by the tiled form
// (gem_mapgrid_tiled.hip) the protocol's round counter, the last round that found an active tile plus one
enum { kMapGridStarted = 0, kMapGridGoalX = 1, kMapGridGoalY = 2, kMapGridLevels = 3, kMapGridStatusWords = 4 };

struct MapGridArgs {
    const unsigned char* grid;
    const int* cells;                   // per point of the adjusted plan: y * sx + x, or -1 off the map (pinned host memory)
    int n;
    uint32_t sx, sy, nw;                // nw = ceil(sx / 64): words per row
    int* dist[2];                       // per workgroup of the launch: the grid it fills ...
    int* status[2];                     // ... its status words ...
    int goal[2];                        // ... and whether it is the goal grid (one source) or the path grid (the whole run)
};

inline uint32_t mapgrid_row_words(uint32_t sx) { return (sx + 63u) / 64u; }
inline size_t mapgrid_lds_bytes(uint32_t words) { return (size_t)kMapGridPlanes * words * 8; }

// dist[0 .. n_grids) all UN
hipError_t launch_mapgrid_fill(hipStream_t st, int* d0, int* d1, uint32_t cells, int value);
hipError_t launch_mapgrid_distance(hipStream_t st, const MapGridArgs& a, int n_grids);

struct MapGridScoreArgs {
    const FootPose* poses;
    const int* dist;
    long long* out;
    long long n_traj;
    int T;
    double xshift;
    int stop_on_failure, sum;
};
hipError_t launch_mapgrid_score(hipStream_t st, const CostGeom& g, const MapGridScoreArgs& a);

} // namespace gem
