// gem_mapgrid_tiled.hpp -- path and goal distance grids on a costmap of ANY size (internal header): argument block and host launchers
// of gem_mapgrid_tiled.hip, the tile-round protocol's third client (gem_tile_round.hpp; the other two are k_nav_round and k_front_round).
//   seed   behind launch_mapgrid_fill (gem_mapgrid.hpp: the requested grids are UN): the run of the plan's cells, 0 into the sources,
//          the status words, both active maps of every requested grid cleared, the sources' tiles and their four neighbours marked
//   round  one launch over the tiles of every requested grid: an active tile relaxes to its local fixed point in LDS, stores what
//          changed and marks the neighbours whose facing edge changed
//   close  one wave behind a chunk of rounds: "a tile is still marked" or not, and the round counter, through pinned words
//   rim    once, behind convergence: OB on the blocked rim of the reached set
// The contract is in include/gem_hip_mapgrid.h.
#pragma once

#include "gem_mapgrid.hpp"
#include "gem_tile_round.hpp"

namespace gem {

constexpr int kMgtStride = kNavTile + 3;                            // LDS row of the distances with its two halo cells, odd
constexpr int kMgtSeedThreads = 1024;

// the pinned words the kernels answer through (the call waits, so one block serves every costmap of a handle)
enum { kMgtConverged = 0, kMgtRounds = 1, kMgtStarted = 2, kMgtGoalX = 3, kMgtGoalY = 4, kMgtPinWords = 8 };

struct MapGridTiledArgs {
    const unsigned char* grid;
    const int* cells;                   // per point of the adjusted plan: y * sx + x, or -1 off the map (pinned host memory)
    int n;
    int sx, sy, ntx, nty;
    int n_grids;                        // 1 or 2
    int* dist[2];                       // per requested grid: the distances ...
    int* status[2];                     // ... its status words (kMapGridLevels is the protocol's round counter) ...
    int goal[2];                        // ... and whether it is a goal grid (one source) or the path grid (the whole run)
    int* act;                           // [n_grids][2][ntx * nty]: round r reads map r & 1 and marks map (r + 1) & 1
    int* pin;                           // kMgtPinWords of pinned host memory
    int round;                          // the round of this launch (close: the next one)
};

hipError_t launch_mgt_seed(hipStream_t st, const MapGridTiledArgs& a);
hipError_t launch_mgt_round(hipStream_t st, const MapGridTiledArgs& a);
hipError_t launch_mgt_close(hipStream_t st, const MapGridTiledArgs& a);
hipError_t launch_mgt_rim(hipStream_t st, const MapGridTiledArgs& a);

} // namespace gem
