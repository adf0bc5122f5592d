// gem_navplan.hpp -- the global plan on the device costmap (internal header): argument block and host launchers of gem_navplan.hip.
//   init     the potential becomes UNREACHED with 0 at the start, both active maps are cleared and the start's tile and its four
//            neighbours marked, the weight table is copied from pinned host memory, the status words are reset
//   round    one launch over the tiles: an active tile relaxes to its local fixed point in LDS, stores what changed and marks the
//            neighbours whose facing edge changed
//   finish   one wave: a tile still marked -> "not converged"; otherwise GridPath::getPath from the goal, and the status
// The contract is in include/gem_hip_navplan.h.
#pragma once

#include "gem_navpath.hpp"
#include "gem_tile_round.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gem {

constexpr int kNavPotStride = kNavTile + 3;                         // LDS row of the potentials with its two halo cells, odd
constexpr int kNavWStride = kNavTile + 1;
constexpr unsigned kNavBlockedWeight = 0x80000000u;                 // an impassable cell's weight in LDS: v + it is above every potential

// status words, on the device and in their pinned host copy
enum { kNavConverged = 0, kNavFound = 1, kNavNPath = 2, kNavRounds = 3, kNavGoalPot = 4, kNavStatusWords = 8 };

struct NavArgs {
    const unsigned char* grid;
    int* w;                             // the weight table on the device [256]
    int* pot;                           // [sy][sx]
    int* act;                           // [2][ntx * nty]: round r reads map r & 1 and marks map (r + 1) & 1
    int* path;                          // [sx * sy]: the walk writes from the END backwards, so the path reads forwards from path + cells - n
    int* status;                        // kNavStatusWords on the device
    int* pin;                           // pinned host memory: w [256] | the status words
    int sx, sy, ntx, nty;
    int start, goal;                    // linear cells, -1 off the map
    int outline;
    int round;                          // the round of this launch (finish: the next one)
    int passes;                         // k_navquad_round alone: in-tile passes a tile is allowed in one round
};

hipError_t launch_nav_init(hipStream_t st, const NavArgs& a);
hipError_t launch_nav_round(hipStream_t st, const NavArgs& a);
hipError_t launch_nav_finish(hipStream_t st, const NavArgs& a);

} // namespace gem
