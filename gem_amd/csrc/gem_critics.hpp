// gem_critics.hpp -- the best trajectory on the device costmap (internal header): argument blocks and host launcher of gem_critics.hip.
//   critics  every critic of every trajectory in list order, combined as SimpleScoredSamplingPlanner::scoreTrajectory does; one
//            candidate (total, index) and a valid count per workgroup
//   pick     one workgroup reduces the candidates and writes the 32-byte result
// The contract is in include/gem_hip_critics.h.
#pragma once

#include "gem_mapgrid.hpp"

namespace gem {

constexpr int kCriticsMax = 8;                                     // GEM_CRITIC_MAX
constexpr int kCriticsThreads = 256;
constexpr int kCriticsMaxBlocks = 1024;                            // workgroups of the first pass: the groups stride over the rest
constexpr int kCriticObstacle = 1, kCriticMapGrid = 2, kCriticExternal = 3;
constexpr int kCriticCentreCost = 4;                               // GEM_CRITIC_CENTRE_COST

// a critic as the kernel reads it: `grid` is the slot of the distance grid (0 path | 1 goal | 2 front)
struct CriticDev {
    int kind, grid, flags, column;
    double scale, xshift;
};

// what a workgroup of the first pass leaves: key = the bits of the smallest valid total (all-ones: none), its index, the valid count
struct CriticsCandidate {
    unsigned long long key;
    long long index, n_valid;
};

// = gem_best_trajectory
struct CriticsBest {
    long long index, n_valid;
    double cost;
    long long reserved;
};

struct CriticsArgs {
    const unsigned char* grid;
    const int* dist[3];
    const FootPose* poses;
    const int* traj_len;                // [n_traj] or NULL
    const double* ext;                  // [columns * n_traj] or NULL
    double* out_total;                  // [n_traj] or NULL
    CriticsCandidate* cand;             // [blocks of the first pass]
    CriticsBest* out_best;
    long long n_traj;
    int T, n_critics;
    CriticDev c[kCriticsMax];
};

// the lane-group width: the smallest of 8 / 16 / 32 / 64 with a lane beyond the vertices, and no smaller than launch_mapgrid_score
// picks for T poses a trajectory
int critics_group_width(int n_vertices, int T);

// both launches; n_traj = 0 is the pick alone (it answers "no winner").  a.cand holds kCriticsMaxBlocks candidates.
hipError_t launch_critics(hipStream_t st, const CostGeom& g, const FootSpec& spec, const CriticsArgs& a);

} // namespace gem
