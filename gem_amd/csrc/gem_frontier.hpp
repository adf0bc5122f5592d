// gem_frontier.hpp -- frontier search on the device costmap (internal header): argument block and host launchers of gem_frontier.hip.
//   classify   one pass over the cells: label[c] = c for a frontier cell, kFrontNone otherwise; the tiles that hold one are marked in
//              round 0's active map; the frontier cells are counted
//   round      one launch over the tiles: an active tile relaxes its labels to its local fixed point in LDS (8-connectivity), stores
//              what changed and marks the up to eight neighbours whose facing edge or corner cell changed
//   check      one wave behind a chunk of rounds: "a tile is still marked" goes to the pinned words
//   reduce     the roots (label[c] == c) are compacted into a dense list in ascending cell order (gem_compact.hpp), every frontier
//              cell adds itself to its root's record with integer atomics, and one workgroup computes the costs, compacts the kept
//              records and picks the winner
// The contract is in include/gem_hip_frontier.h.
#pragma once

#include "gem_navplan.hpp"

#include "../../include/gem_hip.h"

namespace gem {

constexpr int kFrontNone = 0x7fffffff;                              // the label of a cell that is no frontier cell
constexpr int kFrontStride = kNavTile + 3;                          // LDS row of the labels with its two halo cells, odd
constexpr int kFrontPickThreads = 1024;

// device words | their pinned host copy
enum { kFrontCells = 0, kFrontRounds = 1, kFrontRoots = 2, kFrontWords = 4 };
struct FrontPin {
    int converged, rounds;
    gem_frontier_status status;
};

// the records, field by field: every field of record r is touched by integer atomics alone
struct FrontRec {
    int* root;                          // the record's root cell, written by the roots' scatter, which also resets the other fields
    int* size;
    unsigned long long* sum_x;
    unsigned long long* sum_y;
    unsigned long long* key;            // (access potential << 32) | access cell
};

struct FrontArgs {
    const unsigned char* grid;
    const int* pot;
    int* label;                         // [sy][sx]
    int* index;                         // [sy][sx]: a root's list index at the root's cell; nothing else is ever read
    int* act;                           // [2][ntx * nty]: round r reads map r & 1 and marks map (r + 1) & 1
    int* words;                         // kFrontWords on the device
    FrontRec rec;
    gem_frontier* out;                  // the kept list
    FrontPin* pin;                      // pinned host memory
    int sx, sy, ntx, nty;
    int round;                          // the round of this launch (check: the next one)
    double resolution;
    gem_frontier_params params;
};

// records a map can need: two components are never 8-adjacent, so one cell of each in every 2 x 2 block at most
inline long long front_max_records(int sx, int sy) { return (long long)((sx + 1) / 2) * ((sy + 1) / 2); }

hipError_t launch_front_classify(hipStream_t st, const FrontArgs& a);
hipError_t launch_front_round(hipStream_t st, const FrontArgs& a);
hipError_t launch_front_check(hipStream_t st, const FrontArgs& a);
// block_cnt: compact_blocks(cells) words, then one word for the total
hipError_t launch_front_reduce(hipStream_t st, const FrontArgs& a, uint32_t* block_cnt);

} // namespace gem
