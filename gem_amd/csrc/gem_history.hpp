// gem_history.hpp -- the history cloud on the device (internal header): the box table of gem_history.hip.
//   visualCloud_ of ElevationMapping (EMg.cpp:750-760 push_back, :788 clear, :894-897 rebuild) is one flat log of records here; block
//   b of it is records [4096 b, min(4096 (b + 1), len)), the 4096 consecutive inputs a mark workgroup takes (kCostChunk), and has a box
//   {min_x, min_y, max_x, max_y} over its records' x and y: NaN ignored (fminf / fmaxf), +-inf taking part, a block without a
//   coordinate {+inf, +inf, -inf, -inf}.  The table is a pure function of the log: a box is always recomputed from its records.
#pragma once

#include "gem_costmap.hpp"

namespace gem {

inline long long history_blocks(long long len) { return cost_mark_blocks(len); }

// box[b] for b in [first_block, first_block + n_blocks) from rec[0, len): one workgroup per block
hipError_t launch_history_boxes(hipStream_t st, const LocalRecord* rec, long long len, long long first_block, long long n_blocks, float4* box);

} // namespace gem
