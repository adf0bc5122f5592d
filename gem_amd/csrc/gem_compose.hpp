// gem_compose.hpp -- pointCloudtoOctomap's outlier filter and road / obstacle split on the previous capture (internal header):
// argument blocks and host launchers of gem_compose.hip.  The contract is stated in include/gem_hip.h (gem_local_compose).
//   index    the capture's records scattered into an L x L grid of record indices, addressed by UNWRAPPED cell (uy * L + ux)
//   knn      the mean_k + 1 smallest squared distances of every record, by a ring walk over an LDS tile; lanes the tile's halo could
//            not close go to the far list
//   knn_far  the far list, finished exactly by a ring walk over global memory
//   (the ordered double sums of the threshold are taken on the host, from the downloaded distances: DESIGN.md has what the device
//   forms cost)
//   split    one stable compaction (gem_compact.hpp) over three classes: road, obstacle, removed; only the first two are written
#pragma once

#include "gem_local.hpp"

namespace gem {

constexpr int kComposeTile = 16;                                    // a workgroup owns 16 x 16 unwrapped cells (256 lanes)
constexpr int kComposeHalo = 8;                                     // rings the LDS tile can answer
constexpr int kComposeSide = kComposeTile + 2 * kComposeHalo;       // 32 cells: 32 * 32 * 16 B = 16 KB of LDS per workgroup
constexpr int kComposeMaxK = 32;

struct ComposeKnnArgs {
    const LocalRecord* rec; const int* lin; const uint32_t* count;  // the previous capture
    LocalGeom g;
    int* grid;                          // [L^2] record index of the unwrapped cell, -1 when the cell is not in the capture
    float* dist;                        // [L^2] mean neighbour distance per record
    int* far; uint32_t* far_count;      // records left to k_compose_knn_far
    int mean_k, sqrt_double;
};

struct ComposeSplitArgs {
    const LocalRecord* rec; const float* dist; const uint32_t* count;
    double threshold, travers_threshold;
    int filter;                         // 0: n <= mean_k, nothing is removed
    LocalRecord* road; LocalRecord* obstacle;       // either may be NULL: counted only
};

hipError_t launch_compose_knn(hipStream_t st, const ComposeKnnArgs& a, uint32_t n);
// block_cnt: [3 * compact_blocks(n)] scratch; totals[3]: road, obstacle, removed
hipError_t launch_compose_split(hipStream_t st, const ComposeSplitArgs& a, uint32_t n, uint32_t* block_cnt, uint32_t* totals);

} // namespace gem
