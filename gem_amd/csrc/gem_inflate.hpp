// gem_inflate.hpp -- inflation on the device costmap (internal header): argument block and host launchers of gem_inflate.hip.
//   seeds    the seed predicate (== 254 inside the widened window) packed into 64-bit words along x, and a flag per block of cells
//   inflate  the exact squared distance to the nearest seed, truncated at R, by a row pass over the bit words and a column pass over
//            LDS; then the table, the NO_INFORMATION rule and a store where the byte changes
//   reset    Costmap2D::resetMap over a window
// The contract is in include/gem_hip_inflate.h.
#pragma once

#include "gem_costmap.hpp"

namespace gem {

constexpr int kInflateMaxCells = 127;                              // GEM_INFLATE_MAX_CELLS: a row distance fits a byte with 255 to spare
constexpr int kInflateThreads = 256;
#ifndef GEM_INFLATE_TILE_ROWS
#define GEM_INFLATE_TILE_ROWS 32                                    // (A/B builds: GEM_BUILD_DEFINES)
#endif
#ifndef GEM_INFLATE_FLAG_ROWS
#define GEM_INFLATE_FLAG_ROWS 16
#endif
constexpr uint32_t kInflateTileRows = GEM_INFLATE_TILE_ROWS;       // a tile of the main kernel: 64 columns (one bit word) x this many rows
constexpr uint32_t kInflateFlagRows = GEM_INFLATE_FLAG_ROWS;       // a flag covers one bit word x this many rows of the seed region
constexpr unsigned char kCostInscribed = 253;

// Regions are half-open cell boxes on the map.  seed: the window widened by R and clamped; out: the seed region widened by R and
// clamped, the only cells the call can change.  bits[(y - seed.y0) * nw + (w - w0)] holds the seed predicate of cells 64 w .. 64 w + 63
// of row y; flags[(y - seed.y0) / kInflateFlagRows * nw + (w - w0)] is non-zero iff one of its kInflateFlagRows words is.
struct InflateBox { uint32_t x0, y0, x1, y1; };
struct InflateArgs {
    uint32_t sx, sy;
    InflateBox seed, out;
    uint32_t w0, nw;                    // the seed region's first word column and their number
    uint32_t ow0, onw;                  // the same for the output region: the tile columns
    uint32_t R;
    int inflate_unknown;
};

inline size_t inflate_flag_rows(const InflateArgs& a) { return (a.seed.y1 - a.seed.y0 + kInflateFlagRows - 1) / kInflateFlagRows; }
inline size_t inflate_bits_bytes(const InflateArgs& a) { return (size_t)(a.seed.y1 - a.seed.y0) * a.nw * 8; }
inline size_t inflate_flags_bytes(const InflateArgs& a) { return inflate_flag_rows(a) * a.nw * 4; }

// the window [min_i, max_i) x [min_j, max_j) (not empty, on the map) -> the two regions and the word ranges
InflateArgs inflate_args(uint32_t sx, uint32_t sy, int min_i, int min_j, int max_i, int max_j, uint32_t R, int inflate_unknown);

hipError_t launch_inflate_seeds(hipStream_t st, const unsigned char* grid, const InflateArgs& a, unsigned long long* bits, uint32_t* flags);
hipError_t launch_inflate(hipStream_t st, unsigned char* grid, const InflateArgs& a, const unsigned long long* bits, const uint32_t* flags,
                          const unsigned char* table);
hipError_t launch_inflate_reset(hipStream_t st, unsigned char* grid, uint32_t sx, InflateBox w, unsigned char value);

} // namespace gem
