// gem_tile_round.hpp -- one round of a tiled fixed-point computation on the device costmap (internal header): the protocol under
// k_nav_round (gem_navplan.hip) and k_front_round (gem_frontier.hip).  A grid of 32-bit values lives in global memory and is relaxed
// TILE BY TILE, a launch per round (the host loop is run_tile_rounds, gem_rounds.hpp): one workgroup -- one wave -- per tile of 64 x 64
// cells.  A tile that is not marked in this round's active map leaves at once (tile_round_enter).  An active tile clears its mark, loads
// its values and a one-cell halo into LDS (tile_load), relaxes to the tile's LOCAL fixed point (the kernel's own part), stores the cells
// that changed and marks the neighbour tiles whose facing edge -- or corner cell, under 8-connectivity -- changed (tile_store_and_mark).
// The active maps are double-buffered: round r reads map r & 1 and writes marks (plain stores of 1) into map (r + 1) & 1; a tile is
// the only one that clears its own word.  The computation has converged when a round marks nothing (tiles_still_marked).
//
// Why stale halo reads are safe.  Inside a launch a tile may read a neighbour's edge while the neighbour rewrites it; nothing orders
// the two, and nothing needs to, given two properties of the relaxation that each kernel's file argues for its own values:
//   1. values only fall: every store writes a value below the one the same workgroup loaded from that cell, and a cell is written by
//      its own tile's workgroup alone (and by the kernel that initialises the grid before the first round);
//   2. every stored value is a VALID one: derived from valid values, the halo's included, it is never below the fixed point.  So a
//      tile that works from old halo values computes values that are too large at worst;
//   3. an aligned 32-bit load sees the old or the new value of a cell, never a mixture;
//   4. a tile whose neighbour's facing edge or corner cell changed in round r is marked by that neighbour and runs in round r + 1,
//      behind the kernel boundary that makes round r's stores visible to every CU.  So whatever a tile missed it sees one round later.
// At the fixed point no edge changes, no tile is marked, and the relaxation's equation holds inside every tile with the true halo.
//
// No workgroup waits for another one: there is no spin-wait, no grid-wide barrier, no cooperative launch and no residency
// requirement; every loop is bounded by a count stated in its condition.  Global memory is touched by vector loads, stores and one
// vector atomic (the round counter) only.  That counter is the last round that found an active tile, plus one; it depends on timing
// (point 4: a tile may or may not already see the new edge), the values do not.
#pragma once

#include <hip/hip_runtime.h>

namespace gem {

constexpr int kNavTile = 64;                                        // a tile is 64 x 64 cells, one wave: lane t owns row t, then column t
constexpr int kTileLoadBatch = 22;                                  // rows of a tile (with its two halo rows: 66) whose loads are in flight together
static_assert(kNavTile == 64, "a tile's row and column are a wave wide");
static_assert((kNavTile + 2) % kTileLoadBatch == 0, "the load phase takes the tile's rows and its two halo rows in whole batches");

inline int nav_tiles(int n) { return (n + kNavTile - 1) / kNavTile; }

// A word another launch wrote, read with a vector load: a plain load at a uniform address would be moved to the scalar unit, and
// global memory is touched by vector instructions only here.
__device__ __forceinline__ int tile_load_word(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct TileRound {
    int tile, tx, ty, x0, y0;           // the workgroup's tile, its place in the tile grid and its first cell
    int* act_next;                      // the next round's active map
};

// false (uniform): no tile, or not marked in this round's map.  Otherwise the mark is cleared, *rounds_word raised to round + 1, t filled.
__device__ __forceinline__ bool tile_round_enter(int* act, int round, int ntx, int nty, int* rounds_word, TileRound& t)
{
    const int nt = ntx * nty;
    t.tile = (int)blockIdx.x;
    if (t.tile >= nt) return false;
    int* act_cur = act + (round & 1) * nt;
    t.act_next = act + ((round + 1) & 1) * nt;
    if (tile_load_word(act_cur + t.tile) == 0) return false;           // (uniform: the whole wave read the same word)
    if (threadIdx.x == 0) {
        act_cur[t.tile] = 0;                                            // read: cleared by its own tile
        atomicMax(rounds_word, round + 1);
    }
    t.ty = t.tile / ntx; t.tx = t.tile - t.ty * ntx;
    t.x0 = t.tx * kNavTile; t.y0 = t.ty * kNavTile;
    return true;
}

// What a kernel loads beside its values, inside the same batches (the same memory round trips): nothing.
struct TileNoExtra {
    __device__ __forceinline__ void load(int, size_t) {}                // row j of the batch: issue the loads at cell idx (clamped: always readable)
    __device__ __forceinline__ void ready() {}                          // every load of the batch is issued: dependent lookups, in flight together
    __device__ __forceinline__ void row(int, int, int, int, bool) {}    // row j of the batch is the tile's own row r: cell (gx, gy), in the map or not
};

// Load: rows -1 .. 64 of the tile's columns and the two halo columns, with CORNERS the four corner cells, into s_val [row + 1][column + 1]
// of stride STRIDE; a cell off the map is `none`.  Every load of a batch of rows is issued before the first of them is used --
// unconditional loads at clamped addresses, the selects afterwards -- so a batch costs one memory round trip, not one per row.  s_old
// [row][column] keeps the tile's own cells as memory holds them.  Returns (uniform) whether an own cell differs from `none`; the
// caller's barrier follows.
template <int STRIDE, bool CORNERS, class Extra>
__device__ __forceinline__ bool tile_load(const int* src, int sx, int sy, TileRound t, int none, int* s_val, int* s_old, Extra& extra)
{
    static_assert(STRIDE % 2 == 1 && STRIDE >= kNavTile + 2, "an odd LDS stride: a wave's lanes on rows t hit different banks");
    const int lane = (int)threadIdx.x, gx = t.x0 + lane, hy = t.y0 + lane;
    int halo[2], corner = none;
    bool halo_in[2], corner_in = false, has = false;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const int hx = side ? t.x0 + kNavTile : t.x0 - 1;
        halo_in[side] = hy < sy && hx >= 0 && hx < sx;
        halo[side] = src[halo_in[side] ? (size_t)hy * (size_t)sx + (size_t)hx : (size_t)0];
    }
    const int cside = lane & 1, cbottom = (lane >> 1) & 1;              // lanes 0 .. 3 take a corner each, the others repeat them
    if (CORNERS) {
        const int cx = cside ? t.x0 + kNavTile : t.x0 - 1, cy = cbottom ? t.y0 + kNavTile : t.y0 - 1;
        corner_in = cx >= 0 && cx < sx && cy >= 0 && cy < sy;
        corner = src[corner_in ? (size_t)cy * (size_t)sx + (size_t)cx : (size_t)0];
    }
#pragma unroll 1
    for (int r0 = 0; r0 < kNavTile + 2; r0 += kTileLoadBatch) {
        int v[kTileLoadBatch];
#pragma unroll
        for (int j = 0; j < kTileLoadBatch; ++j) {
            const int gy = t.y0 + r0 + j - 1;
            const bool in = gy >= 0 && gy < sy && gx < sx;
            const size_t idx = in ? (size_t)gy * (size_t)sx + (size_t)gx : (size_t)0;
            v[j] = src[idx];
            extra.load(j, idx);
        }
        extra.ready();
#pragma unroll
        for (int j = 0; j < kTileLoadBatch; ++j) {
            const int r = r0 + j, gy = t.y0 + r - 1;
            const bool in = gy >= 0 && gy < sy && gx < sx;
            const int val = in ? v[j] : none;
            s_val[r * STRIDE + lane + 1] = val;
            if (r >= 1 && r <= kNavTile) {
                extra.row(j, r - 1, gx, gy, in);
                s_old[(r - 1) * kNavTile + lane] = val;                 // what memory holds: the store phase compares with it
                has |= val != none;
            }
        }
    }
#pragma unroll
    for (int side = 0; side < 2; ++side) s_val[(lane + 1) * STRIDE + (side ? kNavTile + 1 : 0)] = halo_in[side] ? halo[side] : none;
    if (CORNERS && lane < 4) s_val[(cbottom ? kNavTile + 1 : 0) * STRIDE + (cside ? kNavTile + 1 : 0)] = corner_in ? corner : none;
    return __any(has);
}

// Store what changed; mark the neighbour tiles whose facing edge (with CORNERS: or corner cell) did.  The old values are the LDS copy
// of the load phase: only this workgroup writes these cells, so memory still holds them and nothing is read again.
template <int STRIDE, bool CORNERS>
__device__ __forceinline__ void tile_store_and_mark(int* dst, int sx, int sy, int ntx, int nty, TileRound t, const int* s_val, const int* s_old)
{
    const int lane = (int)threadIdx.x, gx = t.x0 + lane;
    int edges = 0;                                                      // 1 top | 2 bottom | 4 left | 8 right | 16 .. 128 the corners
#pragma unroll 8
    for (int r = 0; r < kNavTile; ++r) {
        const int gy = t.y0 + r;
        const int old = s_old[r * kNavTile + lane], now = s_val[(r + 1) * STRIDE + lane + 1];
        if (gy < sy && gx < sx && now != old) {
            dst[(size_t)gy * (size_t)sx + (size_t)gx] = now;
            const bool top = r == 0, b = r == kNavTile - 1, l = lane == 0, rt = lane == kNavTile - 1;
            edges |= (top ? 1 : 0) | (b ? 2 : 0) | (l ? 4 : 0) | (rt ? 8 : 0);
            if (CORNERS) edges |= (top && l ? 16 : 0) | (top && rt ? 32 : 0) | (b && l ? 64 : 0) | (b && rt ? 128 : 0);
        }
    }
    int all = 0;
#pragma unroll
    for (int bit = 0; bit < (CORNERS ? 8 : 4); ++bit) all |= __any(edges & (1 << bit)) ? (1 << bit) : 0;
    if (lane == 0) {
        const bool up = t.ty > 0, down = t.ty + 1 < nty, lft = t.tx > 0, rgt = t.tx + 1 < ntx;
        if ((all & 1) && up) t.act_next[t.tile - ntx] = 1;
        if ((all & 2) && down) t.act_next[t.tile + ntx] = 1;
        if ((all & 4) && lft) t.act_next[t.tile - 1] = 1;
        if ((all & 8) && rgt) t.act_next[t.tile + 1] = 1;
        if ((all & 16) && up && lft) t.act_next[t.tile - ntx - 1] = 1;  // (bits 16 .. 128 are set with CORNERS alone)
        if ((all & 32) && up && rgt) t.act_next[t.tile - ntx + 1] = 1;
        if ((all & 64) && down && lft) t.act_next[t.tile + ntx - 1] = 1;
        if ((all & 128) && down && rgt) t.act_next[t.tile + ntx + 1] = 1;
    }
}

// one wave: is a tile marked in the map round `round` would read?  (uniform)
__device__ __forceinline__ bool tiles_still_marked(const int* act, int round, int nt)
{
    const int* cur = act + (round & 1) * nt;
    bool marked = false;
    for (int i = (int)threadIdx.x; i < nt; i += 64) marked |= cur[i] != 0;   // (bounded by the tile count)
    return __any(marked);
}

} // namespace gem
