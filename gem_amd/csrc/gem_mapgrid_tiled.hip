// gem_mapgrid_tiled.hip -- base_local_planner's MapGrid on a device costmap of any size, gfx950: computeTargetDistance as a tiled
// fixed point in global memory.  The contract is the one of include/gem_hip_mapgrid.h, unchanged; k_mapgrid_distance (gem_mapgrid.hip)
// keeps the whole search in one workgroup's LDS and so stops at GEM_MAPGRID_MAX_WORDS, this form does not.  Integer code only.
//
// computeTargetDistance is the unit-weight, multi-source case of the relaxation under k_nav_round: d[c] = 0 at a source, otherwise
// d[c] = min(d[c], min4(d) + 1) at a cell that is not blocked, and a blocked cell that is no source keeps UN (it passes nothing on:
// UN + 1 is above every value).  The protocol -- active maps, load, store, marks, and why a tile may read old halo values -- is
// gem_tile_round.hpp's; this file's part:
//   k_mgt_seed    ONE workgroup, behind k_mapgrid_fill (every requested grid is UN).  The run a .. b of the plan's cells by two
//                 integer min-reductions in LDS, as k_mapgrid_distance's prologue finds it: the cells come from pinned memory, the bytes
//                 are read when the kernel runs.  0 into the sources (points a .. b-1 of the path grid, point b-1 alone of a goal or
//                 front grid), the status words, both active maps of every requested grid cleared and, behind a barrier, every source's
//                 tile and its four neighbours marked in map 0.  A source never changes, so its tile's round may store nothing and mark
//                 nobody: a source on a tile's edge reaches the neighbour through the neighbour's halo alone, hence the four marks
//                 (k_nav_init argues the same for its single start; a diagonal tile is reached through one of the four, whose edge
//                 changes).  Up to 2^20 points are walked by this one workgroup's bounded loops, as the capped form does: the walk is
//                 at most 1024 trips a thread over pinned memory and a plan is a few hundred points in practice, a grid-stride form
//                 would add a launch and a device word for the two reductions and save nothing there.
//   k_mgt_round   one wave per tile of 64 x 64 cells, blockIdx.y the requested grid (at most two a launch).  Beside the distances the
//                 tile loads its bytes in tile_load's batches (the same memory round trips); "blocked" (byte >= 253, or off the map)
//                 is one 64-bit register a lane, its own column bit by bit, and goes from there into LDS: a blocked cell carries the
//                 SIGN BIT on top of its value, in s_val and in s_old.  The local fixed point comes from the four directional scans
//                 of k_nav_round with the running value in a register: at a blocked cell v = old, at any other v = min(old, v + 1);
//                 with the bit, `v + 1 < old` in signed arithmetic is false at a blocked cell without a test of its own.  A blocked
//                 cell is never written (UN stays UN; a blocked source holds 0 and its neighbours extend from it).  No wrap: UN + 1
//                 <= 2^30 + 2.  A pass of the four scans extends every in-tile shortest path by a straight segment at least, a path
//                 has at most 4096 cells: the loop's bound.  (A row word from a ballot and a column word, tested bit by bit in the
//                 chain, was measured first and was slower: profiles/mapgrid_tiled_c2.txt.  No s_w array either way.)
//   k_mgt_close   one wave behind a chunk of rounds: is a tile of any requested grid marked in the map the next round would read?
//                 The answer and the round counter go to pinned words.
//   k_mgt_rim     once, behind convergence, element-wise and IN PLACE: a cell whose byte is blocked and whose value is not 0 becomes OB
//                 if a 4-neighbour inside the map holds a value below OB.  In place is safe: the cells this pass writes hold UN
//                 before and OB after, both >= OB, and the cells whose value decides hold one below OB and are never written by it;
//                 whether a neighbour is read before or behind its own store, the test answers the same.
//
// The protocol's four properties for these values.  1. Values only fall: a round stores v only where v < the value it loaded, a cell
// is written by its own tile's wave alone (before the first round by fill and seed, behind the last by the rim pass).  2. Every stored
// value is a valid one: a value below UN is the length of a real 4-connected path from a source whose cells behind the source are not
// blocked (induction: 0 at a source; v + 1 at a non-blocked cell extends the path v stands for, a halo value included), so it is never
// BELOW the true distance, and a tile working from old halo values is too large at worst.  3. The values are aligned 32-bit words.
// 4. The marks are tile_store_and_mark's, 4-connected: the four edges mark, no corner.  At the fixed point d[c] = min4(d) + 1 holds
// at every non-blocked non-source cell with the true halo: the shortest distance, or UN where no source connects.
//
// LDS: s_val 66 x 67 x 4 = 17 688 B and s_old 64 x 64 x 4 = 16 384 B, 34 072 B a workgroup: FOUR tiles a CU of 160 KB (k_nav_round's
// weight plane and table make it 51 736 B: three).
//
// No hang by construction: every loop is bounded by a count stated in its condition, there is no spin-wait, no workgroup waits for
// another, no cooperative launch.  Global memory is touched by vector loads, stores and the protocol's one vector atomicMax (the round
// counter, kMapGridLevels of the grid's status words) only.
#include "gem_mapgrid_tiled.hpp"

#include <algorithm>

namespace gem {

static_assert(kMgtStride % 2 == 1, "an odd LDS stride: a wave's lanes on rows t hit different banks");

__global__ __launch_bounds__(kMgtSeedThreads) void k_mgt_seed(MapGridTiledArgs a)
{
    __shared__ int s_run[2];
    const int tid = (int)threadIdx.x, nt = a.ntx * a.nty;
    for (int i = tid; i < a.n_grids * 2 * nt; i += kMgtSeedThreads) a.act[i] = 0;      // (bounded by the maps' words)
    if (tid == 0) { s_run[0] = a.n; s_run[1] = a.n; }
    __syncthreads();
    // the run: a = the first accepted point
    for (int i = tid; i < a.n; i += kMgtSeedThreads) {
        const int c = a.cells[i];
        if (c >= 0 && a.grid[c] != kCostNoInfo) { atomicMin(&s_run[0], i); break; }    // (i only grows in a thread)
    }
    __syncthreads();
    const int ra = s_run[0];
    if (ra >= a.n) {                                                    // no accepted point: the grids stay UN, nothing is marked (uniform exit)
        if (tid < a.n_grids) {
            int* status = tid ? a.status[1] : a.status[0];
            status[kMapGridStarted] = 0; status[kMapGridGoalX] = -1; status[kMapGridGoalY] = -1; status[kMapGridLevels] = 0;
        }
        if (tid == 0) { a.pin[kMgtStarted] = 0; a.pin[kMgtGoalX] = -1; a.pin[kMgtGoalY] = -1; }
        return;
    }
    // b = the first point above a that is not accepted
    for (int i = ra + 1 + tid; i < a.n; i += kMgtSeedThreads) {
        const int c = a.cells[i];
        if (!(c >= 0 && a.grid[c] != kCostNoInfo)) { atomicMin(&s_run[1], i); break; }
    }
    __syncthreads();                                                    // (also: the maps' zeros are in memory before the first mark)
    const int rb = s_run[1];
    for (int g = 0; g < a.n_grids; ++g) {                               // (at most two)
        int* dist = g ? a.dist[1] : a.dist[0];
        int* act0 = a.act + (size_t)g * 2 * nt;                         // round 0 reads map 0
        const int first = (g ? a.goal[1] : a.goal[0]) ? rb - 1 : ra;
        for (int i = first + tid; i < rb; i += kMgtSeedThreads) {       // (bounded by the run)
            const int c = a.cells[i], y = c / a.sx, x = c - y * a.sx;
            dist[c] = 0;
            const int tx = x / kNavTile, ty = y / kNavTile, tile = ty * a.ntx + tx;
            act0[tile] = 1;
            if (tx > 0) act0[tile - 1] = 1;
            if (tx + 1 < a.ntx) act0[tile + 1] = 1;
            if (ty > 0) act0[tile - a.ntx] = 1;
            if (ty + 1 < a.nty) act0[tile + a.ntx] = 1;
        }
    }
    const int c = tile_load_word(a.cells + (rb - 1)), gx = c % a.sx, gy = c / a.sx;
    if (tid < a.n_grids) {
        int* status = tid ? a.status[1] : a.status[0];
        status[kMapGridStarted] = 1; status[kMapGridGoalX] = gx; status[kMapGridGoalY] = gy; status[kMapGridLevels] = 0;
    }
    if (tid == 0) { a.pin[kMgtStarted] = 1; a.pin[kMgtGoalX] = gx; a.pin[kMgtGoalY] = gy; }
}

// What k_mgt_round loads beside the distances, inside tile_load's batches: the costmap byte (the same memory round trip as the
// distance), kept as one 64-bit word a lane: bit y of the lane's column.  A cell off the map is blocked: nothing runs through it.
struct MgtBlocked {
    const unsigned char* grid;
    unsigned long long col_word;
    unsigned char byte[kTileLoadBatch];
    __device__ __forceinline__ void load(int j, size_t idx) { byte[j] = grid[idx]; }
    __device__ __forceinline__ void ready() {}
    __device__ __forceinline__ void row(int j, int r, int, int, bool in)
    {
        col_word |= (unsigned long long)((!in || byte[j] >= kMapGridBlocked) ? 1u : 0u) << r;
    }
};

// In LDS a blocked cell carries the SIGN BIT on top of its value (a value is at most UN <= 2^30 + 1): `cand < old` in signed
// arithmetic is then false at every blocked cell without a test of its own, and the running value takes the cell's value with the
// bit masked off.  s_old carries the bit too, so the store phase sees a blocked cell unchanged, which it is.
constexpr int kMgtValueMask = 0x7fffffff;

// One directional scan of a lane's line: `p` points at the line's first cell in LDS and advances by PS; v enters as the halo cell in
// front of the line (a halo cell carries no bit).  The line's cells are read kMgtScanBatch at a time BEFORE the chain that depends on
// v runs over them: a lane's line is written by that lane alone inside a scan (rows in the row scans, columns in the column scans, a
// barrier in between), so a cell read ahead is the cell the chain would have read, and a batch costs one LDS round trip, not one a
// cell.
constexpr int kMgtScanBatch = 16;
static_assert(kNavTile % kMgtScanBatch == 0, "a line is scanned in whole batches");

template <int PS>
__device__ __forceinline__ bool mgt_scan(int* p, int v)
{
    bool changed = false;
#pragma unroll
    for (int k0 = 0; k0 < kNavTile; k0 += kMgtScanBatch) {              // (bounded by the line's cells)
        int old[kMgtScanBatch];
#pragma unroll
        for (int j = 0; j < kMgtScanBatch; ++j) old[j] = p[(k0 + j) * PS];
#pragma unroll
        for (int j = 0; j < kMgtScanBatch; ++j) {
            const int cand = v + 1;                                     // v <= UN <= 2^30 + 1: no wrap
            const bool lower = cand < old[j];                           // (never at a blocked cell: it is negative)
            v = lower ? cand : (old[j] & kMgtValueMask);                // a blocked cell: v = old, and nothing is written
            if (lower) { p[(k0 + j) * PS] = cand; changed = true; }
        }
    }
    return changed;
}

__global__ __launch_bounds__(64) void k_mgt_round(MapGridTiledArgs a)
{
    __shared__ int s_val[(kNavTile + 2) * kMgtStride];                  // [row + 1][column + 1] with the halo
    __shared__ int s_old[kNavTile * kNavTile];                          // the distances as they were loaded
    const int lane = (int)threadIdx.x, g = (int)blockIdx.y, nt = a.ntx * a.nty;
    int* const dist = g ? a.dist[1] : a.dist[0];
    int* const status = g ? a.status[1] : a.status[0];
    TileRound t;
    if (!tile_round_enter(a.act + (size_t)g * 2 * nt, a.round, a.ntx, a.nty, status + kMapGridLevels, t)) return;    // (uniform)
    const int UN = a.sx * a.sy + 1;
    MgtBlocked blk{a.grid, 0ull, {}};
    tile_load<kMgtStride, false>(dist, a.sx, a.sy, t, UN, s_val, s_old, blk);
    __syncthreads();
    // the blocked cells of the lane's column get their bit, in both copies (s_old holds what s_val holds: read once, written twice)
#pragma unroll
    for (int r0 = 0; r0 < kNavTile; r0 += kMgtScanBatch) {              // (bounded by the column's cells)
        int val[kMgtScanBatch];
#pragma unroll
        for (int j = 0; j < kMgtScanBatch; ++j) val[j] = s_old[(r0 + j) * kNavTile + lane];
#pragma unroll
        for (int j = 0; j < kMgtScanBatch; ++j) {
            if ((blk.col_word >> (r0 + j)) & 1ull) {
                s_old[(r0 + j) * kNavTile + lane] = val[j] | ~kMgtValueMask;
                s_val[(r0 + j + 1) * kMgtStride + lane + 1] = val[j] | ~kMgtValueMask;
            }
        }
    }
    __syncthreads();

    // ---- relax to the tile's fixed point
    bool any_change = false;
    for (int it = 0; it < kNavTile * kNavTile; ++it) {                  // (bounded by the tile's cell count)
        bool ch = false;
        int* row = s_val + (lane + 1) * kMgtStride;                     // row `lane`: cells row[1 .. 64], halo row[0] and row[65]
        ch |= mgt_scan<1>(row + 1, row[0]);
        ch |= mgt_scan<-1>(row + kNavTile, row[kNavTile + 1]);
        __syncthreads();
        int* col = s_val + lane + 1;                                    // column `lane`: cells col[(1 .. 64) * stride]
        ch |= mgt_scan<kMgtStride>(col + kMgtStride, col[0]);
        ch |= mgt_scan<-kMgtStride>(col + kNavTile * kMgtStride, col[(kNavTile + 1) * kMgtStride]);
        __syncthreads();
        if (!__any(ch)) break;
        any_change = true;
    }
    if (!any_change) return;                                            // (uniform)

    // (a changed cell is not blocked: what is stored carries no bit)
    tile_store_and_mark<kMgtStride, false>(dist, a.sx, a.sy, a.ntx, a.nty, t, s_val, s_old);
}

__global__ __launch_bounds__(64) void k_mgt_close(MapGridTiledArgs a)
{
    const int nt = a.ntx * a.nty;
    bool marked = false;
    int rounds = 0;
    for (int g = 0; g < a.n_grids; ++g) {                               // (at most two)
        marked |= tiles_still_marked(a.act + (size_t)g * 2 * nt, a.round, nt);      // in the map the next round would read
        const int r = tile_load_word((g ? a.status[1] : a.status[0]) + kMapGridLevels);
        rounds = r > rounds ? r : rounds;
    }
    if (threadIdx.x == 0) { a.pin[kMgtRounds] = rounds; a.pin[kMgtConverged] = marked ? 0 : 1; }
}

__global__ __launch_bounds__(256) void k_mgt_rim(MapGridTiledArgs a)
{
    int* const dist = blockIdx.y ? a.dist[1] : a.dist[0];
    const uint32_t sx = (uint32_t)a.sx, sy = (uint32_t)a.sy, cells = sx * sy;
    const int OB = (int)cells;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < cells; i += gridDim.x * 256u) {     // (bounded by the cell count)
        if (a.grid[i] < kMapGridBlocked || dist[i] == 0) continue;      // not blocked, or a blocked source
        const uint32_t y = i / sx, x = i - y * sx;
        // (every value tested is below OB and stays, or is UN / OB, both not below OB: see the file's header)
        const bool rim = (x > 0u && dist[i - 1u] < OB) || (x + 1u < sx && dist[i + 1u] < OB) ||
                         (y > 0u && dist[i - sx] < OB) || (y + 1u < sy && dist[i + sx] < OB);
        if (rim) dist[i] = OB;
    }
}

hipError_t launch_mgt_seed(hipStream_t st, const MapGridTiledArgs& a)
{
    if (a.n_grids < 1 || a.n_grids > 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mgt_seed, dim3(1), dim3(kMgtSeedThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_mgt_round(hipStream_t st, const MapGridTiledArgs& a)
{
    hipLaunchKernelGGL(k_mgt_round, dim3((unsigned)(a.ntx * a.nty), (unsigned)a.n_grids), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_mgt_close(hipStream_t st, const MapGridTiledArgs& a)
{
    hipLaunchKernelGGL(k_mgt_close, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_mgt_rim(hipStream_t st, const MapGridTiledArgs& a)
{
    const uint32_t cells = (uint32_t)a.sx * (uint32_t)a.sy;
    const uint32_t blocks = std::max<uint32_t>(std::min<uint32_t>((cells + 1023u) / 1024u, 2048u), 1u);
    hipLaunchKernelGGL(k_mgt_rim, dim3(blocks, (unsigned)a.n_grids), dim3(256), 0, st, a);
    return hipGetLastError();
}

} // namespace gem
