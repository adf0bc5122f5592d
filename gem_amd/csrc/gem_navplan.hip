// gem_navplan.hip -- global_planner's weighted potential and grid path on the device costmap, gfx950.  The contract is restated in
// include/gem_hip_navplan.h.  Integer code only.
//
// The potential is the first costmap computation that does not fit one workgroup (a global costmap is 1000 x 1000 cells), so it
// lives in global memory and is relaxed TILE BY TILE, a launch per round:
//   k_nav_round   one workgroup -- one wave -- per tile of 64 x 64 cells.  A tile that is not marked in this round's active map leaves
//                 at once.  An active tile clears its mark, loads its weights (the byte through w, the outline applied, impassable =
//                 2^31), its potentials and a one-cell halo into LDS (rows in batches whose loads are all in flight together) and relaxes to the tile's LOCAL fixed point by directional
//                 scans: lane t runs pot[x] = min(pot[x], pot[x - 1] + w[x]) along row t from the left halo to the right and back,
//                 then the same along column t down and up, with the running value in a register.  A straight corridor costs one pass
//                 of the four instead of 64 Jacobi sweeps; a pass of the four extends every in-tile optimal path by at least one
//                 straight segment, a path has at most 4096 cells, hence the loop's bound (stated in its condition).  Then it stores
//                 the cells that changed and marks, in the NEXT round's map, the neighbour tiles whose facing edge changed.
//   k_nav_finish  one wave behind a chunk of rounds.  A tile still marked: "not converged" goes to the pinned status and the host
//                 enqueues another chunk.  Otherwise GridPath::getPath: a dependent chain, one memory round trip per step; lanes
//                 0 .. 7 load the eight neighbours and the step is the wave minimum of potential * 8 + scan order (gem_navpath.hpp,
//                 shared with the host twin).
// The active maps are double-buffered: round r reads map r & 1 and writes marks (plain stores of 1) into map (r + 1) & 1; a tile is
// the only one that clears its own word.  The search has converged when a round marks nothing.
//
// Why stale halo reads are safe.  Inside a launch a tile may read a neighbour's edge while the neighbour rewrites it; nothing orders
// the two, and nothing needs to:
//   1. potentials only fall: every store writes a value below the one the same workgroup loaded from that cell, and a cell is
//      written by its own tile's workgroup alone (and by k_nav_init before the first round);
//   2. every stored value is the length of a real path from the start (induction: a halo value is one, and v + w extends it), so no
//      value ever lies BELOW the fixed point, and a tile that works from old halo values computes values that are too large at worst;
//   3. an aligned 32-bit load sees the old or the new value of a cell, never a mixture;
//   4. a tile whose neighbour's facing edge changed in round r is marked by that neighbour and runs in round r + 1, behind the
//      kernel boundary that makes round r's stores visible to every CU.  So whatever a tile missed it sees one round later.
// At the fixed point no edge changes, no tile is marked, and pot[n] = min4(pot) + w[n] holds inside every tile with the true halo:
// that is the contract's unique fixed point.  The start cell never changes (it is 0 from k_nav_init on), so k_nav_init marks the
// start's tile AND its four neighbours: a start on a tile's edge reaches the neighbour through its halo.
//
// No workgroup waits for another one: there is no spin-wait, no grid-wide barrier, no cooperative launch and no residency
// requirement; every loop is bounded by a count stated in its condition.  Global memory is touched by vector loads, stores and one
// vector atomic (the round counter) only.  status.rounds is the last round that found an active tile, plus one; it depends on timing
// (point 4 above: a tile may or may not already see the new edge), the potential does not.
#include "gem_navplan.hpp"

#include <algorithm>

namespace gem {

static_assert(kNavTile == 64, "a tile's row and column are a wave wide");
static_assert((kNavTile + 2) % kNavLoadBatch == 0, "the load phase takes the tile's rows and its two halo rows in whole batches");
static_assert(kNavPotStride % 2 == 1 && kNavWStride % 2 == 1, "odd LDS strides: a wave's lanes on rows t hit different banks");

// A word another launch wrote, read with a vector load: a plain load at a uniform address would be moved to the scalar unit, and
// global memory is touched by vector instructions only here.
__device__ __forceinline__ int nav_load_word(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(256) void k_nav_init(NavArgs a)
{
    const uint32_t cells = (uint32_t)a.sx * (uint32_t)a.sy, nt = (uint32_t)(a.ntx * a.nty);
    const uint32_t i0 = blockIdx.x * 256u + threadIdx.x;
    for (uint32_t i = i0; i < cells; i += gridDim.x * 256u) a.pot[i] = (int)i == a.start ? 0 : kNavUnreached;
    int stx = -2, sty = -2;
    if (a.start >= 0) { stx = (a.start % a.sx) / kNavTile; sty = (a.start / a.sx) / kNavTile; }
    for (uint32_t i = i0; i < 2u * nt; i += gridDim.x * 256u) {
        const int t = (int)(i < nt ? i : i - nt), ty = t / a.ntx, tx = t - ty * a.ntx;
        const int d = (tx > stx ? tx - stx : stx - tx) + (ty > sty ? ty - sty : sty - ty);
        a.act[i] = (i < nt && d <= 1) ? 1 : 0;                          // round 0 reads map 0: the start's tile and its four neighbours
    }
    if (i0 < 256u) a.w[i0] = a.pin[i0];
    if (i0 < (uint32_t)kNavStatusWords) a.status[i0] = 0;
}

// one directional scan of a lane's line: `p` points at the line's first cell in LDS, `w` at its weight, both advance by the strides
// given; v enters as the halo cell in front of the line
template <int PS, int WS>
__device__ __forceinline__ bool nav_scan(unsigned* p, const unsigned* w, unsigned v)
{
    bool changed = false;
#pragma unroll 8
    for (int k = 0; k < kNavTile; ++k) {                                // (bounded by the line's cells)
        const unsigned old = p[k * PS], cand = v + w[k * WS];           // v <= 2^31 - 1 and w <= 2^31: no wrap
        v = cand < old ? cand : old;
        if (cand < old) { p[k * PS] = v; changed = true; }
    }
    return changed;
}

__global__ __launch_bounds__(64) void k_nav_round(NavArgs a)
{
    __shared__ unsigned s_pot[(kNavTile + 2) * kNavPotStride];          // [row + 1][column + 1] with the halo
    __shared__ unsigned s_w[kNavTile * kNavWStride];
    __shared__ unsigned s_old[kNavTile * kNavTile];                     // the potentials as they were loaded
    __shared__ int s_tab[256];
    const int nt = a.ntx * a.nty, tile = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (tile >= nt) return;
    int* act_cur = a.act + (a.round & 1) * nt;
    int* act_next = a.act + ((a.round + 1) & 1) * nt;
    if (nav_load_word(act_cur + tile) == 0) return;                                     // (uniform: the whole wave read the same word)
    if (lane == 0) {
        act_cur[tile] = 0;                                              // read: cleared by its own tile
        atomicMax(&a.status[kNavRounds], a.round + 1);
    }
    const int ty = tile / a.ntx, tx = tile - ty * a.ntx;
    const int x0 = tx * kNavTile, y0 = ty * kNavTile;

    // ---- load: rows -1 .. 64 of the tile's columns and the two halo columns.  Every load of a batch of rows is issued before the
    //      first of them is used -- unconditional loads at clamped addresses, the selects afterwards -- so a batch costs one memory
    //      round trip, not one per row; the table lookups of a batch are in flight together in the same way.
    {
        const int gx = x0 + lane, hy = y0 + lane;
        int halo[2];
        bool halo_in[2];
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int hx = side ? x0 + kNavTile : x0 - 1;
            halo_in[side] = hy < a.sy && hx >= 0 && hx < a.sx;
            halo[side] = a.pot[halo_in[side] ? (size_t)hy * (size_t)a.sx + (size_t)hx : (size_t)0];
        }
        int tab[4];                                                     // the weight table: four words a lane, in flight with the halo
#pragma unroll
        for (int k = 0; k < 4; ++k) tab[k] = a.w[k * 64 + lane];
#pragma unroll
        for (int k = 0; k < 4; ++k) s_tab[k * 64 + lane] = tab[k];
        __syncthreads();
#pragma unroll 1
        for (int r0 = 0; r0 < kNavTile + 2; r0 += kNavLoadBatch) {
            int p[kNavLoadBatch];
            unsigned char byte[kNavLoadBatch];
            int wv[kNavLoadBatch];
#pragma unroll
            for (int j = 0; j < kNavLoadBatch; ++j) {
                const int gy = y0 + r0 + j - 1;
                const bool in = gy >= 0 && gy < a.sy && gx < a.sx;
                const size_t idx = in ? (size_t)gy * (size_t)a.sx + (size_t)gx : (size_t)0;
                p[j] = a.pot[idx];
                byte[j] = a.grid[idx];
            }
#pragma unroll
            for (int j = 0; j < kNavLoadBatch; ++j) wv[j] = s_tab[byte[j]];
#pragma unroll
            for (int j = 0; j < kNavLoadBatch; ++j) {
                const int r = r0 + j, gy = y0 + r - 1;
                const bool in = gy >= 0 && gy < a.sy && gx < a.sx;
                const unsigned pv = in ? (unsigned)p[j] : (unsigned)kNavUnreached;
                s_pot[r * kNavPotStride + lane + 1] = pv;
                if (r >= 1 && r <= kNavTile) {
                    int w1 = in ? wv[j] : 0;
                    if (a.outline && (gx == 0 || gy == 0 || gx == a.sx - 1 || gy == a.sy - 1)) w1 = 0;
                    if (in && gy * a.sx + gx == a.start) w1 = 1;        // the source: its potential is 0 and stays, whatever its byte
                    s_w[(r - 1) * kNavWStride + lane] = w1 > 0 ? (unsigned)w1 : kNavBlockedWeight;
                    s_old[(r - 1) * kNavTile + lane] = pv;              // what memory holds: the store phase compares with it
                }
            }
        }
#pragma unroll
        for (int side = 0; side < 2; ++side)
            s_pot[(lane + 1) * kNavPotStride + (side ? kNavTile + 1 : 0)] = halo_in[side] ? (unsigned)halo[side] : (unsigned)kNavUnreached;
    }
    __syncthreads();

    // ---- relax to the tile's fixed point
    bool any_change = false;
    for (int it = 0; it < kNavTile * kNavTile; ++it) {                  // (bounded by the tile's cell count)
        bool ch = false;
        unsigned* row = s_pot + (lane + 1) * kNavPotStride;             // row `lane`: cells row[1 .. 64], halo row[0] and row[65]
        const unsigned* wrow = s_w + lane * kNavWStride;
        ch |= nav_scan<1, 1>(row + 1, wrow, row[0]);
        ch |= nav_scan<-1, -1>(row + kNavTile, wrow + kNavTile - 1, row[kNavTile + 1]);
        __syncthreads();
        unsigned* col = s_pot + lane + 1;                               // column `lane`: cells col[(1 .. 64) * stride]
        const unsigned* wcol = s_w + lane;
        ch |= nav_scan<kNavPotStride, kNavWStride>(col + kNavPotStride, wcol, col[0]);
        ch |= nav_scan<-kNavPotStride, -kNavWStride>(col + kNavTile * kNavPotStride, wcol + (kNavTile - 1) * kNavWStride,
                                                      col[(kNavTile + 1) * kNavPotStride]);
        __syncthreads();
        if (!__any(ch)) break;
        any_change = true;
    }
    if (!any_change) return;                                            // (uniform)

    // ---- store what changed; which edges did.  The old values are the LDS copy of the load phase: only this workgroup writes these
    //      cells, so memory still holds them and nothing is read again.
    int edges = 0;                                                      // 1 top | 2 bottom | 4 left | 8 right
    {
        const int gx = x0 + lane;
#pragma unroll 8
        for (int r = 0; r < kNavTile; ++r) {
            const int gy = y0 + r;
            const unsigned old = s_old[r * kNavTile + lane], now = s_pot[(r + 1) * kNavPotStride + lane + 1];
            if (gy < a.sy && gx < a.sx && now != old) {
                a.pot[(size_t)gy * (size_t)a.sx + (size_t)gx] = (int)now;
                edges |= (r == 0 ? 1 : 0) | (r == kNavTile - 1 ? 2 : 0) | (lane == 0 ? 4 : 0) | (lane == kNavTile - 1 ? 8 : 0);
            }
        }
    }
    const bool top = __any(edges & 1), bottom = __any(edges & 2), left = __any(edges & 4), right = __any(edges & 8);
    if (lane == 0) {
        if (top && ty > 0) act_next[tile - a.ntx] = 1;
        if (bottom && ty + 1 < a.nty) act_next[tile + a.ntx] = 1;
        if (left && tx > 0) act_next[tile - 1] = 1;
        if (right && tx + 1 < a.ntx) act_next[tile + 1] = 1;
    }
}

__global__ __launch_bounds__(64) void k_nav_finish(NavArgs a)
{
    const int nt = a.ntx * a.nty, lane = (int)threadIdx.x;
    const int* act = a.act + (a.round & 1) * nt;                        // the map the next round would read
    bool marked = false;
    for (int i = lane; i < nt; i += 64) marked |= act[i] != 0;
    const int rounds = nav_load_word(a.status + kNavRounds);
    int* pin = a.pin + 256;
    if (__any(marked)) {                                                // (uniform) another chunk of rounds
        if (lane == 0) { pin[kNavRounds] = rounds; pin[kNavConverged] = 0; }
        return;
    }
    const long long cells = (long long)a.sx * a.sy;
    int n = 0, found = 0, goal_pot = kNavUnreached;
    if (a.goal >= 0) goal_pot = nav_load_word(a.pot + a.goal);
    if (a.start >= 0 && a.goal >= 0 && goal_pot != kNavUnreached) {
        int c = a.goal;
        const int k = lane & 7;                                         // lanes 8 .. 63 repeat lanes 0 .. 7
        for (long long step = 0; c != a.start && step < cells - 1; ++step) {   // (bounded by the cell count: the potential strictly falls)
            if (lane == 0) a.path[cells - 1 - n] = c;
            ++n;
            const int cx = c % a.sx, cy = c / a.sx;
            const int x = cx + nav_xd(k), y = cy + nav_yd(k);
            const bool in = x >= 0 && y >= 0 && x < a.sx && y < a.sy;
            const int p = a.pot[in ? (size_t)y * (size_t)a.sx + (size_t)x : (size_t)0];
            unsigned long long key = in ? nav_key(p, k) : kNavNoKey;
#pragma unroll
            for (int off = 1; off < 8; off <<= 1) {
                const unsigned long long o = __shfl_xor(key, off, 8);
                key = o < key ? o : key;
            }
            if (key == kNavNoKey) break;                                // (uniform: every group of eight holds the same key)
            const int kb = (int)(key & 7ull);
            c = (cy + nav_yd(kb)) * a.sx + cx + nav_xd(kb);
        }
        if (lane == 0) a.path[cells - 1 - n] = c;
        ++n;
        found = c == a.start ? 1 : 0;
        if (!found) n = 0;
    }
    if (lane == 0) {
        const int words[5] = {1, found, n, rounds, goal_pot};
#pragma unroll
        for (int i = 0; i < 5; ++i) { a.status[i] = words[i]; pin[i] = words[i]; }
    }
}

hipError_t launch_nav_init(hipStream_t st, const NavArgs& a)
{
    const uint32_t cells = (uint32_t)a.sx * (uint32_t)a.sy;
    const uint32_t blocks = std::max<uint32_t>(std::min<uint32_t>((cells + 1023u) / 1024u, 2048u), 1u);
    hipLaunchKernelGGL(k_nav_init, dim3(blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_nav_round(hipStream_t st, const NavArgs& a)
{
    hipLaunchKernelGGL(k_nav_round, dim3((unsigned)(a.ntx * a.nty)), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_nav_finish(hipStream_t st, const NavArgs& a)
{
    hipLaunchKernelGGL(k_nav_finish, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError();
}

} // namespace gem
