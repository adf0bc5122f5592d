// gem_navplan.hip -- global_planner's weighted potential and grid path on the device costmap, gfx950.  The contract is restated in
// include/gem_hip_navplan.h.  Integer code only.
//
// The potential is the first costmap computation that does not fit one workgroup (a global costmap is 1000 x 1000 cells), so it
// lives in global memory and is relaxed tile by tile, a launch per round.  The protocol -- active maps, load, store, marks, and why
// a tile may read old halo values -- is gem_tile_round.hpp's; this file's own part:
//   k_nav_round   an active tile loads, beside its potentials, its weights (the byte through w, the outline applied, impassable =
//                 2^31) and relaxes to the tile's LOCAL fixed point by directional scans: lane t runs pot[x] = min(pot[x],
//                 pot[x - 1] + w[x]) along row t from the left halo to the right and back, then the same along column t down and
//                 up, with the running value in a register.  A straight corridor costs one pass of the four instead of 64 Jacobi
//                 sweeps; a pass of the four extends every in-tile optimal path by at least one straight segment, a path has at
//                 most 4096 cells, hence the loop's bound (stated in its condition).  Connectivity is 4: the four edges mark, no
//                 corner.
//   k_nav_finish  one wave behind a chunk of rounds.  A tile still marked: "not converged" goes to the pinned status and the host
//                 enqueues another chunk.  Otherwise GridPath::getPath: a dependent chain, one memory round trip per step; lanes
//                 0 .. 7 load the eight neighbours and the step is the wave minimum of potential * 8 + scan order (gem_navpath.hpp,
//                 shared with the host twin).
// Why its values are valid ones (point 2 there): every stored potential is the length of a real path from the start (induction: a
// halo value is one, and v + w extends it), so no value ever lies BELOW the fixed point.  That fixed point is pot[n] = min4(pot) + w[n]
// inside every tile with the true halo, the contract's unique one.  The start cell never changes (it is 0 from k_nav_init on), so
// k_nav_init marks the start's tile AND its four neighbours: a start on a tile's edge reaches the neighbour through its halo.
// status.rounds is the protocol's round counter: it depends on timing, the potential does not.
#include "gem_navplan.hpp"

#include <algorithm>

namespace gem {

static_assert(kNavWStride % 2 == 1, "an odd LDS stride: a wave's lanes on rows t hit different banks");

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

// What k_nav_round loads beside the potentials, inside tile_load's batches: the costmap byte (the same memory round trip as the
// potential), the table lookups of a batch in flight together, and the weight with the outline and the source rule into s_w.
struct NavWeights {
    const NavArgs& a;
    const int* s_tab;
    unsigned* s_w;
    unsigned char byte[kTileLoadBatch];
    int wv[kTileLoadBatch];
    __device__ __forceinline__ void load(int j, size_t idx) { byte[j] = a.grid[idx]; }
    __device__ __forceinline__ void ready()
    {
#pragma unroll
        for (int j = 0; j < kTileLoadBatch; ++j) wv[j] = s_tab[byte[j]];
    }
    __device__ __forceinline__ void row(int j, int r, int gx, int gy, bool in)
    {
        int w1 = in ? wv[j] : 0;
        if (a.outline && (gx == 0 || gy == 0 || gx == a.sx - 1 || gy == a.sy - 1)) w1 = 0;
        if (in && gy * a.sx + gx == a.start) w1 = 1;                    // the source: its potential is 0 and stays, whatever its byte
        s_w[r * kNavWStride + (int)threadIdx.x] = w1 > 0 ? (unsigned)w1 : kNavBlockedWeight;
    }
};

__global__ __launch_bounds__(64) void k_nav_round(NavArgs a)
{
    __shared__ unsigned s_pot[(kNavTile + 2) * kNavPotStride];          // [row + 1][column + 1] with the halo
    __shared__ unsigned s_w[kNavTile * kNavWStride];
    __shared__ int s_old[kNavTile * kNavTile];                          // the potentials as they were loaded
    __shared__ int s_tab[256];
    const int lane = (int)threadIdx.x;
    int* const s_val = reinterpret_cast<int*>(s_pot);                   // (the shared code only copies and compares for inequality)
    TileRound t;
    if (!tile_round_enter(a.act, a.round, a.ntx, a.nty, &a.status[kNavRounds], t)) return;   // (uniform)
    int tab[4];                                                         // the weight table: four words a lane
#pragma unroll
    for (int k = 0; k < 4; ++k) tab[k] = a.w[k * 64 + lane];
#pragma unroll
    for (int k = 0; k < 4; ++k) s_tab[k * 64 + lane] = tab[k];
    __syncthreads();
    NavWeights weights{a, s_tab, s_w};
    tile_load<kNavPotStride, false>(a.pot, a.sx, a.sy, t, kNavUnreached, s_val, s_old, weights);
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

    tile_store_and_mark<kNavPotStride, false>(a.pot, a.sx, a.sy, a.ntx, a.nty, t, s_val, s_old);
}

__global__ __launch_bounds__(64) void k_nav_finish(NavArgs a)
{
    const int nt = a.ntx * a.nty, lane = (int)threadIdx.x;
    const bool marked = tiles_still_marked(a.act, a.round, nt);         // in the map the next round would read
    const int rounds = tile_load_word(a.status + kNavRounds);
    int* pin = a.pin + 256;
    if (marked) {                                                       // (uniform) another chunk of rounds
        if (lane == 0) { pin[kNavRounds] = rounds; pin[kNavConverged] = 0; }
        return;
    }
    const long long cells = (long long)a.sx * a.sy;
    int n = 0, found = 0, goal_pot = kNavUnreached;
    if (a.goal >= 0) goal_pot = tile_load_word(a.pot + a.goal);
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
