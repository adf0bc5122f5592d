// gem_navquad.hip -- the quadratic potential on the device costmap, gfx950: the round kernel of gem_costmap_navplan_quadratic.  The
// contract is in include/gem_hip_navquad.h, the cell update in gem_navquad.hpp (shared with the host twin); k_nav_init and k_nav_finish
// (gem_navplan.hip) run in front of and behind the rounds as they do for the linear plan.  Integer results only.
//
// k_navquad_round is a further client of gem_tile_round.hpp (after k_nav_round, k_front_round and the tiled MapGrid): 4-connectivity,
// no corners, tile_round_enter, tile_load and tile_store_and_mark as they stand.  Its own part:
//   the table     a lane turns four of the 256 weights into table words (gem_navquad.hpp: the weight and a reciprocal of 10000 * hf in
//                 one word) and the tile keeps them in LDS; a cell's word -- the outline and the source rule applied, 0 = impassable --
//                 is looked up inside tile_load's batches and lies in s_w, where the linear plan keeps the weight.
//   the passes    an update needs both axes, so a directional scan carries ONE neighbour in a register and reads the other three from
//                 LDS: lane t runs along row t from the left halo to the right and back, then along column t down and up; a cell
//                 takes min(old, T).  The strides are odd, so the lanes of a step hit different banks.  Lanes read cells that other
//                 lanes write in the same scan; whatever they see is a value that was stored, and any order of updates is a correct
//                 one -- the order only decides how many passes a tile needs.
//   the bound     a pass is the four scans; a round allows a tile a.passes of them (kNavQuadPasses; stated in the loop's condition).
//                 A pass that changed nothing read only current values, so the update's equation holds in the tile: its local fixed
//                 point.  A tile that still changed in its last allowed pass stores what it has and MARKS ITS OWN WORD in the next
//                 round's active map: it goes on a round later.
// Why points 1 - 4 of gem_tile_round.hpp hold.  (1) a cell is stored only as min(old, T) and only when that is below old.  (2) T is
// monotone in every neighbour (include/gem_hip_navquad.h), so from values at or above the greatest fixed point P* it gives
// T(values) >= T(P*) = P*: by induction from k_nav_init's grid (UNREACHED, 0 at the source, which never changes: T >= 1 there) no
// stored value lies below P*, the halo's age notwithstanding, and an unfinished tile's values are as valid as a finished one's.
// (3) as there.  (4) a tile marking itself is a new WRITER OF A MARK, not of a value: it stores 1 into the next round's map as its
// neighbours do, the tile clears its own word of this round's map alone, and the computation has converged when a round marks
// nothing -- then every tile ended on a pass without a change, with the true halo.  So the result is P* whatever the pass bound.
// The source's tile and its four neighbours are marked by k_nav_init, as for the linear plan.
#include "gem_navplan.hpp"
#include "gem_navquad.hpp"

namespace gem {

// One directional scan of a lane's line.  `p` points at the line's first cell in LDS and `w` at its table word; P and W step along the
// line, Q steps to the two neighbours beside it.  v enters as the halo cell in front of the line and carries the cell just left.
template <int P, int Q, int W>
__device__ __forceinline__ bool navquad_scan(int* p, const unsigned* w, int v)
{
    bool changed = false;
#pragma unroll 8
    for (int k = 0; k < kNavTile; ++k) {                                // (bounded by the line's cells)
        const int old = p[k * P];
        const int t = navquad_update(w[k * W], v, p[(k + 1) * P], p[k * P - Q], p[k * P + Q]);
        v = t < old ? t : old;
        if (t < old) { p[k * P] = v; changed = true; }
    }
    return changed;
}

// What k_navquad_round loads beside the potentials, inside tile_load's batches: the costmap byte, the table lookups of a batch in
// flight together, and the cell's table word with the outline and the source rule into s_w.
struct NavQuadWords {
    const NavArgs& a;
    const unsigned* s_tab;
    unsigned* s_w;
    unsigned char byte[kTileLoadBatch];
    unsigned wv[kTileLoadBatch];
    __device__ __forceinline__ void load(int j, size_t idx) { byte[j] = a.grid[idx]; }
    __device__ __forceinline__ void ready()
    {
#pragma unroll
        for (int j = 0; j < kTileLoadBatch; ++j) wv[j] = s_tab[byte[j]];
    }
    __device__ __forceinline__ void row(int j, int r, int gx, int gy, bool in)
    {
        unsigned w1 = in ? wv[j] : 0u;
        if (a.outline && (gx == 0 || gy == 0 || gx == a.sx - 1 || gy == a.sy - 1)) w1 = 0u;
        if (in && gy * a.sx + gx == a.start) w1 = navquad_word(1);      // the source: T >= 1 there, its 0 stays whatever its byte
        s_w[r * kNavWStride + (int)threadIdx.x] = w1;
    }
};

__global__ __launch_bounds__(64) void k_navquad_round(NavArgs a)
{
    __shared__ int s_pot[(kNavTile + 2) * kNavPotStride];               // [row + 1][column + 1] with the halo
    __shared__ unsigned s_w[kNavTile * kNavWStride];
    __shared__ int s_old[kNavTile * kNavTile];                          // the potentials as they were loaded
    __shared__ unsigned s_tab[256];
    const int lane = (int)threadIdx.x;
    TileRound t;
    if (!tile_round_enter(a.act, a.round, a.ntx, a.nty, &a.status[kNavRounds], t)) return;   // (uniform)
    int tab[4];                                                         // the weight table: four weights a lane
#pragma unroll
    for (int k = 0; k < 4; ++k) tab[k] = a.w[k * 64 + lane];
#pragma unroll
    for (int k = 0; k < 4; ++k) s_tab[k * 64 + lane] = navquad_word(tab[k]);
    __syncthreads();
    NavQuadWords words{a, s_tab, s_w};
    tile_load<kNavPotStride, false>(a.pot, a.sx, a.sy, t, kNavUnreached, s_pot, s_old, words);
    __syncthreads();

    // ---- relax: at most a.passes passes
    bool any_change = false, last = false;
    for (int it = 0; it < a.passes; ++it) {                             // (bounded by the pass count)
        bool ch = false;
        int* row = s_pot + (lane + 1) * kNavPotStride;                  // row `lane`: cells row[1 .. 64], halo row[0] and row[65]
        const unsigned* wrow = s_w + lane * kNavWStride;
        ch |= navquad_scan<1, kNavPotStride, 1>(row + 1, wrow, row[0]);
        ch |= navquad_scan<-1, kNavPotStride, -1>(row + kNavTile, wrow + kNavTile - 1, row[kNavTile + 1]);
        __syncthreads();
        int* col = s_pot + lane + 1;                                    // column `lane`: cells col[(1 .. 64) * stride]
        const unsigned* wcol = s_w + lane;
        ch |= navquad_scan<kNavPotStride, 1, kNavWStride>(col + kNavPotStride, wcol, col[0]);
        ch |= navquad_scan<-kNavPotStride, 1, -kNavWStride>(col + kNavTile * kNavPotStride, wcol + (kNavTile - 1) * kNavWStride,
                                                             col[(kNavTile + 1) * kNavPotStride]);
        __syncthreads();
        last = __any(ch);
        if (!last) break;
        any_change = true;
    }
    if (!any_change) return;                                            // (uniform)

    tile_store_and_mark<kNavPotStride, false>(a.pot, a.sx, a.sy, a.ntx, a.nty, t, s_pot, s_old);
    if (last && lane == 0) t.act_next[t.tile] = 1;                      // not at its fixed point yet: the tile goes on a round later
}

hipError_t launch_navquad_round(hipStream_t st, const NavArgs& a)
{
    hipLaunchKernelGGL(k_navquad_round, dim3((unsigned)(a.ntx * a.nty)), dim3(64), 0, st, a);
    return hipGetLastError();
}

} // namespace gem
