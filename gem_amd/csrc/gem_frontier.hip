// gem_frontier.hip -- frontier search on the device costmap, gfx950: the frontier cells labelled into 8-connected frontiers, each reduced
// to a record, one winner.  The contract is restated in include/gem_hip_frontier.h.  Integer code only, except the pick's cost.
//
// Labelling is a connected-component problem above one workgroup (a global costmap is 1000 x 1000 cells), so it takes the form of
// gem_navplan.hip: the labels live in global memory and are relaxed tile by tile, a launch per round.  The protocol -- active maps,
// load, store, marks, and why a tile may read old halo values -- is gem_tile_round.hpp's; this file's own part:
//   k_front_classify  one pass over the cells: the byte, the four neighbours' bytes and potentials.  label[c] = c for a frontier cell,
//                     kFrontNone (2^31 - 1) otherwise; every tile that holds a frontier cell is marked in round 0's active map; the
//                     frontier cells are counted, one atomic per wave and trip at most.
//   k_front_round     an active tile loads its labels and a one-cell halo WITH the four corner cells (connectivity is 8: 66 x 66),
//                     leaves if it holds no frontier cell (nothing can change), and relaxes to the tile's LOCAL fixed point:
//                     every frontier cell takes the minimum of its own label and its eight neighbours',
//                     cells that are no frontier cells stay kFrontNone and carry nothing.  Lane t runs a running minimum along row t
//                     from the left halo to the right and back, then along column t down and up, then along the two wrapped
//                     diagonals through (0, t) -- the minimum resets at a cell that is no frontier cell.  A line's 64 cells are held
//                     in registers between one batch of LDS loads and one of stores, and a step is arithmetic without a branch.  A
//                     straight run in any of the eight directions costs one pass instead of 64 sweeps (measured on the ragged rim of
//                     tools/bench_frontier.py: a step that waits for its own load and branches round its store, with one diagonal
//                     step per pass, took 12.2 ms where this form takes 5.6 ms); a pass extends the reach of a component's smallest
//                     label along every in-tile chain
//                     by at least one cell, a chain has at most 4096 cells, hence the loop's bound (stated in its condition).  Each of
//                     the up to EIGHT neighbour tiles is marked whose facing edge or corner cell changed.
//   k_front_check     one wave behind a chunk of rounds: "a tile is still marked" goes to the pinned words and the host enqueues
//                     another chunk, or the reduction.
// Why its values are valid ones (point 2 there): every stored label is the linear index of a cell of the SAME component (induction: a
// cell's own index is one, and a label taken from an 8-neighbour that is a frontier cell is one -- the halo's included), so no label
// ever lies BELOW the component's smallest cell.  The same holds inside a tile's LDS: a lane may read a neighbour row's cell before or
// after its owner lowers it, both are labels of the component, and a pass that changes nothing has read no cell that was written in
// it, so it has seen the fixed point itself.  That fixed point is label[c] = min(label[c], min8(label)) for every frontier cell with
// the true halo: two 8-adjacent frontier cells carry the same label, so a component carries one label, which is at most its smallest
// cell's own index (that cell started with it, and labels only fall) and not below it: every frontier cell carries its component's
// smallest cell.
//
// The reduction needs no order either.  The roots (label[c] == c) go through the stable count / scan / scatter of gem_compact.hpp into
// a dense list in ascending cell order; the scatter writes each root's list index at the root's cell of a cells-sized scratch (only
// root positions are ever read, so it is never cleared) and resets the root's record.  k_front_accumulate then adds every frontier
// cell into its root's record: the size by a 32-bit add, the two coordinate sums by 64-bit integer adds, the access key
// (potential << 32) | cell by a 64-bit unsigned minimum -- vector atomics on integers, whose result does not depend on their order.
// A wave whose frontier cells all share one root (the 64 consecutive cells of a row mostly do) combines them in registers first and
// issues one lane's atomics; that spares same-address atomics and is not claimed as a measured gain.  k_front_pick, one workgroup,
// computes cost and kept flag per record, compacts the kept records in order, takes the minimum of (cost, root) and writes the winner
// and the counts to the pinned status.
//
// As in the rounds, no workgroup waits for another one here, every loop is bounded by a count stated in its condition, and global
// memory is touched by vector loads, stores and vector atomics only.  status.rounds is the protocol's round counter: it depends on
// timing, nothing else does.
#include "gem_frontier.hpp"

#include "gem_compact.hpp"

#include <algorithm>

namespace gem {

static_assert(kFrontNone == kNavUnreached, "one 'nothing' for labels and potentials");
static_assert(sizeof(gem_frontier) == 40, "the record of the header");

constexpr unsigned long long kFrontNoKey = ~0ull;

// the access key of cell (x, y): the smallest (potential << 32) | cell over its doors, kFrontNoKey without one.  The four neighbours'
// loads are unconditional at clamped addresses, the selects afterwards: one memory round trip.
__device__ __forceinline__ unsigned long long front_access_key(const FrontArgs& a, int x, int y)
{
    unsigned char byte[4];
    int p[4], n[4];
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int nx = x + (k == 0 ? -1 : k == 1 ? 1 : 0), ny = y + (k == 2 ? -1 : k == 3 ? 1 : 0);
        in[k] = nx >= 0 && ny >= 0 && nx < a.sx && ny < a.sy;
        n[k] = in[k] ? ny * a.sx + nx : 0;
        byte[k] = a.grid[n[k]];
        p[k] = a.pot[n[k]];
    }
    unsigned long long key = kFrontNoKey;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long cand = ((unsigned long long)(unsigned)p[k] << 32) | (unsigned)n[k];     // a potential is not negative
        if (in[k] && byte[k] != 255 && p[k] != kNavUnreached && cand < key) key = cand;
    }
    return key;
}

__global__ __launch_bounds__(256) void k_front_classify(FrontArgs a)
{
    const uint32_t cells = (uint32_t)a.sx * (uint32_t)a.sy;
    uint32_t count = 0;
    for (uint32_t base = blockIdx.x * 256u; base < cells; base += gridDim.x * 256u) {   // (workgroup-uniform; bounded by the cell count)
        const uint32_t i = base + threadIdx.x;
        bool fr = false;
        if (i < cells) {
            const int y = (int)(i / (uint32_t)a.sx), x = (int)(i - (uint32_t)y * (uint32_t)a.sx);
            fr = a.grid[i] == 255 && front_access_key(a, x, y) != kFrontNoKey;
            a.label[i] = fr ? (int)i : kFrontNone;
            if (fr) a.act[(y / kNavTile) * a.ntx + x / kNavTile] = 1;   // round 0 reads map 0
        }
        count += (uint32_t)__popcll(__ballot(fr));                      // wave-uniform
    }
    if (lane_id() == 0 && count) atomicAdd(&a.words[kFrontCells], (int)count);
}

// one step of a running minimum that resets at a cell that is no frontier cell, in arithmetic: kFrontNone + 1 is the one value with
// the sign bit set, so (old + 1) >> 31 is all ones for it alone, and min(run, old) | kFrontNone is kFrontNone (no label is negative)
__device__ __forceinline__ int front_step(int run, int old)
{
    const int none = (int)((unsigned)old + 1u) >> 31;
    return (run < old ? run : old) | (none & kFrontNone);
}

// Both directional scans of a lane's line: `p` points at the line's first cell in LDS and advances by S; `before` and `after` are the
// halo cells at its two ends.  The 64 cells are loaded into registers in one go (the loads are all in flight together), the running
// minimum -- it resets at a cell that is no frontier cell -- runs forward and back in registers without a branch, and the line is
// stored back whole: a step that waits for its own LDS load and branches round its store costs a memory latency per cell.
template <int S>
__device__ __forceinline__ bool front_line(int* p, int before, int after)
{
    int v[kNavTile];
#pragma unroll
    for (int k = 0; k < kNavTile; ++k) v[k] = p[k * S];
    int diff = 0;                                                       // the bits in which any cell changed
    int run = before;
#pragma unroll
    for (int k = 0; k < kNavTile; ++k) {                                // (bounded by the line's cells)
        const int old = v[k];
        run = front_step(run, old);
        diff |= run ^ old;
        v[k] = run;
    }
    run = after;
#pragma unroll
    for (int k = kNavTile - 1; k >= 0; --k) {                           // (bounded by the line's cells)
        const int old = v[k];
        run = front_step(run, old);
        diff |= run ^ old;
        v[k] = run;
    }
#pragma unroll
    for (int k = 0; k < kNavTile; ++k) p[k * S] = v[k];
    return diff != 0;
}

// The same along a WRAPPED diagonal: lane t takes the cells (row k, column (t + DC * k) mod 64), k = 0 .. 63 -- two real diagonals of
// the tile, every cell of the tile on exactly one lane's line, a step's 64 cells in 64 different banks.  A cell's neighbour along
// the line is the line's previous cell, except at the line's two ends and on both sides of the wrap, where it is a halo cell.
template <int DC>
__device__ __forceinline__ bool front_diagonal(int* s, int lane)
{
    constexpr int T = kNavTile, ST = kFrontStride;
    int kw = DC > 0 ? (lane == 0 ? -1 : T - lane) : (lane == T - 1 ? -1 : lane + 1);            // the first cell behind the wrap; -1: no wrap
    asm volatile("" : "+v"(kw));                                        // (not loop-invariant to the compiler: 128 hoisted compare masks would spill)
    const int kwc = kw < 0 ? 1 : kw;                                    // (an address on the tile for the lane without a wrap)
    int v[T];
#pragma unroll
    for (int k = 0; k < T; ++k) v[k] = s[(k + 1) * ST + ((lane + DC * k) & (T - 1)) + 1];
    const int c_last = (lane + DC * (T - 1)) & (T - 1);
    const int top = s[lane + 1 - DC];                                   // in front of cell 0 = (0, t): (-1, t - DC)
    const int bottom = s[(T + 1) * ST + c_last + 1 + DC];               // behind cell 63
    const int side_f = s[kwc * ST + (DC > 0 ? 0 : T + 1)];              // in front of cell kw: (kw - 1, -1) or (kw - 1, 64)
    const int side_b = s[(kwc + 1) * ST + (DC > 0 ? T + 1 : 0)];        // behind cell kw - 1: (kw, 64) or (kw, -1)
    int diff = 0;
    int run = top;
#pragma unroll
    for (int k = 0; k < T; ++k) {                                       // (bounded by the line's cells)
        run = k == kw ? side_f : run;
        const int old = v[k];
        run = front_step(run, old);
        diff |= run ^ old;
        v[k] = run;
    }
    run = bottom;
#pragma unroll
    for (int k = T - 1; k >= 0; --k) {                                  // (bounded by the line's cells)
        run = k == kw - 1 ? side_b : run;
        const int old = v[k];
        run = front_step(run, old);
        diff |= run ^ old;
        v[k] = run;
    }
#pragma unroll
    for (int k = 0; k < T; ++k) s[(k + 1) * ST + ((lane + DC * k) & (T - 1)) + 1] = v[k];
    return diff != 0;
}

__global__ __launch_bounds__(64) void k_front_round(FrontArgs a)
{
    __shared__ int s_lab[(kNavTile + 2) * kFrontStride];                // [row + 1][column + 1] with the halo
    __shared__ int s_old[kNavTile * kNavTile];                          // the labels as they were loaded
    const int lane = (int)threadIdx.x;
    TileRound t;
    if (!tile_round_enter(a.act, a.round, a.ntx, a.nty, &a.words[kFrontRounds], t)) return;   // (uniform)
    TileNoExtra none;
    if (!tile_load<kFrontStride, true>(a.label, a.sx, a.sy, t, kFrontNone, s_lab, s_old, none)) return;   // (uniform) no frontier cell here
    __syncthreads();

    // ---- relax to the tile's fixed point
    bool any_change = false;
    for (int it = 0; it < kNavTile * kNavTile; ++it) {                  // (bounded by the tile's cell count)
        bool ch = false;
        int* row = s_lab + (lane + 1) * kFrontStride;                   // row `lane`: cells row[1 .. 64], halo row[0] and row[65]
        ch |= front_line<1>(row + 1, row[0], row[kNavTile + 1]);
        __syncthreads();
        int* col = s_lab + lane + 1;                                    // column `lane`: cells col[(1 .. 64) * stride]
        ch |= front_line<kFrontStride>(col + kFrontStride, col[0], col[(kNavTile + 1) * kFrontStride]);
        __syncthreads();
        ch |= front_diagonal<1>(s_lab, lane);
        __syncthreads();
        ch |= front_diagonal<-1>(s_lab, lane);
        __syncthreads();
        if (!__any(ch)) break;
        any_change = true;
    }
    if (!any_change) return;                                            // (uniform)

    tile_store_and_mark<kFrontStride, true>(a.label, a.sx, a.sy, a.ntx, a.nty, t, s_lab, s_old);
}

__global__ __launch_bounds__(64) void k_front_check(FrontArgs a)
{
    const bool any = tiles_still_marked(a.act, a.round, a.ntx * a.nty); // in the map the next round would read
    const int rounds = tile_load_word(a.words + kFrontRounds);
    if (threadIdx.x == 0) { a.pin->rounds = rounds; a.pin->converged = any ? 0 : 1; }
}

// ---- the reduction ---------------------------------------------------------------------------------------------------------------------
// the roots, compacted in ascending cell order; the scatter writes the root's list index at the root's cell and resets its record
struct FrontRootSrc : CompactSrc {
    const int* label;
    int* index;
    FrontRec rec;
    uint32_t cells, cap;
    struct Item { int l; };
    __device__ size_t size() const { return cells; }
    __device__ Item load(size_t i) const { return {label[i]}; }
    __device__ int cls(size_t i, Item v) const { return v.l == (int)i ? 0 : -1; }
    __device__ bool emit(int, size_t i, Item, size_t o) const
    {
        if (o >= cap) return false;                                     // (never: front_max_records)
        index[i] = (int)o;
        rec.root[o] = (int)i; rec.size[o] = 0; rec.sum_x[o] = 0ull; rec.sum_y[o] = 0ull; rec.key[o] = kFrontNoKey;
        return false;
    }
};

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ unsigned long long wave_min64(unsigned long long v)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_front_accumulate(FrontArgs a, const uint32_t* n_roots_p)
{
    const uint32_t cells = (uint32_t)a.sx * (uint32_t)a.sy;
    const uint32_t n_roots = (uint32_t)tile_load_word(reinterpret_cast<const int*>(n_roots_p));
    for (uint32_t base = blockIdx.x * 256u; base < cells; base += gridDim.x * 256u) {   // (workgroup-uniform; bounded by the cell count)
        const uint32_t i = base + threadIdx.x;
        const int l = i < cells ? a.label[i] : kFrontNone;
        bool fr = l != kFrontNone;
        if (i < cells && !fr) a.label[i] = -1;                          // the label grid a read returns: -1 for a cell that is no frontier cell
        const uint64_t m = __ballot(fr);
        if (m == 0ull) continue;                                        // (wave-uniform)
        uint32_t r = 0u;
        unsigned long long key = kFrontNoKey, x = 0ull, y = 0ull;
        if (fr) {
            r = (uint32_t)a.index[l];                                   // l is a root's cell at the fixed point
            const int cy = (int)(i / (uint32_t)a.sx), cx = (int)(i - (uint32_t)cy * (uint32_t)a.sx);
            key = front_access_key(a, cx, cy);
            x = (unsigned long long)cx; y = (unsigned long long)cy;
            fr = r < n_roots;                                           // (always: a guard for the stores below)
        }
        const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)r, __ffsll((unsigned long long)m) - 1);
        if (__all(!fr || r == first)) {                                 // (wave-uniform) one root: combine in registers, one lane's atomics
            const uint64_t mm = __ballot(fr);
            const unsigned long long sx = wave_sum64(fr ? x : 0ull), sy = wave_sum64(fr ? y : 0ull), kk = wave_min64(fr ? key : kFrontNoKey);
            if (lane_id() == 0 && mm != 0ull) {
                atomicAdd(&a.rec.size[first], (int)__popcll(mm));
                atomicAdd(&a.rec.sum_x[first], sx);
                atomicAdd(&a.rec.sum_y[first], sy);
                atomicMin(&a.rec.key[first], kk);
            }
        } else if (fr) {
            atomicAdd(&a.rec.size[r], 1);
            atomicAdd(&a.rec.sum_x[r], x);
            atomicAdd(&a.rec.sum_y[r], y);
            atomicMin(&a.rec.key[r], key);
        }
    }
}

// record r as the header's struct, its cost included; whether it is kept
__device__ __forceinline__ gem_frontier front_record(const FrontArgs& a, int r, bool& kept)
{
    gem_frontier f;
    const unsigned long long key = a.rec.key[r];
    f.root = a.rec.root[r]; f.size = a.rec.size[r];
    f.sum_x = (long long)a.rec.sum_x[r]; f.sum_y = (long long)a.rec.sum_y[r];
    f.access_potential = (int)(key >> 32); f.access_cell = (int)(key & 0xffffffffull);
    const double gain = (double)f.size * a.resolution;
    const double travel = a.params.potential_scale * (double)f.access_potential;
    const double gained = a.params.gain_scale * gain;
    f.cost = travel - gained;                                           // (four operations, each rounded on its own: -ffp-contract=off)
    kept = gain >= a.params.min_frontier_size;
    return f;
}

struct FrontBest { double cost; int root, idx, rec; };                 // root < 0: none
__device__ __forceinline__ FrontBest front_better(FrontBest p, FrontBest q)
{
    const bool take = q.root >= 0 && (p.root < 0 || q.cost < p.cost || (q.cost == p.cost && q.root < p.root));
    FrontBest r;                                                        // (field by field: a select of two structs goes through a stack)
    r.cost = take ? q.cost : p.cost; r.root = take ? q.root : p.root; r.idx = take ? q.idx : p.idx; r.rec = take ? q.rec : p.rec;
    return r;
}

__global__ __launch_bounds__(kFrontPickThreads) void k_front_pick(FrontArgs a, const uint32_t* n_roots_p, uint32_t cap)
{
    constexpr int NT = kFrontPickThreads, NW = NT / 64;
    __shared__ uint32_t s_scan[16];
    __shared__ double s_cost[NW];
    __shared__ int s_root[NW], s_idx[NW], s_rec[NW];
    const uint32_t n_all = (uint32_t)tile_load_word(reinterpret_cast<const int*>(n_roots_p));
    const int n = (int)(n_all < cap ? n_all : cap);
    uint32_t carry = 0;
    FrontBest best{0.0, -1, -1, -1};
    for (int r0 = 0; r0 < n; r0 += NT) {                                // (workgroup-uniform; bounded by the record count)
        const int r = r0 + (int)threadIdx.x;
        bool kept;
        const gem_frontier f = front_record(a, r < n ? r : n - 1, kept);   // (past the end: the last record again, dropped)
        kept = kept && r < n;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<NT>(kept ? 1u : 0u, s_scan, &tot);
        if (kept) {
            const int o = (int)(carry + ex);
            a.out[o] = f;
            best = front_better(best, FrontBest{f.cost, f.root, o, r}); // a thread's records come in ascending root order
        }
        carry += tot;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        FrontBest o;
        o.cost = __shfl_xor(best.cost, off, 64); o.root = __shfl_xor(best.root, off, 64);
        o.idx = __shfl_xor(best.idx, off, 64); o.rec = __shfl_xor(best.rec, off, 64);
        best = front_better(best, o);
    }
    const int w = (int)(threadIdx.x >> 6);
    if (lane_id() == 0) { s_cost[w] = best.cost; s_root[w] = best.root; s_idx[w] = best.idx; s_rec[w] = best.rec; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < NW; ++i) best = front_better(best, FrontBest{s_cost[i], s_root[i], s_idx[i], s_rec[i]});   // (bounded by the waves)
        gem_frontier_status* st = &a.pin->status;                       // (field by field: no copy of the struct on a stack)
        st->n_cells = tile_load_word(a.words + kFrontCells);
        st->n_frontiers = n;
        st->n_kept = (int)carry;
        st->best = best.idx;
        st->rounds = tile_load_word(a.words + kFrontRounds);
        st->chunks = 0;
        bool kept;
        const gem_frontier f = front_record(a, best.root >= 0 ? best.rec : 0, kept);      // (record 0 of the arena: readable, not used)
        const bool have = best.root >= 0;
        st->best_frontier.root = have ? f.root : -1;
        st->best_frontier.size = have ? f.size : 0;
        st->best_frontier.sum_x = have ? f.sum_x : 0ll;
        st->best_frontier.sum_y = have ? f.sum_y : 0ll;
        st->best_frontier.access_potential = have ? f.access_potential : 0;
        st->best_frontier.access_cell = have ? f.access_cell : 0;
        st->best_frontier.cost = have ? f.cost : 0.0;
    }
}

hipError_t launch_front_classify(hipStream_t st, const FrontArgs& a)
{
    const uint32_t cells = (uint32_t)a.sx * (uint32_t)a.sy;
    const uint32_t blocks = std::max<uint32_t>(std::min<uint32_t>((cells + 255u) / 256u, 4096u), 1u);
    hipLaunchKernelGGL(k_front_classify, dim3(blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_front_round(hipStream_t st, const FrontArgs& a)
{
    hipLaunchKernelGGL(k_front_round, dim3((unsigned)(a.ntx * a.nty)), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_front_check(hipStream_t st, const FrontArgs& a)
{
    hipLaunchKernelGGL(k_front_check, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_front_reduce(hipStream_t st, const FrontArgs& a, uint32_t* block_cnt)
{
    const long long cells = (long long)a.sx * a.sy;
    const uint32_t cap = (uint32_t)front_max_records(a.sx, a.sy);
    uint32_t* total = block_cnt + compact_blocks(cells);
    FrontRootSrc src;
    src.label = a.label; src.index = a.index; src.rec = a.rec; src.cells = (uint32_t)cells; src.cap = cap;
    hipError_t e = compact(st, src, cells, block_cnt, total);
    if (e != hipSuccess) return e;
    const uint32_t blocks = std::max<uint32_t>(std::min<uint32_t>(((uint32_t)cells + 255u) / 256u, 4096u), 1u);
    hipLaunchKernelGGL(k_front_accumulate, dim3(blocks), dim3(256), 0, st, a, (const uint32_t*)total);
    hipLaunchKernelGGL(k_front_pick, dim3(1), dim3(kFrontPickThreads), 0, st, a, (const uint32_t*)total, cap);
    return hipGetLastError();
}

} // namespace gem
