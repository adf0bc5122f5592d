// gem_frame_lean.hpp -- the argument block of k_frame's lean form, its host fill and the block -> tile map (internal header).
//
// The generic k_frame takes FuseArgs + BinArgs by value: 936 bytes of kernel arguments, of which the lean form (bucket records,
// fast laser projection, no colours, one sweep) reads about a third, scattered over fifteen 64-byte lines -- the compiler fetched
// them in dependent hops, each a scalar-cache round trip a wave waits out before its first vector load.  FrameLeanArgs holds
// exactly what the lean kernel reads, once each: the tile half first (with the words both halves branch on at its head), the
// binning half behind it, each one contiguous run.  launch_frame_lean fills it from the FuseArgs / BinArgs it is handed
// (frame_lean_args, a pure function), so nothing upstream of the launch knows about it; the words a wave needs before its first
// vector load are passed once more in front of it, as scalar parameters the hardware preloads (FrameLeanHead, below).
// Everything here compiles for the host alone (tests/cpp/frame_lean_check.cpp).
#pragma once

#include "gem_kernels.hpp"

namespace gem {

constexpr int kFrameRunBits = 3;                    // runs of 2^kFrameRunBits neighbouring tiles per XCD (runs of 2 / 4 / 8: FETCH_SIZE 4.9 / 4.35 / 4.03 MB per C2 frame, 8.56 / 8.41 / 8.40 us per step)
constexpr int kFrameGridUnit = 8 << kFrameRunBits;  // ... the tile blocks come in multiples of this

// The tile half: the field names are FuseArgs' (frame_tile is one template over either).
struct FrameLeanTile {
    int       nf;                      // tile blocks of the launch: T rounded up to kFrameGridUnit (the binning blocks follow)
    int       T, tiles_per_row;
    uint32_t  tile_div;                // frame_div_mul(tiles_per_row): rank / tiles_per_row as a multiply-high
    unsigned long long* dbg;           // optional: [T][16] cycle stamps
    const uint32_t* bkt; uint32_t* bcount;
    float *elevation, *variance, *lowest;
    uint4*    spill; uint32_t* ctl; uint32_t* form_seen;         // slow path only
    int   L, center_tr, center_tc, row0, row1, start0, start1;
    int   n_pending; float pending[kMaxPending];
    int   dense; float mahal, var_floor;
    uint32_t nspill;                   // B_total * U: spill slots the slow path scans
};

// The binning half: BinArgs' names for the buffers, FrameConst's for what project_bin_laser_fast and
// height_variance<kModelLaserFast> read of the frame (they are templates over either).
struct FrameLeanBin {
    const float4* xyzi;
    int       B; uint32_t n;           // units, points (a single sweep: at most 2^22)
    int       keep_sentinel, tile_bits, tiles_per_row;
    int       filter_on;
    uint32_t* bkt; uint32_t* bcount; uint4* spill; uint32_t* ctl;
    unsigned long long* dbg;           // optional: [blocks][16] cycle stamps
    float  T[12];
    float  lower_f, upper_f;
    float  fbx, fby, fband, fplane;
    float  cx, cy; int sx, sy, L; float res;
    int    row0, row1;
    float  beam_a, beam_c, t2;
    float  Js[2];
};

struct FrameLeanArgs { FrameLeanTile t; FrameLeanBin b; };
// 320 bytes were the aim.  The two halves work on different pass buffer sets (the fuse half on the previous pass's, the binning on
// this pass's), so bkt / bcount / spill / ctl are there twice: eight words.  tiles_per_row, L, row0 / row1 and the dbg pointer are in
// both halves too (six words): each half stays one contiguous run under the names FuseArgs / BinArgs / FrameConst give them, and
// frame_lean_args stays a copy -- the binning's come from the frame being binned, the tile's from the pass being fused.
static_assert(sizeof(FrameLeanArgs) <= 352, "the lean form's kernel arguments: six 64-byte lines at most");

// n / d for 0 <= n < 2^18 and 1 <= d <= 2^12 as the high word of 2 n * m, m = floor(2^31 / d) + 1: the error term n (m d - 2^31) / (2^31 d)
// stays below 1 / d while n d < 2^31.  (2^31 and not 2^32: the multiplier of d = 1 has to fit a word.)
__host__ __device__ inline uint32_t frame_div_mul(int d) { return (uint32_t)((1ull << 31) / (unsigned long long)d) + 1u; }
__host__ __device__ inline int frame_div_by(int n, uint32_t m) { return (int)(((unsigned long long)((uint32_t)n << 1) * m) >> 32); }

__host__ __device__ inline int frame_rank_div(const FuseArgs& a, int rnk) { return rnk / a.tiles_per_row; }
__host__ __device__ inline int frame_rank_div(const FrameLeanTile& a, int rnk) { return frame_div_by(rnk, a.tile_div); }
__host__ __device__ inline uint32_t frame_spill_slots(const FuseArgs& a) { return (uint32_t)a.B_total * (uint32_t)a.U; }
__host__ __device__ inline uint32_t frame_spill_slots(const FrameLeanTile& a) { return a.nspill; }

// block -> tile: centre-first in dispatch order (the heaviest tiles of a robot-centric map start first), and XCD-AWARE --
// workgroup b runs on XCD b % 8, each XCD has its own L2, and four tiles that follow each other in a tile row share their
// 128-byte lines of the layers: runs of 2^kFrameRunBits consecutive ranks go to ONE XCD (with plain rank = block the neighbours
// sat on eight different XCDs and every shared line was fetched twice: FETCH_SIZE 5.6 MB per frame instead of 3.6,
// profiles/r05_c2_bench.txt).  Rows c, c-1, c+1, ...; columns in runs of neighbours on alternating sides: 0 1 2 3 | -1 -2 -3 -4 | 4 5 6 7 | ...
template <class A>
__host__ __device__ inline bool frame_tile_of(const A& a, int block, int& tr, int& tc)
{
    const int tpr = a.tiles_per_row;
    const int x = block & 7, i = block >> 3;
    const int rnk = ((((i >> kFrameRunBits) << 3) + x) << kFrameRunBits) + (i & ((1 << kFrameRunBits) - 1));
    if (rnk >= a.T) return false;
    const int bi = frame_rank_div(a, rnk), bj = rnk - bi * tpr;
    const int oi = (bi & 1) ? -((bi + 1) >> 1) : (bi >> 1);
    const int cj = bj >> kFrameRunBits, t = bj & ((1 << kFrameRunBits) - 1);
    const int oj = (cj & 1) ? -(((cj - 1) >> 1) << kFrameRunBits) - 1 - t : ((cj >> 1) << kFrameRunBits) + t;
    tr = a.center_tr + oi; tr = tr < 0 ? tr + tpr : (tr >= tpr ? tr - tpr : tr);
    tc = a.center_tc + oj; tc = tc < 0 ? tc + tpr : (tc >= tpr ? tc - tpr : tc);
    return true;
}

__host__ __device__ inline int frame_tile_blocks(int T) { return (T + kFrameGridUnit - 1) & ~(kFrameGridUnit - 1); }

// the lean kernel's arguments from the generic ones (launch_frame): copies, the block count, the multiplier and the slot count
inline FrameLeanArgs frame_lean_args(const FuseArgs& fa, const BinArgs& ba)
{
    FrameLeanArgs la{};
    FrameLeanTile& t = la.t;
    t.nf = frame_tile_blocks(fa.T); t.T = fa.T; t.tiles_per_row = fa.tiles_per_row;
    t.tile_div = frame_div_mul(fa.tiles_per_row > 0 ? fa.tiles_per_row : 1);
    t.dbg = fa.dbg; t.bkt = fa.bkt; t.bcount = fa.bcount;
    t.elevation = fa.elevation; t.variance = fa.variance; t.lowest = fa.lowest;
    t.spill = fa.spill; t.ctl = fa.ctl; t.form_seen = fa.form_seen;
    t.L = fa.L; t.center_tr = fa.center_tr; t.center_tc = fa.center_tc; t.row0 = fa.row0; t.row1 = fa.row1;
    t.start0 = fa.start0; t.start1 = fa.start1;
    t.n_pending = fa.n_pending;
    for (int i = 0; i < kMaxPending; ++i) t.pending[i] = fa.pending[i];
    t.dense = fa.dense; t.mahal = fa.mahal; t.var_floor = fa.var_floor;
    t.nspill = (uint32_t)fa.B_total * (uint32_t)fa.U;
    FrameLeanBin& b = la.b;
    const FrameConst& fc = ba.frame0;
    b.xyzi = ba.xyzi; b.B = ba.B; b.n = (uint32_t)ba.n;
    b.keep_sentinel = ba.keep_sentinel; b.tile_bits = ba.tile_bits; b.tiles_per_row = ba.tiles_per_row;
    b.filter_on = fc.filter_on;
    b.bkt = ba.bkt; b.bcount = ba.bcount; b.spill = ba.spill; b.ctl = ba.ctl; b.dbg = ba.dbg;
    for (int i = 0; i < 12; ++i) b.T[i] = fc.T[i];
    b.lower_f = fc.lower_f; b.upper_f = fc.upper_f;
    b.fbx = fc.fbx; b.fby = fc.fby; b.fband = fc.fband; b.fplane = fc.fplane;
    b.cx = fc.cx; b.cy = fc.cy; b.sx = fc.sx; b.sy = fc.sy; b.L = fc.L; b.res = fc.res;
    b.row0 = fc.row0; b.row1 = fc.row1;
    b.beam_a = fc.beam_a; b.beam_c = fc.beam_c; b.t2 = fc.t2;
    b.Js[0] = fc.Js[0]; b.Js[1] = fc.Js[1];
    return la;
}

// The HEAD of a lean launch: the words a wave needs before its first vector loads can leave -- the tile / binning branch, the
// block -> tile map, the bucket and its count for a tile block; the cloud and its size for a binning block.  The lean kernels take
// them as leading scalar parameters IN THIS ORDER, in front of the block (gem_frame_lean.hip), and that file is built with
// kernel-argument preloading: the command processor writes the first kFrameHeadDwords dwords of the kernel arguments into user SGPRs
// where a wave starts, so none of them is a scalar load the wave waits for.  The hardware preloads 14 dwords at most (16 user SGPRs,
// two of them the kernel-argument pointer).  The kernels read these words from the parameters and never from the block.
struct FrameLeanHead {
    int       nf, T, tiles_per_row;
    uint32_t  tile_div;
    int       center_tr, center_tc;
    const uint32_t* bkt; uint32_t* bcount;             // the tile half's (the pass being fused)
    const float4* xyzi; int B; uint32_t n;             // the binning half's
};
constexpr int kFrameHeadDwords = (int)(sizeof(FrameLeanHead) / 4);
static_assert(sizeof(FrameLeanHead) == 56 && kFrameHeadDwords <= 14, "the head of a lean launch: no padding, at most the 14 dwords the hardware preloads");

// the head of a filled block (launch_frame_lean): copies
inline FrameLeanHead frame_lean_head(const FrameLeanArgs& la)
{
    FrameLeanHead h{};
    h.nf = la.t.nf; h.T = la.t.T; h.tiles_per_row = la.t.tiles_per_row; h.tile_div = la.t.tile_div;
    h.center_tr = la.t.center_tr; h.center_tc = la.t.center_tc;
    h.bkt = la.t.bkt; h.bcount = la.t.bcount;
    h.xyzi = la.b.xyzi; h.B = la.b.B; h.n = la.b.n;
    return h;
}

} // namespace gem
