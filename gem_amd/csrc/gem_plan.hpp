// gem_plan.hpp -- the pass plan: which pipeline a pass over points on the device takes, and how large every buffer of that pipeline is
// and where its sub-tables sit.  Plain values from pure functions (no handle, no HIP call, no heap): run_pipeline / run_sort_pipeline
// size and bind their buffers from a plan, gem_reserve plans the extremal passes inside its bounds and allocates through the same
// ensure_* functions (gem_capi_pipeline.cpp), and tests/cpp/plan_cover.cpp checks on the CPU that the second covers the first.
#pragma once

#include "gem_kernels.hpp"
#include <algorithm>

namespace gem {

constexpr int       kUnit = 64;                      // points per unit (one wave of k_bin_wave)
constexpr long long kSweepPoints = 2048ll * kUnit;   // a single cloud longer than this is processed as a batch of sweeps of this size
inline int ceil_log2(int v) { int b = 0; while ((1 << b) < v) ++b; return b; }
// k arrays of n 32-bit words in a staging buffer, each 256-byte aligned behind the one before, and a few words behind the last
inline size_t stage_words_bytes(long long n, int k) { return ((size_t)n * 4 + 256) * k; }
// A depth image of the add entries in the staging arena (gem_add_depth*): the depth rows | the colour rows, as the caller has them
// (host images only; at the stride upload_arrays gives a half of the staging buffer) | the XYZI slot the unprojection writes | its
// rgb, each 256-byte aligned.  gem_reserve plans the largest image with tight rows: four-byte depths and a colour image.
struct DepthPlan { size_t o_color, o_xyzi, o_rgb, bytes; };
inline DepthPlan depth_plan(long long n, size_t depth_bytes, size_t color_bytes)
{
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    DepthPlan p{};
    p.o_color = pad(depth_bytes);
    p.o_xyzi = p.o_color + pad(color_bytes);
    p.o_rgb = p.o_xyzi + pad((size_t)n * 16);
    p.bytes = p.o_rgb + pad((size_t)n * 4);
    return p;
}
inline size_t depth_stage_bytes(long long max_points) { return depth_plan(max_points, (size_t)max_points * 4, (size_t)max_points * 3).bytes; }
// What the choice and the sizes depend on, copied from the handle in one place (plan_env)
struct PlanEnv { int L, ts, sort_form, sort_passes, sort_chunk, sort_ring; bool sort_path, track_lowest; long long sort_min_points, sort_min_points_batch; };

// The key geometry of the sorted pipelines for this map, and whether a pass of `n_sweeps` sweeps fits the 32-bit record key.
// block_form: the digits cover the BLOCK id (id >> 8) only and k_fuse_block orders a block's records by cell itself; otherwise
// they cover the whole id and k_fuse_walk streams every cell's run (gem_kernels.hpp).
struct SortGeometry { int tiles_per_row, T, id_bits, n_passes, dshift[3], dbits[3], dbins[3]; bool block_form, ok; };
using BinsFit = bool (*)(int bins);                  // do the sort kernels of a pass with that many bins fit the LDS (gem_capi_pipeline.cpp asks sort_shape)

inline SortGeometry sort_digits(int L, int forced_passes, int n_sweeps, bool block_form, BinsFit fits)
{
    SortGeometry g{};
    g.block_form = block_form;
    g.tiles_per_row = (L + 31) / 32;
    g.T = g.tiles_per_row * g.tiles_per_row;
    g.id_bits = 10 + std::max(1, ceil_log2(g.T));                 // id = tile << 10 | cell in tile
    const int lo = block_form ? 8 : 0;                            // first bit the digits cover
    const long long values = (((long long)g.T) << 10) >> lo;      // ids / block ids in use: 0 .. values - 1
    // Digits of about equal width, at most ten bits: the records of a (chunk, bin) leave k_sort_scatter as one run, and with
    // thousands of bins a 4096-record chunk has one or two records per run -- no coalescing left (cell-sorted, the 2400^2 map in
    // two passes of 2048 / 2813 bins: 206 + 158 us; in three passes of 256 / 256 / 88 bins: see DESIGN.md).  Block ids are
    // different: consecutive points of a scan fall into few blocks, the runs are long whatever the number of bins, and a map of
    // up to kOnePassMaxBins blocks (600^2: 1444) is sorted by ONE pass.
    if (forced_passes) g.n_passes = forced_passes;
    else if (block_form) g.n_passes = values <= kOnePassMaxBins ? 1 : (g.id_bits - lo <= 20 ? 2 : 3);
    else g.n_passes = g.id_bits <= 20 ? 2 : 3;
    int shift = lo;
    for (int i = 0; i < g.n_passes; ++i) {
        const int left = g.n_passes - i;
        // (rounded down: the lowest digit sees the records in input order -- every bin in use, a run per bin and chunk -- and pays
        //  for its bins; the higher digits see them sorted by the lower ones, longer runs.  Cell-sorted 600^2: 512 x 722 bins
        //  28.7 + 26.4 us, 1024 x 361 37.7 + 21.4, 256 x 1444 27.6 + 38.8)
        int bits = (g.id_bits - shift) / left;
        if (i == 0 && !block_form) bits = std::max(bits, 8);      // the 256 cells of a k_fuse_walk workgroup never straddle a bin of the last pass
        if (i == g.n_passes - 1) bits = g.id_bits - shift;
        bits = std::max(bits, 1);
        g.dshift[i] = shift; g.dbits[i] = bits;
        g.dbins[i] = i == g.n_passes - 1 ? (int)(((((long long)g.T) << 10) - 1) >> shift) + 1 : 1 << bits;
        shift += bits;
    }
    const long long max_sweeps = std::min<long long>(512, (1ll << (32 - g.id_bits)) - 1);     // the sweep field is never all ones
    g.ok = g.id_bits <= 26 && n_sweeps <= max_sweeps && g.dshift[g.n_passes - 1] >= 8 && shift == g.id_bits;
    for (int i = 0; i < g.n_passes; ++i)
        g.ok = g.ok && g.dbins[i] <= kSortMaxBins && g.dbits[i] >= 1 && fits(g.dbins[i]);     // (a forced pass count may not fit)
    return g;
}
// Big passes (batches of sweeps, aggregated clouds, depth images) go through the sorted pipeline: a global two-digit counting
// sort of the in-map points by (tile, cell), then one walk per cell (gem_sort.hip).  Small ones -- a single LiDAR sweep -- keep
// the tile pipeline, whose one or two launches cost less than the sort's seven.
// Measured crossover (tools/dbg/crossover.py): batches of LiDAR sweeps -- a few points per cell and sweep -- are faster on the tile
// pipeline up to about 8 sweeps (1 M points); a single dense cloud (a depth image: hundreds of points per cell) from ~150 k points.
// shard: the sort of a sharded step's share -- always sorted, by block (a strip's records are one contiguous range, a block's too).
struct PassChoice { bool fell_back; SortGeometry geo; };      // geo.ok: sorted
inline PassChoice choose_pass(const PlanEnv& e, long long n, int n_sweeps, BinsFit fits, bool shard = false)
{
    PassChoice c{};
    if (!shard && (!e.sort_path || n < (n_sweeps > 1 ? e.sort_min_points_batch : e.sort_min_points) || n >= (1ll << 31))) return c;
    // Batches of sweeps -- a few records per cell and sweep, every batch of a block's records spread over its cells -- take the
    // block-sorted form (one counting-sort pass for the 600^2 map instead of two, no per-cell order in HBM at all); a single
    // dense cloud (a depth image: a quarter of its points in one block, hundreds per cell, image row by image row) needs the
    // whole chip to order it by cell: the cell-sorted form.
    // (Maps of more than kOnePassMaxBins blocks take two passes over the block id and k_block_prefix; with k_fuse_block's rounds
    //  of 512 records for light blocks that is still the shorter way -- C5, 2400^2, same box: 351-365 us cell-sorted in three
    //  passes, 333-340 block-sorted in two.)
    const bool block_form = shard || e.sort_form == 2 || (e.sort_form == 0 && n_sweeps > 1);
    c.geo = sort_digits(e.L, e.sort_passes, n_sweeps, block_form, fits);
    c.fell_back = !c.geo.ok;                        // (a forced form / pass count that does not fit this map: the other form)
    if (c.fell_back) c.geo = sort_digits(e.L, e.sort_passes, n_sweeps, !block_form, fits);
    return c;
}
// A batched pass's device tables, ONE layout for both pipelines: frames | first unit / chunk per sweep | first point per sweep |
// orig0 | variance increments.  total 0: a single sweep, no tables.
struct TablesPlan { size_t o_frames, o_first0, o_first, o_orig, o_var, total; };
inline TablesPlan tables_plan(int n_sweeps)
{
    TablesPlan t{};
    if (n_sweeps <= 1) return t;
    const size_t S = (size_t)n_sweeps;
    t.o_first0 = sizeof(FrameConst) * S;
    t.o_first = (t.o_first0 + sizeof(int) * (S + 1) + 15) & ~(size_t)15;
    t.o_orig = t.o_first + sizeof(long long) * (S + 1);
    t.o_var = t.o_orig + sizeof(int) * S;
    t.total = t.o_var + sizeof(float) * S;
    return t;
}
// The sorted pipeline's buffers in bytes (hv and key: each of the two arrays; src 0 without colours; blkcnt / ranges / shard 0 when
// the pass has no use for them) and the carving of s_misc: segment sums [pass][4][bins] | record count, odd-flag word | bin bases of
// the last pass [bins + 1] | seg_cnt
struct SortPlan {
    size_t hv, key, src, cnt1, cnt2, misc, blkcnt, ranges, shard, blocks;      // (blocks: what blkcnt and ranges have a word / a pair for)
    size_t o_seg[3], o_total, o_base, o_segcnt;
    TablesPlan tables;
};
// n records in nc1 chunks of the first pass (every sweep's rounded up) and nc2 of the later ones; blocks: 4 T when the walk will want
// every block's range (the last pass's bins are not the blocks, or a shard), else 0
inline SortPlan sort_plan(int n_passes, const int dbins[3], long long n, size_t nc1, size_t nc2, int n_sweeps, bool with_src, size_t blocks, bool shard = false)
{
    SortPlan p{};
    const size_t N = (size_t)n;
    p.hv = N * 8 + 64; p.key = N * 4 + 64;          // (+64 bytes: k_fuse_walk fetches whole groups of four records; a cell's last group may reach past the last record)
    p.src = with_src ? N * 4 + 64 : 0;
    int bins_hi = 1;                                // the later passes share one count table
    for (int i = 1; i < n_passes; ++i) bins_hi = std::max(bins_hi, dbins[i]);
    p.cnt1 = nc1 * dbins[0] * 4; p.cnt2 = nc2 * bins_hi * 4 + 16;
    size_t o = 0;
    for (int i = 0; i < n_passes; ++i) { p.o_seg[i] = o; o += (size_t)dbins[i] * 16; }
    p.o_total = o; p.o_base = (o + 8 + 15) & ~(size_t)15;
    p.o_segcnt = (p.o_base + ((size_t)dbins[n_passes - 1] + 1) * 4 + 15) & ~(size_t)15;
    p.misc = p.o_segcnt + nc1 * kSortSegsPerChunk * 4;
    p.blocks = blocks; p.blkcnt = blocks * sizeof(uint32_t); p.ranges = blocks * sizeof(uint2);
    p.shard = shard ? 64 * sizeof(uint32_t) : 0;    // strip ids [16] | strip bounds [16]
    p.tables = tables_plan(n_sweeps);
    return p;
}
inline size_t walk_blocks(const SortGeometry& g, bool shard) { return ((g.block_form && g.n_passes > 1) || shard) ? (size_t)4 * g.T : 0; }
// The sweeps of a pass as the tile pipeline sees them.  A big single cloud becomes a batch of sweeps with one frame: every tile then
// only reads the descriptor rows of the sweeps that reach it (flag[tile][sweep]) instead of one row over all units.
inline int cut_sweeps(long long n, int n_sweeps) { return n_sweeps == 1 && n > kSweepPoints ? (int)((n + kSweepPoints - 1) / kSweepPoints) : n_sweeps; }
// points of sweep s: by the batch's offsets, or (offsets == nullptr) of a single cloud cut every kSweepPoints
inline long long sweep_points(long long n, const long long* offsets, int s)
{
    return offsets ? offsets[s + 1] - offsets[s] : std::min<long long>(n, (s + 1) * kSweepPoints) - std::min<long long>(n, s * kSweepPoints);
}
inline long long sweep_units(long long points) { return ((points + kUnit - 1) / kUnit + 31) & ~31ll; }   // units of 64 points; descriptor rows are flagged in groups of 32 units (64 B)

// The tile pipeline's pass: n_sweeps after the cut, B units in all, bpad of the longest sweep, 1 << ts cells per tile side, and
// its buffers in bytes.  err: 1 = a sweep too large for the descriptor words, 2 = too large for the 16x16 tiles lowest tracking needs.
struct TilePlan {
    int err, n_sweeps, B, bpad, ts, tiles_per_row, T;
    size_t rec, srt, seg, flag, gflag;
    size_t bkt, bcnt, fctl, spill;                  // k_frame may take it (one sweep, 16x16 tiles), else 0
    TablesPlan tables;
};
// ts_auto: the tile shift where the handle leaves the choice to the pass (0: by the size of the descriptor table)
inline TilePlan tile_plan_units(const PlanEnv& e, int n_sweeps, long long B, long long bpad, int ts_auto)
{
    TilePlan p{};
    p.n_sweeps = n_sweeps; p.B = (int)B; p.bpad = (int)bpad;
    if (bpad > 0x3fffffff) { p.err = 1; return p; }
    // tile size of this pass: 16x16 cells (more, lighter workgroups: better balance and latency hiding)
    // unless the [sweep][tile][unit] descriptor table would get too big, then 32x32
    const long long tpr4 = (e.L + 15) / 16;
    const long long table4 = tpr4 * tpr4 * bpad * n_sweeps * (long long)sizeof(uint16_t);
    p.ts = e.ts ? e.ts : (ts_auto ? ts_auto : (table4 <= (1ll << 29) ? 4 : 5));
    // the kernel variants that maintain map_lowest exist for 16x16 tiles only: the choice is made HERE, before the tile
    // geometry (te, tiles_per_row, T, table sizes) is derived from it
    if (e.track_lowest) { if (table4 > (16ll << 30)) { p.err = 2; return p; } p.ts = 4; }
    p.tiles_per_row = (e.L + (1 << p.ts) - 1) >> p.ts;
    p.T = p.tiles_per_row * p.tiles_per_row;
    const size_t T = (size_t)p.T, S = (size_t)n_sweeps;
    p.rec = (size_t)B * kUnit * sizeof(uint4);
    p.srt = p.rec + 16;                             // sorted arena + its bump pointer (last 16 bytes)
    p.seg = S * T * bpad * sizeof(uint16_t);        // descriptor table [sweep][tile][unit in sweep]
    p.flag = T * S * sizeof(uint32_t);              // touched flags [tile][sweep]
    p.gflag = S * T * (bpad / 32) * sizeof(uint32_t);
    if (p.ts == 4 && n_sweeps == 1) {               // k_frame's records (gem_kernels.hpp, kFrameBucket), its two form words, a spill slot per point
        p.bkt = T * kFrameBucket * 3 * sizeof(uint32_t); p.bcnt = T * sizeof(uint32_t); p.fctl = 2 * sizeof(uint32_t);
        p.spill = p.rec;
    }
    p.tables = tables_plan(n_sweeps);
    return p;
}
// ... of n points in n_sweeps sweeps at `offsets` (nullptr: a single cloud)
inline TilePlan tile_plan(const PlanEnv& e, long long n, int n_sweeps, const long long* offsets, int ts_auto = 0)
{
    const int ns = cut_sweeps(n, n_sweeps);
    long long B = 0, bpad = 0;
    for (int s = 0; s < ns; ++s) { const long long u = sweep_units(sweep_points(n, offsets, s)); B += u; bpad = std::max(bpad, u); }
    return tile_plan_units(e, ns, B, bpad, ts_auto);
}
// ---- gem_reserve: the extremal passes inside its bounds, each planned for ANY split into its sweeps the header allows
struct BoundPlan { int kind; SortPlan sort; TilePlan tile; };      // kind: 0 = not reserved (no pipeline takes it / a table beyond 2 GB), 1 = sorted, 2 = tile
inline BoundPlan plan_bound(const PlanEnv& e, long long n, int sweeps, bool shard, bool with_colours, BinsFit fits)
{
    BoundPlan r{};
    const PassChoice c = choose_pass(e, n, sweeps, fits, shard);
    if (c.geo.ok) {
        const size_t chunk = (size_t)sort_chunk_for(n, e.sort_chunk), nc = ((size_t)n + chunk - 1) / chunk;
        r.kind = 1;
        r.sort = sort_plan(c.geo.n_passes, c.geo.dbins, n, nc + (size_t)(sweeps - 1), nc, sweeps, with_colours, walk_blocks(c.geo, shard), shard);    // (every sweep but the last may end inside a chunk)
        return r;
    }
    if (shard) return r;
    // Sized for 16x16 tiles where the pass would choose: a pass that goes to 32x32 needs a quarter of it.  The sweeps of a batch are
    // taken to be at most twice their mean length (or kSweepPoints) -- the table for "all points in one of 32 sweeps" would be 32
    // times the useful one -- and every sweep but one to end just inside a group of 32 units.
    // A batch of fewer sweeps has longer ones: bpad is what makes sweeps x bpad cover s x (units of the longest of s sweeps) for every s.
    long long most = 0;
    for (int s = 2; s <= sweeps; ++s) most = std::max(most, s * sweep_units(std::min(n, std::max(kSweepPoints, 2 * n / s))));
    if (sweeps == 1) r.tile = tile_plan(e, n, 1, nullptr, 4);
    else r.tile = tile_plan_units(e, sweeps, sweep_units(n) + 32ll * (sweeps - 1), ((most + sweeps - 1) / sweeps + 31) & ~31ll, 4);
    r.kind = (r.tile.err || r.tile.seg > ((size_t)1 << 31)) ? 0 : 2;     // (such a descriptor table is left to the pass that wants one)
    return r;
}
constexpr int kMaxBoundPlans = 8;
constexpr long long kSmallChunkPoints = 2ll * 256 * kSortChunkRecords - 1;     // the largest pass sort_chunk_for gives the small chunk
// max_points points in at most max_sweeps sweeps per call; shard_ranks > 0: the bounds are those of a sharded step over that many ranks
inline int bound_plans(const PlanEnv& e, long long max_points, int max_sweeps, int shard_ranks, bool with_colours, BinsFit fits, BoundPlan out[kMaxBoundPlans])
{
    int k = 0;
    const long long P = max_points;
    auto add = [&](long long n, int sweeps) { if (n > 0) out[k++] = plan_bound(e, n, sweeps, shard_ranks > 0, with_colours, fits); };
    if (shard_ranks > 0) {
        const long long share = (P + shard_ranks - 1) / shard_ranks + 1;
        add(share, max_sweeps);                                     // the sharded step's share: this rank sorts its W-th of the points
        add(std::min(share, kSmallChunkPoints), max_sweeps);        // ... while it still takes the small sort chunk: more chunks than the largest share has
        return k;
    }
    add(P, 1);                                                      // the largest single cloud
    add(std::min(P, e.sort_min_points - 1), 1);                     // ... below sort_min_points: the tile pipeline, cut into sweeps (with tables) beyond kSweepPoints
    add(std::min(P, kSweepPoints), 1);                              // the largest cloud that stays one sweep: k_frame's buckets and spill slots
    add(std::min(P, kSmallChunkPoints), 1);                         // the largest one that still takes the small sort chunk: more chunks than the largest has
    if (max_sweeps > 1) {
        add(P, max_sweeps);                                         // the largest batch
        add(std::min(P, e.sort_min_points_batch - 1), max_sweeps);  // ... below sort_min_points_batch: the tile pipeline, no sweep above twice the mean
        add(std::min(P, kSmallChunkPoints), max_sweeps);            // the largest batch that still takes the small sort chunk
    }
    return k;
}

} // namespace gem
