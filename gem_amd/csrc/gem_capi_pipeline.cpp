// gem_capi_pipeline.cpp -- one pass over points that are on the device (see gem_capi_internal.hpp): the tile pipeline (k_frame / k_bin_wave +
// k_fuse_list) and the two sorted forms (gem_sort.hip), their buffers, streams and hand-overs.
#include "gem_capi_internal.hpp"
#include "gem_clean.hpp"

namespace gemi {

static bool sort_bins_fit(int bins) { return sort_shape(bins, true, kSortChunkRecords).lds <= 160 * 1024; }   // what launch_sort checks (the big chunk needs the most)
PlanEnv plan_env(const gem_handle* h)
{
    PlanEnv e{};
    e.L = h->L; e.ts = h->ts; e.sort_form = h->sort_form; e.sort_passes = h->sort_passes; e.sort_chunk = h->sort_chunk; e.sort_ring = h->sort_ring;
    e.sort_path = h->sort_path; e.track_lowest = h->track_lowest; e.sort_min_points = h->sort_min_points; e.sort_min_points_batch = h->sort_min_points_batch;
    return e;
}
SortGeometry sort_geometry(const gem_handle* h, int n_sweeps, bool block_form) { return sort_digits(h->L, h->sort_passes, n_sweeps, block_form, sort_bins_fit); }

// ---- the plans' buffers (gem_plan.hpp) in a set of pass buffers: the pipelines below and gem_reserve allocate through these
// A batched pass's tables and their pinned staging copy (twice the size: the next, slightly longer batch does not allocate again);
// with `host`: the zeroed host block to fill, once the previous upload from it has been read.  Staged in pinned memory so that the upload
// does not make the host wait for the stream (a pageable source would: the call then cost a whole k_bin of host time, 240 us per C4 batch)
static int stage_batch_tables(gem_handle* h, gem_handle::PassBuffers& pb, const TablesPlan& t, unsigned char** host = nullptr)
{
    if (t.total > pb.tables.cap) pb.tab_key.clear();                 // (a new allocation holds nothing, even at the old address)
    const int rc = ensure(h, pb.tables, t.total);
    if (rc) return rc;
    if (t.total > pb.host_cap) {
        if (pb.tables_recorded) GEM_HIP(h, hipEventSynchronize(pb.tables_done));
        if (pb.host_tables) GEM_HIP(h, hipHostFree(pb.host_tables));
        pb.host_tables = nullptr; pb.host_cap = 0;
        GEM_HIP(h, hipHostMalloc(&pb.host_tables, t.total * 2, hipHostMallocDefault));
        pb.host_cap = t.total * 2;
    }
    if (!host || !t.total) return GEM_OK;
    if (!pb.tables_done) GEM_HIP(h, hipEventCreateWithFlags(&pb.tables_done, hipEventDisableTiming));
    if (pb.tables_recorded) GEM_HIP(h, hipEventSynchronize(pb.tables_done));
    pb.tab_key.clear();                                              // (not valid until the upload is enqueued)
    *host = static_cast<unsigned char*>(pb.host_tables);
    memset(*host, 0, t.total);
    return GEM_OK;
}
// ... filled: the frames, the first unit / chunk of every sweep, what the pass input has of the rest.  Returns the k_sort_project
// instantiation the frames take: clouds whose frames all use the laser model (the reference's only GPU model, GPU:403-408) take the one
// without the camera models' double-precision code: 2; with every frame's rotation variance zero (height_variance, kModelLaserFast): 4
static int fill_batch_tables(const gem_handle* h, unsigned char* host, const TablesPlan& t, const PassInput& in, const int* first0)
{
    bool laser = in.src == 0, fast = true;
    for (int s = 0; s < in.n_sweeps; ++s) {
        FrameConst& fc = reinterpret_cast<FrameConst*>(host + t.o_frames)[s];
        fill_frame(h, in.src == 0 ? &in.params[s] : nullptr, fc);
        laser = laser && in.params[s].sensor_model == GEM_MODEL_LASER;
        fast = fast && fc.fast_laser != 0;
    }
    memcpy(host + t.o_first0, first0, sizeof(int) * (in.n_sweeps + 1));
    memcpy(host + t.o_first, in.offsets, sizeof(long long) * (in.n_sweeps + 1));
    if (in.sweep_orig0) memcpy(host + t.o_orig, in.sweep_orig0, sizeof(int) * in.n_sweeps);
    if (in.var_updates) memcpy(host + t.o_var, in.var_updates, sizeof(float) * in.n_sweeps);
    return laser ? (fast ? 4 : 2) : 0;
}
static int ensure_sort_buffers(gem_handle* h, gem_handle::PassBuffers& pb, const SortPlan& p)
{
    int rc;
    if ((rc = ensure(h, pb.s_hv1, p.hv)) || (rc = ensure(h, pb.s_hv2, p.hv)) || (rc = ensure(h, pb.s_key1, p.key)) || (rc = ensure(h, pb.s_key2, p.key)) ||
        (rc = ensure(h, pb.s_src1, p.src)) || (rc = ensure(h, pb.s_src2, p.src)) ||
        (rc = ensure(h, pb.s_cnt1, p.cnt1)) || (rc = ensure(h, pb.s_cnt2, p.cnt2)) || (rc = ensure(h, pb.s_misc, p.misc)) ||
        (rc = ensure_zeroed(h, pb.s_blkcnt, p.blkcnt)) || (rc = ensure(h, pb.s_ranges, p.ranges)) || (rc = ensure(h, pb.s_shard, p.shard))) return rc;
    return stage_batch_tables(h, pb, p.tables);
}
void bind_sort_buffers(const SortPlan& p, int n_passes, const SortBuffers& b, SortArgs& sa)
{
    unsigned char* misc = static_cast<unsigned char*>(b.misc);
    for (int i = 0; i < n_passes; ++i) {
        sa.cnt[i] = static_cast<uint32_t*>(i == 0 ? b.cnt1 : b.cnt2);
        sa.segtot[i] = reinterpret_cast<uint32_t*>(misc + p.o_seg[i]);
    }
    sa.total = reinterpret_cast<uint32_t*>(misc + p.o_total); sa.bin_base = reinterpret_cast<uint32_t*>(misc + p.o_base);
    // (word 1 behind the record count: k_sort_project stores the pass's epoch there when a record is outside the plain range of
    //  the walks' chain loops; epochs never repeat, so the word needs no clearing)
    sa.odd_flag = sa.total + 1;
    sa.seg_cnt = reinterpret_cast<uint32_t*>(misc + p.o_segcnt);
    // arrays a: the projected records in input order, later the final order; arrays b: the order after pass 1
    sa.hv_a = static_cast<uint2*>(b.hv2); sa.hv_b = static_cast<uint2*>(b.hv1);
    sa.key_a = static_cast<uint32_t*>(b.key2); sa.key_b = static_cast<uint32_t*>(b.key1);
    sa.src_a = p.src ? static_cast<uint32_t*>(b.src2) : nullptr; sa.src_b = p.src ? static_cast<uint32_t*>(b.src1) : nullptr;
}
// The tile pipeline's buffers; what a pass expects cleared is cleared on `st` when it is (re)allocated.  frame: k_frame's arenas too
// (only a handle that runs it pays for them); host: the block of a batch's tables to fill (stage_batch_tables)
static int ensure_tile_buffers(gem_handle* h, gem_handle::PassBuffers& pb, const TilePlan& p, hipStream_t st, bool frame, unsigned char** host = nullptr)
{
    int rc;
    if ((rc = ensure(h, pb.rec, p.rec)) || (rc = ensure(h, pb.srt, p.srt))) return rc;
    if (p.seg > pb.seg.cap) {                                        // k_fuse_list zeroes the descriptors it consumes: all-zero between passes
        if ((rc = ensure(h, pb.seg, p.seg))) return rc;
        GEM_HIP(h, hipMemsetAsync(pb.seg.p, 0, pb.seg.cap, st));
    }
    if (p.flag > pb.flag.cap || p.gflag > pb.gflag.cap) {            // the touched flags are stamped with the pass's epoch instead of being cleared
        if ((rc = ensure(h, pb.flag, p.flag)) || (rc = ensure(h, pb.gflag, p.gflag))) return rc;
        GEM_HIP(h, hipMemsetAsync(pb.flag.p, 0, pb.flag.cap, st));
        GEM_HIP(h, hipMemsetAsync(pb.gflag.p, 0, pb.gflag.cap, st));
        pb.epoch = 0;
    }
    if (!frame) return stage_batch_tables(h, pb, p.tables, host);
    // k_frame's records (gem_kernels.hpp, kFrameBucket; sizes 0 where the plan rules it out): the kernel leaves every count zero and
    // every spill slot free behind it, so the arenas are set once, when they are (re)allocated -- on the handle's stream, k_frame's
    if ((rc = ensure(h, pb.bkt, p.bkt)) || (rc = ensure_zeroed(h, pb.bcnt, p.bcnt)) || (rc = ensure_zeroed(h, pb.fctl, p.fctl))) return rc;     // (the form words: bucket form until a tile needs more)
    if (!h->form_seen) {                                             // the word the slow path reports to the host in (gem_handle::form_seen): once per handle
        GEM_HIP(h, hipHostMalloc(reinterpret_cast<void**>(&h->form_seen), 64, hipHostMallocDefault));
        *h->form_seen = 0u;
    }
    if (p.spill > pb.spill.cap) {
        if ((rc = ensure(h, pb.spill, p.spill))) return rc;
        GEM_HIP(h, hipMemsetAsync(pb.spill.p, 0xff, pb.spill.cap, h->stream));     // tile word == kSpillFree
    }
    return stage_batch_tables(h, pb, p.tables, host);
}
// the queued increments and a dirty floor have gone into the pass that was just enqueued
static int pass_done(gem_handle* h, long long n)
{
    h->n_pending = 0;
    h->floor_dirty = false;
    h->stats.points_in = n;
    return GEM_OK;
}
// Passes that ran entirely on the handle's stream (single sweeps, k_frame, a flushed deferred fuse) read either half of the double
// buffer without recording a per-half event.  Before a pass on another stream may overwrite a half, those streams wait for
// everything enqueued on the handle's stream so far (one event at the switch, none per frame).
static int switch_to_bin_streams(gem_handle* h, bool overlap)
{
    if (!overlap) h->main_reads_pb = true;
    if (!overlap || !h->main_reads_pb) return GEM_OK;
    GEM_HIP(h, hipEventRecord(h->switch_done, h->stream));
    GEM_HIP(h, hipStreamWaitEvent(h->bin_stream, h->switch_done, 0));
    if (h->bin_stream2) GEM_HIP(h, hipStreamWaitEvent(h->bin_stream2, h->switch_done, 0));
    if (h->tab_stream) GEM_HIP(h, hipStreamWaitEvent(h->tab_stream, h->switch_done, 0));      // (the batch tables of a pass buffer are uploaded there)
    h->main_reads_pb = false;
    for (auto& b : h->pb) b.fuse_recorded = false;      // covered by the wait above
    return GEM_OK;
}

// Everything a batched pass's device tables are a function of, as bytes: equal keys = equal tables.
void batch_tables_key(const gem_handle* h, const PassInput& in, int kind, const void* device_tables, const std::vector<int>& first_of_sweep, std::vector<unsigned char>& key)
{
    key.clear();
    auto put = [&](const void* p, size_t n) { const unsigned char* b = static_cast<const unsigned char*>(p); key.insert(key.end(), b, b + n); };
    const int head[8] = {kind, in.n_sweeps, in.var_updates ? 1 : 0, in.sweep_orig0 ? 1 : 0, h->L, h->row0, h->row1, h->fast_laser ? 1 : 0};
    put(head, sizeof(head));
    put(&device_tables, sizeof(device_tables));
    put(h->center, sizeof(h->center)); put(h->start, sizeof(h->start)); put(&h->res, sizeof(h->res));
    put(in.params, sizeof(gem_frame_params) * in.n_sweeps);
    put(in.offsets, sizeof(long long) * (in.n_sweeps + 1));
    if (in.var_updates) put(in.var_updates, sizeof(float) * in.n_sweeps);
    if (in.sweep_orig0) put(in.sweep_orig0, sizeof(int) * in.n_sweeps);
    put(first_of_sweep.data(), sizeof(int) * first_of_sweep.size());
}

// One pass through the sorted pipeline (gem_sort.hip): six sort kernels on the binning stream, k_fuse_walk on the handle's.

int run_sort_pipeline(gem_handle* h, const PassInput& in, int attr, const SortGeometry& geo, const ShardOpts* shard)
{
    const bool batched = in.n_sweeps > 1;
    const bool with_src = (attr & 3) != 0;
    const int chunk = sort_chunk_for(in.n, h->sort_chunk);              // 1024-record chunks for passes that 4096-record ones would leave on a third of the chip
    const long long nc2max = (in.n + chunk - 1) / chunk;
    std::vector<int> chunk0(batched ? in.n_sweeps + 1 : 0, 0);        // first chunk of every sweep: a batch's table (a single cloud: no heap)
    for (int s = 0; batched && s < in.n_sweeps; ++s) chunk0[s + 1] = chunk0[s] + (int)((in.offsets[s + 1] - in.offsets[s] + chunk - 1) / chunk);
    const int NC1 = batched ? chunk0[in.n_sweeps] : (int)nc2max;
    const SortPlan plan = sort_plan(geo.n_passes, geo.dbins, in.n, (size_t)NC1, (size_t)nc2max, in.n_sweeps, with_src, walk_blocks(geo, shard != nullptr), shard != nullptr);
    const bool dense = h->n_pending > 0 || h->floor_dirty || (batched && in.var_updates != nullptr);
    const int T = geo.T;
    h->T = T;

    bool overlap = h->overlap && in.n >= std::min(h->overlap_min_points, h->sort_overlap_min_points) && h->stream == h->own_stream && !h->counting &&
                   (!shard || shard->bounds_stay_on_device);          // (the halves' sort returns its strip boundaries to the host: nothing to overlap)
    { const int rcd = flush_deferred(h); if (rcd) return rcd; }
    // this pass leaves its walk to the next call (gem_handle::dwalk) -- and then launches the previous pass's walk late, behind its own sort's launches
    const bool leave_walk = overlap && !shard && h->defer_walk && in.caller_device && attr == 0 && !h->timing && !h->dbg_on;
    if (!leave_walk) { const int rcd = flush_walk(h); if (rcd) return rcd; }
    // a shard bins into the WHOLE map (its records go to the strip owners); the frames carry the strip
    const int keep_row0 = h->row0, keep_row1 = h->row1;
    struct RestoreRows { gem_handle* h; int r0, r1; ~RestoreRows() { h->row0 = r0; h->row1 = r1; } } restore{h, keep_row0, keep_row1};
    if (shard) { h->row0 = 0; h->row1 = h->L; }
    // Consecutive overlapped passes sort on TWO binning streams in turn: the sort of a pass is a chain of six dependent kernels
    // that keep the chip's VALUs busy less than half of the time, so the tail of one pass's chain runs next
    // to the head of the next one's -- and next to the walk of the pass before, which alone has to follow the walk before it
    // (C4 150 -> 125 us per batch, C5 395 -> 355; a third stream: 129 / 365).
    const unsigned seq = overlap ? h->sort_pass++ : 0u;
    const unsigned slot = overlap ? seq % (unsigned)h->sort_ring : 0u;
    gem_handle::PassBuffers& pb = h->pb[slot];
    hipStream_t sbin = overlap ? (((seq & 1u) && h->sort_streams > 1 && h->bin_stream2) ? h->bin_stream2 : h->bin_stream) : h->stream;
    int rc;
    if ((rc = switch_to_bin_streams(h, overlap))) return rc;
    if (h->trace)
        fprintf(stderr, "[gem] sorted pass: n=%lld sweeps=%d overlap=%d (knob %d, min %lld, own stream %d, counting %d, shard %d) slot=%u stream=%s\n",
                (long long)in.n, in.n_sweeps, (int)overlap, (int)h->overlap, (long long)std::min(h->overlap_min_points, h->sort_overlap_min_points), (int)(h->stream == h->own_stream),
                (int)h->counting, (int)(shard != nullptr), slot, sbin == h->stream ? "main" : (sbin == h->bin_stream ? "bin" : "bin2"));

    if ((rc = ensure_sort_buffers(h, pb, plan))) return rc;
    // the walk of pass p-2 has read these buffers (host-side wait, see run_pipeline)
    if (overlap && pb.fuse_recorded) GEM_HIP(h, hipEventSynchronize(pb.fuse_done));

    SortArgs sa{};
    WalkArgs wa{};
    int batch_src = -1;                                               // which k_sort_project instantiation the batch's frames take (cached with the tables)
    if (batched) {
        const TablesPlan& t = plan.tables;
        batch_tables_key(h, in, 0, pb.tables.p, chunk0, h->key_scratch);
        const bool tables_cached = h->cache_tables && h->key_scratch == pb.tab_key;
        if (!tables_cached) {
            unsigned char* host;
            if ((rc = stage_batch_tables(h, pb, t, &host))) return rc;
            pb.tab_src = fill_batch_tables(h, host, t, in, chunk0.data());
            // on a stream of its own when the passes overlap: the upload (a 5 us blit + two kernel boundaries) then runs while the
            // binning stream is still sorting the pass before, instead of at the head of this pass's chain (the buffer's last
            // readers -- the pass before the previous one -- are done: fuse_done above)
            hipStream_t stab = sbin;
            if (overlap && h->tab_stream) stab = h->tab_stream;
            GEM_HIP(h, hipMemcpyAsync(pb.tables.p, host, t.total, hipMemcpyHostToDevice, stab));
            GEM_HIP(h, hipEventRecord(pb.tables_done, stab)); pb.tables_recorded = true;
            if (stab != sbin) GEM_HIP(h, hipStreamWaitEvent(sbin, pb.tables_done, 0));
            pb.tab_key = h->key_scratch;
            pb.tab_upload_stream = stab;
        } else if (pb.tab_upload_stream != sbin && pb.tables_recorded) {
            // the cached upload ran on another stream than this pass's sort (the upload stream, or the other binning stream): long
            // done -- passes of this buffer set have run since -- but the order is stated, not assumed
            GEM_HIP(h, hipStreamWaitEvent(sbin, pb.tables_done, 0));
        }
        batch_src = pb.tab_src;
        unsigned char* d = static_cast<unsigned char*>(pb.tables.p);
        sa.frames = reinterpret_cast<const FrameConst*>(d + t.o_frames);
        sa.sweep_chunk0 = reinterpret_cast<const int*>(d + t.o_first0);
        sa.sweep_first = reinterpret_cast<const long long*>(d + t.o_first);
        sa.sweep_orig0 = in.sweep_orig0 ? reinterpret_cast<const int*>(d + t.o_orig) : nullptr;
        wa.var_updates = in.var_updates ? reinterpret_cast<const float*>(d + t.o_var) : nullptr;
    } else {
        fill_frame(h, in.src == 0 ? in.params : nullptr, sa.frame0);
        sa.orig0_single = in.sweep_orig0 ? in.sweep_orig0[0] : 0;
    }
    sa.n_sweeps = in.n_sweeps; sa.n = in.n; sa.sweep_id0 = shard ? shard->sweep_id0 : 0;
    sa.xyzi = in.xyzi; sa.rgb = in.rgb; sa.orig = in.orig;
    sa.f_index = in.f_index; sa.f_height = in.f_height; sa.f_var = in.f_var;
    sa.f_R = in.f_R; sa.f_G = in.f_G; sa.f_B = in.f_B; sa.f_I = in.f_I;
    sa.keep_sentinel = h->track_lowest ? 1 : 0;
    sa.rank_by_ballot = h->rank_by_ballot ? 1 : 0; sa.few_bins = h->few_bins;
    sa.tiles_per_row = geo.tiles_per_row; sa.T = T;
    sa.id_bits = geo.id_bits; sa.n_passes = geo.n_passes;
    for (int i = 0; i < 3; ++i) { sa.dshift[i] = geo.dshift[i]; sa.dbits[i] = geo.dbits[i]; sa.dbins[i] = geo.dbins[i]; }
    sa.n_chunks1 = NC1; sa.chunk = chunk;
    // Small two-pass sorts (a depth image: 300 k points, six launches of 5-10 us each) let pass 1's scatter count pass 2's digit with
    // atomics: one launch and one pass over the keys less (4.7 us of the chip per frame; the frame's period is its walk and does not
    // move).  Big passes keep k_sort_count: ten million device-scope atomics cost more than its 8 us (k_sort_project's block counts
    // were 4.4 ns each).
    constexpr long long kFuseCountMaxPoints = 600000;
    sa.fuse_count = (geo.n_passes >= 2 && (h->fuse_count == 2 || (h->fuse_count == 1 && in.n <= kFuseCountMaxPoints))) ? 1 : 0;
    bind_sort_buffers(plan, geo.n_passes, {pb.s_hv1.p, pb.s_hv2.p, pb.s_key1.p, pb.s_key2.p, pb.s_src1.p, pb.s_src2.p, pb.s_cnt1.p, pb.s_cnt2.p, pb.s_misc.p}, sa);
    sa.epoch = ++h->sort_epoch; if (sa.epoch == 0u) sa.epoch = ++h->sort_epoch;
    wa.odd_flag = sa.odd_flag; wa.epoch = sa.epoch;
    sa.blk_cnt = nullptr;
    if (plan.blkcnt) {                                                // the walk will want every block's range (the last pass's bins are not the blocks)
        sa.blk_cnt = static_cast<uint32_t*>(pb.s_blkcnt.p);
        // the counts are zero between passes because k_block_prefix leaves them so; a pass that failed between the two leaves them
        // dirty: cleared here before the next one counts
        if (pb.blkcnt_dirty) GEM_HIP(h, hipMemsetAsync(pb.s_blkcnt.p, 0, pb.s_blkcnt.cap, sbin));
        pb.blkcnt_dirty = true;
    }
    sa.counters = h->counting ? h->d_counters : nullptr;

    const bool final_b = (geo.n_passes & 1) != 0;                     // the passes ping-pong between the arrays: a -> b -> a (-> b)
    wa.hv = final_b ? sa.hv_b : sa.hv_a; wa.key = final_b ? sa.key_b : sa.key_a; wa.src = final_b ? sa.src_b : sa.src_a; wa.bin_base = sa.bin_base;
    // centre rows first while (nearly) all of the walk's waves are resident at once: the start order then decides when the long
    // chains under the sensor begin (C4: 62 -> 52 us); a walk of many rounds reads its records front to back instead (C5:
    // 91 us in memory order, 100-120 us in any other)
    wa.walk_order = (h->walk_permute && 4ll * T <= 4096) ? 1 : 0;
    wa.center_tr = ((h->L / 2 + h->start[0]) % h->L) >> 5;
    wa.T = T; wa.tiles_per_row = geo.tiles_per_row; wa.L = h->L; wa.row0 = h->row0; wa.row1 = h->row1;
    wa.id_bits = geo.id_bits; wa.bin_shift = geo.dshift[geo.n_passes - 1]; wa.n_sweeps = in.n_sweeps;
    wa.exact_bins = (geo.block_form && geo.n_passes == 1) ? 1 : 0;
    wa.lane_sort = h->lane_sort ? 1 : 0;
    wa.light_blocks = h->blk_batch ? (h->blk_batch <= 512 ? 1 : 0) : ((long long)in.n <= 768ll * 4 * T ? 1 : 0);   // (by the mean: a heavy block just takes more rounds)
    if (wa.light_blocks) wa.lane_sort = 0;                             // (handing the busiest cells to wave 0 pays for blocks of thousands of records: C5 118 -> 114 us without)
    wa.mahal = h->cfg.mahalanobis_threshold; wa.var_floor = h->cfg.variance_floor;
    wa.dense = dense ? 1 : 0;
    wa.n_pending = h->n_pending;
    for (int i = 0; i < kMaxPending; ++i) wa.pending[i] = h->pending[i];
    wa.plain_env = h->plain_loop ? walk_plain_env(wa.var_floor, wa.mahal, h->pending, h->n_pending, batched ? in.var_updates : nullptr, in.n_sweeps) : 0;
    wa.prio_records = h->walk_prio; wa.lds_pad = h->walk_lds_pad; wa.light_fast = h->light_fast ? 1 : 0;
    wa.elevation = h->layers.elevation; wa.variance = h->layers.variance; wa.lowest = h->layers.lowest;
    wa.start0 = h->start[0]; wa.start1 = h->start[1];
    wa.intensity = h->layers.intensity; wa.colorR = h->layers.colorR; wa.colorG = h->layers.colorG; wa.colorB = h->layers.colorB;
    wa.xyzi = in.xyzi; wa.rgb = in.rgb; wa.f_R = in.f_R; wa.f_G = in.f_G; wa.f_B = in.f_B; wa.f_I = in.f_I;
    wa.counters = sa.counters;
    wa.count_per_pass = batched ? 0 : 1;

    if (h->counting) GEM_HIP(h, hipMemsetAsync(h->d_counters, 0, 2 * sizeof(unsigned long long), h->stream));
    bool ride_bin = false;
    {
        // (a third pass is accounted with the second: count / scan / scatter of the higher digits)
        // (event pairs only for the kernels that are launched: the elapsed time of a pair that was never recorded is an error)
        const bool two = geo.n_passes >= 2, three = geo.n_passes == 3;
        Timed t0(h, 3), t1(h, 4), t2(h, 5), t3(h, two && !sa.fuse_count ? 6 : -1), t4(h, two ? 7 : -1), t5(h, two ? 8 : -1), t6(h, three ? 6 : -1), t7(h, three ? 7 : -1), t8(h, three ? 8 : -1);
        LaunchEvents ev[9] = {t0.events(), t1.events(), t2.events(), t3.events(), t4.events(), t5.events(), t6.events(), t7.events(), t8.events()};
        // The walk waits for the sort across streams: as the STOP EVENT of the sort's last dispatch the event is seen 3 us earlier
        // than a marker recorded behind it (tools/ubench/handover.hip: 7 against 10 us) -- when that kernel is the last thing on the
        // sort's stream before the walk (no k_block_prefix, no strip search behind it) and nothing is being timed.
        ride_bin = overlap && h->ride_events && !h->timing && !shard && !(geo.block_form && geo.n_passes > 1);
        if (ride_bin) ev[3 * geo.n_passes - 1].stop = pb.bin_done;
        int src = in.src;
        if (src == 0 && batched) { if (batch_src > 0) src = batch_src; }
        else if (src == 0) {
            if (in.params[0].sensor_model == GEM_MODEL_LASER) src = sa.frame0.fast_laser ? 4 : 2;      // 4: the rotation variance is zero (height_variance, kModelLaserFast)
        }
        GEM_HIP(h, launch_sort(sbin, sa, src, with_src, ev));
    }
    if (shard) {
        // where the strips begin in the sorted records (one 32-ary search per boundary) and where every block's records are
        // (k_block_prefix): behind the sort, on its stream
        gem_handle::Shard& sd = h->shard;
        sd.valid = false;
        if ((rc = ensure_shard_tables(h))) return rc;
        uint32_t* host = static_cast<uint32_t*>(h->sh_host);
        for (int k = 0; k <= shard->nstrips; ++k) {
            const int tile_row = shard->strip_rows[k] >= h->L ? geo.tiles_per_row : shard->strip_rows[k] / 32;
            host[k] = (uint32_t)(tile_row * geo.tiles_per_row) << 10;                // first cell id of the strip (the same every call)
        }
        uint32_t* d_ids = static_cast<uint32_t*>(pb.s_shard.p), *d_bounds = d_ids + 16;
        const uint32_t* keys = final_b ? sa.key_b : sa.key_a;
        GEM_HIP(h, hipMemcpyAsync(d_ids, host, sizeof(uint32_t) * (shard->nstrips + 1), hipMemcpyHostToDevice, sbin));
        GEM_HIP(h, launch_strip_bounds(sbin, keys, sa.total, geo.id_bits, d_ids, d_bounds, shard->nstrips + 1));
        GEM_HIP(h, launch_block_prefix(sbin, sa.blk_cnt, 4 * T, static_cast<uint2*>(pb.s_ranges.p)));
        pb.blkcnt_dirty = false;
        sd.hv = final_b ? sa.hv_b : sa.hv_a; sd.key = keys; sd.ranges = static_cast<const uint2*>(pb.s_ranges.p);
        sd.d_bounds = d_bounds; sd.nstrips = shard->nstrips; sd.slot = overlap ? (int)slot : -1; sd.stream = sbin;
        h->stats.points_in = in.n;
        if (shard->bounds_stay_on_device) {                  // gem_add_sharded_device all-gathers them from where they are
            for (int k = 0; k <= shard->nstrips; ++k) sd.bounds[k] = 0;
            if (overlap) GEM_HIP(h, hipEventRecord(pb.bin_done, sbin));
            sd.valid = true;
            return GEM_OK;
        }
        GEM_HIP(h, hipMemcpyAsync(host + 32, d_bounds, sizeof(uint32_t) * (shard->nstrips + 1), hipMemcpyDeviceToHost, sbin));
        GEM_HIP(h, hipStreamSynchronize(sbin));
        for (int k = 0; k <= shard->nstrips; ++k) sd.bounds[k] = host[32 + k];
        sd.valid = true;
        return GEM_OK;
    }
    if (geo.block_form && geo.n_passes > 1) {
        // the last digit's bins hold several blocks: where every block's records are (the prefix of the per-block counts
        // k_sort_project took), behind the sort on its stream, instead of a search by every workgroup of the walk
        GEM_HIP(h, launch_block_prefix(sbin, sa.blk_cnt, 4 * T, static_cast<uint2*>(pb.s_ranges.p)));
        pb.blkcnt_dirty = false;
        wa.ranges = static_cast<const uint2*>(pb.s_ranges.p);
    }
    { const int rcd = flush_walk(h); if (rcd) return rcd; }           // the pass before: its sort has had this call's launches to finish
    if (leave_walk) {
        if (!ride_bin) GEM_HIP(h, hipEventRecord(pb.bin_done, sbin));
        h->dwalk.wa = wa; h->dwalk.block_form = geo.block_form; h->dwalk.attr = attr; h->dwalk.slot = slot; h->dwalk.valid = true;
        ++h->walks_left;
        h->dbg_rows = 0;
        return pass_done(h, in.n);
    }
    if (overlap) {
        if (!ride_bin) GEM_HIP(h, hipEventRecord(pb.bin_done, sbin));
        GEM_HIP(h, hipStreamWaitEvent(h->stream, pb.bin_done, 0));
    }
    h->dbg_rows = 0;
    if (h->dbg_on && geo.block_form) {
        if ((rc = ensure(h, h->dbg, (size_t)T * 4 * 16 * 8))) return rc;
        GEM_HIP(h, hipMemsetAsync(h->dbg.p, 0, (size_t)T * 4 * 16 * 8, h->stream));
        wa.dbg = static_cast<unsigned long long*>(h->dbg.p);
        h->dbg_rows = T * 4;
    }
    { Timed t(h, 9); GEM_HIP(h, geo.block_form ? launch_block_walk(h->stream, wa, attr, t.events()) : launch_walk(h->stream, wa, attr, t.events())); }
    if (overlap) { GEM_HIP(h, hipEventRecord(pb.fuse_done, h->stream)); pb.fuse_recorded = true; }
    return pass_done(h, in.n);
}

int run_pipeline(gem_handle* h, const PassInput& in0)
{
    const PlanEnv env = plan_env(h);
    const PassChoice choice = choose_pass(env, in0.n, in0.n_sweeps, sort_bins_fit);
    if (choice.fell_back) ++h->sort_fallbacks;                        // (a forced form / pass count that does not fit this map: counted, gem_debug_get)
    int attr = 0;
    if (in0.src == 0 && in0.rgb) attr = 1;
    if (in0.src == 1 && in0.f_R && in0.f_G && in0.f_B && in0.f_I) attr = 2;
    if (h->track_lowest) attr |= 4;                  // the kernel variants that also maintain map_lowest (16x16 tiles)
    if (choice.geo.ok) return run_sort_pipeline(h, in0, attr, choice.geo);
    { const int rcw = flush_walk(h); if (rcw) return rcw; }           // (a sorted pass's walk still to be launched: before anything of this pass fuses)
    // A big single cloud becomes a batch of sweeps with one frame (cut_sweeps).  The recurrence is unchanged: the per-sweep variance
    // floor is idempotent with the floor at the start of every step (GPU:500-501), and no variance increment is applied between
    // these sweeps.
    // (Fuse's arrays too, src == 1: a descriptor row holds the units of ONE sweep, k_fuse_list reads one chunk of kChunkUnits of it --
    //  until round 4 the cut was only made for clouds, and a Fuse of more than 131 072 points that stayed below the sorted pipeline's
    //  threshold lost every point behind the first 131 072.)
    TilePlan plan = tile_plan(env, in0.n, in0.n_sweeps, in0.offsets);
    if (plan.err) return fail(h, GEM_ERR_INVALID, plan.err == 1 ? "cloud too large" : "lowest tracking: the pass is too large for 16x16 tiles (cut it into smaller calls)");
    PassInput in = in0;
    std::vector<gem_frame_params> cut_params;
    std::vector<long long> cut_offsets;
    std::vector<int> orig0;
    if (plan.n_sweeps != in.n_sweeps) {
        const int ns = plan.n_sweeps;
        if (in.src == 0) cut_params.assign(ns, *in.params);
        cut_offsets.resize(ns + 1); orig0.resize(ns);
        for (int s = 0; s <= ns; ++s) cut_offsets[s] = std::min<long long>(in.n, (long long)s * kSweepPoints);
        for (int s = 0; s < ns; ++s) orig0[s] = (int)cut_offsets[s];
        in.n_sweeps = ns; in.params = in.src == 0 ? cut_params.data() : nullptr; in.offsets = cut_offsets.data(); in.var_updates = nullptr; in.sweep_orig0 = orig0.data();
    }
    const bool batched = in.n_sweeps > 1;
    const int U = kUnit, B = plan.B, bpad = plan.bpad;
    const bool dense = h->n_pending > 0 || h->floor_dirty || (batched && in.var_updates != nullptr);

    if (B == 0) {
        // Fuse with zero points still runs the floor pass (gpu_process.cu:533-534)
        { const int rcd = frame_unpair(h); if (rcd) return rcd; }      // (not a call a held sweep may wait behind)
        if (batched && in.var_updates)
            for (int s = 0; s < in.n_sweeps; ++s) {
                if (h->n_pending == kMaxPending) { int rc = flush_pending(h, true); if (rc) return rc; }
                h->pending[h->n_pending++] = in.var_updates[s];
            }
        return (h->n_pending || h->floor_dirty) ? flush_pending(h, true) : GEM_OK;
    }
    const int ts = plan.ts, tiles_per_row = plan.tiles_per_row, T = plan.T;
    h->T = T;
    if (fuse_lds_bytes(ts, h->fuse_variant, attr & 3) > 160 * 1024) return fail(h, GEM_ERR_INVALID, "fuse kernel geometry exceeds the LDS");

    // k_bin of this pass may run on its own stream, concurrently with the k_fuse of the previous pass
    // (it depends on the cloud and the pose, not on the map).  Only with the handle's own stream:
    // a caller-provided stream keeps everything in order on that stream.  Device-resident inputs
    // must be complete when the call is made (they are not ordered against the handle's streams).
    // The cross-stream event pair costs ~3 us per pass (measured), so it only pays for big passes
    // (batches / aggregated clouds: C4 379 -> 313 us); single sweeps stay on one stream.
    bool overlap = h->overlap && in.n >= h->overlap_min_points && h->stream == h->own_stream && !h->counting && !h->dbg_on;
    // one launch per frame for a stream of single sweeps (k_frame): needs the other half of the double buffer
    const bool defer = h->defer && in.device_input && in.src == 0 && !batched && (attr & 3) == 0 && ts == 4 && !overlap &&
                       !h->counting && (!h->dbg_on || h->dbg_frame);
    if (!defer) { const int rcd = flush_deferred(h); if (rcd) return rcd; }
    // ... and one launch per TWO sweeps once nobody has read in between for a while (gem_frame_pair.hpp): a call may be held or share a
    // launch when that launch is going to be the lean one, the cloud is the caller's own buffer (an arena or a staging half of the
    // handle is refilled by the next call, before a held sweep would have been binned) and the stream is the handle's own (on a
    // caller-provided stream the work is on that stream when the call returns).  Everything else takes the single form, behind a
    // held sweep or a deferred pair if there is one.
    gem::FrameConst frame0{};
    if (!batched) fill_frame(h, in.src == 0 ? in.params : nullptr, frame0);
    bool pairable = defer && h->frame_pair && attr == 0 && in.caller_device && h->stream == h->own_stream && in.n > 0 && !h->dbg_on && !h->counting &&
                    frame0.fast_laser != 0 && !in.rgb && frame_would_lean(h);
    for (int i = 0; pairable && i < h->fstate.deferred; ++i) pairable = h->deferred[i].lean_binned && h->deferred[i].attr == 0;
    if (defer && !pairable) { const int rcd = frame_unpair(h); if (rcd) return rcd; }
    // the deferred and the held sweeps own a buffer set each: this pass takes the first of the four that is free (a stream of singles
    // alternates between the first two, as it always did; the other two are allocated by the first pair, or by gem_reserve)
    unsigned set = 0;
    if (defer) {
        unsigned used = 0;
        for (int i = 0; i < h->fstate.deferred; ++i) used |= 1u << h->deferred[i].set;
        if (h->fstate.held) used |= 1u << h->held.set;
        while (used & (1u << set)) ++set;
    } else if (overlap) set = h->pass++ & 1u;
    gem_handle::PassBuffers& pb = h->pb[set];
    hipStream_t sbin = overlap ? h->bin_stream : h->stream;
    int rc;
    if ((rc = switch_to_bin_streams(h, overlap))) return rc;
    // k_fuse of pass p-2 has read these buffers.  Waited for on the HOST: a hipStreamWaitEvent on an event that is still
    // far from complete delayed the start of k_bin behind it (C5: 1.52 -> 1.64-1.81 ms per pass, the overlap mostly lost);
    // the host stays at most two (big) passes ahead of the device, which costs nothing.
    if (overlap && pb.fuse_recorded) GEM_HIP(h, hipEventSynchronize(pb.fuse_done));
    // k_frame bins into per-tile buckets: the point index rides in 22 bits of a record (a single sweep has at most kSweepPoints)
    static_assert(kSweepPoints <= (1ll << 22), "k_frame's record format");
    unsigned char* host = nullptr;
    if ((rc = ensure_tile_buffers(h, pb, plan, sbin, defer, &host))) return rc;       // (a batch: the sorted pipeline's cached tables of this buffer set are overwritten)
    if (pb.epoch >= kFlagEpochMax) {
        GEM_HIP(h, hipMemsetAsync(pb.flag.p, 0, pb.flag.cap, sbin));
        GEM_HIP(h, hipMemsetAsync(pb.gflag.p, 0, pb.gflag.cap, sbin));
        pb.epoch = 0;
    }
    ++pb.epoch;

    BinArgs ba{};
    FuseArgs fa{};
    const TablesPlan& tab = plan.tables;
    if (batched) {
        std::vector<int> unit0(in.n_sweeps + 1, 0);
        for (int s = 0; s < in.n_sweeps; ++s) unit0[s + 1] = unit0[s] + (int)sweep_units(in.offsets[s + 1] - in.offsets[s]);
        (void)fill_batch_tables(h, host, tab, in, unit0.data());
        GEM_HIP(h, hipMemcpyAsync(pb.tables.p, host, tab.total, hipMemcpyHostToDevice, sbin));
        GEM_HIP(h, hipEventRecord(pb.tables_done, sbin)); pb.tables_recorded = true;
        unsigned char* d = static_cast<unsigned char*>(pb.tables.p);
        ba.frames = reinterpret_cast<const FrameConst*>(d + tab.o_frames);
        ba.sweep_unit0 = reinterpret_cast<const int*>(d + tab.o_first0);
        ba.sweep_first = reinterpret_cast<const long long*>(d + tab.o_first);
        ba.sweep_orig0 = in.sweep_orig0 ? reinterpret_cast<const int*>(d + tab.o_orig) : nullptr;
        fa.sweep_unit0 = ba.sweep_unit0;
        fa.var_updates = in.var_updates ? reinterpret_cast<const float*>(d + tab.o_var) : nullptr;
    } else {
        ba.frame0 = frame0;
    }
    ba.n_sweeps = in.n_sweeps; ba.n = in.n;
    ba.xyzi = in.xyzi; ba.rgb = in.rgb; ba.orig = in.orig;
    ba.f_index = in.f_index; ba.f_height = in.f_height; ba.f_var = in.f_var;
    ba.f_R = in.f_R; ba.f_G = in.f_G; ba.f_B = in.f_B; ba.f_I = in.f_I;
    ba.T = T; ba.tiles_per_row = tiles_per_row; ba.B = B; ba.Bpad = bpad;
    ba.tile_bits = 0; while ((1 << ba.tile_bits) < T) ++ba.tile_bits;
    ba.epoch = pb.epoch;
    ba.rec_words = (attr & 3) != 0 ? 4 : 3;
    ba.rec = static_cast<uint4*>(pb.rec.p); ba.seg = static_cast<uint16_t*>(pb.seg.p); ba.flag = static_cast<uint32_t*>(pb.flag.p); ba.gflag = static_cast<uint32_t*>(pb.gflag.p);
    ba.counters = h->counting ? h->d_counters : nullptr;
    ba.keep_sentinel = h->track_lowest ? 1 : 0;
    ba.srt_top = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(pb.srt.p) + pb.srt.cap - 16);

    fa.epoch = pb.epoch;
    fa.rec = ba.rec; fa.seg = ba.seg; fa.flag = ba.flag; fa.gflag = ba.gflag; fa.B_total = B; fa.U = U; fa.n_sweeps = in.n_sweeps; fa.Bpad = bpad;
    fa.T = T; fa.tiles_per_row = tiles_per_row; fa.L = h->L; fa.row0 = h->row0; fa.row1 = h->row1;
    fa.center_tr = ((h->L / 2 + h->start[0]) % h->L) >> ts; fa.center_tc = ((h->L / 2 + h->start[1]) % h->L) >> ts;
    fa.mahal = h->cfg.mahalanobis_threshold; fa.var_floor = h->cfg.variance_floor;
    fa.dense = dense ? 1 : 0;
    fa.n_pending = h->n_pending;
    for (int i = 0; i < kMaxPending; ++i) fa.pending[i] = h->pending[i];
    fa.elevation = h->layers.elevation; fa.variance = h->layers.variance;
    fa.intensity = h->layers.intensity; fa.colorR = h->layers.colorR; fa.colorG = h->layers.colorG; fa.colorB = h->layers.colorB;
    fa.xyzi = in.xyzi; fa.rgb = in.rgb; fa.f_R = in.f_R; fa.f_G = in.f_G; fa.f_B = in.f_B; fa.f_I = in.f_I;
    fa.counters = ba.counters;
    fa.srt = static_cast<uint4*>(pb.srt.p); fa.srt_top = ba.srt_top; fa.dense_min = h->dense_min;
    fa.lowest = h->layers.lowest; fa.start0 = h->start[0]; fa.start1 = h->start[1];
    fa.count_per_pass = orig0.empty() ? 0 : 1;
    fa.dbg = nullptr;
    fa.dbg_sweep = h->dbg_sweep;
    if (h->dbg_on) {
        // rows [0, T): the tiles' stamps; [T, T + binning blocks): the binning blocks' (k_frame with "dbg_frame": both halves of one launch)
        const int nbin = (B + 3) / 4;
        if ((rc = ensure(h, h->dbg, (size_t)(T + nbin) * 16 * 8))) return rc;
        GEM_HIP(h, hipMemsetAsync(h->dbg.p, 0, (size_t)(T + nbin) * 16 * 8, h->stream));
        fa.dbg = static_cast<unsigned long long*>(h->dbg.p);
        if (h->dbg_frame) { ba.dbg = fa.dbg + (size_t)T * 16; h->dbg_rows = T + nbin; }
    }

    if (defer) {
        ba.bkt = static_cast<uint32_t*>(pb.bkt.p); ba.bcount = static_cast<uint32_t*>(pb.bcnt.p); ba.spill = static_cast<uint4*>(pb.spill.p);
        ba.ctl = static_cast<uint32_t*>(pb.fctl.p);
        fa.bkt = ba.bkt; fa.bcount = ba.bcount; fa.spill = ba.spill; fa.ctl = ba.ctl; fa.form_seen = h->form_seen;
        if (h->fstate.deferred && h->deferred[0].attr != attr) { const int rcd = flush_deferred(h); if (rcd) return rcd; }   // (cannot happen: toggling the tracking flushes)
        // hold, or launch: the plan is frame_pair_step's (a flush the event asks for has been made above: frame_unpair).  The host's
        // pick of k_frame's form is frame_launch's: the launch is lean as a whole -- its fuse half AND the binning -- or generic
        gem_handle::FrameSweep sw;
        sw.fa = fa; sw.ba = ba; sw.ts = ts; sw.attr = attr; sw.set = (int)set;
        const gem::FramePairPlan fp = gem::frame_pair_step(h->fstate, pairable ? gem::kFramePairable : gem::kFrameSingle);
        if (fp.hold) {
            // nothing is enqueued: the next call, or whatever observes the map, bins it.  The first hold of a handle allocates the
            // sets the pairs are going to rotate through (unless gem_reserve has): here, not one by one in the launches that follow
            for (auto& other : h->pb) if (!other.bkt.p && (rc = ensure_tile_buffers(h, other, plan, h->stream, true))) { h->fstate.held = false; return rc; }
            h->held = sw;
            return pass_done(h, in.n);
        }
        const bool was_held = fp.launch[0].bin == 2;
        h->fstate.deferred = fp.launch[0].fuse; h->fstate.held = false;   // (frame_launch fuses what IS deferred and makes what it bins the deferred)
        gem_handle::FrameSweep* bins[2] = {was_held ? &h->held : &sw, &sw};
        if ((rc = frame_launch(h, bins, fp.launch[0].bin))) { h->fstate = gem::FramePairState{}; return rc; }
        h->main_reads_pb = true;
        return pass_done(h, in.n);
    }
    if (h->counting) GEM_HIP(h, hipMemsetAsync(h->d_counters, 0, 2 * sizeof(unsigned long long), h->stream));
    { Timed t(h, 0); GEM_HIP(h, launch_bin(sbin, ba, in.src, ts, t.events())); }
    if (overlap) {
        GEM_HIP(h, hipEventRecord(pb.bin_done, sbin));
        GEM_HIP(h, hipStreamWaitEvent(h->stream, pb.bin_done, 0));
    }
    { Timed t(h, 1); GEM_HIP(h, launch_fuse(h->stream, fa, ts, attr, h->fuse_variant, t.events())); }
    if (overlap) { GEM_HIP(h, hipEventRecord(pb.fuse_done, h->stream)); pb.fuse_recorded = true; }
    return pass_done(h, in.n);
}

} // namespace gemi

// Arenas for the largest pass the caller is going to make, allocated NOW: the arenas only ever grow, but growing means waiting for
// everything in flight, hipFree and hipMalloc -- in the middle of a stream of frames that is a stall of a millisecond or more the
// first time a bigger cloud arrives (measured: tools/bench_configs.py --configs reserve).  max_points points in at most max_sweeps
// sweeps per call (1 for gem_add*); colours as they will be passed.  Every extremal pass inside the bounds (bound_plans,
// gem_plan.hpp) is planned as the pipelines plan theirs and allocated through the same ensure_* functions: the sorted forms in the
// buffer sets their overlapped passes rotate through, the tile pipeline in its two.  On a handle that joined a communicator with
// tile strips, max_points / max_sweeps bound the GLOBAL points / sweeps of a gem_add_sharded_device step: the shard's sort (its W-th
// of the points), both sets of receive buffers (no strip gets more records than the step has points) and the small tables.
int gem_reserve(gem_handle* h, long long max_points, int max_sweeps, int with_colours)
{
    if (!h || max_points < 0 || max_sweeps < 1 || max_points >= (1ll << 31)) return h ? fail(h, GEM_ERR_INVALID, "gem_reserve: bad argument") : GEM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    { const int rcd = settle(h); if (rcd) return rcd; }
    if (max_points == 0) return GEM_OK;
    int rc;
    // staging of host-pointer inputs: a host cloud of the add entries (cloud_layout, where the clean mask also writes), gem_fuse's
    // seven arrays, gem_process_points' nine, a depth image and the cloud unprojected from it (depth_plan)
    if ((rc = ensure(h, h->stage, std::max({cloud_layout(max_points, true, true).bytes, stage_words_bytes(max_points, 9), depth_stage_bytes(max_points)})))) return rc;
    // (the raw-cloud compactions, gem_capi_clean.cpp, add a count per 1024 points)
    if ((rc = ensure(h, h->clean_cnt, clean_scratch_bytes(max_points)))) return rc;
    if ((rc = voxel_reserve(h, max_points))) return rc;        // (the VoxelGrid entries, gem_capi_voxel.cpp)
    // ... and its pinned counterpart.  The deferred / zero-copy uploads (upload_arrays) keep TWO calls' arrays in the buffer, a half
    // each: gem_fuse's seven arrays are the largest (28 B per point; gem_add with rgb + orig_index: 24), as long as one call stays
    // below the 16 MB from which uploads go to the runtime's pageable path; callers with host arrays (gem_process_points: nine arrays;
    // gem_map_feature: nine layers) where that is a modest amount: larger ones grow on first use
    const size_t one = stage_words_bytes(max_points, 7);
    size_t want = one < (16u << 20) ? 2 * one + 512 : 0;
    for (const size_t nine : {stage_words_bytes(max_points, 9), stage_words_bytes(h->cells, 9)}) if (nine <= (64u << 20)) want = std::max(want, nine);
    if (want) (void)host_stage(h, want);
    const bool sharded = h->tp_x && h->tile_strips;          // (a handle of the sharded path: its steps are what the bounds describe)
    const PlanEnv env = plan_env(h);
    BoundPlan plan[kMaxBoundPlans];
    const int n_plans = bound_plans(env, max_points, max_sweeps, sharded ? h->nranks : 0, with_colours != 0, sort_bins_fit, plan);
    for (int i = 0; i < n_plans; ++i) {
        const BoundPlan& p = plan[i];
        for (int k = 0; p.kind == 1 && k < env.sort_ring; ++k) if ((rc = ensure_sort_buffers(h, h->pb[k], p.sort))) return rc;
        // (16x16 tiles: the two further sets a pair launch bins into, gem_frame_pair.hpp -- 13 MB a set at 600^2 cells)
        const int tile_sets = (p.kind == 2 && p.tile.ts == 4 && h->frame_pair && h->defer && !h->track_lowest) ? 4 : 2;
        for (int k = 0; p.kind == 2 && k < tile_sets; ++k) if ((rc = ensure_tile_buffers(h, h->pb[k], p.tile, h->stream, true))) return rc;
        if (sharded && p.kind == 1 && (rc = ensure_shard_tables(h, p.sort.blocks))) return rc;
    }
    if (sharded) {                                           // every strip's owner receives at most all of the step's points
        h->recv_bound = max_points;
        for (int q = 0; h->nranks > 1 && q < 2; ++q) if ((rc = ensure_recv(h, q, (size_t)max_points + 4 * h->nranks))) return rc;
    } else if (h->track_lowest && (rc = ensure_ray(h))) return rc;
    GEM_HIP(h, hipStreamSynchronize(h->stream));
    return GEM_OK;
}
