// gem_capi_internal.hpp -- what the translation units of the C ABI share: the handle, its arenas and staging, the pass pipelines,
// the multi-rank step.  Internal to libgem_hip.so (nothing here is installed); the ABI itself is include/gem_hip.h.
//   gem_capi_core.cpp      errors, arenas, the pinned staging buffer and the host <-> device transfers, frame constants, the deferred
//                          launches (flush_* / settle), the process-lifetime stream pools
//   gem_plan.hpp           the pass plan: which pipeline a pass takes and the size and layout of every buffer of it (pure functions)
//   gem_capi_pipeline.cpp  run_pipeline / run_sort_pipeline: which kernels a pass takes, on which streams, in the buffers of its plan;
//                          gem_reserve: the same plans for the extremal passes inside its bounds
//   gem_capi.cpp           the extern "C" entry points of include/gem_hip.h (single-device part) and include/gem_hip_debug.h
//   gem_capi_comm.cpp      communicators, the all-gather of the layers, the sharded step (gem_add_sharded_device and its halves)
//   gem_costmap_host.hpp   the costmap family's shared host pieces (gem_capi_costmap / _inflate / _footprint / _mapgrid / _critics /
//                          _navplan / _frontier / _obstacle / _voxlayer / _rollout .cpp): the lookup by id, geometry and grid, the staleness checks of a plan and a search,
//                          the bounds read-back, a window read or written
//   gem_observe_host.hpp   what gem_capi_obstacle.cpp and gem_capi_voxlayer.cpp share: the staged observations, the common ObsParams, touch
//   gem_rounds.hpp         the host loop of the tiled fixed-point kernels (plan, frontier labels): chunks of rounds up to the bound (pure C++)
#pragma once

#include "../../include/gem_hip.h"
#include "../../include/gem_hip_debug.h"
#include "gem_kernels.hpp"
#include "gem_frame_pair.hpp"
#include "gem_plan.hpp"
#include "gem_hostcopy.hpp"
#include "gem_transport.hpp"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

using namespace gem;

namespace gem { struct CriticsArgs; struct FootSpec; struct CostGeom; }

namespace gemi {

extern thread_local std::string g_create_error;

struct Arena {
    void*  p = nullptr;
    size_t cap = 0;
};

struct EventPair { hipEvent_t a, b; int kind; };

} // namespace gemi

using namespace gemi;

struct StreamSet { hipStream_t s[4] = {nullptr, nullptr, nullptr, nullptr}; };   // own, bin, bin2, tab (see acquire_streams)

struct gem_handle {
    std::mutex  mu;
    std::string err;
    int         device = 0;
    hipStream_t own_stream = nullptr;
    StreamSet streams;                  // own, bin, bin2, tab as they were taken from the pool (given back together)
    hipStream_t stream = nullptr;
    gem_map_config cfg{};
    int   L = 0, cells = 0;
    float res = 0.f;
    LayerPtrs layers{};
    float center[2] = {0.f, 0.f};
    int   start[2] = {0, 0};
    float sensor_z = 0.f;
    int   row0 = 0, row1 = 0;
    int   ts = 0, T = 0;           // tile shift (0 = per pass), tiles of the last pass

    Arena stage;        // staging of host-pointer inputs / outputs
    // Pipeline intermediates, double-buffered: k_bin of pass p+1 runs on `bin_stream` while k_fuse of
    // pass p runs on `stream` (binning does not depend on the map, only on the cloud and the pose).
    struct PassBuffers {
        Arena rec, srt, seg, flag, gflag;   // records, descriptor table, touched stamps per (tile, sweep) and per (sweep, tile, 32 units)
        Arena bkt, bcnt, spill, fctl;       // k_frame's per-tile buckets, their counts (all-zero between passes), the spill slots (all free), its two form words
        Arena s_hv1, s_hv2, s_key1, s_key2, s_src1, s_src2, s_cnt1, s_cnt2, s_misc;   // the sorted pipeline of big passes (gem_sort.hip)
        bool blkcnt_dirty = false;     // k_sort_project has been asked to count into s_blkcnt and k_block_prefix has not cleared it yet
        Arena s_blkcnt;                // [4 T] records per block, zero between passes (k_sort_project adds, k_block_prefix reads and clears)
        Arena s_ranges, s_shard;       // multi-GPU shard: every block's range in the sorted records; strip ids [16] | strip bounds [16]
        Arena tables;                  // batched-call tables (frames, sweep_unit0, sweep_first, var_updates)
        void* host_tables = nullptr;   // their pinned staging copy: the upload is asynchronous, `tables_done` guards its reuse
        size_t host_cap = 0;
        hipEvent_t tables_done = nullptr;
        bool tables_recorded = false;
        // what the device copy of the tables was built from (batch_tables_key): a stream of batches with the same frames, offsets,
        // increments and map pose -- a mapping loop replaying a fixed sensor rig, the benchmarks -- skips the 2 x 32 fill_frame,
        // the memset and the upload of the call (60-100 us of host time per C4 call before, against a 95 us device period)
        std::vector<unsigned char> tab_key;
        int tab_src = 0;
        hipStream_t tab_upload_stream = nullptr;
        hipEvent_t bin_done = nullptr, fuse_done = nullptr;
        bool fuse_recorded = false;
        uint32_t epoch = 0;            // touched-flag stamp of the last pass (0 = the flag table holds no live stamps)
    } pb[4];            // the tile pipeline alternates between the first two; the sorted pipeline's overlapped passes rotate through all four
    unsigned pass = 0, sort_pass = 0;
    uint32_t sort_epoch = 0;            // a number per sorted pass (SortArgs::epoch)
    int sort_streams = 2;               // binning streams the overlapped passes of the sorted pipeline alternate between (debug knob)
    bool trace = false;                 // debug knob: one line on stderr per pass of the sorted pipeline (which streams / buffers it took)
    int sort_ring = 3;                  // buffer sets they rotate through (debug knob, 2..4).  The sort of pass p may start once the walk of pass p - ring has
                                        // read its buffers: with two sets that wait -- a host round trip and then the whole sort chain -- sat between consecutive walks
                                        // (C4 block-sorted: 120 us per batch with two sets, 104 with three, 109 with four)
    // A stream of single device-resident sweeps runs as ONE launch per frame: k_frame fuses the previous
    // frame's records next to the binning of the new cloud.  The fuse of the newest frame is therefore
    // deferred until the next gem_add_device -- or until anything observes or modifies the map.
    // A stream nobody reads in between goes one step further (gem_frame_pair.hpp): every other call is HELD -- accepted, its
    // arguments built, nothing enqueued -- and the call behind it launches one grid for both sweeps, so up to two sweeps are
    // deferred and one held.  Each of them owns one of the four pass buffer sets (`set`; a launch bins into sets none of them holds).
    // fstate.deferred of `deferred` are live, oldest first; `held` is live while fstate.held.  flush_deferred settles all of it.
    struct FrameSweep { FuseArgs fa{}; BinArgs ba{}; int ts = 0, attr = 0, set = 0; bool lean_binned = false; };   // lean_binned: its binning ran with BinArgs::lean
    FrameSweep deferred[2], held;
    gem::FramePairState fstate;
    bool frame_pair = true;             // debug knob "frame_pair": 0 = one launch per sweep, as before
    bool frame_pair_overlap = true;     // debug knob "frame_pair_overlap": 0 = a launch of two fuses with pair_k_frame (two plain rounds per tile), as before
    long long frame_pairs = 0, frame_held_flushed = 0;   // launches that carried two sweeps; held sweeps settled by a flush (gem_debug_get)
    // k_frame has two forms (gem_kernels.hip): the generic one, which switches a buffer set to the descriptor form on the device, and
    // a lean one that carries the bucket form only.  The HOST picks per launch: lean while the word `form_seen` -- pinned host memory
    // that frame_tile's slow path stores 1 into -- reads zero and the pass to fuse was binned lean; generic for good after that.  The
    // word is read with a plain load on every call, no event and no wait: a lean launch enqueued before the store lands is still
    // right (the lean form has the slow path), only slow.
    uint32_t* form_seen = nullptr;      // allocated once, with k_frame's arenas (ensure_tile_buffers)
    int  frame_lean = 2;                // debug knob "frame_lean": 0 = always generic, 1 = always lean, 2 = the host's choice as above
    long long frame_lean_launches = 0, frame_generic_launches = 0;   // launches of either form: k_frame, the first frame's binning, the fuse-only flush
    // The sorted pipeline's walk of an overlapped pass is launched by the NEXT call (or by whatever observes the map): by then its sort
    // has usually completed, and a walk that need not be put behind a hipStreamWaitEvent starts 1.4 us after the walk before it
    // instead of 5-7 (tools/ubench/handover.hip: the wait costs that much even when the event completed long before).  A stream of
    // depth images is bound by exactly that chain of walks (C3: 45.7 us per frame = 38 us walk + the hand-over).
    struct DeferredWalk { bool valid = false; WalkArgs wa{}; bool block_form = false; int attr = 0; unsigned slot = 0; } dwalk;
    bool defer_walk = true;             // (debug knob "defer_walk")
    // what the LAST sharded step's exchange and the LAST all-gather moved on this rank, in bytes (gem_debug_get "step_exchange_bytes_out" / "_in",
    // "gather_bytes_out" / "_in"; bench.py --gpus N prices them against the xGMI links)
    long long xbytes_out = 0, xbytes_in = 0, gbytes_out = 0, gbytes_in = 0;
    bool roctx = false;                             // roctx ranges around the entry points (gem_debug_set "roctx"; ApiRange)
    bool walk_always_wait = false;                  // a walk left to the next call waits for its sort's event even when the host has seen it complete (flush_walk)
    long long walks_unwaited = 0, walks_left = 0;   // walks left to the next call (gem_debug_get "walks_left"); of those, launched without a stream wait ("walks_unwaited")
    bool defer = true;
    hipStream_t bin_stream = nullptr;
    hipStream_t bin_stream2 = nullptr;  // the sorted pipeline sorts consecutive big passes on two streams (see run_sort_pipeline)
    hipStream_t tab_stream = nullptr;   // uploads a batched pass's tables while the binning stream is still busy with the pass before
    hipEvent_t switch_done = nullptr;   // recorded on `stream` when a pass moves its binning to `bin_stream` after passes that did not
    bool main_reads_pb = false;         // work enqueued on `stream` since the last such switch reads the pass buffers
    bool overlap = true;
    long long overlap_min_points = 1000000;        // tile pipeline: a cross-stream event pair costs 3 us, the second stream only pays for big passes
    long long sort_overlap_min_points = 100000;    // sorted pipeline: its walk is a few long chains on a mostly idle chip; the next pass's sort fits beside it (depth image 120 -> 83 us)
    bool sort_path = true;              // passes of at least sort_min_points points run the sorted pipeline (gem_sort.hip)
    // single cloud / batch of sweeps (tools/dbg/crossover.py).  Batches: block-sorted from three LiDAR sweeps on (393 k points: 43 us
    // against the tile pipeline's 46; four sweeps 43 / 56, two 46 / 35); single clouds: a 131 k-point LiDAR sweep takes 10 us on
    // the tile pipeline and 35 sorted, a 150 k-point depth image 60 and 38
    long long sort_min_points = 200000, sort_min_points_batch = 390000;
    bool walk_permute = true;           // k_fuse_walk: blocks take the tile rows centre-first
    int  sort_passes = 0;               // 0 = by map size and form (sort_geometry); 1 / 2 / 3 force it
    int few_bins = 0;                   // k_sort_scatter's ballots per wave instruction before the LDS way (0 = the built-in 8; debug knob)
    int blk_batch = 0;                  // k_fuse_block's round: 0 = by the pass's mean block load, 512 / 2048 forced (debug knob)
    int ray_depth = 4, ray_lanes = 16;  // k_raytracing: loads in flight per lane, lanes per ray (debug knobs; 16 x 4 measured best on C2)
    bool fast_laser = true;             // frames that qualify use the zero-rotation-variance form of the laser variance (fill_frame; debug knob)
    bool rank_by_ballot = false;        // k_sort_scatter ranks by ballot in every pass (debug knob)
    bool lane_sort = true;              // k_fuse_block: cells to threads by record count (debug knob)
    bool ride_events = true;            // the sort's last dispatch carries the event the walk waits for (no marker behind it)
    int  walk_lds_pad = 0;              // k_fuse_block: extra dynamic LDS per workgroup (debug knob: fewer workgroups per CU)
    int  walk_prio = 4096;              // k_fuse_block: blocks of at least this many records run at raised issue priority (debug knob, 0 = off)
    int  fuse_count = 1;                // pass 2's counts from pass 1's scatter (SortArgs::fuse_count): 0 = never, 1 = passes of up to kFuseCountMaxPoints points, 2 = always (debug knob)
    int  sort_chunk = 0;                // records per counting-sort chunk: 0 = by the pass's size (sort_chunk_for), 1024 / 4096 forced (debug knob)
    bool light_fast = true;             // k_fuse_block's light rounds by arrival slots + sorting network (debug knob)
    bool cache_tables = true;           // batched calls: skip building / uploading tables equal to the ones the buffer set already holds (debug knob)
    std::vector<unsigned char> key_scratch;
    bool plain_loop = true;             // the walks' plain chain loop for blocks whose values are in range (debug knob: 0 = the guarded loop everywhere)
    int  sort_form = 0;                 // 0 = batches of sweeps BLOCK-sorted (k_fuse_block), single clouds CELL-sorted (k_fuse_walk); 1 / 2 force cell / block
    int dbg_sweep = 0;                  // debug stamps of the dense path: which sweep (GEM_DBG_SWEEP)
    bool track_lowest = false;          // also maintain map_lowest in the fuse kernels (gem_set_lowest_tracking, for gem_raytracing)
    unsigned dense_min = 2048;          // records of one sweep in one 16x16 tile above which the tile is counting-sorted (k_fuse_list, dense path)
    Arena scratch;      // layer export
    unsigned long long* d_counters = nullptr;

    float pending[kMaxPending] = {0, 0, 0, 0};
    int   n_pending = 0;
    bool  floor_dirty = true;          // some cell may hold variance < floor (init / clear / set_layer)

    bool  timing = false, counting = false;
    std::vector<EventPair> events;     // recorded, not yet folded
    std::vector<EventPair> pool;
    gem_stats stats{};
    hipEvent_t copy_done = nullptr;

    // ---- caller-owned pageable arrays (gem_hostcopy.hpp): the handle's pinned staging buffer, the DMA between it and the device,
    //      a few threads between it and the caller's arrays.  copy_threads 0 = the runtime's own pageable path.
    static constexpr int kStageEvents = 24;
    void*  hstage = nullptr;            // hipHostMalloc'ed
    size_t hstage_cap = 0;
    bool   hstage_failed = false;       // an allocation failed: not tried again
    size_t hstage_max = 256u << 20;     // larger transfers go through the runtime
    int    copy_threads = 4;            // the calling thread + 3 workers (gem_debug_set "copy_threads")
    int    download_groups = 8;         // pieces a download is cut into: the device writes piece g + 1 into the staging buffer while the copy threads move piece g on (gem_debug_set "download_groups")
    hipEvent_t ev_stage[kStageEvents] = {};      // host-visible: a segment's DMA into the staging buffer is done
    hipEvent_t stage_read = nullptr;    // the last DMA OUT of the staging buffer is done (it may be written again)
    bool   stage_read_pending = false;
    // deferred uploads (gem_add, gem_add_batch): the call returns once the caller's arrays have been READ into one half of the staging
    // buffer and the DMA out of it is enqueued; the next call fills the other half meanwhile.  A half is reused when the DMA that read
    // it two calls ago is done.
    hipEvent_t ev_half[2] = {nullptr, nullptr};
    bool   half_pending[2] = {false, false};
    unsigned stage_par = 0;
    long long hstage_allocations = 0;
    long long xfer_ns[5] = {0, 0, 0, 0, 0};    // host time so far: upload memcpy, upload enqueue, download enqueue, download wait, download memcpy

    // ---- multi-GPU.  Two communicators, each with a stream of its own: `tp_x` carries a step's boundary
    //      all-gather and record exchange on `comm_stream`, `tp_g` the all-gather of the fused layers on `gather_stream` -- step
    //      p + 1's exchange does not queue behind step p's 46 MB of layers.  (RCCL over xGMI; W handles of one process on one
    //      device through the loopback of gem_transport.hpp in the tests.)
    std::unique_ptr<Transport> tp_x, tp_g;
    int nranks = 1, rank = 0;
    int strip_row[kMaxRanks + 1] = {0};  // storage rows [strip_row[k], strip_row[k+1]) belong to rank k (gem_comm_init / gem_comm_init_tiles)
    bool tile_strips = false;           // strips are whole rows of 32x32 tiles (needed by the sharded path)
    // points sharded (gem_shard_sort_device / gem_shard_fuse_device / gem_add_sharded_device)
    struct Shard {
        bool valid = false;
        const uint2* hv = nullptr; const uint32_t* key = nullptr;     // this device's sorted records
        const uint2* ranges = nullptr;                                 // [4 T] where every block's records are in them (k_block_prefix)
        uint32_t bounds[kMaxRanks + 1] = {0};                          // first record of every strip in them
        const uint32_t* d_bounds = nullptr;                            // ... on the device (16 words)
        int nstrips = 0, n_global_sweeps = 0;
        long long points = 0;                                          // points this device sorted for the step
        int slot = -1;                                                 // pass-buffer set the sort ran in on a binning stream (its bin_done / fuse_done events), -1: on the handle's stream
        hipStream_t stream = nullptr;                                  // the stream the sort was enqueued on
    } shard;
    // A step of gem_add_sharded_device whose SECOND HALF -- exchange, walk, all-gather of the layers if one was asked for -- is
    // still to come: the call returns once the step's sort and the all-gather of its strip boundaries are enqueued; the next call
    // (or whatever observes the map) finishes it.  That way the host never waits for a sort it has just enqueued: when it needs the
    // boundaries of step p, the sort of step p + 1 is already queued behind it (shard_finish_locked).
    struct Step {
        bool valid = false;
        int parity = 0;                                                // which of the two sets of staging / receive buffers
        int n_global_sweeps = 0;
        bool has_vu = false; float vu[512];
        Shard sd;
        bool gather = false; int gather_attrs = 0;                     // gem_allgather_layers was called behind it
    } step;
    unsigned step_seq = 0;                                             // steps begun so far (parity = step_seq & 1)
    Arena sh_dev, sh_ranges;                                           // ids / bounds / gathered bounds / variance increments (two sets); an empty shard's block ranges
    Arena sh_recv_hv[2], sh_recv_key[2], sh_recv_rng[2];               // records and block ranges received from the other ranks, one set per parity
    hipStream_t comm_stream = nullptr, gather_stream = nullptr;
    hipEvent_t ev_sorted = nullptr, ev_exchanged = nullptr;
    hipEvent_t ev_bounds[2] = {nullptr, nullptr};                      // the gathered boundaries of that parity are on the host
    hipEvent_t ev_walked[2] = {nullptr, nullptr};                      // the walk that read that parity's receive buffers is done
    bool walk_recorded[2] = {false, false};
    hipEvent_t ev_vu[2] = {nullptr, nullptr};                          // the upload of that variance-increment staging buffer is done
    bool vu_recorded[2] = {false, false};
    unsigned vu_seq = 0;
    // all-gather of the layers: sends read a PUBLISHED COPY of this rank's strip (two, rotating), receives write the other ranks' strips
    Arena published[2];
    hipEvent_t ev_published[2] = {nullptr, nullptr}, ev_gathered[2] = {nullptr, nullptr};
    bool gather_outstanding[2] = {false, false};                       // that gather has not been waited for by the handle's stream yet
    bool gathered_recorded[2] = {false, false};
    unsigned gather_seq = 0;
    long long recv_bound = 0;                                          // gem_reserve on a communicator handle: records a step may bring to this rank at most
    void* sh_host = nullptr;            // pinned staging of the small tables (kShardHostBytes)
    // optional time stamps of the last finished step's phases (gem_set_timing; gem_debug_get "step_*_ns")
    hipEvent_t ev_t[10] = {};
    bool step_timed = false;

    Arena dbg;          // optional k_fuse phase stamps
    Arena ray;          // gem_raytracing: the cells that walk, their number (two counters in turn), the snapshot of the lowest scan points
    unsigned ray_calls = 0;
    Arena color;        // gem_colorize: its own sort arrays and tables (never shared with a pass in flight on the binning stream)
    Arena clean_cnt;    // the compactions' per-workgroup counts (gem_clean.hip; sized by gem_reserve)
    // the VoxelGrid pre-filter (gem_voxel_*, gem_capi_voxel.cpp; kernels in gem_voxel.hip), all sized by gem_reserve
    Arena vox_state, vox_hist;          // VoxState and the two digit histograms: all-zero between stages (zeroed when allocated)
    Arena vox_rec, vox_tmp;             // the records of the sort passes | a chain's two intermediate clouds
    Arena vox_out[2];                   // gem_add_voxel*: the filtered cloud, the two in turn (vox_flip)
    unsigned vox_flip = 0;
    // the rolling-window local map (gem_local_*, gem_capi_local.cpp; kernels in gem_local.hip)
    struct Local {
        bool enabled = false;
        struct Capture { Arena rec, lin; double off = 0, res = 0, px = 0, py = 0; int sx = 0, sy = 0; } slot[2];
        int cur = -1, prev = -1;        // the slot the last capture wrote / the slot keep_previous kept (-1: none)
        Arena log[2];                   // the log of upserts and its compaction target, in turn (`act` is the log)
        int act = 0;
        Arena keys, vals;               // the open-addressing table: key -> log position
        Arena spill_cnt, exp_cnt;       // per-workgroup counts of the spill / capture and of the export compactions
        Arena small;                    // device words: capture counts [2] | spill total | export total | new keys
        long long log_cap = 0, log_len = 0, table_cap = 0, live = 0;
    } local;
    // composingGlobalMap's outlier filter and road / obstacle split on the previous capture (gem_local_compose*, gem_capi_compose.cpp;
    // kernels in gem_compose.hip): part of the local map, freed with it
    struct Compose {
        Arena grid, dist, far;          // [cells] record index per unwrapped cell | mean neighbour distance per record | the far list
        Arena road, obstacle;           // [cells] records each: the two compactions
        Arena cnt;                      // per-workgroup counts of the three classes
        Arena small;                    // device words: far count | totals [3]
        std::vector<float> host_dist;   // the distances on the host: the ordered double sums of the threshold are taken there
        long long far_points = 0;       // records the last call left to k_compose_knn_far (gem_debug_get "compose_far_points")
        long long sum_ns = 0;           // host time the last call spent on the ordered double sums ("compose_sum_ns")
    } compose;
    // the submap stack of updateGlobalMap (gem_global_*, gem_capi_global.cpp; kernels in gem_global.hip)
    struct Global {
        bool enabled = false;
        Arena stack[2];                 // the records of every submap, one arena in use (`act`), the other the target when it grows
        int act = 0;
        long long cap = 0, used = 0;    // records the active arena holds / records up to the end of the last submap's room
        std::vector<long long> off, room, cnt;      // per submap: first record, records it may hold, records it holds
        Arena cnts;                     // per submap record counts on the device, read by a loop closure's kernels
        Arena out[2], keys[2], tkeys[2], tvals[2], blk[2];  // a pair step's sides (0 = old, 1 = new): output, keys, table, counts
        Arena small;                    // device words: the sides' totals [2] | fused keys | the local map's export total
    } global;
    // the costmap layers (gem_costmap_*, gem_capi_costmap.cpp; kernels in gem_costmap.hip)
    struct Costmaps {
        static constexpr int kMax = 8;  // a few per handle: a local one, a global one, a master
        struct Map {
            bool used = false;
            gem_costmap_config cfg{};   // the origin is the one after the last roll
            Arena grid[2];              // the byte grid (`act`) and the target of the next roll
            int act = 0;
            Arena stamps;               // a word per cell (padded to four): the verdict of a mark in flight, all-zero between calls
            Arena infl_table;           // gem_costmap_inflate's cost table on the device, made for infl_key at this resolution
            gem_inflation_params infl_key{};
            bool infl_valid = false;
            Arena mg_dist[3];           // gem_costmap_mapgrid_prepare's / _prepare_front's grids (gem_capi_mapgrid.cpp): path | goal | front, an int per cell
            Arena mg_status;            // per grid four ints: started, goal cell x, y, levels
            Arena mg_act;               // gem_costmap_mapgrid_prepare_tiled: per requested grid (at most two) the tiles' two active maps
            unsigned long long gen = 0; // the costmap's generation: new at create, at every roll that moves it and at every gem_costmap_observe*
            unsigned long long mg_gen[3] = {0, 0, 0};   // the generation each grid was prepared in (0: never)
            // gem_costmap_navplan (gem_capi_navplan.cpp): the potential, an int per cell | the tiles' two active maps | the path, an int
            // per cell, written from the end | the status words
            Arena nav_pot, nav_act, nav_path, nav_status;
            unsigned long long nav_gen = 0;             // the generation the last plan ran in (0: never)
            int nav_n_path = 0;                         // its path's cells
            gem_navplan_status nav_last{};              // ... and its status (gem_costmap_navplan_status)
            // gem_costmap_navplan_paths (gem_capi_navpath.cpp): the goals' cells, two ints per goal | the waiting form's results and points
            Arena np_goal, np_res, np_pts;
            // gem_costmap_frontiers (gem_capi_frontier.cpp): the labels, an int per cell | each root's list index at the root's cell,
            // an int per cell, never cleared | the tiles' two active maps | the records, field by field, one per possible component |
            // the kept list (gem_frontier) | the device words
            Arena fr_label, fr_index, fr_act, fr_rec, fr_out, fr_words;
            unsigned long long fr_gen = 0;              // the generation the last search ran in (0: never, or a plan was made since)
            int fr_n_kept = 0;                          // its kept list's length
            // gem_costmap_voxels_create (gem_capi_voxlayer.cpp): a 32-bit voxel column per cell (`vox_act`) and the target of the next
            // roll, as the byte grids
            bool has_vox = false;
            gem_voxel_config vox_cfg{};
            Arena vox[2];
            int vox_act = 0;
        } map[kMax];
        unsigned long long generation = 0;      // the last generation handed out
        Arena small;                    // device words (64-bit): the bounds keys a mark accumulates [4] | the ones its resolve pass published [4]
        Arena in, win;                  // a host cloud of gem_costmap_mark_points | the packed window of gem_costmap_read / _write
        std::vector<unsigned char> host_rows;   // that window on the host when the caller's row stride is wider
        Arena infl_bits, infl_flags;            // gem_costmap_inflate (gem_capi_inflate.cpp): the seed words of the widened window | a flag per block of them
        // gem_costmap_mapgrid_* (gem_capi_mapgrid.cpp): the plan's cells in pinned host memory, two buffers taking turns, each with the
        // event behind the launch that reads it | the host-array forms' poses and results | the adjusted plan on the host
        void* mg_pin[2] = {nullptr, nullptr};
        size_t mg_pin_cap[2] = {0, 0};
        hipEvent_t mg_ev[2] = {nullptr, nullptr};
        bool mg_ev_pending[2] = {false, false};
        unsigned mg_turn = 0;
        Arena mg_pose, mg_traj;
        std::vector<double> mg_plan;
        void* mgt_pin = nullptr;        // gem_costmap_mapgrid_prepare_tiled: the pinned words its kernels answer through (the call waits: one block serves every costmap)
        // gem_costmap_navplan: the weight table on the device | pinned host memory, the table a call hands over and the status words its
        // kernels answer with (the call waits, so one block serves every costmap) | the path's cells on the host
        Arena nav_w;
        void* nav_pin = nullptr;
        std::vector<int> nav_cells;
        std::vector<int> np_cells;      // gem_costmap_navplan_paths: the goals' cells on the host
        // gem_costmap_frontiers: the compaction's block counts and total | pinned host memory its kernels answer through (the call
        // waits, so one block serves every costmap)
        Arena fr_blocks;
        void* fr_pin = nullptr;
        // gem_costmap_best_trajectory* (gem_capi_critics.cpp): the first pass's candidates | the host-array form's poses, lengths, external
        // columns, totals and the 32-byte result
        Arena cr_cand, cr_pose, cr_len, cr_ext, cr_total, cr_best;
        Arena tg_pose, tg_len, tg_ext;          // gem_costmap_dwa_best* (gem_capi_trajgen.cpp): the generated poses, lengths and the two external columns
        Arena ro_cost, ro_ahead, ro_best;       // gem_costmap_rollout_best* (gem_capi_rollout.cpp): the candidates' costs and `ahead`, the 64-byte answer
        // gem_costmap_observe* (gem_capi_obstacle.cpp): the end-cell and mark bitmaps, all-zero between calls | the ray list | the
        // compaction's block counts and total
        Arena ob_bits, ob_rays, ob_cnt;
        // gem_costmap_voxel_observe* (gem_capi_voxlayer.cpp): the new-marks word and the touched byte per cell, all-zero between calls |
        // the ray list, 64 bits per record
        Arena vx_marks, vx_touched, vx_rays;
        Arena fp_pose, fp_cost, fp_traj;        // the host-array forms of gem_costmap_footprint_cost / _score_trajectories (gem_capi_footprint.cpp): poses | pose costs | trajectory costs
    } costmap;
    // the history cloud (gem_history_*, gem_capi_history.cpp; the box table's kernel in gem_history.hip): visualCloud_ of ElevationMapping
    struct History {
        bool enabled = false;
        Arena log[2];                   // the records in history order, one arena in use (`act`), the other the target when it grows
        int act = 0;
        long long len = 0, cap = 0;     // records the log holds / records the active arena has room for
        Arena box;                      // four floats per block of kCostChunk records (gem_history.hpp)
        long long box_cap = 0;          // blocks the table has room for
        Arena small;                    // device words: workgroups the last gem_costmap_mark_history culled
    } history;
    int  nav_chunk = 0;                 // debug knob "nav_chunk": rounds gem_costmap_navplan enqueues per host round trip (0 = tiles_x + tiles_y)
    int  navquad_passes = 0;            // debug knob "navquad_passes": in-tile passes a round of gem_costmap_navplan_quadratic allows a tile (0 = kNavQuadPasses)
    int  front_chunk = 0;               // debug knob "front_chunk": label rounds gem_costmap_frontiers enqueues per host round trip (0 = tiles_x + tiles_y)
    int  mapgrid_chunk = 0;             // debug knob "mapgrid_chunk": rounds gem_costmap_mapgrid_prepare_tiled enqueues per host round trip (0 = tiles_x + tiles_y)
    bool obstacle_direct = true;       // debug knob "obstacle_direct": gem_costmap_observe* walks a ray per accepted record (the default: measured faster) or one per distinct end cell
    bool history_cull = true;          // debug knob "history_cull": gem_costmap_mark_history hands the box table to its kernel
    // pointCloudtoOctomap's insertion loop and fullMapToMsg (gem_octree_*, gem_capi_octree.cpp; kernels in gem_octree.hip)
    struct Octree {
        static constexpr int kSlots = 4;
        Arena state, hist;              // OctState and the two digit histograms: kept between builds as the kernels leave them
        bool dirty = false;             // a build did not run to its end: both are set again before the next one
        Arena tab;                      // value (float) and blend p (double) per hit count
        double tab_key[3] = {-1, -1, -1};   // the probabilities the device tables were built from
        Arena in, work;                 // a host cloud of gem_octree_build | everything sized by the call's n (gem_capi_octree.cpp carves it)
        struct Slot {
            Arena out;                  // the stream
            long long bytes = 0;
            gem_octree_stats stats{};
        } slot[kSlots];
    } octree;
    bool  dbg_on = false;
    bool  dbg_frame = false;            // debug knob: with the stamps on, a stream of single sweeps still runs as k_frame (its tiles AND its binning blocks are stamped)
    long long sort_fallbacks = 0;      // passes whose forced sorted form / pass count did not fit the map and took the other form (gem_debug_get)
    long long arena_allocations = 0;   // hipMalloc calls of ensure() so far (gem_debug_get: a stream of frames after gem_reserve must not add any)
    int   dbg_rows = 0;  // rows of `dbg` the last pass wrote, if it was a block-sorted one (else h->T rows)
    int fuse_variant = 12;
};

namespace gemi {

int fail(gem_handle* h, int code, const char* what, hipError_t e = hipSuccess);

// Optional roctx ranges around the entry points (tracing): off by default and free when off (one load of a flag);
// gem_debug_set(h, "roctx", 1) resolves roctxRangePushA / roctxRangePop from the ROCm marker library at run time (the library does
// not link against it) -- `rocprofv3 --kernel-trace --marker-trace` then shows which call enqueued which kernels.
bool roctx_load();                                   // true when the marker library was found (process-wide, once)
void roctx_push(const char* name);
void roctx_pop();
struct ApiRange {
    bool on;
    ApiRange(const gem_handle* h, const char* name);
    ~ApiRange() { if (on) roctx_pop(); }
};

#define GEM_HIP(h, call)                                                        \
    do { hipError_t _e = (call); if (_e != hipSuccess) return fail(h, GEM_ERR_HIP, #call, _e); } while (0)

// The prelude of an entry point that takes the handle's lock for the whole call: the optional roctx range, the NULL handle, the lock,
// the handle's device.  Nothing else belongs here; an entry point that needs an `rc` declares it.
#define GEM_ENTRY(name)                                                         \
    ApiRange api_range(h, name);                                                \
    if (!h) return GEM_ERR_INVALID;                                             \
    std::lock_guard<std::mutex> lk(h->mu);                                      \
    hipSetDevice(h->device)

// ... inside a multi-rank step, between its collectives: a rank that fails there takes the communicators down with it, so that the
// peers' pending receives fail instead of waiting for it (step_abort)
int step_abort(gem_handle* h, int rc);
#define GEM_HIP_STEP(h, call)                                                   \
    do { hipError_t _e = (call); if (_e != hipSuccess) return step_abort(h, fail(h, GEM_ERR_HIP, #call, _e)); } while (0)

int ensure(gem_handle* h, Arena& a, size_t bytes);
int ensure_zeroed(gem_handle* h, Arena& a, size_t bytes);
int ensure_ray(gem_handle* h);                  // gem_capi.cpp: gem_raytracing's arena

struct HostXfer { void* host; void* dev; size_t bytes; };

inline long long host_ns()
{
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

unsigned char* host_stage(gem_handle* h, size_t bytes);
int drain_staging(gem_handle* h);
int upload_arrays(gem_handle* h, const HostXfer* x, int n, bool defer_ok = false, unsigned char** zero_copy_region = nullptr, int* zero_copy_half = nullptr);
int download_arrays(gem_handle* h, const HostXfer* x, int n, size_t stage_off);

// A host cloud of the add entries in h->stage, at the stride upload_arrays gives a half of the staging buffer: XYZI at 0, then rgb,
// then orig, each present array 256-byte aligned behind the one before; `bytes` covers them all
struct CloudLayout { size_t rgb, orig, bytes; };
CloudLayout cloud_layout(long long n, bool rgb, bool orig);
// ... staged by a deferred upload: what the kernels read (the zero-copy half of the pinned staging buffer or the arena), the arena's
// own XYZI slot (where a mask or a filter may write) and the half it holds (-1: none, release_half then does nothing)
struct StagedCloud {
    const float4* xyzi = nullptr; const uint32_t* rgb = nullptr; const int* orig = nullptr;
    float4* arena_xyzi = nullptr;
    int half = -1;
};
int stage_cloud(gem_handle* h, long long n, const float* xyzi, const uint32_t* rgb, const int* orig, StagedCloud& out);
// a held half is handed back behind everything enqueued on h->stream, the pass that read it included -- whether or not the call
// failed: returns rc, or the record's failure if rc is GEM_OK
int release_half(gem_handle* h, int half, int rc);
float to_float_rn(double v);                   // double -> float, round to nearest even, +-inf beyond FLT_MAX (defined for every double)

void fill_frame(const gem_handle* h, const gem_frame_params* p, FrameConst& f);
hipEvent_t get_event(gem_handle* h);

// Optional per-kernel timing: the dispatch is time-stamped through a (start, stop) event pair
// handed to hipExtLaunchKernelGGL, so the figure is the kernel's own duration on its stream.
struct Timed {
    gem_handle* h; EventPair ep{};
    bool on;
    Timed(gem_handle* hh, int kind) : h(hh), on(hh->timing && kind >= 0)
    {
        if (!on) return;
        if (!h->pool.empty()) { ep = h->pool.back(); h->pool.pop_back(); }
        else { ep.a = get_event(h); ep.b = get_event(h); }
        ep.kind = kind;
    }
    LaunchEvents events() const { LaunchEvents e; if (on) { e.start = ep.a; e.stop = ep.b; } return e; }
    ~Timed() { if (on) h->events.push_back(ep); }
};

void fold_events(gem_handle* h);
int flush_deferred(gem_handle* h);
bool frame_would_lean(const gem_handle* h);                              // ... the knob and the pinned word alone: what a launch of lean-binned, fast-laser sweeps would pick now
bool frame_launch_lean(gem_handle* h, bool fused_lean, bool bin_fast, int sweeps = 1);   // the host's pick of k_frame's form for the next launch (gem_handle::form_seen)
// One k_frame launch: fuses every deferred sweep of the handle, oldest first, beside the binning of bins[0 .. nb), which are the
// deferred ones behind it (nb == 0: the fuse-only launch).  Two sweeps in either half: the pair kernel, or -- the launch is not
// lean -- the single generic launches it stands for.
int frame_launch(gem_handle* h, gem_handle::FrameSweep* const* bins, int nb);
int frame_unpair(gem_handle* h);                                        // a call that may not share a launch: a held sweep or a deferred pair is settled first
int flush_walk(gem_handle* h);
int flush_local(gem_handle* h);
int wait_gather(gem_handle* h);
void local_free(gem_handle* h);                 // gem_capi_local.cpp: the local map's arenas (gem_destroy, gem_local_enable(0))
// gem_capi_local.cpp, for gem_global_push_local: the record count of the last capture (downloaded; GEM_ERR_INVALID without one), and
// the local map's export followed by that capture's grid cloud written to dst (device), the map emptied afterwards with clear
int local_grid_count(gem_handle* h, uint32_t* n);
int local_export_to(gem_handle* h, void* dst, uint32_t n_grid, bool clear);
void compose_free(gem_handle* h);               // gem_capi_compose.cpp: the compose arenas (local_free)
// gem_capi_compose.cpp, for gem_local_compose_octrees: gem_local_compose's argument checks, and its filter and split with the two
// lists left in Compose::road / Compose::obstacle on the device; tot[3]: road, obstacle, removed
int compose_check(gem_handle* h, const gem_compose_params* p, const char* what);
int compose_split(gem_handle* h, const gem_compose_params* p, bool want_road, bool want_obstacle, uint32_t tot[3], double* out_threshold);
void octree_free(gem_handle* h);                // gem_capi_octree.cpp: the octree builder's arenas and the slots' streams (gem_destroy)
void global_free(gem_handle* h);                // gem_capi_global.cpp: the submap stack's arenas (gem_destroy, gem_global_enable(0))
void history_free(gem_handle* h);               // gem_capi_history.cpp: the history cloud's arenas (gem_destroy, gem_history_enable(0))
// gem_capi_history.cpp, for gem_local_spill: whether n more records fit the stamp limit of a mark (GEM_ERR_INVALID otherwise), room for
// them (the only step that allocates), and n records at d_src (device) appended on h->stream with their blocks' boxes recomputed
int history_check_room(gem_handle* h, long long n, const char* what);
int history_reserve(gem_handle* h, long long extra);
int history_append_device(gem_handle* h, const void* d_src, long long n);
int history_blocks_culled(gem_handle* h, long long* out);      // the last gem_costmap_mark_history's count, downloaded
// gem_capi_critics.cpp, for gem_costmap_dwa_best (gem_capi_trajgen.cpp): a best-trajectory call as its entry points describe it, and
// its checks (GEM_ERR_INVALID, nothing enqueued), the candidates' arena and the kernel's argument block with everything but the
// arrays.  own_arrays: poses, traj_len and ext are arenas of the handle that the caller binds afterwards (they may be NULL here).
struct CriticsCall {
    const char* what;
    const gem_critic* critics;
    int n_critics;
    const gem_footprint_pose* poses;
    const int* traj_len;
    long long n_traj;
    int T;
    const double* spec_xy;
    int n_vertices;
    const double* ext;
    int n_ext;
    double* out_total;
    gem_best_trajectory* out_best;
    bool on_device;
    bool own_arrays = false;
};
int critics_prepare(gem_handle* h, int id, const CriticsCall& c, gem::CriticsArgs& a, gem::FootSpec& spec, gem::CostGeom& geom);
void costmap_free(gem_handle* h);               // gem_capi_costmap.cpp: every costmap of the handle and their shared arenas (gem_destroy)
int voxel_reserve(gem_handle* h, long long max_points);   // gem_capi_voxel.cpp: the voxel arenas of a call of max_points points
int settle(gem_handle* h);
int flush_pending(gem_handle* h, bool with_floor);
int index_to_range(int index, int L);          // gpu_process.cu:914-919

// One pipeline pass over up to `n` points that are already on the device.
struct PassInput {
    int src = 0;                       // 0 = XYZI cloud, 1 = Fuse() arrays
    bool device_input = false;         // the caller's device buffers are read directly (no staging copy)
    bool caller_device = false;        // ... and they ARE the caller's (gem_add_device, gem_add_batch_device: untouched until gem_synchronize by contract), not an arena or a staging half of the handle that the next call refills
    int n_sweeps = 1;
    long long n = 0;
    const gem_frame_params* params = nullptr;      // [n_sweeps] (src 0)
    const long long* offsets = nullptr;            // [n_sweeps+1] (batched)
    const float* var_updates = nullptr;            // [n_sweeps]  (batched, host)
    const int* sweep_orig0 = nullptr;              // [n_sweeps]  (batched, host, optional) index inside its sweep of each sweep's first point here
    const float4* xyzi = nullptr; const uint32_t* rgb = nullptr; const int* orig = nullptr;
    const int* f_index = nullptr; const float* f_height = nullptr; const float* f_var = nullptr;
    const int* f_R = nullptr; const int* f_G = nullptr; const int* f_B = nullptr; const float* f_I = nullptr;
};

// Events between the handle's OWN streams on its own device (a pass's sort -> its walk, a walk -> the sort that reuses its buffers)
// carry no system-scope fence: the kernel boundary already writes the producer's L2 lines back for the consumer's XCDs, and
// nothing on the host or on another device reads data behind them (round 4: C3 -1.8 us, C4 -2.2 us per call).  Whatever a PEER
// device or the host reads -- the record exchange and the all-gathers of the multi-rank step -- is ordered by events WITH the
// fence (ev_sorted and the other step events, comm_attach), never by these.
constexpr unsigned  kDeviceEventFlags = hipEventDisableTiming | hipEventDisableSystemFence;

hipError_t acquire_streams(int device, StreamSet& out);
void release_streams(int device, const StreamSet& set);
hipError_t acquire_comm_stream(int device, hipStream_t* out);
void release_comm_stream(int device, hipStream_t st);

// gem_capi_pipeline.cpp: the plans (gem_plan.hpp) of this handle
PlanEnv plan_env(const gem_handle* h);
SortGeometry sort_geometry(const gem_handle* h, int n_sweeps, bool block_form);      // sort_digits for this map, the kernels' LDS checked
// the sort kernels' pointers into buffers of a plan's sizes: arrays 1 / 2, the two count tables, the carved s_misc
struct SortBuffers { void *hv1, *hv2, *key1, *key2, *src1, *src2, *cnt1, *cnt2, *misc; };
void bind_sort_buffers(const SortPlan& p, int n_passes, const SortBuffers& b, SortArgs& sa);

// pinned host staging of the sharded path: per parity (4096 B each) strip ids at word 0, own bounds at word 32, the gathered bounds
// [W][16] at word 64; the variance increments' two buffers at byte 8192 + 2048 b.  The device twin has the same layout.
constexpr size_t kShardHostBytes = 8192 + 2 * 2048, kShardDevBytes = 8192 + 2 * 2048;
struct ShardOpts { int sweep_id0; int nstrips; const int* strip_rows; bool bounds_stay_on_device; };   // sort only: the walk happens on the strip owners

int run_sort_pipeline(gem_handle* h, const PassInput& in, int attr, const SortGeometry& geo, const ShardOpts* shard = nullptr);
int run_pipeline(gem_handle* h, const PassInput& in0);

// The add entries (gem_add*, gem_add_raw*, gem_add_voxel*, gem_add_aos*, gem_add_depth*) as one body (gem_capi.cpp): a cloud from one
// of four sources, one of three front ends between it and the pass
enum class AddSource { host, device, aos, depth };     // XYZI (+ rgb, + orig) in host arrays | in device buffers | host point structs | a depth image (+ colour image)
enum class FrontEnd { none, clean, voxel };     // the pass reads the cloud | a copy with the dropped points' x, y, z NaN | the centroids
struct DepthSource {             // a checked gem_depth_image (gem_capi_depth.cpp: depth_source): strides filled in, constants computed
    gem_depth_image img;
    float k[4], unit;            // kx, ky, cxf, cyf | metres per count
    bool on_device;              // the images are in device memory (gem_add_depth_device), else in the caller's host memory
};
struct AddCloud {
    AddSource source;
    int n;
    const void* xyzi; const void* rgb = nullptr; const void* orig = nullptr;                  // aos: xyzi = the point structs
    int point_step = 0, off_x = 0, off_y = 0, off_z = 0, off_intensity = -1, off_rgb = -1;   // aos
    const DepthSource* image = nullptr;             // depth: xyzi = the depth image, rgb = the colour image or NULL, n = width * height
};
struct AddFront {
    FrontEnd kind = FrontEnd::none;
    const gem_clean_params* clean = nullptr;                        // clean: PASSTHROUGH_Z
    const gem_voxel_params* stages = nullptr; int n_stages = 0;     // voxel
};
int add_cloud(gem_handle* h, const gem_frame_params* p, const AddCloud& c, const AddFront& fe);     // (arguments checked, h->mu held)
bool aos_fields_ok(int point_step, int off_x, int off_y, int off_z, int off_intensity, int off_rgb);
// gem_capi_voxel.cpp: the stages of a gem_add_voxel* call into vox_out[vox_flip], which flips: the n filtered points (NaN tail)
int voxel_front(gem_handle* h, const gem_voxel_params* stages, int ns, int n, const float4* xyzi, const uint32_t* rgb,
                const float4** out, const uint32_t** rgb_out);
bool voxel_stages_ok(const gem_voxel_params* stages, int ns);      // gem_capi_voxel.cpp: what the gem_add_voxel* entries accept
// gem_capi_depth.cpp: the unprojection of `s` (depth / colour as the kernel reads them: device-visible) into xyzi / rgb on h->stream,
// the PASSTHROUGH_Z mask of `clean` (may be NULL) folded in
int depth_unproject(gem_handle* h, const DepthSource& s, const void* depth, const void* color, const gem_clean_params* clean,
                    float4* xyzi, uint32_t* rgb);

// gem_capi_comm.cpp
int shard_finish_locked(gem_handle* h);       // the second half of a pending gem_add_sharded_device step
int ensure_recv(gem_handle* h, int parity, size_t records);
int ensure_shard_tables(gem_handle* h, size_t blocks = 0);     // the small tables' pinned block and device twin; blocks: an empty shard's block ranges too
size_t strip_blocks_of(const gem_handle* h, int p);
bool shard_sort_rotates(const gem_handle* h, long long n);
int shard_checks(gem_handle* h, int n_global_sweeps, SortGeometry* geo);

} // namespace gemi
