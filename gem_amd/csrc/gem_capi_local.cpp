// gem_capi_local.cpp -- the local-map entry points of include/gem_hip.h (ElevationMapping::updateLocalMap, EMg.cpp:609-767, and
// visualPointMap, :520-530).  The kernels are in gem_local.hip.
//
// State (gem_handle::Local):
//   two capture slots        records + linear indices of show's kept cells with the geometry of the call; a capture never writes the
//                            slot keep_previous kept, so keep_previous is an index assignment (prevMap_ = visualMap_ without a copy)
//   the log                  every upsert appended in call order (records of 32 bytes); two arenas in turn, the other one is the
//                            target of the compaction (the live entries in order) when the log is full, and of the export
//   the table                open addressing, key ((float) x, (float) y) -> log position of the key's last write; at most half full
// The entry count (`live`) is known on the host: a spill reads back how many keys its insert added.  Every device buffer comes from
// ensure(), so gem_debug_get("arena_allocations") counts it; the capacities only grow, so a frame loop that has reached its sizes
// allocates nothing.
#include "gem_capi_internal.hpp"
#include "gem_local.hpp"

#include <algorithm>

namespace {

constexpr size_t kRec = sizeof(LocalRecord);
// words of Local::small
constexpr int kWordCapture = 0, kWordSpill = 2, kWordExport = 3, kWordNewKeys = 4;

uint32_t* small_word(gem_handle* h, int w) { return static_cast<uint32_t*>(h->local.small.p) + w; }
LocalRecord* log_at(gem_handle* h, int which) { return static_cast<LocalRecord*>(h->local.log[which].p); }

LocalTable table_of(gem_handle* h)
{
    return LocalTable{static_cast<unsigned long long*>(h->local.keys.p), static_cast<int*>(h->local.vals.p),
                      (unsigned long long)h->local.table_cap - 1};
}

int usable(gem_handle* h, const char* what)
{
    if (h->tp_x) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": not on a handle with a communicator").c_str());
    if (!h->local.enabled) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": the local map is not enabled (gem_local_enable)").c_str());
    return GEM_OK;
}

int clear_table(gem_handle* h)
{
    GEM_HIP(h, hipMemsetAsync(h->local.keys.p, 0xff, (size_t)h->local.table_cap * 8, h->stream));
    GEM_HIP(h, hipMemsetAsync(h->local.vals.p, 0xff, (size_t)h->local.table_cap * 4, h->stream));
    return GEM_OK;
}

// table of `cap` slots (a power of two), then every log entry inserted again: the larger position of a key wins, the live one
int rebuild_table(gem_handle* h, long long cap)
{
    auto& lc = h->local;
    int rc;
    if ((rc = ensure(h, lc.keys, (size_t)cap * 8)) || (rc = ensure(h, lc.vals, (size_t)cap * 4))) return rc;
    lc.table_cap = cap;
    if ((rc = clear_table(h))) return rc;
    GEM_HIP(h, launch_local_insert(h->stream, log_at(h, lc.act), 0, lc.log_len, table_of(h), nullptr));
    return GEM_OK;
}

// both log arenas hold `cap` entries and the export counts cover them.  The active arena is empty or already that large (a spill
// grows the log by compacting it into the other arena first), so ensure() drops nothing that is still needed.
int size_logs(gem_handle* h, long long cap)
{
    auto& lc = h->local;
    int rc;
    if ((rc = ensure(h, lc.log[0], (size_t)cap * kRec)) || (rc = ensure(h, lc.log[1], (size_t)cap * kRec))) return rc;
    if ((rc = ensure(h, lc.exp_cnt, (size_t)compact_blocks(cap) * 4 + 64))) return rc;
    lc.log_cap = std::max(lc.log_cap, cap);
    return GEM_OK;
}

long long pow2_at_least(long long v)
{
    long long c = 64;
    while (c < v) c <<= 1;
    return c;
}

} // namespace

namespace gemi {

void local_free(gem_handle* h)
{
    auto& lc = h->local;
    if (h->stream) hipStreamSynchronize(h->stream);
    for (Arena* a : {&lc.slot[0].rec, &lc.slot[0].lin, &lc.slot[1].rec, &lc.slot[1].lin, &lc.log[0], &lc.log[1], &lc.keys, &lc.vals,
                     &lc.spill_cnt, &lc.exp_cnt, &lc.small}) {
        if (a->p) hipFree(a->p);
        a->p = nullptr; a->cap = 0;
    }
    lc = gem_handle::Local{};
    compose_free(h);
}

int local_grid_count(gem_handle* h, uint32_t* n)
{
    auto& lc = h->local;
    if (!lc.enabled || lc.cur < 0) return fail(h, GEM_ERR_INVALID, "the local map is not enabled or has no capture");
    int rc;
    HostXfer c{n, small_word(h, kWordCapture + lc.cur), 4};
    if ((rc = download_arrays(h, &c, 1, 0))) return rc;
    if (*n > (uint32_t)h->cells) return fail(h, GEM_ERR_HIP, "local_grid_count: capture count out of range");
    return GEM_OK;
}

// gem_local_export's compaction straight into dst, then the capture's records behind it; the live count is checked on the host
int local_export_to(gem_handle* h, void* dst, uint32_t n_grid, bool clear)
{
    auto& lc = h->local;
    int rc;
    LocalRecord* out = static_cast<LocalRecord*>(dst);
    uint32_t n = 0;
    if (lc.live > 0) {
        LocalExportArgs e{log_at(h, lc.act), lc.log_len, table_of(h), out};
        GEM_HIP(h, launch_local_export(h->stream, e, static_cast<uint32_t*>(lc.exp_cnt.p), small_word(h, kWordExport)));
    }
    if (n_grid) GEM_HIP(h, hipMemcpyAsync(out + lc.live, lc.slot[lc.cur].rec.p, (size_t)n_grid * kRec, hipMemcpyDeviceToDevice, h->stream));
    if (lc.live > 0) {
        HostXfer c{&n, small_word(h, kWordExport), 4};
        if ((rc = download_arrays(h, &c, 1, 0))) return rc;
        if ((long long)n != lc.live) return fail(h, GEM_ERR_HIP, "local_export_to: live entry count mismatch");
    }
    if (clear) {                                                   // localMap_.swap(tmp)
        if ((rc = clear_table(h))) return rc;
        lc.log_len = lc.live = 0;
    }
    return GEM_OK;
}

} // namespace gemi

extern "C" {

int gem_local_enable(gem_handle* h, long long capacity)
{
    ApiRange api_range(h, "gem_local_enable");
    if (!h) return GEM_ERR_INVALID;
    if (capacity < 0 || capacity > (1ll << 30)) return fail(h, GEM_ERR_INVALID, "gem_local_enable: capacity out of range");
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    if (h->tp_x) return fail(h, GEM_ERR_INVALID, "gem_local_enable: not on a handle with a communicator");
    if (capacity == 0) { local_free(h); return GEM_OK; }
    auto& lc = h->local;
    int rc;
    if ((rc = ensure(h, lc.small, 64))) return rc;
    if ((rc = ensure(h, lc.spill_cnt, (size_t)compact_blocks(h->cells) * 4 + 64))) return rc;
    lc.cur = lc.prev = -1;
    lc.log_len = lc.live = 0;
    if ((rc = size_logs(h, std::max(lc.log_cap, capacity)))) return rc;
    if ((rc = rebuild_table(h, std::max(lc.table_cap, pow2_at_least(2 * lc.log_cap))))) return rc;
    lc.enabled = true;
    return GEM_OK;
}

int gem_local_capture(gem_handle* h, double map_length, double resolution, const double position[2])
{
    ApiRange api_range(h, "gem_local_capture");
    if (!h) return GEM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    int rc;
    if ((rc = usable(h, "gem_local_capture"))) return rc;
    if ((rc = flush_pending(h, false))) return rc;
    auto& lc = h->local;
    const int target = lc.prev == 0 ? 1 : 0;                   // never the slot keep_previous kept
    auto& s = lc.slot[target];
    if ((rc = ensure(h, s.rec, (size_t)h->cells * kRec)) || (rc = ensure(h, s.lin, (size_t)h->cells * 4))) return rc;
    const double res = resolution > 0.0 ? resolution : (double)h->res;           // gem_show's geometry rules
    const double len = map_length > 0.0 ? map_length : (double)h->L * res;
    s.res = res; s.off = 0.5 * len - 0.5 * res;
    s.px = position ? position[0] : (double)h->center[0];
    s.py = position ? position[1] : (double)h->center[1];
    s.sx = h->start[0]; s.sy = h->start[1];
    LocalCaptureArgs a{};
    a.m = h->layers;
    a.g = LocalGeom{s.off, s.res, s.px, s.py, h->L, s.sx, s.sy};
    a.rec = static_cast<LocalRecord*>(s.rec.p); a.lin = static_cast<int*>(s.lin.p);
    GEM_HIP(h, launch_local_capture(h->stream, a, static_cast<uint32_t*>(lc.spill_cnt.p), small_word(h, kWordCapture + target)));
    lc.cur = target;
    return GEM_OK;
}

int gem_local_keep_previous(gem_handle* h)
{
    ApiRange api_range(h, "gem_local_keep_previous");
    if (!h) return GEM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    int rc;
    if ((rc = usable(h, "gem_local_keep_previous"))) return rc;
    if (h->local.cur < 0) return fail(h, GEM_ERR_INVALID, "gem_local_keep_previous: no capture yet");
    h->local.prev = h->local.cur;
    return GEM_OK;
}

int gem_local_grid_cloud(gem_handle* h, void* points, int* out_count)
{
    ApiRange api_range(h, "gem_local_grid_cloud");
    if (!h) return GEM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    int rc;
    if ((rc = usable(h, "gem_local_grid_cloud"))) return rc;
    auto& lc = h->local;
    if (lc.cur < 0) return fail(h, GEM_ERR_INVALID, "gem_local_grid_cloud: no capture yet");
    uint32_t n = 0;
    HostXfer c{&n, small_word(h, kWordCapture + lc.cur), 4};
    if ((rc = download_arrays(h, &c, 1, 0))) return rc;
    if (n > (uint32_t)h->cells) return fail(h, GEM_ERR_HIP, "gem_local_grid_cloud: capture count out of range");
    if (points && n) {
        HostXfer d{points, lc.slot[lc.cur].rec.p, (size_t)n * kRec};
        if ((rc = download_arrays(h, &d, 1, 0))) return rc;
    }
    if (out_count) *out_count = (int)n;
    return GEM_OK;
}

int gem_local_spill(gem_handle* h, const float current_position[2], const float position_shift[2],
                    void* points, int* out_count, int* out_replaced)
{
    ApiRange api_range(h, "gem_local_spill");
    if (!h) return GEM_ERR_INVALID;
    if (!current_position || !position_shift) return fail(h, GEM_ERR_INVALID, "gem_local_spill: null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    int rc;
    if ((rc = usable(h, "gem_local_spill"))) return rc;
    auto& lc = h->local;
    if (lc.cur < 0) return fail(h, GEM_ERR_INVALID, "gem_local_spill: no capture yet");
    if (lc.prev < 0) return fail(h, GEM_ERR_INVALID, "gem_local_spill: no previous capture kept (gem_local_keep_previous)");
    const auto& pc = lc.slot[lc.prev];
    LocalSpillArgs a{};
    a.rec = static_cast<const LocalRecord*>(pc.rec.p); a.lin = static_cast<const int*>(pc.lin.p);
    a.count = small_word(h, kWordCapture + lc.prev);
    a.g = LocalGeom{pc.off, pc.res, pc.px, pc.py, h->L, pc.sx, pc.sy};
    const double half = h->L * pc.res / 2;                                         // length_ * resolution_ / 2 (EMg.cpp:726)
    a.lo_x = current_position[0] - half; a.hi_x = current_position[0] + half;      // float current_x promoted
    a.lo_y = current_position[1] - half; a.hi_y = current_position[1] + half;
    a.dx = position_shift[0]; a.dy = position_shift[1];
    uint32_t* cnt = static_cast<uint32_t*>(lc.spill_cnt.p);
    GEM_HIP(h, launch_local_spill(h->stream, a, h->cells, cnt, small_word(h, kWordSpill), false));
    uint32_t n = 0;
    { HostXfer c{&n, small_word(h, kWordSpill), 4}; if ((rc = download_arrays(h, &c, 1, 0))) return rc; }
    if (n > (uint32_t)h->cells) return fail(h, GEM_ERR_HIP, "gem_local_spill: spill count out of range");
    // the history cloud takes the same records (visualCloud_.push_back, EMg.cpp:750-760): its limit and its room before anything changes
    if (h->history.enabled && ((rc = history_check_room(h, n, "gem_local_spill")) || (rc = history_reserve(h, n)))) return rc;
    // room for n more entries: compact a full log (growing it when less than half of it would be free), keep the table at most half full
    bool rebuild = false;
    if (lc.log_len + n > lc.log_cap) {
        const long long need = lc.live + n;
        const long long cap = need > lc.log_cap / 2 ? std::max(2 * lc.log_cap, 2 * need) : lc.log_cap;
        if ((rc = ensure(h, lc.log[1 - lc.act], (size_t)cap * kRec))) return rc;
        if ((rc = ensure(h, lc.exp_cnt, (size_t)compact_blocks(std::max(cap, lc.log_len)) * 4 + 64))) return rc;
        LocalExportArgs e{log_at(h, lc.act), lc.log_len, table_of(h), log_at(h, 1 - lc.act)};
        GEM_HIP(h, launch_local_export(h->stream, e, static_cast<uint32_t*>(lc.exp_cnt.p), small_word(h, kWordExport)));
        lc.act = 1 - lc.act;
        lc.log_len = lc.live;
        if ((rc = size_logs(h, cap))) return rc;
        rebuild = true;
    }
    long long tcap = lc.table_cap;
    if (2 * (lc.live + n) > tcap) { tcap = pow2_at_least(4 * (lc.live + n)); rebuild = true; }
    if (rebuild && (rc = rebuild_table(h, tcap))) return rc;
    a.out = log_at(h, lc.act) + lc.log_len;
    GEM_HIP(h, launch_local_spill(h->stream, a, h->cells, cnt, small_word(h, kWordSpill), true));
    if (h->history.enabled && (rc = history_append_device(h, a.out, n))) return rc;     // from the log, before anything can compact it
    GEM_HIP(h, hipMemsetAsync(small_word(h, kWordNewKeys), 0, 4, h->stream));
    GEM_HIP(h, launch_local_insert(h->stream, log_at(h, lc.act), lc.log_len, n, table_of(h), small_word(h, kWordNewKeys)));
    uint32_t added = 0;
    HostXfer d[2] = {{&added, small_word(h, kWordNewKeys), 4}, {points, a.out, (size_t)n * kRec}};
    if ((rc = download_arrays(h, d, points && n ? 2 : 1, 0))) return rc;
    if (added > n) return fail(h, GEM_ERR_HIP, "gem_local_spill: inserted key count out of range");
    lc.log_len += n;
    lc.live += added;
    if (out_count) *out_count = (int)n;
    if (out_replaced) *out_replaced = (int)(n - added);
    return GEM_OK;
}

int gem_local_export(gem_handle* h, void* points, long long max_points, long long* out_count, int clear)
{
    ApiRange api_range(h, "gem_local_export");
    if (!h) return GEM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    int rc;
    if ((rc = usable(h, "gem_local_export"))) return rc;
    auto& lc = h->local;
    if (points && max_points < lc.live) return fail(h, GEM_ERR_INVALID, "gem_local_export: max_points below the entry count");
    if (points && lc.live > 0) {
        // the live entries in log order into the other log arena (which holds log_cap >= log_len entries), then to the host
        LocalExportArgs e{log_at(h, lc.act), lc.log_len, table_of(h), log_at(h, 1 - lc.act)};
        GEM_HIP(h, launch_local_export(h->stream, e, static_cast<uint32_t*>(lc.exp_cnt.p), small_word(h, kWordExport)));
        uint32_t n = 0;
        HostXfer d[2] = {{&n, small_word(h, kWordExport), 4}, {points, e.out, (size_t)lc.live * kRec}};
        if ((rc = download_arrays(h, d, 2, 0))) return rc;
        if ((long long)n != lc.live) return fail(h, GEM_ERR_HIP, "gem_local_export: live entry count mismatch");
    }
    if (out_count) *out_count = lc.live;
    if (clear) {                                                   // localMap_.swap(tmp)
        if ((rc = clear_table(h))) return rc;
        lc.log_len = lc.live = 0;
    }
    return GEM_OK;
}

int gem_local_size(gem_handle* h, long long* out_count)
{
    if (!h) return GEM_ERR_INVALID;
    if (!out_count) return fail(h, GEM_ERR_INVALID, "gem_local_size: null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    int rc;
    if ((rc = usable(h, "gem_local_size"))) return rc;
    *out_count = h->local.live;
    return GEM_OK;
}

} // extern "C"
