// gem_capi_history.cpp -- the history-cloud entry points of include/gem_hip_history.h (visualCloud_ of ElevationMapping: the push_back
// of the "Local mapping" block, EMg.cpp:750-760, clear() and the "Visual step" of updateGlobalMap, :788 and :894-897, visualPointMap,
// :520-530).  The box table's kernel is in gem_history.hip; gem_costmap_mark_history is with the other marks in gem_capi_costmap.cpp.
//
// State (gem_handle::History):
//   the log        one record arena in history order; growing copies it device to device into the other arena, at least twice as
//                  large, and the two swap (ensure() does not keep contents)
//   the box table  four floats per block of kCostChunk records, recomputed from the records for every block an append reaches (the
//                  first of them may be a partial block with older records), and for all blocks when the table itself had to grow
// Every device buffer comes from ensure(), so gem_debug_get("arena_allocations") counts it; the capacities only grow, so a frame loop
// that has reached its sizes allocates nothing.
#include "gem_capi_internal.hpp"
#include "gem_history.hpp"

#include <algorithm>

namespace {

constexpr size_t kRec = sizeof(LocalRecord);
constexpr long long kMaxInputs = 2147483646ll;                      // 2^31 - 2: the stamp limit of a mark (gem_capi_costmap.cpp)

LocalRecord* log_at(gem_handle* h, long long at) { return static_cast<LocalRecord*>(h->history.log[h->history.act].p) + at; }
float4* boxes(gem_handle* h) { return static_cast<float4*>(h->history.box.p); }

int usable(gem_handle* h, const char* what)
{
    if (h->tp_x) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": not on a handle with a communicator").c_str());
    if (!h->history.enabled) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": the history is not enabled (gem_history_enable)").c_str());
    return GEM_OK;
}

// the boxes of the blocks that records [from, len) reach
int refresh_boxes(gem_handle* h, long long from)
{
    auto& hs = h->history;
    if (from >= hs.len) return GEM_OK;
    const long long first = from / kCostChunk, last = (hs.len - 1) / kCostChunk;
    GEM_HIP(h, launch_history_boxes(h->stream, log_at(h, 0), hs.len, first, last - first + 1, boxes(h)));
    return GEM_OK;
}

} // namespace

namespace gemi {

void history_free(gem_handle* h)
{
    auto& hs = h->history;
    if (h->stream) hipStreamSynchronize(h->stream);
    for (Arena* a : {&hs.log[0], &hs.log[1], &hs.box, &hs.small}) {
        if (a->p) hipFree(a->p);
        a->p = nullptr; a->cap = 0;
    }
    hs = gem_handle::History{};
}

int history_check_room(gem_handle* h, long long n, const char* what)
{
    if (n < 0 || n > kMaxInputs || h->history.len + n > kMaxInputs)
        return fail(h, GEM_ERR_INVALID, (std::string(what) + ": the history would pass 2^31 - 2 records").c_str());
    return GEM_OK;
}

// room for `extra` more records behind the log: a full arena is replaced by one at least twice as large.  The box table follows the
// log's capacity; when it is replaced, the boxes of the records the log holds are computed again.
int history_reserve(gem_handle* h, long long extra)
{
    auto& hs = h->history;
    int rc;
    if (hs.len + extra > hs.cap) {
        const long long need = std::max(2 * hs.cap, hs.len + extra);
        Arena& to = hs.log[1 - hs.act];
        if ((rc = ensure(h, to, (size_t)need * kRec))) return rc;
        if (hs.len) GEM_HIP(h, hipMemcpyAsync(to.p, log_at(h, 0), (size_t)hs.len * kRec, hipMemcpyDeviceToDevice, h->stream));
        hs.act = 1 - hs.act;
        hs.cap = (long long)(to.cap / kRec);
    }
    const long long blocks = history_blocks(hs.cap);
    if (blocks > hs.box_cap) {
        if ((rc = ensure(h, hs.box, (size_t)blocks * sizeof(float4)))) return rc;
        hs.box_cap = (long long)(hs.box.cap / sizeof(float4));
        if ((rc = refresh_boxes(h, 0))) return rc;
    }
    return GEM_OK;
}

// (room reserved by the caller)
int history_append_device(gem_handle* h, const void* d_src, long long n)
{
    auto& hs = h->history;
    if (n <= 0) return GEM_OK;
    if (hs.len + n > hs.cap) return fail(h, GEM_ERR_INVALID, "history_append_device: no room reserved");
    GEM_HIP(h, hipMemcpyAsync(log_at(h, hs.len), d_src, (size_t)n * kRec, hipMemcpyDeviceToDevice, h->stream));
    const long long from = hs.len;
    hs.len += n;
    return refresh_boxes(h, from);
}

int history_blocks_culled(gem_handle* h, long long* out)
{
    *out = 0;
    if (!h->history.enabled || !h->history.small.p) return GEM_OK;
    uint32_t n = 0;
    HostXfer d{&n, h->history.small.p, 4};
    const int rc = download_arrays(h, &d, 1, 0);
    if (rc) return rc;
    *out = n;
    return GEM_OK;
}

} // namespace gemi

extern "C" {

int gem_history_enable(gem_handle* h, long long capacity)
{
    GEM_ENTRY("gem_history_enable");
    int rc;
    if (capacity < 0 || capacity > kMaxInputs) return fail(h, GEM_ERR_INVALID, "gem_history_enable: capacity out of range");
    if (h->tp_x) return fail(h, GEM_ERR_INVALID, "gem_history_enable: not on a handle with a communicator");
    if (capacity == 0) { history_free(h); return GEM_OK; }
    auto& hs = h->history;
    if (!hs.small.p) {
        if ((rc = ensure(h, hs.small, 64))) return rc;
        GEM_HIP(h, hipMemsetAsync(hs.small.p, 0, 64, h->stream));
    }
    hs.len = 0;
    if ((rc = history_reserve(h, capacity))) return rc;
    hs.enabled = true;
    return GEM_OK;
}

int gem_history_append(gem_handle* h, const void* points, long long n)
{
    GEM_ENTRY("gem_history_append");
    int rc;
    if ((rc = usable(h, "gem_history_append"))) return rc;
    if (n < 0 || (n > 0 && !points)) return fail(h, GEM_ERR_INVALID, "gem_history_append: bad cloud");
    if ((rc = history_check_room(h, n, "gem_history_append"))) return rc;
    if (n == 0) return GEM_OK;
    if ((rc = history_reserve(h, n))) return rc;
    auto& hs = h->history;
    HostXfer x{const_cast<void*>(points), log_at(h, hs.len), (size_t)n * kRec};
    if ((rc = upload_arrays(h, &x, 1))) return rc;
    const long long from = hs.len;
    hs.len += n;
    return refresh_boxes(h, from);
}

int gem_history_append_device(gem_handle* h, const void* d_points, long long n)
{
    GEM_ENTRY("gem_history_append_device");
    int rc;
    if ((rc = usable(h, "gem_history_append_device"))) return rc;
    if (n < 0 || (n > 0 && !d_points)) return fail(h, GEM_ERR_INVALID, "gem_history_append_device: bad cloud");
    if ((rc = history_check_room(h, n, "gem_history_append_device"))) return rc;
    if (n == 0) return GEM_OK;
    if ((rc = history_reserve(h, n))) return rc;
    return history_append_device(h, d_points, n);
}

int gem_history_reset_from_global(gem_handle* h)
{
    GEM_ENTRY("gem_history_reset_from_global");
    int rc;
    if ((rc = usable(h, "gem_history_reset_from_global"))) return rc;
    const auto& g = h->global;
    if (!g.enabled) return fail(h, GEM_ERR_INVALID, "gem_history_reset_from_global: the submap stack is not enabled (gem_global_enable)");
    long long total = 0;
    for (long long c : g.cnt) total += c;
    if (total > kMaxInputs) return fail(h, GEM_ERR_INVALID, "gem_history_reset_from_global: the history would pass 2^31 - 2 records");
    auto& hs = h->history;
    hs.len = 0;                                                          // visualCloud_.clear(): nothing to carry over when the log grows
    if ((rc = history_reserve(h, total))) return rc;
    const LocalRecord* stack = static_cast<const LocalRecord*>(g.stack[g.act].p);
    long long at = 0;
    for (size_t s = 0; s < g.cnt.size(); ++s) {                          // visualCloud_ += globalMap_[i], every submap
        if (!g.cnt[s]) continue;
        GEM_HIP(h, hipMemcpyAsync(log_at(h, at), stack + g.off[s], (size_t)g.cnt[s] * kRec, hipMemcpyDeviceToDevice, h->stream));
        at += g.cnt[s];
    }
    hs.len = total;
    return refresh_boxes(h, 0);
}

int gem_history_clear(gem_handle* h)
{
    GEM_ENTRY("gem_history_clear");
    int rc;
    if ((rc = usable(h, "gem_history_clear"))) return rc;
    h->history.len = 0;
    return GEM_OK;
}

int gem_history_size(gem_handle* h, long long* out_count)
{
    GEM_ENTRY("gem_history_size");
    int rc;
    if (!out_count) return fail(h, GEM_ERR_INVALID, "gem_history_size: null argument");
    if ((rc = usable(h, "gem_history_size"))) return rc;
    *out_count = h->history.len;
    return GEM_OK;
}

int gem_history_export(gem_handle* h, int with_grid_cloud, void* points, long long max_points, long long* out_count)
{
    GEM_ENTRY("gem_history_export");
    int rc;
    if ((rc = usable(h, "gem_history_export"))) return rc;
    auto& hs = h->history;
    uint32_t n_grid = 0;
    if (with_grid_cloud) {
        if (!h->local.enabled || h->local.cur < 0)
            return fail(h, GEM_ERR_INVALID, "gem_history_export: with_grid_cloud, but the local map is not enabled or has no capture");
        if ((rc = local_grid_count(h, &n_grid))) return rc;
    }
    const long long total = hs.len + n_grid;
    if (points && max_points < total) return fail(h, GEM_ERR_INVALID, "gem_history_export: max_points below the record count");
    if (points) {
        HostXfer d[2];
        int k = 0;
        if (hs.len) d[k++] = HostXfer{points, log_at(h, 0), (size_t)hs.len * kRec};
        if (n_grid) d[k++] = HostXfer{static_cast<unsigned char*>(points) + (size_t)hs.len * kRec, h->local.slot[h->local.cur].rec.p, (size_t)n_grid * kRec};
        for (int i = 0; i < k; ++i)
            if ((rc = download_arrays(h, &d[i], 1, 0))) return rc;
    }
    if (out_count) *out_count = total;
    return GEM_OK;
}

} // extern "C"
