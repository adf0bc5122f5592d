// gem_capi_global.cpp -- the submap-stack entry points of include/gem_hip.h (globalMap_ of ElevationMapping: the push of
// updateLocalMap's new-keyframe branch, EMg.cpp:630-687, and updateGlobalMap, :773-905).  The kernels are in gem_global.hip.
//
// State (gem_handle::Global):
//   the stack      one record arena; submap s holds cnt[s] records from off[s] on, with room[s] >= cnt[s] behind it (a loop closure
//                  only shrinks submaps, in place).  Growing copies the submaps, packed, into the other arena.
//   a loop closure uploads the counts, transforms, and runs its pair steps back to back on the stream: each step reads its counts on
//                  the device and sizes its grids from the counts at the start (upper bounds), and writes both sides through scratch
//                  (out[]) back into their rooms.  The counts come back to the host once, at the end.
// Every device buffer comes from ensure(), so gem_debug_get("arena_allocations") counts it; the capacities only grow, so a second
// identical loop closure allocates nothing.
#include "gem_capi_internal.hpp"
#include "gem_global.hpp"

#include <algorithm>
#include <array>
#include <cmath>

namespace {

constexpr size_t kRec = sizeof(LocalRecord);
// words of Global::small
constexpr int kWordSide = 0, kWordFused = 2;

uint32_t* small_word(gem_handle* h, int w) { return static_cast<uint32_t*>(h->global.small.p) + w; }
LocalRecord* stack_at(gem_handle* h, long long off) { return static_cast<LocalRecord*>(h->global.stack[h->global.act].p) + off; }

int usable(gem_handle* h, const char* what)
{
    if (h->tp_x) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": not on a handle with a communicator").c_str());
    if (!h->global.enabled) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": the submap stack is not enabled (gem_global_enable)").c_str());
    return GEM_OK;
}

long long pow2_at_least(long long v)
{
    long long c = 64;
    while (c < v) c <<= 1;
    return c;
}

// room for `extra` more records behind the last submap: a full arena is replaced by one at least twice as large, the submaps copied
// into it packed (each one's room becomes its count)
int reserve(gem_handle* h, long long extra)
{
    auto& g = h->global;
    if (g.used + extra <= g.cap) return GEM_OK;
    long long live = 0;
    for (long long c : g.cnt) live += c;
    const long long need = std::max(2 * g.cap, live + extra);
    Arena& to = g.stack[1 - g.act];
    int rc;
    if ((rc = ensure(h, to, (size_t)need * kRec))) return rc;
    LocalRecord* dst = static_cast<LocalRecord*>(to.p);
    long long at = 0;
    for (size_t s = 0; s < g.cnt.size(); ++s) {
        if (g.cnt[s]) GEM_HIP(h, hipMemcpyAsync(dst + at, stack_at(h, g.off[s]), (size_t)g.cnt[s] * kRec, hipMemcpyDeviceToDevice, h->stream));
        g.off[s] = at; g.room[s] = g.cnt[s];
        at += g.cnt[s];
    }
    g.act = 1 - g.act;
    g.cap = (long long)(to.cap / kRec);
    g.used = at;
    return GEM_OK;
}

// the slot of a new submap of n records; its records are written by the caller
int append(gem_handle* h, long long n, int* index)
{
    auto& g = h->global;
    g.off.push_back(g.used); g.room.push_back(n); g.cnt.push_back(n);
    g.used += n;
    if (index) *index = (int)g.cnt.size() - 1;
    return GEM_OK;
}

// the neighbour list of submap i among centres [0, n): d2 = dx * dx + dy * dy (float), d2 < r2, ascending (d2, j)
std::vector<int> neighbours(const float* c, int n, int i, float r2)
{
    std::vector<std::pair<float, int>> hits;
    for (int j = 0; j < n; ++j) {
        const float dx = c[2 * j] - c[2 * i], dy = c[2 * j + 1] - c[2 * i + 1];
        const float d2 = dx * dx + dy * dy;
        if (d2 < r2) hits.emplace_back(d2, j);
    }
    std::sort(hits.begin(), hits.end());
    std::vector<int> out;
    for (const auto& p : hits) out.push_back(p.second);
    return out;
}

} // namespace

namespace gemi {

void global_free(gem_handle* h)
{
    auto& g = h->global;
    if (h->stream) hipStreamSynchronize(h->stream);
    for (Arena* a : {&g.stack[0], &g.stack[1], &g.cnts, &g.out[0], &g.out[1], &g.keys[0], &g.keys[1], &g.tkeys[0], &g.tkeys[1],
                     &g.tvals[0], &g.tvals[1], &g.blk[0], &g.blk[1], &g.small}) {
        if (a->p) hipFree(a->p);
        a->p = nullptr; a->cap = 0;
    }
    g = gem_handle::Global{};
}

} // namespace gemi

extern "C" {

int gem_global_enable(gem_handle* h, long long capacity)
{
    ApiRange api_range(h, "gem_global_enable");
    if (!h) return GEM_ERR_INVALID;
    if (capacity < 0 || capacity > (1ll << 31)) return fail(h, GEM_ERR_INVALID, "gem_global_enable: capacity out of range");
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    if (h->tp_x) return fail(h, GEM_ERR_INVALID, "gem_global_enable: not on a handle with a communicator");
    if (capacity == 0) { global_free(h); return GEM_OK; }
    auto& g = h->global;
    int rc;
    if ((rc = ensure(h, g.small, 64))) return rc;
    g.off.clear(); g.room.clear(); g.cnt.clear();
    g.used = 0;
    if (capacity > g.cap) {
        if ((rc = ensure(h, g.stack[g.act], (size_t)capacity * kRec))) return rc;
        g.cap = (long long)(g.stack[g.act].cap / kRec);
    }
    g.enabled = true;
    return GEM_OK;
}

int gem_global_push_local(gem_handle* h, int clear_local, int* out_index)
{
    ApiRange api_range(h, "gem_global_push_local");
    if (!h) return GEM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    int rc;
    if ((rc = usable(h, "gem_global_push_local"))) return rc;
    if (!h->local.enabled || h->local.cur < 0)
        return fail(h, GEM_ERR_INVALID, "gem_global_push_local: the local map is not enabled or has no capture");
    uint32_t n_grid = 0;
    if ((rc = local_grid_count(h, &n_grid))) return rc;
    const long long n = h->local.live + n_grid;
    if ((rc = reserve(h, n))) return rc;
    if ((rc = local_export_to(h, stack_at(h, h->global.used), n_grid, clear_local != 0))) return rc;
    return append(h, n, out_index);
}

int gem_global_push(gem_handle* h, const void* points, long long n, int* out_index)
{
    ApiRange api_range(h, "gem_global_push");
    if (!h) return GEM_ERR_INVALID;
    if (n < 0 || n > (1ll << 31) || (n > 0 && !points)) return fail(h, GEM_ERR_INVALID, "gem_global_push: bad cloud");
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    int rc;
    if ((rc = usable(h, "gem_global_push"))) return rc;
    if ((rc = reserve(h, n))) return rc;
    if (n) {
        HostXfer x{const_cast<void*>(points), stack_at(h, h->global.used), (size_t)n * kRec};
        if ((rc = upload_arrays(h, &x, 1))) return rc;
    }
    return append(h, n, out_index);
}

int gem_global_loop_closure(gem_handle* h, int n_opt, const float* transforms, const float* centres, float radius,
                            double resolution, long long* out_fused)
{
    ApiRange api_range(h, "gem_global_loop_closure");
    if (!h) return GEM_ERR_INVALID;
    if (n_opt < 0) return fail(h, GEM_ERR_INVALID, "gem_global_loop_closure: n_opt < 0");
    if (n_opt > 1 && (!transforms || !centres)) return fail(h, GEM_ERR_INVALID, "gem_global_loop_closure: null transforms or centres");
    if (!std::isfinite(radius) || radius < 0.f) return fail(h, GEM_ERR_INVALID, "gem_global_loop_closure: radius not finite and >= 0");
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    int rc;
    if ((rc = usable(h, "gem_global_loop_closure"))) return rc;
    auto& g = h->global;
    const int n = std::min(n_opt, (int)g.cnt.size());                               // optKeyframeNum clamped (EMg.cpp:784-786)
    const double res = resolution > 0.0 ? resolution : (double)h->res;
    const float r2 = (float)((double)radius * (double)radius);
    // the pair steps (i, k) in the reference's order: lists of more than two entries, from position 1 on (EMg.cpp:844-846)
    std::vector<std::array<int, 2>> steps;
    for (int i = 0; i < n && centres; ++i) {
        const std::vector<int> list = neighbours(centres, n, i, r2);
        if (list.size() > 2)
            for (size_t p = 1; p < list.size(); ++p) steps.push_back({i, list[p]});
    }
    long long maxb = 1;
    for (int s = 0; s < n; ++s) maxb = std::max(maxb, g.cnt[s]);
    // every buffer before the first launch
    const long long tcap = pow2_at_least(2 * maxb);
    if ((rc = ensure(h, g.cnts, (size_t)std::max(n, 1) * 4))) return rc;
    for (int side = 0; side < 2; ++side) {
        if ((rc = ensure(h, g.out[side], (size_t)maxb * kRec)) || (rc = ensure(h, g.keys[side], (size_t)maxb * 8)) ||
            (rc = ensure(h, g.tkeys[side], (size_t)tcap * 8)) || (rc = ensure(h, g.tvals[side], (size_t)tcap * 4)) ||
            (rc = ensure(h, g.blk[side], (size_t)compact_blocks(maxb) * 4 + 64))) return rc;
    }
    std::vector<uint32_t> cnt(std::max(n, 1));
    for (int s = 0; s < n; ++s) cnt[s] = (uint32_t)g.cnt[s];
    uint32_t* d_cnt = static_cast<uint32_t*>(g.cnts.p);
    if (n) {
        HostXfer x{cnt.data(), d_cnt, (size_t)n * 4};
        if ((rc = upload_arrays(h, &x, 1))) return rc;
    }
    GEM_HIP(h, hipMemsetAsync(small_word(h, kWordFused), 0, 4, h->stream));
    // transforms: submaps 1 .. n-1 (entry 0 is ignored, EMg.cpp:795)
    for (int i = 1; i < n; ++i) {
        GlobalXform m;
        std::copy(transforms + 16 * i, transforms + 16 * (i + 1), m.m);
        GEM_HIP(h, launch_global_transform(h->stream, stack_at(h, g.off[i]), g.cnt[i], m));
    }
    // pair steps: old = hash(i), new = hash(k), both from the state before the step; then k := export(new), i := export(old)
    for (const auto& st : steps) {
        const int idx[2] = {st[0], st[1]};                                           // side 0 = old (i), side 1 = new (k)
        GlobalCloud c[2];
        for (int side = 0; side < 2; ++side) {
            const long long b = g.cnt[idx[side]];
            c[side].rec = stack_at(h, g.off[idx[side]]);
            c[side].count = d_cnt + idx[side];
            c[side].keys = static_cast<unsigned long long*>(g.keys[side].p);
            c[side].t = LocalTable{static_cast<unsigned long long*>(g.tkeys[side].p), static_cast<int*>(g.tvals[side].p),
                                   (unsigned long long)pow2_at_least(2 * b) - 1};
            GEM_HIP(h, launch_global_keys(h->stream, c[side], b, res));
        }
        for (int side = 1; side >= 0; --side) {
            GlobalSideArgs a{c[side], c[1 - side], side == 1, static_cast<LocalRecord*>(g.out[side].p),
                             side == 1 ? small_word(h, kWordFused) : nullptr};
            GEM_HIP(h, launch_global_side(h->stream, a, g.cnt[idx[side]], static_cast<uint32_t*>(g.blk[side].p), small_word(h, kWordSide + side)));
        }
        for (int side = 1; side >= 0; --side) {                                      // k first, then i: for k == i the old map wins
            if (g.cnt[idx[side]])
                GEM_HIP(h, hipMemcpyAsync(stack_at(h, g.off[idx[side]]), g.out[side].p, (size_t)g.cnt[idx[side]] * kRec,
                                          hipMemcpyDeviceToDevice, h->stream));
            GEM_HIP(h, hipMemcpyAsync(d_cnt + idx[side], small_word(h, kWordSide + side), 4, hipMemcpyDeviceToDevice, h->stream));
        }
    }
    uint32_t fused = 0;
    HostXfer d[2] = {{&fused, small_word(h, kWordFused), 4}, {cnt.data(), d_cnt, (size_t)n * 4}};
    if ((rc = download_arrays(h, d, n ? 2 : 1, 0))) return rc;
    for (int s = 0; s < n; ++s) {
        if ((long long)cnt[s] > g.cnt[s]) return fail(h, GEM_ERR_HIP, "gem_global_loop_closure: submap count out of range");
        g.cnt[s] = cnt[s];
    }
    if (out_fused) *out_fused = fused;
    return GEM_OK;
}

int gem_global_export(gem_handle* h, int index, void* points, long long max_points, long long* out_count)
{
    ApiRange api_range(h, "gem_global_export");
    if (!h) return GEM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    int rc;
    if ((rc = usable(h, "gem_global_export"))) return rc;
    auto& g = h->global;
    const int S = (int)g.cnt.size();
    if (index < -1 || index >= S) return fail(h, GEM_ERR_INVALID, "gem_global_export: index out of range");
    const int first = index < 0 ? 0 : index, last = index < 0 ? S : index + 1;
    long long total = 0;
    for (int s = first; s < last; ++s) total += g.cnt[s];
    if (points && max_points < total) return fail(h, GEM_ERR_INVALID, "gem_global_export: max_points below the record count");
    if (points) {
        long long at = 0;
        for (int s = first; s < last; ++s) {
            if (!g.cnt[s]) continue;
            HostXfer x{static_cast<unsigned char*>(points) + (size_t)at * kRec, stack_at(h, g.off[s]), (size_t)g.cnt[s] * kRec};
            if ((rc = download_arrays(h, &x, 1, 0))) return rc;
            at += g.cnt[s];
        }
    }
    if (out_count) *out_count = total;
    return GEM_OK;
}

int gem_global_count(gem_handle* h, int* out_submaps)
{
    if (!h) return GEM_ERR_INVALID;
    if (!out_submaps) return fail(h, GEM_ERR_INVALID, "gem_global_count: null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    int rc;
    if ((rc = usable(h, "gem_global_count"))) return rc;
    *out_submaps = (int)h->global.cnt.size();
    return GEM_OK;
}

} // extern "C"
