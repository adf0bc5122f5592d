// gem_capi_compose.cpp -- gem_local_compose / gem_local_compose_distances of include/gem_hip.h: what composingGlobalMap does to
// prevMap_ before the octree insertion (gridMaptoPointCloud, pcl::StatisticalOutlierRemoval, the split by travers; EMg.cpp:482-514,
// :1146-1170) on the previous capture of the local map.  The kernels are in gem_compose.hip.
//
// One call: the capture's count (readback) -> index grid, ring walks, far list -> the distances to the host, where the ordered
// double sums and the threshold are computed (a chain of dependent adds is what a CPU core does best: DESIGN.md has what one lane
// and one wave of the device took) -> count / scan / scatter of the two classes -> their totals (readback) -> the records through the handle's pinned staging.  Every device buffer
// comes from ensure() and is sized by the map, so a second call allocates nothing.
#include "gem_capi_internal.hpp"
#include "gem_compose.hpp"

#include <cmath>
#include <limits>

namespace {

constexpr size_t kRec = sizeof(LocalRecord);
// words of Compose::small
constexpr int kWordFar = 0, kWordTotals = 1;

uint32_t* word(gem_handle* h, int w) { return static_cast<uint32_t*>(h->compose.small.p) + w; }

int check(gem_handle* h, const gem_compose_params* p, const char* what)
{
    const std::string w(what);
    if (h->tp_x) return fail(h, GEM_ERR_INVALID, (w + ": not on a handle with a communicator").c_str());
    if (!h->local.enabled) return fail(h, GEM_ERR_INVALID, (w + ": the local map is not enabled (gem_local_enable)").c_str());
    if (h->local.prev < 0) return fail(h, GEM_ERR_INVALID, (w + ": no previous capture kept (gem_local_keep_previous)").c_str());
    if (!p) return fail(h, GEM_ERR_INVALID, (w + ": null parameters").c_str());
    if (p->mean_k < 1 || p->mean_k > kComposeMaxK) return fail(h, GEM_ERR_INVALID, (w + ": mean_k out of range (1 .. 32)").c_str());
    if (!std::isfinite(p->stddev_mul)) return fail(h, GEM_ERR_INVALID, (w + ": stddev_mul is not finite").c_str());
    return GEM_OK;
}

// The distances of the previous capture's n records in Compose::dist and the threshold; filter = 0 for n <= mean_k (every distance
// +inf, the threshold +inf: nothing is removed).  The distances are also left in Compose::host_dist.
int distances(gem_handle* h, const gem_compose_params* p, uint32_t* out_n, double* out_threshold, int* out_filter)
{
    auto& cp = h->compose;
    const auto& pc = h->local.slot[h->local.prev];
    int rc;
    uint32_t n = 0;
    { HostXfer c{&n, static_cast<uint32_t*>(h->local.small.p) + h->local.prev, 4}; if ((rc = download_arrays(h, &c, 1, 0))) return rc; }
    if (n > (uint32_t)h->cells) return fail(h, GEM_ERR_HIP, "gem_local_compose: capture count out of range");
    const size_t cells = (size_t)h->cells;
    if ((rc = ensure(h, cp.small, 64)) || (rc = ensure(h, cp.grid, cells * 4)) || (rc = ensure(h, cp.dist, cells * 4)) ||
        (rc = ensure(h, cp.far, cells * 4))) return rc;
    *out_n = n;
    cp.far_points = 0;
    cp.sum_ns = 0;
    float* dist = static_cast<float*>(cp.dist.p);
    if (n <= (uint32_t)p->mean_k) {
        if (n) GEM_HIP(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(dist), 0x7f800000, n, h->stream));
        cp.host_dist.assign(n, std::numeric_limits<float>::infinity());
        *out_threshold = std::numeric_limits<double>::infinity();
        *out_filter = 0;
        return GEM_OK;
    }
    ComposeKnnArgs a{};
    a.rec = static_cast<const LocalRecord*>(pc.rec.p); a.lin = static_cast<const int*>(pc.lin.p);
    a.count = static_cast<uint32_t*>(h->local.small.p) + h->local.prev;
    a.g = LocalGeom{pc.off, pc.res, pc.px, pc.py, h->L, pc.sx, pc.sy};
    a.grid = static_cast<int*>(cp.grid.p); a.dist = dist;
    a.far = static_cast<int*>(cp.far.p); a.far_count = word(h, kWordFar);
    a.mean_k = p->mean_k; a.sqrt_double = (p->flags & GEM_COMPOSE_SQRT_DOUBLE) ? 1 : 0;
    GEM_HIP(h, launch_compose_knn(h->stream, a, n));
    uint32_t far = 0;
    if (cp.host_dist.size() < cells) cp.host_dist.resize(cells);
    HostXfer d[2] = {{&far, word(h, kWordFar), 4}, {cp.host_dist.data(), dist, (size_t)n * 4}};
    if ((rc = download_arrays(h, d, 2, 0))) return rc;
    // sum += d; sq_sum += d * d (a float product, widened when added), in index order
    const long long t0 = host_ns();
    const float* v = cp.host_dist.data();
    double sums[2] = {0.0, 0.0};
    for (uint32_t i = 0; i < n; ++i) { sums[0] += (double)v[i]; sums[1] += (double)(v[i] * v[i]); }
    cp.sum_ns = host_ns() - t0;
    if (far > n) return fail(h, GEM_ERR_HIP, "gem_local_compose: far count out of range");
    cp.far_points = far;
    const double nd = (double)n;
    const double mean = sums[0] / nd;
    const double variance = (sums[1] - sums[0] * sums[0] / nd) / (nd - 1.0);
    *out_threshold = mean + p->stddev_mul * std::sqrt(variance);
    *out_filter = 1;
    return GEM_OK;
}

} // namespace

namespace gemi {

int compose_check(gem_handle* h, const gem_compose_params* p, const char* what) { return check(h, p, what); }

// the filter and the split of the previous capture into Compose::road / Compose::obstacle (device; a list that is not wanted is only
// counted); tot[3]: road, obstacle, removed
int compose_split(gem_handle* h, const gem_compose_params* p, bool want_road, bool want_obstacle, uint32_t tot[3], double* out_threshold)
{
    auto& cp = h->compose;
    const size_t cells = (size_t)h->cells;
    int rc;
    if ((rc = ensure(h, cp.road, cells * kRec)) || (rc = ensure(h, cp.obstacle, cells * kRec)) ||
        (rc = ensure(h, cp.cnt, (size_t)compact_blocks(h->cells) * 3 * 4 + 64))) return rc;
    uint32_t n = 0;
    double thr = 0.0;
    int filter = 0;
    if ((rc = distances(h, p, &n, &thr, &filter))) return rc;
    ComposeSplitArgs s{};
    s.rec = static_cast<const LocalRecord*>(h->local.slot[h->local.prev].rec.p);
    s.dist = static_cast<const float*>(cp.dist.p);
    s.count = static_cast<uint32_t*>(h->local.small.p) + h->local.prev;
    s.threshold = thr; s.travers_threshold = p->travers_threshold; s.filter = filter;
    s.road = want_road ? static_cast<LocalRecord*>(cp.road.p) : nullptr;
    s.obstacle = want_obstacle ? static_cast<LocalRecord*>(cp.obstacle.p) : nullptr;
    GEM_HIP(h, launch_compose_split(h->stream, s, n, static_cast<uint32_t*>(cp.cnt.p), word(h, kWordTotals)));
    tot[0] = tot[1] = tot[2] = 0;
    { HostXfer c{tot, word(h, kWordTotals), 12}; if ((rc = download_arrays(h, &c, 1, 0))) return rc; }
    if ((unsigned long long)tot[0] + tot[1] + tot[2] > n) return fail(h, GEM_ERR_HIP, "gem_local_compose: class counts out of range");
    *out_threshold = thr;
    return GEM_OK;
}

void compose_free(gem_handle* h)
{
    auto& cp = h->compose;
    for (Arena* a : {&cp.grid, &cp.dist, &cp.far, &cp.road, &cp.obstacle, &cp.cnt, &cp.small}) {
        if (a->p) hipFree(a->p);
        a->p = nullptr; a->cap = 0;
    }
    cp = gem_handle::Compose{};
}

} // namespace gemi

extern "C" {

int gem_local_compose(gem_handle* h, const gem_compose_params* p, void* road, void* obstacle, int out_counts[3], double* out_threshold)
{
    ApiRange api_range(h, "gem_local_compose");
    if (!h) return GEM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    int rc;
    if ((rc = compose_check(h, p, "gem_local_compose"))) return rc;
    auto& cp = h->compose;
    uint32_t tot[3] = {0, 0, 0};
    double thr = 0.0;
    if ((rc = compose_split(h, p, road != nullptr, obstacle != nullptr, tot, &thr))) return rc;
    HostXfer d[2];
    int nd = 0;
    if (road && tot[0]) d[nd++] = HostXfer{road, cp.road.p, (size_t)tot[0] * kRec};
    if (obstacle && tot[1]) d[nd++] = HostXfer{obstacle, cp.obstacle.p, (size_t)tot[1] * kRec};
    if (nd && (rc = download_arrays(h, d, nd, 0))) return rc;
    if (out_counts) { out_counts[0] = (int)tot[0]; out_counts[1] = (int)tot[1]; out_counts[2] = (int)tot[2]; }
    if (out_threshold) *out_threshold = thr;
    return GEM_OK;
}

int gem_local_compose_distances(gem_handle* h, const gem_compose_params* p, float* distances_out, int* out_count)
{
    ApiRange api_range(h, "gem_local_compose_distances");
    if (!h) return GEM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    int rc;
    if ((rc = check(h, p, "gem_local_compose_distances"))) return rc;
    uint32_t n = 0;
    double thr = 0.0;
    int filter = 0;
    if ((rc = distances(h, p, &n, &thr, &filter))) return rc;
    if (distances_out && n) memcpy(distances_out, h->compose.host_dist.data(), (size_t)n * 4);
    if (out_count) *out_count = (int)n;
    return GEM_OK;
}

} // extern "C"
