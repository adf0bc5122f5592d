// gem_capi_voxel.cpp -- the VoxelGrid entry points of include/gem_hip.h: the filter on the device (gem_voxel_device) and its fused
// forms in front of the add path (gem_add_voxel, gem_add_voxel_device).  The kernels are in gem_voxel.hip: seven launches per stage,
// enqueued on the handle's stream, the host never waits.
// Arenas: the stage state and the two digit histograms are all-zero between stages (zeroed once when allocated, the kernels leave
// them so); the records, a chain's two intermediates and the fused path's filtered clouds are plain arenas.  gem_reserve sizes all
// of them (voxel_reserve), so a stream of voxel frames inside the reserved bounds allocates nothing.
// The fused path writes the filtered cloud into vox_out[vox_flip] and flips: a pass that leaves work to the next call (k_frame's
// deferred fuse, which reads the binned records only) never has its input rewritten by the next call's filter (voxel_front; the rest
// of the add path is add_cloud, gem_capi.cpp).
#include "gem_capi_internal.hpp"
#include "gem_voxel.hpp"

#include <cstddef>

namespace {

bool stages_ok(const gem_voxel_params* s, int ns)
{
    if (!s || ns < 1 || ns > 4) return false;
    for (int i = 0; i < ns; ++i) {
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(s[i].leaf[k]) || !(s[i].leaf[k] > 0.0f)) return false;
        if (s[i].field < GEM_VOXEL_FIELD_NONE || s[i].field > GEM_VOXEL_FIELD_INTENSITY) return false;
    }
    return true;
}

size_t out_bytes(long long n) { return ((size_t)n * 16 + 256) + ((size_t)n * 4 + 256) + 256; }

int arenas(gem_handle* h, long long n, int ns)
{
    int rc;
    if ((rc = ensure_zeroed(h, h->vox_state, vox_state_bytes()))) return rc;
    if ((rc = ensure_zeroed(h, h->vox_hist, vox_hist_bytes(n)))) return rc;
    if ((rc = ensure(h, h->vox_rec, vox_rec_bytes(n)))) return rc;
    if (ns > 1 && (rc = ensure(h, h->vox_tmp, vox_tmp_bytes(n)))) return rc;
    return GEM_OK;
}

// the stages of one call on h->stream (n > 0, arenas in place)
int enqueue(gem_handle* h, const gem_voxel_params* stages, int ns, long long n, const float4* in, const uint32_t* rgb_in,
            float4* out, uint32_t* rgb_out, int* count_out)
{
    const long long nb = vox_blocks(n);
    if (nb > 0x7fffffffll) return fail(h, GEM_ERR_INVALID, "gem_voxel: cloud too large");
    VoxState* st = static_cast<VoxState*>(h->vox_state.p);
    unsigned char* rec = static_cast<unsigned char*>(h->vox_rec.p);
    unsigned char* hist = static_cast<unsigned char*>(h->vox_hist.p);
    const size_t R = (size_t)n * 4 + 256, HB = (size_t)nb * kVoxBins * sizeof(uint32_t);
    unsigned char* tmp = static_cast<unsigned char*>(h->vox_tmp.p);
    const size_t TX = (size_t)n * 16 + 256, TC = (size_t)n * 4 + 256;
    for (int s = 0; s < ns; ++s) {
        const gem_voxel_params& p = stages[s];
        const bool last = s == ns - 1;
        VoxStageArgs a{};
        a.n = n; a.nb = (int)nb;
        a.n_dev = s == 0 ? nullptr : &st->count[s - 1];
        a.in = s == 0 ? in : reinterpret_cast<const float4*>(tmp + ((s - 1) & 1) * TX);
        a.rgb_in = !rgb_in ? nullptr : s == 0 ? rgb_in : reinterpret_cast<const uint32_t*>(tmp + 2 * TX + ((s - 1) & 1) * TC);
        a.out = last ? out : reinterpret_cast<float4*>(tmp + (s & 1) * TX);
        a.rgb_out = last ? rgb_out : rgb_in ? reinterpret_cast<uint32_t*>(tmp + 2 * TX + (s & 1) * TC) : nullptr;
        a.count_out = last ? count_out : &st->count[s];
        for (int k = 0; k < 3; ++k) a.leaf[k] = p.leaf[k];
        a.field = p.field;
        a.lo = p.limit_min; a.hi = p.limit_max;
        a.lo_f = to_float_rn(p.limit_min); a.hi_f = to_float_rn(p.limit_max);
        a.negative = p.limit_negative != 0;
        a.st = st;
        a.hist[0] = reinterpret_cast<uint32_t*>(hist); a.hist[1] = reinterpret_cast<uint32_t*>(hist + HB);
        a.key[0] = reinterpret_cast<uint32_t*>(rec);         a.src[0] = reinterpret_cast<uint32_t*>(rec + R);
        a.key[1] = reinterpret_cast<uint32_t*>(rec + 2 * R); a.src[1] = reinterpret_cast<uint32_t*>(rec + 3 * R);
        a.heads = reinterpret_cast<uint32_t*>(rec + 4 * R);
        GEM_HIP(h, launch_voxel_stage(h->stream, a));
    }
    return GEM_OK;
}

} // namespace

namespace gemi {

bool voxel_stages_ok(const gem_voxel_params* stages, int ns) { return stages_ok(stages, ns); }

int voxel_front(gem_handle* h, const gem_voxel_params* stages, int ns, int n, const float4* xyzi, const uint32_t* rgb,
                const float4** out, const uint32_t** rgb_out)
{
    int rc;
    if ((rc = arenas(h, n, ns))) return rc;
    Arena& o = h->vox_out[h->vox_flip & 1u];
    if ((rc = ensure(h, o, out_bytes(n)))) return rc;
    h->vox_flip ^= 1u;
    unsigned char* d = static_cast<unsigned char*>(o.p);
    float4* fx = reinterpret_cast<float4*>(d);
    uint32_t* fc = rgb ? reinterpret_cast<uint32_t*>(d + (size_t)n * 16 + 256) : nullptr;
    int* cnt = reinterpret_cast<int*>(d + (size_t)n * 20 + 512);
    if ((rc = enqueue(h, stages, ns, n, xyzi, rgb, fx, fc, cnt))) return rc;
    *out = fx; *rgb_out = fc;
    return GEM_OK;
}

int voxel_reserve(gem_handle* h, long long max_points)
{
    int rc;
    if ((rc = arenas(h, max_points, 4))) return rc;
    for (Arena& o : h->vox_out)
        if ((rc = ensure(h, o, out_bytes(max_points)))) return rc;
    return GEM_OK;
}

} // namespace gemi

extern "C" {

int gem_voxel_device(gem_handle* h, const gem_voxel_params* stages, int n_stages, int n, const void* d_xyzi, const void* d_rgb,
                     void* d_xyzi_out, void* d_rgb_out, void* d_count_out)
{
    ApiRange api_range(h, "gem_voxel_device");
    if (!h || !stages_ok(stages, n_stages) || n < 0 || !d_count_out || (n > 0 && (!d_xyzi || !d_xyzi_out)))
        return h ? fail(h, GEM_ERR_INVALID, "gem_voxel_device: bad argument") : GEM_ERR_INVALID;
    if (h->tp_x) return fail(h, GEM_ERR_INVALID, "gem_voxel_device: not on a handle with a communicator");
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    if (n == 0) { GEM_HIP(h, hipMemsetAsync(d_count_out, 0, sizeof(int), h->stream)); return GEM_OK; }
    int rc;
    if ((rc = arenas(h, n, n_stages))) return rc;
    return enqueue(h, stages, n_stages, n, static_cast<const float4*>(d_xyzi), static_cast<const uint32_t*>(d_rgb),
                   static_cast<float4*>(d_xyzi_out), static_cast<uint32_t*>(d_rgb_out), static_cast<int*>(d_count_out));
}

int gem_add_voxel_device(gem_handle* h, const gem_frame_params* p, const gem_voxel_params* stages, int n_stages, int n,
                         const void* d_xyzi, const void* d_rgb)
{
    ApiRange api_range(h, "gem_add_voxel_device");
    if (!h || !p || !stages_ok(stages, n_stages) || n < 0 || (n > 0 && !d_xyzi))
        return h ? fail(h, GEM_ERR_INVALID, "gem_add_voxel_device: bad argument") : GEM_ERR_INVALID;
    if (h->tp_x) return fail(h, GEM_ERR_INVALID, "gem_add_voxel_device: not on a handle with a communicator");
    std::lock_guard<std::mutex> lk(h->mu);
    return add_cloud(h, p, {AddSource::device, n, d_xyzi, d_rgb}, {FrontEnd::voxel, nullptr, stages, n_stages});
}

int gem_add_voxel(gem_handle* h, const gem_frame_params* p, const gem_voxel_params* stages, int n_stages, int n, const float* xyzi,
                  const uint32_t* rgb)
{
    ApiRange api_range(h, "gem_add_voxel");
    if (!h || !p || !stages_ok(stages, n_stages) || n < 0 || (n > 0 && !xyzi))
        return h ? fail(h, GEM_ERR_INVALID, "gem_add_voxel: bad argument") : GEM_ERR_INVALID;
    if (h->tp_x) return fail(h, GEM_ERR_INVALID, "gem_add_voxel: not on a handle with a communicator");
    std::lock_guard<std::mutex> lk(h->mu);
    return add_cloud(h, p, {AddSource::host, n, xyzi, rgb}, {FrontEnd::voxel, nullptr, stages, n_stages});
}

} // extern "C"
