// gem_capi_clean.cpp -- the cleanPointCloud entry points of include/gem_hip.h (SensorProcessorBase.cpp:89): the compaction on the
// device (gem_clean_device, gem_process_points_raw) and the raw-cloud forms of the fuse entries (gem_add_raw*, gem_add_aos_raw).
// The kernels are in gem_clean.hip.  A REMOVE_NAN / NONE fuse takes the plain entry as it is (projection rejects non-finite points,
// see gem_hip.h); a PASSTHROUGH_Z fuse reads a copy of the cloud with the dropped points' x, y, z set to NaN, written into the
// handle's staging arena on its stream (add_cloud, gem_capi.cpp) -- the arena gem_add's own host path uploads into, sized by
// gem_reserve (so a stream of raw clouds inside the reserved bounds allocates nothing).
#include "gem_capi_internal.hpp"
#include "gem_clean.hpp"

namespace {

bool clean_ok(const gem_clean_params* c)
{
    return c && c->mode >= GEM_CLEAN_NONE && c->mode <= GEM_CLEAN_PASSTHROUGH_Z;
}

} // namespace

extern "C" {

int gem_clean_params_for_model(int sensor_model, double cutoff_min_depth, double cutoff_max_depth, gem_clean_params* out)
{
    if (!out || sensor_model < GEM_MODEL_LASER || sensor_model > GEM_MODEL_PERFECT) return GEM_ERR_INVALID;
    if (sensor_model == GEM_MODEL_STRUCTURED_LIGHT) {              // StructuredLightSensorProcessor.cpp:51-66
        if (std::isnan(cutoff_min_depth) || std::isnan(cutoff_max_depth)) return GEM_ERR_INVALID;
        out->mode = GEM_CLEAN_PASSTHROUGH_Z;
        out->z_min = to_float_rn(cutoff_min_depth);
        out->z_max = to_float_rn(cutoff_max_depth);
    } else {                                                       // Laser / Stereo / Perfect: removeNaNFromPointCloud
        out->mode = GEM_CLEAN_REMOVE_NAN;
        out->z_min = -INFINITY;
        out->z_max = INFINITY;
    }
    return GEM_OK;
}

int gem_clean_device(gem_handle* h, const gem_clean_params* clean, int n, const void* d_xyzi, const void* d_rgb,
                     void* d_xyzi_out, void* d_rgb_out, void* d_orig_out, void* d_count_out)
{
    ApiRange api_range(h, "gem_clean_device");
    if (!h || !clean_ok(clean) || n < 0 || !d_count_out || (n > 0 && !d_xyzi))
        return h ? fail(h, GEM_ERR_INVALID, "gem_clean_device: bad argument") : GEM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    int rc;
    if ((rc = ensure(h, h->clean_cnt, clean_scratch_bytes(n)))) return rc;
    CleanArgs a{};
    a.n = n; a.mode = clean->mode; a.z_min = clean->z_min; a.z_max = clean->z_max;
    a.xyzi = static_cast<const float4*>(d_xyzi); a.rgb = static_cast<const uint32_t*>(d_rgb);
    a.xyzi_out = static_cast<float4*>(d_xyzi_out); a.rgb_out = static_cast<uint32_t*>(d_rgb_out);
    a.orig_out = static_cast<int*>(d_orig_out);
    a.block_cnt = static_cast<uint32_t*>(h->clean_cnt.p); a.count_out = static_cast<int*>(d_count_out);
    GEM_HIP(h, launch_clean(h->stream, a, false));
    return GEM_OK;
}

int gem_add_raw(gem_handle* h, const gem_frame_params* p, const gem_clean_params* clean, int n, const float* xyzi, const uint32_t* rgb)
{
    if (!h || !clean_ok(clean)) return h ? fail(h, GEM_ERR_INVALID, "gem_add_raw: bad argument") : GEM_ERR_INVALID;
    if (clean->mode != GEM_CLEAN_PASSTHROUGH_Z) return gem_add(h, p, n, xyzi, rgb, nullptr);
    ApiRange api_range(h, "gem_add_raw");
    if (!p || n < 0 || (n > 0 && !xyzi)) return fail(h, GEM_ERR_INVALID, "gem_add_raw: bad argument");
    std::lock_guard<std::mutex> lk(h->mu);
    return add_cloud(h, p, {AddSource::host, n, xyzi, rgb}, {FrontEnd::clean, clean});
}

int gem_add_raw_device(gem_handle* h, const gem_frame_params* p, const gem_clean_params* clean, int n, const void* d_xyzi, const void* d_rgb)
{
    if (!h || !clean_ok(clean)) return h ? fail(h, GEM_ERR_INVALID, "gem_add_raw_device: bad argument") : GEM_ERR_INVALID;
    if (clean->mode != GEM_CLEAN_PASSTHROUGH_Z) return gem_add_device(h, p, n, d_xyzi, d_rgb, nullptr);
    ApiRange api_range(h, "gem_add_raw_device");
    if (!p || n < 0 || (n > 0 && !d_xyzi)) return fail(h, GEM_ERR_INVALID, "gem_add_raw_device: bad argument");
    std::lock_guard<std::mutex> lk(h->mu);
    return add_cloud(h, p, {AddSource::device, n, d_xyzi, d_rgb}, {FrontEnd::clean, clean});
}

int gem_add_aos_raw(gem_handle* h, const gem_frame_params* p, const gem_clean_params* clean, int n, const void* points, int point_step,
                    int off_x, int off_y, int off_z, int off_intensity, int off_rgb)
{
    if (!h || !clean_ok(clean)) return h ? fail(h, GEM_ERR_INVALID, "gem_add_aos_raw: bad argument") : GEM_ERR_INVALID;
    if (clean->mode != GEM_CLEAN_PASSTHROUGH_Z) return gem_add_aos(h, p, n, points, point_step, off_x, off_y, off_z, off_intensity, off_rgb);
    ApiRange api_range(h, "gem_add_aos_raw");
    if (!p || n < 0 || (n > 0 && !points)) return fail(h, GEM_ERR_INVALID, "gem_add_aos_raw: bad argument");
    if (!aos_fields_ok(point_step, off_x, off_y, off_z, off_intensity, off_rgb))
        return fail(h, GEM_ERR_INVALID, "gem_add_aos_raw: fields must be 4-byte aligned inside point_step");
    std::lock_guard<std::mutex> lk(h->mu);
    return add_cloud(h, p, {AddSource::aos, n, points, nullptr, nullptr, point_step, off_x, off_y, off_z, off_intensity, off_rgb},
                     {FrontEnd::clean, clean});
}

int gem_process_points_raw(gem_handle* h, const gem_frame_params* p, const gem_clean_params* clean, int n,
                           const float* x, const float* y, const float* z, int* n_kept, int* orig_out,
                           int* map_index, float* var, float* x_ts, float* y_ts, float* height)
{
    ApiRange api_range(h, "gem_process_points_raw");
    if (!h || !p || !clean_ok(clean) || n < 0 || (n > 0 && (!x || !y || !z)))
        return h ? fail(h, GEM_ERR_INVALID, "gem_process_points_raw: bad argument") : GEM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    if (n_kept) *n_kept = 0;
    if (n == 0) return GEM_OK;
    const size_t S = (size_t)n * 4, SP = (S + 255) & ~(size_t)255;
    int rc;
    // nine arrays of SP bytes in the staging arena (what gem_reserve sizes for gem_process_points) + the kept count:
    //   0-2 the raw x, y, z -- after the compaction the outputs index, var, x_ts | 3-5 the kept x, y, z | 6 their raw positions |
    //   7-8 the outputs y_ts, height | 9 SP + 0 the kept count
    if ((rc = ensure(h, h->stage, stage_words_bytes(n, 9)))) return rc;
    if ((rc = ensure(h, h->clean_cnt, clean_scratch_bytes(n)))) return rc;
    unsigned char* o = static_cast<unsigned char*>(h->stage.p);
    float* dx = reinterpret_cast<float*>(o); float* dy = reinterpret_cast<float*>(o + SP); float* dz = reinterpret_cast<float*>(o + 2 * SP);
    HostXfer up[3] = {{const_cast<float*>(x), dx, S}, {const_cast<float*>(y), dy, S}, {const_cast<float*>(z), dz, S}};
    if ((rc = upload_arrays(h, up, 3))) return rc;
    float* kx = reinterpret_cast<float*>(o + 3 * SP);  float* ky = reinterpret_cast<float*>(o + 4 * SP);
    float* kz = reinterpret_cast<float*>(o + 5 * SP);  int* korig = reinterpret_cast<int*>(o + 6 * SP);
    int* kidx = reinterpret_cast<int*>(o);             float* kvar = reinterpret_cast<float*>(o + SP);
    float* kxt = reinterpret_cast<float*>(o + 2 * SP); float* kyt = reinterpret_cast<float*>(o + 7 * SP);
    float* kzt = reinterpret_cast<float*>(o + 8 * SP); int* kcount = reinterpret_cast<int*>(o + 9 * SP);
    CleanArgs a{};
    a.n = n; a.mode = clean->mode; a.z_min = clean->z_min; a.z_max = clean->z_max;
    a.x = dx; a.y = dy; a.z = dz; a.x_out = kx; a.y_out = ky; a.z_out = kz; a.orig_out = korig;
    a.block_cnt = static_cast<uint32_t*>(h->clean_cnt.p); a.count_out = kcount;
    GEM_HIP(h, launch_clean(h->stream, a, true));
    int k = 0;
    GEM_HIP(h, hipMemcpyAsync(&k, kcount, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GEM_HIP(h, hipStreamSynchronize(h->stream));
    if (k < 0 || k > n) return fail(h, GEM_ERR_HIP, "gem_process_points_raw: kept count out of range");
    if (n_kept) *n_kept = k;
    if (k == 0) return GEM_OK;
    FrameConst fc; fill_frame(h, p, fc);
    // the kept points' raw positions are their orig indices (StereoSensorProcessor.cpp:37-48: indices_)
    GEM_HIP(h, launch_project(h->stream, fc, 0, k, kx, ky, kz, korig, 0, kidx, kvar, kxt, kyt, kzt));
    const size_t K = (size_t)k * 4;
    HostXfer down[6]; int nd = 0;
    if (orig_out)  down[nd++] = {orig_out, korig, K};
    if (map_index) down[nd++] = {map_index, kidx, K};
    if (var)       down[nd++] = {var, kvar, K};
    if (x_ts)      down[nd++] = {x_ts, kxt, K};
    if (y_ts)      down[nd++] = {y_ts, kyt, K};
    if (height)    down[nd++] = {height, kzt, K};
    if (nd) return download_arrays(h, down, nd, 0);
    GEM_HIP(h, hipStreamSynchronize(h->stream));
    return GEM_OK;
}

} // extern "C"
