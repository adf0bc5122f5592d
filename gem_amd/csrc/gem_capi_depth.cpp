// gem_capi_depth.cpp -- the depth-image entry points of include/gem_hip.h: the four host constants (gem_depth_constants), the
// unprojection on its own (gem_depth_unproject_device) and in front of the add path (gem_add_depth, gem_add_depth_device).  The kernel
// is in gem_depth.hip; the add path itself is add_cloud (gem_capi.cpp), where a depth image is the fourth source: uploaded as it is,
// unprojected into the staging arena with the PASSTHROUGH_Z mask folded in, then fused like a raw or a voxel-filtered cloud.
#include "gem_capi_internal.hpp"
#include "gem_depth.hpp"

namespace {

constexpr long long kMaxPixels = 1ll << 26;

// the image checked (no pointers), its strides filled in and its constants computed; false: GEM_ERR_INVALID
bool depth_source(const gem_depth_image* img, bool on_device, DepthSource& s)
{
    if (!img) return false;
    const gem_depth_image& g = *img;
    if (g.width < 0 || g.height < 0 || (long long)g.width * g.height > kMaxPixels) return false;
    if (g.format != GEM_DEPTH_U16 && g.format != GEM_DEPTH_F32) return false;
    if (g.color_format < GEM_COLOR_NONE || g.color_format > GEM_COLOR_RGB8) return false;
    const size_t esz = g.format == GEM_DEPTH_U16 ? 2 : 4;
    if (g.row_stride && (g.row_stride % esz || g.row_stride < (size_t)g.width * esz)) return false;
    if (g.color_row_stride && g.color_row_stride < (size_t)g.width * 3) return false;
    if (!std::isfinite(g.fx) || !std::isfinite(g.fy) || g.fx == 0.0 || g.fy == 0.0 || !std::isfinite(g.cx) || !std::isfinite(g.cy)) return false;
    if (!std::isfinite(g.depth_unit) || g.depth_unit < 0.0f) return false;
    s.img = g;
    if (!s.img.row_stride) s.img.row_stride = (size_t)g.width * esz;
    if (!s.img.color_row_stride) s.img.color_row_stride = (size_t)g.width * 3;
    s.unit = g.depth_unit == 0.0f ? 0.001f : g.depth_unit;                     // DepthTraits<uint16_t>::toMeters
    const double unit = g.format == GEM_DEPTH_U16 ? (double)s.unit : 1.0;
    s.k[0] = to_float_rn(unit / g.fx); s.k[1] = to_float_rn(unit / g.fy);
    s.k[2] = to_float_rn(g.cx); s.k[3] = to_float_rn(g.cy);
    s.on_device = on_device;
    return true;
}

// ... and the pointers that come with it: present where there are pixels, a device depth image aligned to its element
bool images_ok(const DepthSource& s, const void* depth, const void* color)
{
    if ((long long)s.img.width * s.img.height == 0) return true;
    if (!depth || (s.on_device && reinterpret_cast<uintptr_t>(depth) % (s.img.format == GEM_DEPTH_U16 ? 2 : 4))) return false;
    return s.img.color_format == GEM_COLOR_NONE || color;
}

bool clean_ok(const gem_clean_params* c) { return !c || (c->mode >= GEM_CLEAN_NONE && c->mode <= GEM_CLEAN_PASSTHROUGH_Z); }

int add_depth(gem_handle* h, const char* what, const gem_frame_params* p, const gem_depth_image* img, const void* depth, const void* color,
              const gem_clean_params* clean, const gem_voxel_params* stages, int n_stages, bool on_device)
{
    if (!h) return GEM_ERR_INVALID;
    ApiRange api_range(h, what);
    DepthSource s;
    const bool voxel = stages || n_stages;
    if (!p || !depth_source(img, on_device, s) || !images_ok(s, depth, color) || !clean_ok(clean) || (clean && voxel) ||
        (voxel && !voxel_stages_ok(stages, n_stages)))
        return fail(h, GEM_ERR_INVALID, "gem_add_depth: bad argument");
    if (voxel && h->tp_x) return fail(h, GEM_ERR_INVALID, "gem_add_depth: no voxel stages on a handle with a communicator");
    // (no orig array: the pixel index is the raw position, which is what getI / getJ divide by the width)
    if (p->sensor_model == GEM_MODEL_STEREO && p->original_width != s.img.width)
        return fail(h, GEM_ERR_INVALID, "gem_add_depth: a stereo frame's original_width must be the image's width");
    AddFront fe;
    if (voxel) fe = {FrontEnd::voxel, nullptr, stages, n_stages};
    else if (clean && clean->mode == GEM_CLEAN_PASSTHROUGH_Z) fe = {FrontEnd::clean, clean};
    AddCloud c{AddSource::depth, s.img.width * s.img.height, depth, color};
    c.image = &s;
    std::lock_guard<std::mutex> lk(h->mu);
    return add_cloud(h, p, c, fe);
}

} // namespace

namespace gemi {

int depth_unproject(gem_handle* h, const DepthSource& s, const void* depth, const void* color, const gem_clean_params* clean,
                    float4* xyzi, uint32_t* rgb)
{
    DepthArgs a{};
    a.width = s.img.width; a.height = s.img.height;
    a.format = s.img.format; a.color_format = rgb && color ? s.img.color_format : GEM_COLOR_NONE;
    a.depth = static_cast<const unsigned char*>(depth); a.color = static_cast<const unsigned char*>(color);
    a.depth_stride = s.img.row_stride; a.color_stride = s.img.color_row_stride;
    a.kx = s.k[0]; a.ky = s.k[1]; a.cxf = s.k[2]; a.cyf = s.k[3];
    a.unit = s.unit; a.intensity = s.img.intensity;
    a.mask = clean && clean->mode == GEM_CLEAN_PASSTHROUGH_Z;
    if (a.mask) { a.z_min = clean->z_min; a.z_max = clean->z_max; }
    a.xyzi = xyzi; a.rgb = rgb;
    GEM_HIP(h, launch_depth_unproject(h->stream, a));
    return GEM_OK;
}

} // namespace gemi

extern "C" {

int gem_depth_constants(const gem_depth_image* img, float out[4])
{
    DepthSource s;
    if (!out || !depth_source(img, false, s)) return GEM_ERR_INVALID;
    for (int i = 0; i < 4; ++i) out[i] = s.k[i];
    return GEM_OK;
}

int gem_depth_unproject_device(gem_handle* h, const gem_depth_image* img, const void* d_depth, const void* d_color,
                               const gem_clean_params* clean, void* d_xyzi_out, void* d_rgb_out)
{
    if (!h) return GEM_ERR_INVALID;
    ApiRange api_range(h, "gem_depth_unproject_device");
    DepthSource s;
    if (!depth_source(img, true, s) || !images_ok(s, d_depth, d_color) || !clean_ok(clean))
        return fail(h, GEM_ERR_INVALID, "gem_depth_unproject_device: bad argument");
    const bool pixels = (long long)s.img.width * s.img.height > 0;
    if (pixels && (!d_xyzi_out || reinterpret_cast<uintptr_t>(d_xyzi_out) % 16 || reinterpret_cast<uintptr_t>(d_rgb_out) % 4))
        return fail(h, GEM_ERR_INVALID, "gem_depth_unproject_device: the XYZI output must be 16-byte aligned, the rgb output 4-byte");
    std::lock_guard<std::mutex> lk(h->mu);
    hipSetDevice(h->device);
    if (!pixels) return GEM_OK;
    return depth_unproject(h, s, d_depth, d_color, clean, static_cast<float4*>(d_xyzi_out), static_cast<uint32_t*>(d_rgb_out));
}

int gem_add_depth(gem_handle* h, const gem_frame_params* p, const gem_depth_image* img, const void* depth, const void* color,
                  const gem_clean_params* clean, const gem_voxel_params* stages, int n_stages)
{
    return add_depth(h, "gem_add_depth", p, img, depth, color, clean, stages, n_stages, false);
}

int gem_add_depth_device(gem_handle* h, const gem_frame_params* p, const gem_depth_image* img, const void* d_depth, const void* d_color,
                         const gem_clean_params* clean, const gem_voxel_params* stages, int n_stages)
{
    return add_depth(h, "gem_add_depth_device", p, img, d_depth, d_color, clean, stages, n_stages, true);
}

} // extern "C"
