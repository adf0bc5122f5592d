// gem_depth.hip -- the pinhole unprojection of a depth image (include/gem_hip.h: depth_image_proc::convert<T>, restated), gfx950.
//
// Element-wise and memory-bound: 2 or 4 bytes of depth and 3 of colour in, 16 + 4 bytes out per pixel.  A lane takes four consecutive
// pixels of one row: one 8-byte (U16) or 16-byte (F32) depth load, three dwords of colour, four float4 stores and one 16-byte rgb
// store.  The wide loads are taken only where the image's base address and row stride make them naturally aligned in every row (one
// choice per launch, so wave-uniform); everything else -- and the last width % 4 pixels of a row -- goes pixel by pixel.  No LDS, no
// atomics.  Byte offsets of a row are 64-bit, everything else 32-bit (width * height <= 2^26).
//
// The arithmetic of a pixel is (a - b) * c * d and a * b: no add behind a multiply, so there is nothing the compiler could contract
// into an FMA -- the kernel RELIES on that (and the library is built with -ffp-contract=off anyway); each operation is rounded to
// float, which is what tests/depth_ref.py computes.
#include "gem_depth.hpp"

namespace gem {

constexpr int kFastDepth = 1, kFastColor = 2, kFastRgbOut = 4;

template <int FMT, int COLOR, bool MASK>
__global__ __launch_bounds__(256) void k_depth_unproject(DepthArgs a, int groups_per_row, int lanes, int fast)
{
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= lanes) return;
    const int v = t / groups_per_row, u0 = (t - v * groups_per_row) * 4;
    const int npx = min(4, a.width - u0);                  // (1 .. 4: the pixels of this lane, all inside row v)
    const bool whole = npx == 4;

    float df[4] = {0.f, 0.f, 0.f, 0.f};
    bool valid[4] = {false, false, false, false};
    if constexpr (FMT == GEM_DEPTH_U16) {
        const unsigned char* row = a.depth + (size_t)a.depth_stride * (size_t)v + (size_t)u0 * 2;
        uint32_t c[4] = {0u, 0u, 0u, 0u};
        if ((fast & kFastDepth) && whole) {
            const uint2 w = *reinterpret_cast<const uint2*>(row);
            c[0] = w.x & 0xffffu; c[1] = w.x >> 16; c[2] = w.y & 0xffffu; c[3] = w.y >> 16;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < npx) c[k] = reinterpret_cast<const unsigned short*>(row)[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { valid[k] = c[k] != 0u; df[k] = (float)c[k]; }
    } else {
        const unsigned char* row = a.depth + (size_t)a.depth_stride * (size_t)v + (size_t)u0 * 4;
        if ((fast & kFastDepth) && whole) {
            const float4 w = *reinterpret_cast<const float4*>(row);
            df[0] = w.x; df[1] = w.y; df[2] = w.z; df[3] = w.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < npx) df[k] = reinterpret_cast<const float*>(row)[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) valid[k] = __builtin_isfinite(df[k]);
    }

    uint32_t px[4] = {0u, 0u, 0u, 0u};                      // byte 0 | byte 1 << 8 | byte 2 << 16 of each pixel
    if constexpr (COLOR != GEM_COLOR_NONE) {
        const unsigned char* row = a.color + (size_t)a.color_stride * (size_t)v + (size_t)u0 * 3;
        if ((fast & kFastColor) && whole) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(row);
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
            px[0] = w0 & 0xffffffu; px[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8); px[2] = (w1 >> 16) | ((w2 & 0xffu) << 16); px[3] = w2 >> 8;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < npx) px[k] = (uint32_t)row[3 * k] | ((uint32_t)row[3 * k + 1] << 8) | ((uint32_t)row[3 * k + 2] << 16);
        }
        // BGR8: b, g, r in memory -- the word is 0x00RRGGBB already; RGB8: bytes 0 and 2 change places
        if constexpr (COLOR == GEM_COLOR_RGB8) {
#pragma unroll
            for (int k = 0; k < 4; ++k) px[k] = ((px[k] & 0xffu) << 16) | (px[k] & 0xff00u) | (px[k] >> 16);
        }
    }

    const float qnan = __builtin_nanf("");
    const float yv = (float)v - a.cyf;
    const int i0 = v * a.width + u0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < npx) {
            float x = (((float)(u0 + k) - a.cxf) * df[k]) * a.kx;
            float y = (yv * df[k]) * a.ky;
            float z = FMT == GEM_DEPTH_U16 ? df[k] * a.unit : df[k];
            bool keep = valid[k];
            // (the cleanPointCloud mask of the fuse entries, clean_keep of gem_clean.hip: PassThrough on z over the finite points)
            if constexpr (MASK) keep = keep && __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z) && z >= a.z_min && z <= a.z_max;
            if (!keep) { x = qnan; y = qnan; z = qnan; }
            a.xyzi[i0 + k] = make_float4(x, y, z, a.intensity);
        }
    }
    if constexpr (COLOR != GEM_COLOR_NONE) {
        if ((fast & kFastRgbOut) && whole) {
            *reinterpret_cast<uint4*>(a.rgb + i0) = make_uint4(px[0], px[1], px[2], px[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < npx) a.rgb[i0 + k] = px[k];
        }
    }
}

template <int FMT, int COLOR>
static void launch_masked(hipStream_t st, const DepthArgs& a, unsigned blocks, int gw, int lanes, int fast)
{
    if (a.mask) hipLaunchKernelGGL((k_depth_unproject<FMT, COLOR, true>), dim3(blocks), dim3(256), 0, st, a, gw, lanes, fast);
    else hipLaunchKernelGGL((k_depth_unproject<FMT, COLOR, false>), dim3(blocks), dim3(256), 0, st, a, gw, lanes, fast);
}

template <int FMT>
static void launch_coloured(hipStream_t st, const DepthArgs& a, unsigned blocks, int gw, int lanes, int fast)
{
    switch (a.color_format) {
    case GEM_COLOR_BGR8: launch_masked<FMT, GEM_COLOR_BGR8>(st, a, blocks, gw, lanes, fast); break;
    case GEM_COLOR_RGB8: launch_masked<FMT, GEM_COLOR_RGB8>(st, a, blocks, gw, lanes, fast); break;
    default: launch_masked<FMT, GEM_COLOR_NONE>(st, a, blocks, gw, lanes, fast); break;
    }
}

hipError_t launch_depth_unproject(hipStream_t st, const DepthArgs& a)
{
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    const int gw = (a.width + 3) / 4;
    const long long lanes = (long long)gw * a.height;       // <= 2^26
    const unsigned blocks = (unsigned)((lanes + 255) / 256);
    const size_t wide = a.format == GEM_DEPTH_U16 ? 8 : 16;
    int fast = 0;
    if (reinterpret_cast<uintptr_t>(a.depth) % wide == 0 && a.depth_stride % wide == 0) fast |= kFastDepth;
    if (a.color_format != GEM_COLOR_NONE) {
        if (reinterpret_cast<uintptr_t>(a.color) % 4 == 0 && a.color_stride % 4 == 0) fast |= kFastColor;
        if (a.width % 4 == 0 && reinterpret_cast<uintptr_t>(a.rgb) % 16 == 0) fast |= kFastRgbOut;
    }
    if (a.format == GEM_DEPTH_U16) launch_coloured<GEM_DEPTH_U16>(st, a, blocks, gw, (int)lanes, fast);
    else launch_coloured<GEM_DEPTH_F32>(st, a, blocks, gw, (int)lanes, fast);
    return hipGetLastError();
}

} // namespace gem
