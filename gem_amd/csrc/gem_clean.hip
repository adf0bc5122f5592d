// gem_clean.hip -- cleanPointCloud (SensorProcessorBase.cpp:89) on the device, gfx950.
//
// One stable stream compaction (gem_compact.hpp) over CleanSrc: a point is loaded once per kernel and stays in registers until it is
// written, so the scatter reads nothing twice.  k_clean_mask is the fuse path's form: no compaction, dropped points get NaN.
#include "gem_clean.hpp"

namespace gem {

__device__ __forceinline__ bool clean_keep(float x, float y, float z, int mode, float z_min, float z_max)
{
    if (mode == GEM_CLEAN_NONE) return true;
    const bool finite = __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);   // pcl::removeNaNFromPointCloud
    return mode == GEM_CLEAN_PASSTHROUGH_Z ? finite && z >= z_min && z <= z_max : finite;           // pcl::PassThrough<PointT> on z (float limits)
}

template <bool SOA>
__device__ __forceinline__ float4 clean_load(const CleanArgs& a, size_t i)
{
    if constexpr (SOA) return make_float4(a.x[i], a.y[i], a.z[i], 0.0f);
    else return a.xyzi[i];
}

template <bool SOA>
struct CleanSrc : CompactSrc {
    CleanArgs a;
    struct Item { float4 p; uint32_t rgb; };
    __device__ bool with_rgb() const { return !SOA && a.rgb && a.rgb_out; }
    __device__ size_t size() const { return (size_t)a.n; }
    __device__ Item load(size_t i) const { return {clean_load<SOA>(a, i), with_rgb() ? a.rgb[i] : 0u}; }
    __device__ int cls(size_t, const Item& v) const { return clean_keep(v.p.x, v.p.y, v.p.z, a.mode, a.z_min, a.z_max) ? 0 : -1; }
    __device__ bool emit(int, size_t i, const Item& v, size_t o) const
    {
        if constexpr (SOA) {
            if (a.x_out) a.x_out[o] = v.p.x;
            if (a.y_out) a.y_out[o] = v.p.y;
            if (a.z_out) a.z_out[o] = v.p.z;
        } else {
            if (a.xyzi_out) a.xyzi_out[o] = v.p;
            if (with_rgb()) a.rgb_out[o] = v.rgb;
        }
        if (a.orig_out) a.orig_out[o] = (int)i;
        return false;
    }
};

// (in == out is allowed: each point is read and written by one thread)
__global__ __launch_bounds__(256) void k_clean_mask(const float4* in, float4* out, long long n, int mode,
                                                    float z_min, float z_max)
{
    const float qnan = __builtin_nanf("");
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * blockDim.x) {
        float4 v = in[i];
        if (!clean_keep(v.x, v.y, v.z, mode, z_min, z_max)) { v.x = qnan; v.y = qnan; v.z = qnan; }
        out[i] = v;
    }
}

static inline unsigned stride_grid(long long work, int block)
{
    const long long g = (work + block - 1) / block;
    return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));           // grid-stride beyond 2 M threads
}

hipError_t launch_clean(hipStream_t st, const CleanArgs& a, bool soa)
{
    uint32_t* const count = reinterpret_cast<uint32_t*>(a.count_out);       // a count fits both
    return soa ? compact(st, CleanSrc<true>{{}, a}, a.n, a.block_cnt, count) : compact(st, CleanSrc<false>{{}, a}, a.n, a.block_cnt, count);
}

hipError_t launch_clean_mask(hipStream_t st, const float4* in, float4* out, long long n, int mode, float z_min, float z_max)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_clean_mask, dim3(stride_grid(n, 256)), dim3(256), 0, st, in, out, n, mode, z_min, z_max);
    return hipGetLastError();
}

} // namespace gem
