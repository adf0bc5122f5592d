// gem_clean.hip -- cleanPointCloud (SensorProcessorBase.cpp:89) on the device, gfx950.
//
// Stable stream compaction in the form of the counting sort of gem_sort.hip: three launches, so that no workgroup ever waits for
// another one (no look-back, no flag to spin on: the kernel boundaries are the only hand-overs).
//   k_clean_count    workgroup b counts the kept points of its 1024 (one ballot + s_bcnt1 per wave and item)
//   k_clean_scan     ONE workgroup turns the counts into exclusive offsets (chunks of 1024 with a running carry) and writes the total
//   k_clean_scatter  workgroup b ranks its kept points (ballot + mbcnt inside the wave, the waves' counts through LDS) and writes them
// Thread t of workgroup b takes points b * 1024 + k * 256 + t, k = 0..3: every wave load is 64 consecutive points, and the order
// (k, wave, lane) IS the input order, which keeps the compaction stable.  Positions are 64-bit throughout.
#include "gem_clean.hpp"
#include "gem_wave.hpp"

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

__device__ __forceinline__ uint32_t wave_rank(uint64_t m)        // kept lanes below this one
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

template <bool SOA>
__global__ __launch_bounds__(kCleanThreads) void k_clean_count(CleanArgs a)
{
    __shared__ uint32_t s_w[kCleanThreads / 64];
    const size_t base = (size_t)blockIdx.x * kCleanTile, n = (size_t)a.n;
    float4 v[kCleanItems];
#pragma unroll
    for (int k = 0; k < kCleanItems; ++k) {
        const size_t i = base + (size_t)k * kCleanThreads + threadIdx.x;
        v[k] = i < n ? clean_load<SOA>(a, i) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < kCleanItems; ++k) {
        const size_t i = base + (size_t)k * kCleanThreads + threadIdx.x;
        const bool keep = i < n && clean_keep(v[k].x, v[k].y, v[k].z, a.mode, a.z_min, a.z_max);
        c += (uint32_t)__popcll(__ballot(keep));                  // wave-uniform: s_bcnt1
    }
    if (lane_id() == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kCleanThreads / 64; ++w) t += s_w[w];
        a.block_cnt[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(1024) void k_clean_scan(uint32_t* __restrict__ cnt, int nb, int* __restrict__ count_out)
{
    __shared__ uint32_t s[16];
    uint32_t carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 1024) {                       // workgroup-uniform trip count
        const int i = b0 + (int)threadIdx.x;
        const uint32_t v = i < nb ? cnt[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<1024>(v, s, &tot);
        if (i < nb) cnt[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *count_out = (int)carry;
}

template <bool SOA>
__global__ __launch_bounds__(kCleanThreads) void k_clean_scatter(CleanArgs a)
{
    constexpr int NW = kCleanThreads / 64;
    __shared__ uint32_t s_cnt[kCleanItems * NW];
    const size_t base = (size_t)blockIdx.x * kCleanTile, n = (size_t)a.n;
    const int w = (int)(threadIdx.x >> 6);
    const bool with_rgb = !SOA && a.rgb && a.rgb_out;
    float4 v[kCleanItems];
    uint32_t c[kCleanItems];
#pragma unroll
    for (int k = 0; k < kCleanItems; ++k) {
        const size_t i = base + (size_t)k * kCleanThreads + threadIdx.x;
        v[k] = i < n ? clean_load<SOA>(a, i) : make_float4(0.f, 0.f, 0.f, 0.f);
        c[k] = with_rgb && i < n ? a.rgb[i] : 0u;
    }
    uint64_t m[kCleanItems];
#pragma unroll
    for (int k = 0; k < kCleanItems; ++k) {
        const size_t i = base + (size_t)k * kCleanThreads + threadIdx.x;
        m[k] = __ballot(i < n && clean_keep(v[k].x, v[k].y, v[k].z, a.mode, a.z_min, a.z_max));
        if (lane_id() == 0) s_cnt[k * NW + w] = (uint32_t)__popcll(m[k]);
    }
    __syncthreads();
    uint32_t run = a.block_cnt[blockIdx.x];                       // kept points of the workgroups before this one
#pragma unroll
    for (int k = 0; k < kCleanItems; ++k) {
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) {
            const uint32_t cw = s_cnt[k * NW + ww];
            before += ww < w ? cw : 0u;
            total += cw;
        }
        if ((m[k] >> lane_id()) & 1ull) {
            const size_t o = (size_t)run + before + wave_rank(m[k]);
            const size_t i = base + (size_t)k * kCleanThreads + threadIdx.x;
            if constexpr (SOA) {
                if (a.x_out) a.x_out[o] = v[k].x;
                if (a.y_out) a.y_out[o] = v[k].y;
                if (a.z_out) a.z_out[o] = v[k].z;
            } else {
                if (a.xyzi_out) a.xyzi_out[o] = v[k];
                if (with_rgb) a.rgb_out[o] = c[k];
            }
            if (a.orig_out) a.orig_out[o] = (int)i;
        }
        run += total;
    }
}

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
    if (a.n <= 0) return hipMemsetAsync(a.count_out, 0, sizeof(int), st);
    const long long nb = clean_blocks(a.n);
    if (nb > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(soa ? k_clean_count<true> : k_clean_count<false>, dim3((unsigned)nb), dim3(kCleanThreads), 0, st, a);
    hipLaunchKernelGGL(k_clean_scan, dim3(1), dim3(1024), 0, st, a.block_cnt, (int)nb, a.count_out);
    hipLaunchKernelGGL(soa ? k_clean_scatter<true> : k_clean_scatter<false>, dim3((unsigned)nb), dim3(kCleanThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_clean_mask(hipStream_t st, const float4* in, float4* out, long long n, int mode, float z_min, float z_max)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_clean_mask, dim3(stride_grid(n, 256)), dim3(256), 0, st, in, out, n, mode, z_min, z_max);
    return hipGetLastError();
}

} // namespace gem
