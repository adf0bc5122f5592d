// gem_global.hip -- the submap stack of ElevationMapping::updateGlobalMap (EMg.cpp:773-905) on the device, gfx950.
//
// A loop closure transforms submaps 1 .. n-1 (k_global_transform) and then runs pair steps (i, k) in the host's order.  A step hashes
// both submaps into their own open-addressing table (k_global_keys: pointCloudtoHash's key in double, the first record of a key wins by
// atomicMin on its position, NaN keys bypass the table) and writes both sides through one stable compaction each, in gem_clean.hip's
// form: k_global_count -> k_global_scan -> k_global_scatter.  Thread t of workgroup b takes items b * 1024 + k * 256 + t, k = 0..3: the
// order (k, wave, lane) IS the item order, ranked by ballot + mbcnt inside the wave and the waves' counts through LDS.  A side keeps
// the first record of every key (and every NaN-key record) in input order and writes it as localHashtoPointCloud writes its entry,
// fused with the other side's first record of the key where the match test of EMg.cpp:858-863 holds.  Counts are read on the device,
// grids are sized from host bounds, so nothing in a step waits for the host.
#include "gem_global.hpp"
#include "gem_wave.hpp"

#include <limits.h>

namespace gem {

__device__ __forceinline__ uint32_t global_wave_rank(uint64_t m)       // kept lanes below this one
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ bool global_nan_key(unsigned long long key)
{
    const float x = __uint_as_float((uint32_t)key), y = __uint_as_float((uint32_t)(key >> 32));
    return x != x || y != y;
}

// pointCloudtoHash (EMg.cpp:1184-1185): (float) (ceil(x / res) * res - res / 2.0), in double
__device__ __forceinline__ float global_quantise(float v, double res)
{
    return (float)__dsub_rn(__dmul_rn(ceil(__ddiv_rn((double)v, res)), res), __ddiv_rn(res, 2.0));
}

// x' = x * m00 + (y * m01 + (z * m02 + m03)), rows 0..3 into x, y, z, pad; every product and sum rounded in float
__global__ __launch_bounds__(kGlobalThreads) void k_global_transform(LocalRecord* __restrict__ rec, long long n, GlobalXform m)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    LocalRecord r = rec[j];
    float o[4];
#pragma unroll
    for (int row = 0; row < 4; ++row)
        o[row] = __fadd_rn(__fmul_rn(r.x, m.m[row]), __fadd_rn(__fmul_rn(r.y, m.m[4 + row]), __fadd_rn(__fmul_rn(r.z, m.m[8 + row]), m.m[12 + row])));
    r.x = o[0]; r.y = o[1]; r.z = o[2]; r.pad = o[3];
    rec[j] = r;
}

__global__ __launch_bounds__(kGlobalThreads) void k_global_keys(GlobalCloud c, double res)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (long long)*c.count) return;
    const LocalRecord& r = c.rec[j];
    const unsigned long long key = local_key(global_quantise(r.x, res), global_quantise(r.y, res));
    c.keys[j] = key;
    if (!global_nan_key(key)) local_upsert<LocalWins::First>(c.t, key, (int)j);
}

struct GlobalSide {
    GlobalSideArgs a;
    __device__ size_t size() const { return (size_t)*a.self.count; }
    __device__ bool keep(size_t j) const
    {
        const unsigned long long key = a.self.keys[j];
        return global_nan_key(key) || a.self.t.vals[local_find(a.self.t, key)] == (int)j;
    }
    // localHashtoPointCloud's record of the entry (EMg.cpp:1128-1137); returns whether it was fused
    __device__ bool emit(size_t j, size_t o) const
    {
        const LocalRecord& r = a.self.rec[j];
        const unsigned long long key = a.self.keys[j];
        LocalRecord w;
        w.x = __uint_as_float((uint32_t)key); w.y = __uint_as_float((uint32_t)(key >> 32));
        w.z = r.z; w.pad = 1.0f; w.bgra = r.bgra & 0x00ffffffu;
        w.covariance = r.covariance; w.intensity = r.intensity; w.travers = r.travers;
        bool fused = false;
        if (!global_nan_key(key)) {
            const unsigned long long s = local_find(a.other.t, key);
            if (a.other.t.keys[s] == key) {
                const LocalRecord& q = a.other.rec[a.other.t.vals[s]];
                const LocalRecord& nw = a.self_is_new ? r : q;
                const LocalRecord& od = a.self_is_new ? q : r;
                if (od.covariance > 0.0f && od.covariance < 1.0f) {            // EMg.cpp:858
                    // EMg.cpp:862-863 as C++ precedence parses them (pow(v, 2) of a float is exact in double)
                    const double nv = (double)nw.covariance, ov = (double)od.covariance, ne = (double)nw.z, oe = (double)od.z;
                    const double nv2 = nv * nv, ov2 = ov * ov;
                    w.z = (float)(((nv2 * oe) + ((ov2 * ne) / ov2)) + nv2);
                    w.covariance = (float)(((ov2 * nv2) / ov2) + nv2);
                    w.bgra = nw.bgra & 0x00ffffffu; w.intensity = nw.intensity; w.travers = nw.travers;
                    fused = true;
                }
            }
        }
        a.out[o] = w;
        return fused;
    }
};

__global__ __launch_bounds__(kGlobalThreads) void k_global_count(GlobalSide src, uint32_t* __restrict__ block_cnt)
{
    __shared__ uint32_t s_w[kGlobalThreads / 64];
    const size_t base = (size_t)blockIdx.x * kGlobalTile, n = src.size();
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < kGlobalItems; ++k) {
        const size_t i = base + (size_t)k * kGlobalThreads + threadIdx.x;
        c += (uint32_t)__popcll(__ballot(i < n && src.keep(i)));           // wave-uniform: s_bcnt1
    }
    if (lane_id() == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kGlobalThreads / 64; ++w) t += s_w[w];
        block_cnt[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kGlobalThreads) void k_global_scan(uint32_t* __restrict__ cnt, int nb, uint32_t* __restrict__ total)
{
    __shared__ uint32_t s[16];
    uint32_t carry = 0;
    for (int b0 = 0; b0 < nb; b0 += kGlobalThreads) {                      // workgroup-uniform trip count
        const int i = b0 + (int)threadIdx.x;
        const uint32_t v = i < nb ? cnt[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<kGlobalThreads>(v, s, &tot);
        if (i < nb) cnt[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(kGlobalThreads) void k_global_scatter(GlobalSide src, const uint32_t* __restrict__ block_off)
{
    constexpr int NW = kGlobalThreads / 64;
    __shared__ uint32_t s_cnt[kGlobalItems * NW];
    const size_t base = (size_t)blockIdx.x * kGlobalTile, n = src.size();
    const int w = (int)(threadIdx.x >> 6);
    uint64_t m[kGlobalItems];
#pragma unroll
    for (int k = 0; k < kGlobalItems; ++k) {
        const size_t i = base + (size_t)k * kGlobalThreads + threadIdx.x;
        m[k] = __ballot(i < n && src.keep(i));
        if (lane_id() == 0) s_cnt[k * NW + w] = (uint32_t)__popcll(m[k]);
    }
    __syncthreads();
    uint32_t run = block_off[blockIdx.x];                                   // kept items of the workgroups before this one
    uint32_t fused = 0;
#pragma unroll
    for (int k = 0; k < kGlobalItems; ++k) {
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) {
            const uint32_t cw = s_cnt[k * NW + ww];
            before += ww < w ? cw : 0u;
            total += cw;
        }
        bool f = false;
        if ((m[k] >> lane_id()) & 1ull)
            f = src.emit(base + (size_t)k * kGlobalThreads + threadIdx.x, (size_t)run + before + global_wave_rank(m[k]));
        fused += (uint32_t)__popcll(__ballot(f));                            // wave-uniform
        run += total;
    }
    if (src.a.fused && lane_id() == 0 && fused)
        __hip_atomic_fetch_add(src.a.fused, fused, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

hipError_t launch_global_transform(hipStream_t st, LocalRecord* rec, long long n, const GlobalXform& m)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_global_transform, dim3((unsigned)((n + kGlobalThreads - 1) / kGlobalThreads)), dim3(kGlobalThreads), 0, st, rec, n, m);
    return hipGetLastError();
}

hipError_t launch_global_keys(hipStream_t st, const GlobalCloud& c, long long bound, double res)
{
    const size_t cap = (size_t)c.t.mask + 1;
    hipError_t e;
    if ((e = hipMemsetAsync(c.t.keys, 0xff, cap * 8, st)) != hipSuccess) return e;                        // kLocalEmpty
    if ((e = hipMemsetD32Async((hipDeviceptr_t)c.t.vals, INT_MAX, cap, st)) != hipSuccess) return e;       // above every position
    if (bound <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_global_keys, dim3((unsigned)((bound + kGlobalThreads - 1) / kGlobalThreads)), dim3(kGlobalThreads), 0, st, c, res);
    return hipGetLastError();
}

hipError_t launch_global_side(hipStream_t st, const GlobalSideArgs& a, long long bound, uint32_t* block_cnt, uint32_t* total)
{
    const unsigned nb = global_blocks(bound);
    if (nb == 0) return hipMemsetAsync(total, 0, sizeof(uint32_t), st);
    const GlobalSide src{a};
    hipLaunchKernelGGL(k_global_count, dim3(nb), dim3(kGlobalThreads), 0, st, src, block_cnt);
    hipLaunchKernelGGL(k_global_scan, dim3(1), dim3(kGlobalThreads), 0, st, block_cnt, (int)nb, total);
    hipLaunchKernelGGL(k_global_scatter, dim3(nb), dim3(kGlobalThreads), 0, st, src, block_cnt);
    return hipGetLastError();
}

} // namespace gem
