// gem_global.hip -- the submap stack of ElevationMapping::updateGlobalMap (EMg.cpp:773-905) on the device, gfx950.
//
// A loop closure transforms submaps 1 .. n-1 (k_global_transform) and then runs pair steps (i, k) in the host's order.  A step hashes
// both submaps into their own open-addressing table (k_global_keys: pointCloudtoHash's key in double, the first record of a key wins by
// atomicMin on its position, NaN keys bypass the table) and writes both sides through one stable compaction each (gem_compact.hpp,
// over GlobalSide; the fused keys are its per-wave tally).  A side keeps the first record of every key (and every NaN-key record) in input order and writes it as localHashtoPointCloud writes its entry,
// fused with the other side's first record of the key where the match test of EMg.cpp:858-863 holds.  Counts are read on the device,
// grids are sized from host bounds, so nothing in a step waits for the host.
#include "gem_global.hpp"

#include <limits.h>

namespace gem {

constexpr int kGlobalThreads = 256;                         // k_global_transform, k_global_keys: one record per thread

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

struct GlobalSide : CompactSrc {
    GlobalSideArgs a;
    __device__ size_t size() const { return (size_t)*a.self.count; }
    __device__ int cls(size_t j, Item) const
    {
        const unsigned long long key = a.self.keys[j];
        return global_nan_key(key) || a.self.t.vals[local_find(a.self.t, key)] == (int)j ? 0 : -1;
    }
    // localHashtoPointCloud's record of the entry (EMg.cpp:1128-1137); returns whether it was fused
    __device__ bool emit(int, size_t j, Item, size_t o) const
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
    __device__ void done(uint32_t fused) const                                // one atomic per wave
    {
        if (a.fused && lane_id() == 0 && fused) __hip_atomic_fetch_add(a.fused, fused, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

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
    return compact(st, GlobalSide{{}, a}, bound, block_cnt, total);
}

} // namespace gem
