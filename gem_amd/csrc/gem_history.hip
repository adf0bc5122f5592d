// gem_history.hip -- the box table of the history cloud, gfx950 (gem_history.hpp).  One workgroup per block of 4096 records: every
// lane folds its 16 records, a shuffle tree folds the wave, four LDS slots fold the workgroup, thread 0 stores the four floats with
// one vector store.  No atomics: whatever the timing, a box holds the same bits for the same records.
#include "gem_history.hpp"
#include "gem_wave.hpp"

namespace gem {

__global__ __launch_bounds__(kCostThreads) void k_history_boxes(const LocalRecord* __restrict__ rec, uint32_t len, uint32_t first_block,
                                                                float4* __restrict__ box)
{
    __shared__ float4 s_box[kCostThreads / 64];
    const uint32_t b = first_block + blockIdx.x;
    const size_t lo = (size_t)b * kCostChunk;
    const size_t hi = lo + kCostChunk < (size_t)len ? lo + kCostChunk : (size_t)len;
    float lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
#pragma unroll 4
    for (int k = 0; k < kCostItems; ++k) {
        const size_t i = lo + (size_t)k * kCostThreads + threadIdx.x;
        if (i < hi) {
            const float2 p = *reinterpret_cast<const float2*>(&rec[i].x);
            lo_x = fminf(lo_x, p.x); hi_x = fmaxf(hi_x, p.x);
            lo_y = fminf(lo_y, p.y); hi_y = fmaxf(hi_y, p.y);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo_x = fminf(lo_x, __shfl_xor(lo_x, off)); hi_x = fmaxf(hi_x, __shfl_xor(hi_x, off));
        lo_y = fminf(lo_y, __shfl_xor(lo_y, off)); hi_y = fmaxf(hi_y, __shfl_xor(hi_y, off));
    }
    if (lane_id() == 0) s_box[threadIdx.x >> 6] = make_float4(lo_x, lo_y, hi_x, hi_y);
    __syncthreads();
    if (threadIdx.x == 0) {
        float4 r = s_box[0];
#pragma unroll
        for (int w = 1; w < kCostThreads / 64; ++w) {
            const float4 v = s_box[w];
            r.x = fminf(r.x, v.x); r.y = fminf(r.y, v.y); r.z = fmaxf(r.z, v.z); r.w = fmaxf(r.w, v.w);
        }
        box[b] = r;
    }
}

hipError_t launch_history_boxes(hipStream_t st, const LocalRecord* rec, long long len, long long first_block, long long n_blocks, float4* box)
{
    if (n_blocks <= 0) return hipSuccess;
    if (len <= 0 || len > 0xffffffffll || first_block < 0 || first_block + n_blocks > history_blocks(len)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_history_boxes, dim3((unsigned)n_blocks), dim3(kCostThreads), 0, st, rec, (uint32_t)len, (uint32_t)first_block, box);
    return hipGetLastError();
}

} // namespace gem
