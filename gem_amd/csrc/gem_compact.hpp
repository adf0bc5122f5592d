// gem_compact.hpp -- the one stable stream compaction of the gfx950 kernels (internal header; DESIGN.md section 7a has the form).
//
// Three launches, so that no workgroup ever waits for another one (no look-back, no flag to spin on: the kernel boundaries are the
// only hand-overs):
//   compact_count    workgroup b counts the items of every class among its 1024 (one ballot + s_bcnt1 per wave, item and class)
//   compact_scan     ONE workgroup per class turns the counts into exclusive offsets (chunks of 1024 with a running carry) and
//                    writes the class total
//   compact_scatter  workgroup b ranks its items (ballot + mbcnt inside the wave, the waves' counts through LDS) and writes them
// Thread t of workgroup b takes items b * 1024 + k * 256 + t, k = 0..3: every wave load is 64 consecutive items, and the order
// (k, wave, lane) IS the input order, which keeps the compaction stable.  Positions are 64-bit throughout.
//
// What is compacted is a source type, passed by value to both kernels:
//   kCounted, kWritten   classes counted (scratch and totals are [class][block] and [class]) and, the first of them, written
//   size()               items, a host value or a device word
//   Item, load(i)        what a thread keeps of item i (< size()) in registers from its load to its write; every load of a tile is
//                        issued before the first cls.  CompactSrc's empty Item costs nothing.
//   cls(i, item)         the item's class; anything outside [0, kCounted) drops it
//   writes(j)            whether class j is written at all (workgroup-uniform)
//   emit(j, i, item, o)  writes item i as entry o of class j; returns whether it counts towards the wave's tally
//   done(tally)          called once by every lane with its wave's tally (wave-uniform)
#pragma once

#include "gem_wave.hpp"

#include <limits.h>

namespace gem {

constexpr int kCompactThreads = 256;                                // one workgroup = 4 waves
constexpr int kCompactItems = 4;                                    // items per thread
constexpr int kCompactTile = kCompactThreads * kCompactItems;       // items per workgroup (1024)
constexpr int kCompactScanThreads = 1024;                           // block counts per trip of the scan

// workgroups of a compaction over n items = words of scratch per counted class
inline long long compact_blocks(long long n) { return n > 0 ? (n + kCompactTile - 1) / kCompactTile : 0; }

// the defaults of a source: one class, always written, nothing held in registers, no tally
struct CompactSrc {
    static constexpr int kCounted = 1, kWritten = 1;
    struct Item {};
    __device__ Item load(size_t) const { return {}; }
    __device__ bool writes(int) const { return true; }
    __device__ void done(uint32_t) const {}
};

template <class Src>
__global__ __launch_bounds__(kCompactThreads) void compact_count(Src src, uint32_t nb, uint32_t* __restrict__ block_cnt)
{
    constexpr int NW = kCompactThreads / 64, NC = Src::kCounted;
    __shared__ uint32_t s_w[NC * NW];
    const size_t base = (size_t)blockIdx.x * kCompactTile, n = src.size();
    typename Src::Item v[kCompactItems];                                    // past the end: never set, never read
#pragma unroll
    for (int k = 0; k < kCompactItems; ++k) {
        const size_t i = base + (size_t)k * kCompactThreads + threadIdx.x;
        if (i < n) v[k] = src.load(i);
    }
    uint32_t c[NC] = {};
#pragma unroll
    for (int k = 0; k < kCompactItems; ++k) {
        const size_t i = base + (size_t)k * kCompactThreads + threadIdx.x;
        const int cls = i < n ? src.cls(i, v[k]) : -1;
#pragma unroll
        for (int j = 0; j < NC; ++j) c[j] += (uint32_t)__popcll(__ballot(cls == j));     // wave-uniform: s_bcnt1
    }
    if (lane_id() == 0) {
#pragma unroll
        for (int j = 0; j < NC; ++j) s_w[j * NW + (threadIdx.x >> 6)] = c[j];
    }
    __syncthreads();
    if (threadIdx.x < NC) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += s_w[threadIdx.x * NW + w];
        block_cnt[(size_t)threadIdx.x * nb + blockIdx.x] = t;
    }
}

// workgroup j scans the counts of class j (a template like the other two, so that a file that only sizes scratch emits no kernel)
template <int NT>
__global__ __launch_bounds__(NT) void compact_scan(uint32_t* __restrict__ cnt_all, int nb, uint32_t* __restrict__ totals)
{
    __shared__ uint32_t s[16];
    uint32_t* cnt = cnt_all + (size_t)blockIdx.x * nb;
    uint32_t carry = 0;
    for (int b0 = 0; b0 < nb; b0 += NT) {                                 // workgroup-uniform trip count
        const int i = b0 + (int)threadIdx.x;
        const uint32_t v = i < nb ? cnt[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<NT>(v, s, &tot);
        if (i < nb) cnt[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

template <class Src>
__global__ __launch_bounds__(kCompactThreads) void compact_scatter(Src src, uint32_t nb, const uint32_t* __restrict__ block_off)
{
    constexpr int NW = kCompactThreads / 64, NC = Src::kWritten;
    __shared__ uint32_t s_cnt[NC * kCompactItems * NW];
    const size_t base = (size_t)blockIdx.x * kCompactTile, n = src.size();
    const int w = (int)(threadIdx.x >> 6);
    typename Src::Item v[kCompactItems];                                    // past the end: never set, never read
#pragma unroll
    for (int k = 0; k < kCompactItems; ++k) {
        const size_t i = base + (size_t)k * kCompactThreads + threadIdx.x;
        if (i < n) v[k] = src.load(i);
    }
    uint64_t m[NC][kCompactItems];
#pragma unroll
    for (int k = 0; k < kCompactItems; ++k) {
        const size_t i = base + (size_t)k * kCompactThreads + threadIdx.x;
        const int cls = i < n ? src.cls(i, v[k]) : -1;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            m[j][k] = __ballot(cls == j);
            if (lane_id() == 0) s_cnt[(j * kCompactItems + k) * NW + w] = (uint32_t)__popcll(m[j][k]);
        }
    }
    __syncthreads();
    uint32_t tally = 0;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        if (!src.writes(j)) continue;                                        // workgroup-uniform
        uint32_t run = block_off[(size_t)j * nb + blockIdx.x];              // class-j items of the workgroups before this one
#pragma unroll
        for (int k = 0; k < kCompactItems; ++k) {
            uint32_t before = 0, total = 0;
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) {
                const uint32_t cw = s_cnt[(j * kCompactItems + k) * NW + ww];
                before += ww < w ? cw : 0u;
                total += cw;
            }
            bool t = false;
            if ((m[j][k] >> lane_id()) & 1ull)
                t = src.emit(j, base + (size_t)k * kCompactThreads + threadIdx.x, v[k], (size_t)run + before + wave_rank(m[j][k]));
            tally += (uint32_t)__popcll(__ballot(t));                        // wave-uniform
            run += total;
        }
    }
    src.done(tally);
}

// The launches of one compaction over at most `bound` items on `st`.  block_cnt: [kCounted][compact_blocks(bound)] scratch, counts
// and then their exclusive prefixes; totals: [kCounted] (device).  count: the first two launches; scatter: the third, which needs
// the first two done on the same scratch.  No workgroups (bound <= 0): count only zeroes the totals.
template <class Src>
hipError_t compact(hipStream_t st, const Src& src, long long bound, uint32_t* block_cnt, uint32_t* totals, bool count = true,
                   bool scatter = true)
{
    const long long nb = compact_blocks(bound);
    if (nb > INT_MAX) return hipErrorInvalidValue;
    if (nb == 0) return count ? hipMemsetAsync(totals, 0, Src::kCounted * sizeof(uint32_t), st) : hipSuccess;
    if (count) {
        hipLaunchKernelGGL(compact_count<Src>, dim3((unsigned)nb), dim3(kCompactThreads), 0, st, src, (uint32_t)nb, block_cnt);
        hipLaunchKernelGGL(compact_scan<kCompactScanThreads>, dim3(Src::kCounted), dim3(kCompactScanThreads), 0, st, block_cnt, (int)nb, totals);
    }
    if (scatter)
        hipLaunchKernelGGL(compact_scatter<Src>, dim3((unsigned)nb), dim3(kCompactThreads), 0, st, src, (uint32_t)nb, block_cnt);
    return hipGetLastError();
}

} // namespace gem
