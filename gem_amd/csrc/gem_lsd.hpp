// gem_lsd.hpp -- the stable LSD radix sort over (key, input position) that the VoxelGrid pre-filter (gem_voxel.hip) and the octree
// builder (gem_octree.hip) share (internal header): the record layout of a workgroup, the hand-over to the last workgroup to arrive,
// the scan of the digit histograms and one scatter pass, templated on the key type and on where a pass reads its records.
//
// Records: workgroup b owns positions [b * 4096, b * 4096 + 4096); wave w of it the 512 from b * 4096 + w * 512, item k the 64 from
// there + k * 64.  The order (w, k, lane) IS the position order, so every per-workgroup rank below is stable.
// Hand-overs inside a launch: every workgroup publishes with plain stores / atomics, fences (agent release) and adds one to the
// launch's ticket; the workgroup that draws the last ticket acquires and finishes the step.  Nothing waits for another workgroup.
// The histograms: [nb][kLsdBins] words, two of them taking turns, all-zero between sorts.  The kernel in front of pass 0 counts
// digit 0 of every record into its own workgroup's row and has the last arriver scan it (lsd_scan_hist); pass k counts digit k + 1
// into the row of the workgroup that will hold the record in pass k + 1 and zeroes the row it read.
#pragma once

#include "gem_wave.hpp"

namespace gem {

constexpr int kLsdThreads = 512;                      // 8 waves
constexpr int kLsdItems = 8;                          // records per thread
constexpr int kLsdTile = kLsdThreads * kLsdItems;     // records per workgroup (4096)
constexpr int kLsdDigit = 11;                         // bits per pass
constexpr int kLsdBins = 1 << kLsdDigit;

static_assert(kLsdThreads * 4 == kLsdBins, "thread t owns digits 4t .. 4t + 3");

__device__ __forceinline__ long long lsd_pos(int k)
{
    return (long long)blockIdx.x * kLsdTile + (long long)(threadIdx.x >> 6) * (64 * kLsdItems) + k * 64 + lane_id();
}

// every thread fences its own stores / atomics (agent release), ONE lane draws a ticket; true in the workgroup that drew the last
// one (which resets the ticket for the next launch and acquires: its loads below see every other workgroup's data)
__device__ __forceinline__ bool last_arrival(uint32_t* ticket, int nb, uint32_t* s_flag)
{
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = t == (uint32_t)nb - 1u;
        if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *s_flag = last ? 1u : 0u;
    }
    __syncthreads();
    const bool last = *s_flag != 0u;
    if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return last;
}

// in place: counts [nb][kLsdBins] -> the position of every (workgroup, digit) run in the next pass's output (digit-major, then
// workgroup).  One workgroup of kLsdThreads; thread t owns digits 4t .. 4t + 3.
__device__ inline void lsd_scan_hist(uint32_t* hist, int nb, uint32_t* s_scan)
{
    uint4* h4 = reinterpret_cast<uint4*>(hist);
    uint4 tot = make_uint4(0u, 0u, 0u, 0u);
    for (int b = 0; b < nb; ++b) {
        const uint4 v = h4[(size_t)b * (kLsdBins / 4) + threadIdx.x];
        tot.x += v.x; tot.y += v.y; tot.z += v.z; tot.w += v.w;
    }
    uint32_t all;
    const uint32_t ex = block_exclusive_scan<kLsdThreads>(tot.x + tot.y + tot.z + tot.w, s_scan, &all);
    uint4 run = make_uint4(ex, ex + tot.x, ex + tot.x + tot.y, ex + tot.x + tot.y + tot.z);
    for (int b = 0; b < nb; ++b) {
        const uint4 v = h4[(size_t)b * (kLsdBins / 4) + threadIdx.x];
        h4[(size_t)b * (kLsdBins / 4) + threadIdx.x] = run;
        run.x += v.x; run.y += v.y; run.z += v.z; run.w += v.w;
    }
}

// One pass over digit (key >> shift) & (kLsdBins - 1).  load(j, key, src) gives the record at position j of the pass's input and
// whether there is one.  hist_cur: this pass's scanned histogram (the workgroup's row is zeroed behind the read).  MAY_COUNT: a pass
// can follow this one (false: the counting code is not compiled, so a key type's last pass never forms the shift past its width);
// then, with count_next, digit shift + kLsdDigit is counted into hist_next and the last arriver scans it.
template <class Key, bool MAY_COUNT, class Load>
__device__ __forceinline__ void lsd_scatter_pass(int shift, bool count_next, Load load, Key* key_out, uint32_t* src_out,
                                                 uint32_t* hist_cur, uint32_t* hist_next, uint32_t* ticket, int nb)
{
    constexpr int NW = kLsdThreads / 64;
    __shared__ uint32_t s_off[kLsdBins];
    __shared__ uint16_t s_w[NW][kLsdBins];               // per wave: running count per digit, then the waves' exclusive prefix
    __shared__ uint32_t s_scan[16];
    __shared__ uint32_t s_last;
    {   // this workgroup's run positions; the row is zeroed behind the read (the pass after the next counts into it)
        uint4* row = reinterpret_cast<uint4*>(hist_cur) + (size_t)blockIdx.x * (kLsdBins / 4);
        reinterpret_cast<uint4*>(s_off)[threadIdx.x] = row[threadIdx.x];
        row[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
        uint32_t* w32 = reinterpret_cast<uint32_t*>(&s_w[0][0]);
        for (int i = threadIdx.x; i < NW * kLsdBins / 2; i += kLsdThreads) w32[i] = 0u;
    }
    __syncthreads();
    const int w = (int)(threadIdx.x >> 6);
    const uint64_t lt = lanemask_lt();
    Key key[kLsdItems];
    uint32_t src[kLsdItems], rank[kLsdItems];
    bool valid[kLsdItems];
#pragma unroll
    for (int k = 0; k < kLsdItems; ++k) {
        key[k] = 0; src[k] = 0u;
        valid[k] = load(lsd_pos(k), key[k], src[k]);
        const uint32_t d = (uint32_t)(key[k] >> shift) & (kLsdBins - 1);
        const uint64_t peers = wave_peers(valid[k], d, kLsdDigit);
        const uint32_t before = (uint32_t)__popcll(peers & lt);
        rank[k] = 0u;
        if (valid[k]) {
            const uint32_t run = s_w[w][d];
            rank[k] = run + before;
            if (before == 0u) s_w[w][d] = (uint16_t)(run + (uint32_t)__popcll(peers));
        }
    }
    __syncthreads();
    for (int d = threadIdx.x; d < kLsdBins; d += kLsdThreads) {
        uint32_t acc = 0u;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) { const uint32_t c = s_w[ww][d]; s_w[ww][d] = (uint16_t)acc; acc += c; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kLsdItems; ++k) {
        const uint32_t d = (uint32_t)(key[k] >> shift) & (kLsdBins - 1);
        uint32_t p = 0u;
        if (valid[k]) {
            p = s_off[d] + s_w[w][d] + rank[k];
            key_out[p] = key[k];
            src_out[p] = src[k];
        }
        if constexpr (MAY_COUNT) if (count_next) {        // the record's next digit, counted for the workgroup that reads it next
            const uint32_t comb = (p / (uint32_t)kLsdTile) * (uint32_t)kLsdBins + ((uint32_t)(key[k] >> (shift + kLsdDigit)) & (kLsdBins - 1));
            const uint64_t pe = wave_peers_few(valid[k], comb, 32);
            if (valid[k] && (pe & lt) == 0ull) atomicAdd(&hist_next[comb], (uint32_t)__popcll(pe));
        }
    }
    if constexpr (MAY_COUNT) {
        if (count_next && last_arrival(ticket, nb, &s_last)) lsd_scan_hist(hist_next, nb, s_scan);
    }
}

} // namespace gem
