// gem_frame_sort.hpp -- the sorting networks of frame_tile's owner phase, sized by the wave (internal header).
//
// The owner of a cell sorts the keys (point index << 10 | slot) of its <= kRankMax records; entries at or beyond its count are
// ~0u and sort behind the live keys.  The wave picks the network by its LARGEST count: 2 keys (one exchange), 4 keys (five) or
// 8 keys (nineteen).  All live keys of every lane then lie in the first N entries, the rest is ~0u, so the network over the first
// N entries leaves them in the order the full one would -- tests/cpp/frame_sort_check.cpp runs every permutation through both.
// Compiles for the host alone as well.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace gem {

__host__ __device__ inline void frame_cswap(uint32_t& a, uint32_t& b) { const uint32_t lo = a < b ? a : b, hi = a < b ? b : a; a = lo; b = hi; }

// network size for a wave whose largest count per cell is nmax (1 <= nmax <= 7; a count of 1 needs no key at all)
__host__ __device__ constexpr int frame_sort_size(int nmax) { return nmax <= 2 ? 2 : nmax <= 4 ? 4 : 8; }

// sorts k[0 .. N) ascending: N = 2, 4 or 8
template <int N>
__host__ __device__ inline void frame_sort_keys(uint32_t* k)
{
    static_assert(N == 2 || N == 4 || N == 8, "networks of 2, 4 and 8 keys");
    if constexpr (N == 2) {
        frame_cswap(k[0], k[1]);
    } else if constexpr (N == 4) {
        frame_cswap(k[0], k[1]); frame_cswap(k[2], k[3]);
        frame_cswap(k[0], k[2]); frame_cswap(k[1], k[3]);
        frame_cswap(k[1], k[2]);
    } else {
        frame_cswap(k[0], k[1]); frame_cswap(k[2], k[3]); frame_cswap(k[4], k[5]); frame_cswap(k[6], k[7]);
        frame_cswap(k[0], k[2]); frame_cswap(k[1], k[3]); frame_cswap(k[4], k[6]); frame_cswap(k[5], k[7]);
        frame_cswap(k[1], k[2]); frame_cswap(k[5], k[6]); frame_cswap(k[0], k[4]); frame_cswap(k[3], k[7]);
        frame_cswap(k[1], k[5]); frame_cswap(k[2], k[6]);
        frame_cswap(k[1], k[4]); frame_cswap(k[3], k[6]);
        frame_cswap(k[2], k[4]); frame_cswap(k[3], k[5]);
        frame_cswap(k[3], k[4]);
    }
}

} // namespace gem
