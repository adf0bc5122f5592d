// gem_local.hpp -- the rolling-window local map on the device (internal header): argument blocks and host launchers of gem_local.hip.
//   capture  stable compaction of the cells ElevationMap::show keeps (EM.cpp:101) into 32-byte records + their linear indices
//   spill    the L-shaped band of the previous capture that left the window (EMg.cpp:715-764), appended to the local map's log
//   insert   upsert of log entries into the open-addressing table (key -> log position, the larger position wins)
//   export   stable compaction of the live log entries (an entry is live while the table points at it)
// Every compaction is gem_compact.hpp's.
#pragma once

#include "gem_compact.hpp"
#include "gem_kernels.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gem {

constexpr unsigned long long kLocalEmpty = ~0ull;           // empty table slot: the bits of the key (NaN, NaN), never a finite position

// PointXYZRGBICT (include/gem/gem.hpp): x, y, z, pad | b, g, r, a | covariance, intensity, travers
struct LocalRecord {
    float x, y, z, pad;
    uint32_t bgra;
    float covariance, intensity, travers;
};
static_assert(sizeof(LocalRecord) == 32, "PointXYZRGBICT is 32 bytes");

// grid_map's getPositionFromIndex for a capture: (px + off) - res * unwrapped index, off = 0.5 * map_length - 0.5 * resolution
struct LocalGeom {
    double off, res, px, py;
    int L, sx, sy;
};

// getPositionFromIndex of the cell at linear index `lin` (the formula of k_show_emit)
__device__ __forceinline__ void local_position(const LocalGeom& g, size_t lin, double& x, double& y)
{
    const int ix = (int)(lin % (size_t)g.L), iy = (int)(lin / (size_t)g.L);
    int ux = ix - g.sx, uy = iy - g.sy;                                     // getIndexFromBufferIndex
    ux += ux < 0 ? g.L : 0; uy += uy < 0 ? g.L : 0;
    x = (g.px + g.off) + g.res * (double)(-ux);
    y = (g.py + g.off) + g.res * (double)(-uy);
}

struct LocalCaptureArgs {
    LayerPtrs m; LocalGeom g;
    LocalRecord* rec; int* lin;         // [L^2] the kept cells in iteration order, their linear (column-major buffer) index
};

struct LocalSpillArgs {
    const LocalRecord* rec; const int* lin; const uint32_t* count;   // the previous capture
    LocalGeom g;
    double lo_x, hi_x, lo_y, hi_y;      // current_{x,y} -/+ length * resolution / 2 (double)
    float dx, dy;                       // position_shift (float compares)
    LocalRecord* out;                   // the log, at its current length
};

struct LocalTable {
    unsigned long long* keys;           // [cap] (x bits | y bits << 32), -0 stored as +0; kLocalEmpty when free
    int* vals;                          // [cap] log position, -1 when free
    unsigned long long mask;            // cap - 1 (cap a power of two)
};

struct LocalExportArgs {
    const LocalRecord* log; long long n;
    LocalTable t;
    LocalRecord* out;
};

// The table's device side, shared by the local map (gem_local.hip) and the submap stack (gem_global.hip).
__device__ __forceinline__ unsigned long long local_key(float x, float y)
{
    x = x == 0.0f ? 0.0f : x;                                               // -0 == +0 (GridPointEqual compares floats)
    y = y == 0.0f ? 0.0f : y;
    return (unsigned long long)__float_as_uint(x) | ((unsigned long long)__float_as_uint(y) << 32);
}

__device__ __forceinline__ unsigned long long local_hash(unsigned long long k)      // murmur3's 64-bit finaliser
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    return k ^ (k >> 33);
}

__device__ __forceinline__ unsigned long long local_find(const LocalTable& t, unsigned long long key)
{
    unsigned long long s = local_hash(key) & t.mask;
    for (unsigned long long probe = 0; probe <= t.mask; ++probe) {
        const unsigned long long k = t.keys[s];
        if (k == key || k == kLocalEmpty) return s;
        s = (s + 1) & t.mask;
    }
    return s;
}

// Which position a key keeps when several entries carry it: the last (atomicMax; free slots hold -1) or the first (atomicMin; free
// slots hold INT_MAX).  The key's slot is claimed by CAS from empty with linear probing; returns whether this call added the key.
enum class LocalWins { Last, First };

template <LocalWins W>
__device__ __forceinline__ bool local_upsert(const LocalTable& t, unsigned long long key, int pos)
{
    bool added = false;
    unsigned long long s = local_hash(key) & t.mask;
    for (unsigned long long probe = 0; probe <= t.mask; ++probe) {
        unsigned long long prev = kLocalEmpty;
        if (__hip_atomic_compare_exchange_strong(t.keys + s, &prev, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            added = true;
            break;
        }
        if (prev == key) break;
        s = (s + 1) & t.mask;
    }
    if (W == LocalWins::Last) __hip_atomic_fetch_max(t.vals + s, pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else __hip_atomic_fetch_min(t.vals + s, pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return added;
}

// block_cnt: [compact_blocks(n)] scratch; *total: kept items (device)
hipError_t launch_local_capture(hipStream_t st, const LocalCaptureArgs& a, uint32_t* block_cnt, uint32_t* total);
hipError_t launch_local_spill(hipStream_t st, const LocalSpillArgs& a, long long bound, uint32_t* block_cnt, uint32_t* total, bool scatter);
hipError_t launch_local_export(hipStream_t st, const LocalExportArgs& a, uint32_t* block_cnt, uint32_t* total);
// log[p0, p0 + n) into the table; *new_keys (may be NULL) += keys that were not present
hipError_t launch_local_insert(hipStream_t st, const LocalRecord* log, long long p0, long long n, LocalTable t, uint32_t* new_keys);

} // namespace gem
