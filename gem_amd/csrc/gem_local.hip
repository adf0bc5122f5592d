// gem_local.hip -- the rolling-window local map of ElevationMapping::updateLocalMap (EMg.cpp:609-767) on the device, gfx950.
//
// Three stable compactions (gem_compact.hpp), each over a source type:
//   CaptureSrc  the L^2 cells in grid_map's iteration order, kept as ElevationMap::show keeps them (EM.cpp:101, = k_show_emit)
//   SpillSrc    the K records of the previous capture, selected by the predicate of EMg.cpp:724-733 (positions recomputed in double)
//   ExportSrc   the log entries the table still points at (last-write order)
// k_local_insert upserts log entries into an open-addressing table with 64-bit agent-scope CAS on the key; duplicates of one key in
// one launch settle by atomicMax on the slot's log position, so the larger position -- the later cell -- wins whatever the timing.
#include "gem_local.hpp"

namespace gem {

struct CaptureSrc : CompactSrc {
    LocalCaptureArgs a;
    __device__ size_t size() const { return (size_t)a.g.L * a.g.L; }
    __device__ int cls(size_t lin, Item) const
    {
        const size_t index = (lin % (size_t)a.g.L) * a.g.L + lin / (size_t)a.g.L;       // EM.cpp:98-100
        const float tr = a.m.traver[index];
        return a.m.elevation[index] != kEmptyElevation && tr != -10.0f && !(tr != tr) ? 0 : -1;   // EM.cpp:101
    }
    __device__ bool emit(int, size_t lin, Item, size_t o) const
    {
        const size_t index = (lin % (size_t)a.g.L) * a.g.L + lin / (size_t)a.g.L;
        double px, py;
        local_position(a.g, lin, px, py);
        const uint32_t r8 = (unsigned char)(int)(float)a.m.colorR[index], g8 = (unsigned char)(int)(float)a.m.colorG[index],
                       b8 = (unsigned char)(int)(float)a.m.colorB[index];
        LocalRecord r;
        r.x = (float)px; r.y = (float)py; r.z = a.m.elevation[index]; r.pad = 1.0f;
        r.bgra = b8 | (g8 << 8) | (r8 << 16);
        r.covariance = a.m.variance[index]; r.intensity = a.m.intensity[index]; r.travers = a.m.traver[index];
        a.rec[o] = r;
        a.lin[o] = (int)lin;
        return false;
    }
};

struct SpillSrc : CompactSrc {
    LocalSpillArgs a;
    __device__ size_t size() const { return (size_t)*a.count; }
    __device__ bool keep(size_t i) const
    {
        if (!((double)a.rec[i].travers >= 0.0)) return false;                // EMg.cpp:724 (NaN fails; elevation != -10 by capture)
        double x, y;
        local_position(a.g, (size_t)a.lin[i], x, y);
        const float dx = a.dx, dy = a.dy;
        return ((x < a.lo_x || y < a.lo_y) && (dx > 0 && dy > 0))                // EMg.cpp:726-733, verbatim
            || ((x > a.hi_x || y > a.hi_y) && (dx < 0 && dy < 0))
            || ((x < a.lo_x || y > a.hi_y) && (dx > 0 && dy < 0))
            || ((x > a.hi_x || y < a.lo_y) && (dx < 0 && dy > 0))
            || ((x < a.lo_x) && (dx > 0 && dy == 0))
            || ((x > a.hi_x) && (dx < 0 && dy == 0))
            || ((y < a.lo_y) && (dy > 0 && dx == 0))
            || ((y > a.hi_y) && (dy < 0 && dx == 0));
    }
    __device__ int cls(size_t i, Item) const { return keep(i) ? 0 : -1; }
    __device__ bool emit(int, size_t i, Item, size_t o) const { a.out[o] = a.rec[i]; return false; }
};

struct ExportSrc : CompactSrc {
    LocalExportArgs a;
    __device__ size_t size() const { return (size_t)a.n; }
    __device__ bool keep(size_t i) const
    {
        const LocalRecord& r = a.log[i];
        const unsigned long long key = local_key(r.x, r.y);
        const unsigned long long s = local_find(a.t, key);
        return a.t.keys[s] == key && a.t.vals[s] == (int)i;
    }
    __device__ int cls(size_t i, Item) const { return keep(i) ? 0 : -1; }
    __device__ bool emit(int, size_t i, Item, size_t o) const { a.out[o] = a.log[i]; return false; }
};

// One thread per log entry: claim the key's slot (CAS from empty, linear probing; the host keeps the load at most one half), count the
// keys it added, then raise the slot's position to its own.  The table is read by later launches only.
__global__ __launch_bounds__(256) void k_local_insert(const LocalRecord* __restrict__ log, long long p0, long long n, LocalTable t,
                                                      uint32_t* __restrict__ new_keys)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool added = false;
    if (j < n) {
        const long long p = p0 + j;
        added = local_upsert<LocalWins::Last>(t, local_key(log[p].x, log[p].y), (int)p);
    }
    if (new_keys) {
        const uint64_t m = __ballot(added);
        if (lane_id() == 0 && m) __hip_atomic_fetch_add(new_keys, (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

hipError_t launch_local_capture(hipStream_t st, const LocalCaptureArgs& a, uint32_t* block_cnt, uint32_t* total)
{
    return compact(st, CaptureSrc{{}, a}, (long long)a.g.L * a.g.L, block_cnt, total);
}

hipError_t launch_local_spill(hipStream_t st, const LocalSpillArgs& a, long long bound, uint32_t* block_cnt, uint32_t* total, bool scatter)
{
    return compact(st, SpillSrc{{}, a}, bound, block_cnt, total, !scatter, scatter);
}

hipError_t launch_local_export(hipStream_t st, const LocalExportArgs& a, uint32_t* block_cnt, uint32_t* total)
{
    return compact(st, ExportSrc{{}, a}, a.n, block_cnt, total);
}

hipError_t launch_local_insert(hipStream_t st, const LocalRecord* log, long long p0, long long n, LocalTable t, uint32_t* new_keys)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_local_insert, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, log, p0, n, t, new_keys);
    return hipGetLastError();
}

} // namespace gem
