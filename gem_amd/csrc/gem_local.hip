// gem_local.hip -- the rolling-window local map of ElevationMapping::updateLocalMap (EMg.cpp:609-767) on the device, gfx950.
//
// Three stable compactions share one form (gem_clean.hip's): k_local_count -> k_local_scan -> k_local_scatter, so that no workgroup
// ever waits for another.  Thread t of workgroup b takes items b * 1024 + k * 256 + t, k = 0..3: the order (k, wave, lane) IS the
// item order, ranked by ballot + mbcnt inside the wave and the waves' counts through LDS.  What is compacted is a source type:
//   CaptureSrc  the L^2 cells in grid_map's iteration order, kept as ElevationMap::show keeps them (EM.cpp:101, = k_show_emit)
//   SpillSrc    the K records of the previous capture, selected by the predicate of EMg.cpp:724-733 (positions recomputed in double)
//   ExportSrc   the log entries the table still points at (last-write order)
// k_local_insert upserts log entries into an open-addressing table with 64-bit agent-scope CAS on the key; duplicates of one key in
// one launch settle by atomicMax on the slot's log position, so the larger position -- the later cell -- wins whatever the timing.
#include "gem_local.hpp"
#include "gem_wave.hpp"

namespace gem {

__device__ __forceinline__ uint32_t local_wave_rank(uint64_t m)        // kept lanes below this one
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// getPositionFromIndex of the cell at linear index `lin` (the formula of k_show_emit)
__device__ __forceinline__ void local_position(const LocalGeom& g, size_t lin, double& x, double& y)
{
    const int ix = (int)(lin % (size_t)g.L), iy = (int)(lin / (size_t)g.L);
    int ux = ix - g.sx, uy = iy - g.sy;                                     // getIndexFromBufferIndex
    ux += ux < 0 ? g.L : 0; uy += uy < 0 ? g.L : 0;
    x = (g.px + g.off) + g.res * (double)(-ux);
    y = (g.py + g.off) + g.res * (double)(-uy);
}

struct CaptureSrc {
    LocalCaptureArgs a;
    __device__ size_t size() const { return (size_t)a.g.L * a.g.L; }
    __device__ bool keep(size_t lin) const
    {
        const size_t index = (lin % (size_t)a.g.L) * a.g.L + lin / (size_t)a.g.L;       // EM.cpp:98-100
        const float tr = a.m.traver[index];
        return a.m.elevation[index] != kEmptyElevation && tr != -10.0f && !(tr != tr);   // EM.cpp:101
    }
    __device__ void emit(size_t lin, size_t o) const
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
    }
};

struct SpillSrc {
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
    __device__ void emit(size_t i, size_t o) const { a.out[o] = a.rec[i]; }
};

struct ExportSrc {
    LocalExportArgs a;
    __device__ size_t size() const { return (size_t)a.n; }
    __device__ bool keep(size_t i) const
    {
        const LocalRecord& r = a.log[i];
        const unsigned long long key = local_key(r.x, r.y);
        const unsigned long long s = local_find(a.t, key);
        return a.t.keys[s] == key && a.t.vals[s] == (int)i;
    }
    __device__ void emit(size_t i, size_t o) const { a.out[o] = a.log[i]; }
};

template <class Src>
__global__ __launch_bounds__(kLocalThreads) void k_local_count(Src src, uint32_t* __restrict__ block_cnt)
{
    __shared__ uint32_t s_w[kLocalThreads / 64];
    const size_t base = (size_t)blockIdx.x * kLocalTile, n = src.size();
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < kLocalItems; ++k) {
        const size_t i = base + (size_t)k * kLocalThreads + threadIdx.x;
        c += (uint32_t)__popcll(__ballot(i < n && src.keep(i)));           // wave-uniform: s_bcnt1
    }
    if (lane_id() == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kLocalThreads / 64; ++w) t += s_w[w];
        block_cnt[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(1024) void k_local_scan(uint32_t* __restrict__ cnt, int nb, uint32_t* __restrict__ total)
{
    __shared__ uint32_t s[16];
    uint32_t carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 1024) {                                 // workgroup-uniform trip count
        const int i = b0 + (int)threadIdx.x;
        const uint32_t v = i < nb ? cnt[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<1024>(v, s, &tot);
        if (i < nb) cnt[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

template <class Src>
__global__ __launch_bounds__(kLocalThreads) void k_local_scatter(Src src, const uint32_t* __restrict__ block_off)
{
    constexpr int NW = kLocalThreads / 64;
    __shared__ uint32_t s_cnt[kLocalItems * NW];
    const size_t base = (size_t)blockIdx.x * kLocalTile, n = src.size();
    const int w = (int)(threadIdx.x >> 6);
    uint64_t m[kLocalItems];
#pragma unroll
    for (int k = 0; k < kLocalItems; ++k) {
        const size_t i = base + (size_t)k * kLocalThreads + threadIdx.x;
        m[k] = __ballot(i < n && src.keep(i));
        if (lane_id() == 0) s_cnt[k * NW + w] = (uint32_t)__popcll(m[k]);
    }
    __syncthreads();
    uint32_t run = block_off[blockIdx.x];                                   // kept items of the workgroups before this one
#pragma unroll
    for (int k = 0; k < kLocalItems; ++k) {
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) {
            const uint32_t cw = s_cnt[k * NW + ww];
            before += ww < w ? cw : 0u;
            total += cw;
        }
        if ((m[k] >> lane_id()) & 1ull)
            src.emit(base + (size_t)k * kLocalThreads + threadIdx.x, (size_t)run + before + local_wave_rank(m[k]));
        run += total;
    }
}

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

template <class Src>
static hipError_t compact(hipStream_t st, const Src& src, long long bound, uint32_t* block_cnt, uint32_t* total, bool count, bool scatter)
{
    const unsigned nb = local_blocks(bound);
    if (nb == 0) return count ? hipMemsetAsync(total, 0, sizeof(uint32_t), st) : hipSuccess;
    if (count) {
        hipLaunchKernelGGL(k_local_count<Src>, dim3(nb), dim3(kLocalThreads), 0, st, src, block_cnt);
        hipLaunchKernelGGL(k_local_scan, dim3(1), dim3(1024), 0, st, block_cnt, (int)nb, total);
    }
    if (scatter) hipLaunchKernelGGL(k_local_scatter<Src>, dim3(nb), dim3(kLocalThreads), 0, st, src, block_cnt);
    return hipGetLastError();
}

hipError_t launch_local_capture(hipStream_t st, const LocalCaptureArgs& a, uint32_t* block_cnt, uint32_t* total)
{
    return compact(st, CaptureSrc{a}, (long long)a.g.L * a.g.L, block_cnt, total, true, true);
}

hipError_t launch_local_spill(hipStream_t st, const LocalSpillArgs& a, long long bound, uint32_t* block_cnt, uint32_t* total, bool scatter)
{
    return compact(st, SpillSrc{a}, bound, block_cnt, total, !scatter, scatter);
}

hipError_t launch_local_export(hipStream_t st, const LocalExportArgs& a, uint32_t* block_cnt, uint32_t* total)
{
    return compact(st, ExportSrc{a}, a.n, block_cnt, total, true, true);
}

hipError_t launch_local_insert(hipStream_t st, const LocalRecord* log, long long p0, long long n, LocalTable t, uint32_t* new_keys)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_local_insert, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, log, p0, n, t, new_keys);
    return hipGetLastError();
}

} // namespace gem
