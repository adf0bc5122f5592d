// gem_voxel.hip -- one pcl::VoxelGrid<pcl::PCLPointCloud2> stage (as pcl_ros's nodelet runs it) on the device, gfx950.
// The contract is in include/gem_hip.h (gem_voxel_device); the launch structure in gem_voxel.hpp.
//
// The record layout of a workgroup, the hand-over to the last workgroup to arrive and the stable LSD passes are gem_lsd.hpp's.
#include "gem_voxel.hpp"
#include "gem_wave.hpp"

#include <climits>

namespace gem {

namespace {

__device__ __forceinline__ uint32_t ord_f(float f)          // order-preserving float -> uint32 (finite values)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unord_f(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// (int) of a float as x86's cvttss2si does it: INT_MIN outside the int range (a plain cast is undefined there)
__device__ __forceinline__ int f2i(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : INT_MIN; }

__device__ __forceinline__ bool finite3(float4 p)
{
    return __builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z);
}
__device__ __forceinline__ float field_of(float4 p, int f)
{
    return f == GEM_VOXEL_FIELD_X ? p.x : f == GEM_VOXEL_FIELD_Y ? p.y : f == GEM_VOXEL_FIELD_Z ? p.z : p.w;
}
// getMinMax3D: the limit test against the limits cast to float (NaN fails both comparisons: kept), then finite x, y, z
__device__ __forceinline__ bool in_bounds(float4 p, const VoxStageArgs& a)
{
    if (!finite3(p)) return false;
    if (a.field == GEM_VOXEL_FIELD_NONE) return true;
    const float v = field_of(p, a.field);
    return a.negative ? !(v < a.hi_f && v > a.lo_f) : !(v > a.hi_f || v < a.lo_f);
}
// the point loop: the same test against the double limits
__device__ __forceinline__ bool survives(float4 p, const VoxStageArgs& a)
{
    if (!finite3(p)) return false;
    if (a.field == GEM_VOXEL_FIELD_NONE) return true;
    const double v = (double)field_of(p, a.field);
    return a.negative ? !(v < a.hi && v > a.lo) : !(v > a.hi || v < a.lo);
}

struct Geo { float inv[3]; uint32_t min_b[3], mul[3]; };

__device__ __forceinline__ Geo load_geo(const VoxState* st)
{
    Geo g;
#pragma unroll
    for (int k = 0; k < 3; ++k) { g.inv[k] = st->inv[k]; g.min_b[k] = (uint32_t)st->min_b[k]; g.mul[k] = st->mul[k]; }
    return g;
}

// ijk_k = (int)floor(p_k * inv_k) - min_b_k;  idx = ijk . mul in wrapping int32, taken as uint32
__device__ __forceinline__ uint32_t vox_key(float4 p, const Geo& g)
{
    const uint32_t i = (uint32_t)f2i(floorf(__fmul_rn(p.x, g.inv[0]))) - g.min_b[0];
    const uint32_t j = (uint32_t)f2i(floorf(__fmul_rn(p.y, g.inv[1]))) - g.min_b[1];
    const uint32_t k = (uint32_t)f2i(floorf(__fmul_rn(p.z, g.inv[2]))) - g.min_b[2];
    return i * g.mul[0] + j * g.mul[1] + k * g.mul[2];
}

__device__ __forceinline__ long long rec_pos(int k) { return lsd_pos(k); }

__device__ __forceinline__ long long input_count(const VoxStageArgs& a) { return a.n_dev ? (long long)*a.n_dev : a.n; }

} // namespace

// ---- 1: bounds, survivors, geometry -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kVoxThreads) void k_vox_bounds(VoxStageArgs a)
{
    constexpr int NW = kVoxThreads / 64;
    __shared__ uint32_t s_red[NW][8];
    __shared__ uint32_t s_last;
    const long long n = input_count(a);
    uint32_t r[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < kVoxItems; ++k) {
        const long long i = rec_pos(k);
        if (i < n) {
            const float4 p = a.in[i];
            if (in_bounds(p, a)) {
                r[0] = max(r[0], ord_f(p.x)); r[1] = max(r[1], ord_f(p.y)); r[2] = max(r[2], ord_f(p.z));
                r[3] = max(r[3], ~ord_f(p.x)); r[4] = max(r[4], ~ord_f(p.y)); r[5] = max(r[5], ~ord_f(p.z));
                ++r[6];
            }
            if (survives(p, a)) ++r[7];
        }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) r[j] = wave_inclusive_max(r[j]);
    r[6] = wave_inclusive_scan(r[6]); r[7] = wave_inclusive_scan(r[7]);
    if (lane_id() == 63) {
#pragma unroll
        for (int j = 0; j < 8; ++j) s_red[threadIdx.x >> 6][j] = r[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = s_red[0][j];
        for (int w = 1; w < NW; ++w) {
#pragma unroll
            for (int j = 0; j < 6; ++j) t[j] = max(t[j], s_red[w][j]);
            t[6] += s_red[w][6]; t[7] += s_red[w][7];
        }
        if (t[6]) {
#pragma unroll
            for (int j = 0; j < 6; ++j) atomicMax(&a.st->acc[j], t[j]);
            atomicAdd(&a.st->acc[6], t[6]);
        }
        if (t[7]) atomicAdd(&a.st->acc[7], t[7]);
    }
    if (!last_arrival(&a.st->ticket[0], a.nb, &s_last) || threadIdx.x != 0) return;
    VoxState* st = a.st;
    uint32_t acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        acc[j] = __hip_atomic_load(&st->acc[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&st->acc[j], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    int mode = kVoxEmpty;
    if (acc[6]) {
        float mn[3], mx[3], inv[3];
        bool overflow = false;
        long long d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            mx[k] = unord_f(acc[k]); mn[k] = unord_f(~acc[3 + k]);
            inv[k] = __fdiv_rn(1.0f, a.leaf[k]);
            const float e = __fmul_rn(__fsub_rn(mx[k], mn[k]), inv[k]);        // >= 0 (or +inf)
            if (!(e < 2147483648.0f)) { overflow = true; d[k] = 0; }
            else d[k] = (long long)e + 1;
        }
        if (!overflow) {
            const long long d01 = d[0] * d[1];                                  // <= 2^62
            overflow = d01 > (long long)INT_MAX || d01 * d[2] > (long long)INT_MAX;
        }
        if (overflow) mode = kVoxPassThrough;
        else {
            uint32_t div[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int lo = f2i(floorf(__fmul_rn(mn[k], inv[k]))), hi = f2i(floorf(__fmul_rn(mx[k], inv[k])));
                st->inv[k] = inv[k];
                st->min_b[k] = lo;
                div[k] = (uint32_t)hi - (uint32_t)lo + 1u;
            }
            st->mul[0] = 1u; st->mul[1] = div[0]; st->mul[2] = div[0] * div[1];
            mode = kVoxSort;
        }
    }
    st->mode = mode;
    st->S = acc[7];
}

// ---- 2: output tail / pass-through copy, histogram of digit 0 ---------------------------------------------------------------
__global__ __launch_bounds__(kVoxThreads) void k_vox_hist(VoxStageArgs a)
{
    __shared__ uint32_t s_h[kVoxBins];
    __shared__ uint32_t s_scan[16];
    __shared__ uint32_t s_last;
    const int mode = a.st->mode;
    const long long n = input_count(a);
    const float qnan = __builtin_nanf("");
#pragma unroll
    for (int k = 0; k < kVoxItems; ++k) {                 // every position of the output: the NaN tail from m on is written here
        const long long i = rec_pos(k);
        if (i < a.n) {
            if (mode == kVoxPassThrough) {
                a.out[i] = a.in[i];
                if (a.rgb_out) a.rgb_out[i] = a.rgb_in ? a.rgb_in[i] : 0u;
            } else {
                a.out[i] = make_float4(qnan, qnan, qnan, 0.0f);
                if (a.rgb_out) a.rgb_out[i] = 0u;
            }
        }
    }
    if (mode != kVoxSort) return;                          // (uniform over the grid)
    const Geo g = load_geo(a.st);
    for (int d = threadIdx.x; d < kVoxBins; d += kVoxThreads) s_h[d] = 0u;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kVoxItems; ++k) {
        const long long i = rec_pos(k);
        if (i < n) {
            const float4 p = a.in[i];
            if (survives(p, a)) atomicAdd(&s_h[vox_key(p, g) & (kVoxBins - 1)], 1u);
        }
    }
    __syncthreads();
    reinterpret_cast<uint4*>(a.hist[0])[(size_t)blockIdx.x * (kVoxBins / 4) + threadIdx.x] = reinterpret_cast<const uint4*>(s_h)[threadIdx.x];
    if (last_arrival(&a.st->ticket[1], a.nb, &s_last)) lsd_scan_hist(a.hist[0], a.nb, s_scan);
}

// ---- 3-5: stable LSD passes over (key, input position) ---------------------------------------------------------------------
template <int PASS>
__global__ __launch_bounds__(kVoxThreads) void k_vox_scatter(VoxStageArgs a)
{
    if (a.st->mode != kVoxSort) return;
    const uint32_t S = a.st->S;
    const long long n = input_count(a);
    const Geo g = load_geo(a.st);
    auto load = [&](long long j, uint32_t& key, uint32_t& src) -> bool {
        if constexpr (PASS == 0) {
            src = (uint32_t)j;
            if (j < n) {
                const float4 p = a.in[j];
                if (survives(p, a)) { key = vox_key(p, g); return true; }
            }
            return false;
        } else {
            const bool valid = j < (long long)S;
            key = valid ? a.key[(PASS - 1) & 1][j] : 0u;
            src = valid ? a.src[(PASS - 1) & 1][j] : 0u;
            return valid;
        }
    };
    lsd_scatter_pass<uint32_t, (PASS < 2)>(kVoxDigit * PASS, true, load, a.key[PASS & 1], a.src[PASS & 1], a.hist[PASS & 1], a.hist[(PASS + 1) & 1],
                               &a.st->ticket[2 + PASS], a.nb);
}

// ---- 6: voxel heads, m -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kVoxThreads) void k_vox_heads(VoxStageArgs a)
{
    constexpr int NW = kVoxThreads / 64;
    __shared__ uint32_t s_cnt[NW];
    __shared__ uint32_t s_scan[16];
    __shared__ uint32_t s_last;
    const int mode = a.st->mode;
    if (mode != kVoxSort) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *a.count_out = mode == kVoxPassThrough ? (int)input_count(a) : 0;
        return;
    }
    const uint32_t S = a.st->S;
    const uint32_t* key = a.key[0];
    uint32_t c = 0u;
#pragma unroll
    for (int k = 0; k < kVoxItems; ++k) {
        const long long j = rec_pos(k);
        const bool head = j < (long long)S && (j == 0 || key[j - 1] != key[j]);
        c += (uint32_t)__popcll(__ballot(head));
    }
    if (lane_id() == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0u;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += s_cnt[w];
        a.heads[blockIdx.x] = t;
    }
    if (!last_arrival(&a.st->ticket[4], a.nb, &s_last)) return;
    uint32_t carry = 0u;
    for (int b0 = 0; b0 < a.nb; b0 += kVoxThreads) {      // workgroup-uniform trip count
        const int i = b0 + (int)threadIdx.x;
        const uint32_t v = i < a.nb ? a.heads[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<kVoxThreads>(v, s_scan, &tot);
        if (i < a.nb) a.heads[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *a.count_out = (int)carry;
}

// ---- 7: centroids ----------------------------------------------------------------------------------------------------------
// One lane per voxel head walks its run (input order, by the stable sort) eight records at a time and sums sequentially from +0.
__global__ __launch_bounds__(kVoxThreads) void k_vox_centroid(VoxStageArgs a)
{
    constexpr int NW = kVoxThreads / 64;
    __shared__ uint32_t s_cnt[NW];
    if (a.st->mode != kVoxSort) return;
    const uint32_t S = a.st->S;
    const uint32_t* key = a.key[0];
    const uint32_t* src = a.src[0];
    const int w = (int)(threadIdx.x >> 6);
    const uint64_t lt = lanemask_lt();
    bool head[kVoxItems];
    uint32_t r[kVoxItems], c = 0u;
#pragma unroll
    for (int k = 0; k < kVoxItems; ++k) {
        const long long j = rec_pos(k);
        head[k] = j < (long long)S && (j == 0 || key[j - 1] != key[j]);
        const uint64_t m = __ballot(head[k]);
        r[k] = c + (uint32_t)__popcll(m & lt);
        c += (uint32_t)__popcll(m);
    }
    if (lane_id() == 0) s_cnt[w] = c;
    __syncthreads();
    uint32_t base = a.heads[blockIdx.x];
    for (int ww = 0; ww < w; ++ww) base += s_cnt[ww];
    const bool with_rgb = a.rgb_in && a.rgb_out;
#pragma unroll
    for (int k = 0; k < kVoxItems; ++k) {
        if (!head[k]) continue;
        const uint32_t j = (uint32_t)rec_pos(k);
        const uint32_t k0 = key[j];
        float sx = 0.0f, sy = 0.0f, sz = 0.0f, si = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
        uint32_t cnt = 0u;
        for (uint32_t q = j;; q += 8u) {
            uint32_t kk[8];
            float4 v[8];
            uint32_t cc[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) kk[t] = q + t < S ? key[q + t] : ~k0;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const uint32_t s = kk[t] == k0 ? src[q + t] : 0u;
                v[t] = kk[t] == k0 ? a.in[s] : make_float4(0.f, 0.f, 0.f, 0.f);
                cc[t] = kk[t] == k0 && with_rgb ? a.rgb_in[s] : 0u;
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                if (kk[t] != k0) continue;                // (the run is contiguous: nothing of it follows a mismatch)
                sx = __fadd_rn(sx, v[t].x); sy = __fadd_rn(sy, v[t].y); sz = __fadd_rn(sz, v[t].z); si = __fadd_rn(si, v[t].w);
                if (with_rgb) {
                    sr = __fadd_rn(sr, (float)((cc[t] >> 16) & 255u));
                    sg = __fadd_rn(sg, (float)((cc[t] >> 8) & 255u));
                    sb = __fadd_rn(sb, (float)(cc[t] & 255u));
                }
                ++cnt;
            }
            if (kk[7] != k0) break;
        }
        const float fc = (float)cnt;
        const uint32_t o = base + r[k];
        a.out[o] = make_float4(__fdiv_rn(sx, fc), __fdiv_rn(sy, fc), __fdiv_rn(sz, fc), __fdiv_rn(si, fc));
        if (with_rgb) {
            const uint32_t R = (uint32_t)(int)__fdiv_rn(sr, fc), G = (uint32_t)(int)__fdiv_rn(sg, fc), B = (uint32_t)(int)__fdiv_rn(sb, fc);
            a.rgb_out[o] = (R << 16) | (G << 8) | B;
        }
    }
}

hipError_t launch_voxel_stage(hipStream_t st, const VoxStageArgs& a)
{
    if (a.n <= 0 || a.nb <= 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.nb), block(kVoxThreads);
    hipLaunchKernelGGL(k_vox_bounds, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_vox_hist, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_vox_scatter<0>, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_vox_scatter<1>, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_vox_scatter<2>, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_vox_heads, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_vox_centroid, grid, block, 0, st, a);
    return hipGetLastError();
}

} // namespace gem
