// gem_compose.hip -- pcl::StatisticalOutlierRemoval and the road / obstacle split of pointCloudtoOctomap (EMg.cpp:1146-1170) on the
// previous capture, gfx950.  The contract (what is rounded where) is stated in include/gem_hip.h at gem_local_compose.
//
// The cloud's x and y lie on the map's lattice, so the k nearest neighbours need no tree: the records are scattered into an L x L
// grid of record indices addressed by UNWRAPPED cell (the cell's row / column counted from the capture's start index, which is what
// orders it in space; the window clips at the map's edge, it does not wrap), and every record walks the square rings r = 0, 1, 2, ...
// of cells around its own, keeping the mean_k + 1 smallest squared distances in a sorted register array.
//
// When a walk may stop.  Let xf(u) = (float)((px + off) + res * (double)(-u)) be the capture's own formula for the x of column u
// (local_position in gem_local.hip), likewise yf(v).  Rounding to double and to float is monotone and res > 0, so xf is
// non-increasing in u: a record in column u' with |u' - u| >= r + 1 has |xf(u') - xf(u)| >= bx(r), where
//     bx(r) = min(|xf(u) - xf(u + r + 1)|, |xf(u) - xf(u - r - 1)|),
// computed in float: the float subtraction rounds the exact difference monotonely, so fl|xf(u') - xf(u)| >= fl(bx(r)) too.  The
// float square is monotone on non-negative values, and fl(a + b) >= a for a float a and b >= 0, so the record's
//     d2 = fl(fl(fl(dx * dx) + fl(dy * dy)) + fl(dz * dz)) >= fl(dx * dx) >= fl(bx(r) * bx(r)).
// Everything outside ring r is at least r + 1 columns or r + 1 rows away, hence its d2 >= bound(r) = min(fl(bx * bx), fl(by * by)),
// for the float-rounded positions themselves (far from the origin neighbouring columns round to one float: bx is then 0 for small
// r and the walk simply goes on).  Once bound(r) >= the largest kept value nothing outside can change the kept VALUES: a tie
// replaces a value by an equal one, and the mean distance is a function of the values alone.
//
// k_compose_knn answers from an LDS tile (16 x 16 cells + a halo of 8 rings); lanes still open after the halo -- sparse regions,
// steps whose dz dominates, the map's rim -- are listed, and k_compose_knn_far walks global memory for them from ring 0, at most L
// rings (ring L - 1 covers the whole map from any cell).  Every record gets its exact distance.
#include "gem_compose.hpp"

#include <math.h>

namespace gem {

namespace {

constexpr int T = kComposeTile, R = kComposeHalo, SIDE = kComposeSide;

// The KMAX + 1 smallest values seen, ascending, in registers (every index a compile-time constant).  For mean_k < KMAX the first
// KMAX - mean_k slots hold -inf for good, so that v[KMAX] is always the (mean_k + 1)-th smallest and one body serves every mean_k.
// The values are kept as their bit patterns and ordered as signed integers: a d2 is a sum of squares, so it is +0, positive or +inf,
// where the integer order IS the float order, and -inf (0xff800000) is negative, below them all.  v_min_i32 / v_max_i32 need no
// canonicalising move, which the float min / max would add per slot.
template <int KMAX>
struct Nearest {
    int v[KMAX + 1];
    __device__ __forceinline__ void init(int mean_k)
    {
#pragma unroll
        for (int s = 0; s <= KMAX; ++s) v[s] = (int)__float_as_uint(s < KMAX - mean_k ? -INFINITY : INFINITY);
    }
    __device__ __forceinline__ void insert(float d2)                          // branch-free: the value sinks to its place
    {
        int d = (int)__float_as_uint(d2);
#pragma unroll
        for (int s = 0; s <= KMAX; ++s) {
            const int lo = min(v[s], d);
            d = max(v[s], d);
            v[s] = lo;
        }
    }
    __device__ __forceinline__ float largest() const { return __uint_as_float((uint32_t)v[KMAX]); }
    // (float)(dist_sum / mean_k), dist_sum += s(d2[k]) for k = 1 .. mean_k in ascending order; entry 0 (the query) is slot KMAX - mean_k
    __device__ __forceinline__ float mean_distance(int mean_k, int sqrt_double) const
    {
        double sum = 0.0;
#pragma unroll
        for (int s = 1; s <= KMAX; ++s)
            if (s > KMAX - mean_k) {
                const float d2 = __uint_as_float((uint32_t)v[s]);
                sum += sqrt_double ? sqrt((double)d2) : (double)sqrtf(d2);
            }
        return (float)(sum / (double)mean_k);
    }
};

__device__ __forceinline__ float compose_d2(float qx, float qy, float qz, float x, float y, float z)
{
    const float dx = qx - x, dy = qy - y, dz = qz - z;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

__device__ __forceinline__ float lattice(double origin, double res, int u) { return (float)(origin + res * (double)(-u)); }

// bound(r) of the header comment for the record at unwrapped cell (ux, uy) with positions (qx, qy)
__device__ __forceinline__ float ring_bound(const LocalGeom& g, int ux, int uy, float qx, float qy, int r)
{
    const double ox = g.px + g.off, oy = g.py + g.off;
    const float bx = fminf(fabsf(qx - lattice(ox, g.res, ux + r + 1)), fabsf(qx - lattice(ox, g.res, ux - r - 1)));
    const float by = fminf(fabsf(qy - lattice(oy, g.res, uy + r + 1)), fabsf(qy - lattice(oy, g.res, uy - r - 1)));
    return fminf(bx * bx, by * by);
}

// cell c of ring r, clockwise from its corner (-r, -r); ring 0 is the cell itself
__device__ __forceinline__ int ring_step_x(int c, int r) { return c < 2 * r ? 1 : (c < 4 * r ? 0 : (c < 6 * r ? -1 : 0)); }
__device__ __forceinline__ int ring_step_y(int c, int r) { return c < 2 * r ? 0 : (c < 4 * r ? 1 : (c < 6 * r ? 0 : -1)); }

__device__ __forceinline__ void unwrap(const LocalGeom& g, int lin, int& ux, int& uy)
{
    ux = lin % g.L - g.sx; uy = lin / g.L - g.sy;                            // getIndexFromBufferIndex
    ux += ux < 0 ? g.L : 0; uy += uy < 0 ? g.L : 0;
}

} // namespace

__global__ __launch_bounds__(256) void k_compose_index(ComposeKnnArgs a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= *a.count) return;
    int ux, uy;
    unwrap(a.g, a.lin[i], ux, uy);
    a.grid[(size_t)uy * a.g.L + ux] = (int)i;
}

template <int KMAX>
__global__ __launch_bounds__(256) void k_compose_knn(ComposeKnnArgs a)
{
    __shared__ uint4 s_p[SIDE * SIDE];                                      // x, y, z bits | record index (-1: no record)
    const int L = a.g.L;
    const int ox = (int)blockIdx.x * T - R, oy = (int)blockIdx.y * T - R;
    for (int s = (int)threadIdx.x; s < SIDE * SIDE; s += 256) {
        const int cx = ox + (s % SIDE), cy = oy + (s / SIDE);
        uint4 p = make_uint4(0u, 0u, __float_as_uint(INFINITY), 0xffffffffu);          // z = inf: d2 = inf, never kept
        if (cx >= 0 && cx < L && cy >= 0 && cy < L) {
            const int idx = a.grid[(size_t)cy * L + cx];
            if (idx >= 0) {
                const uint4 q = *reinterpret_cast<const uint4*>(a.rec + idx);
                p = make_uint4(q.x, q.y, q.z, (uint32_t)idx);
            }
        }
        s_p[s] = p;
    }
    __syncthreads();
    const int tx = (int)threadIdx.x % T, ty = (int)threadIdx.x / T;
    const int home = (ty + R) * SIDE + tx + R;
    const uint4 q = s_p[home];
    const int self = (int)q.w;
    if (self < 0) return;
    const float qx = __uint_as_float(q.x), qy = __uint_as_float(q.y), qz = __uint_as_float(q.z);
    const int ux = ox + R + tx, uy = oy + R + ty;
    Nearest<KMAX> nn;
    nn.init(a.mean_k);
    bool open = true;
    for (int r = 0; r <= R && open; ++r) {
        int dx = -r, dy = -r;
        const int cells = r ? 8 * r : 1;
        for (int c = 0; c < cells; ++c) {
            const uint4 p = s_p[home + dy * SIDE + dx];
            nn.insert(compose_d2(qx, qy, qz, __uint_as_float(p.x), __uint_as_float(p.y), __uint_as_float(p.z)));
            dx += ring_step_x(c, r); dy += ring_step_y(c, r);
        }
        open = !(ring_bound(a.g, ux, uy, qx, qy, r) >= nn.largest());
    }
    if (open) a.far[atomicAdd(a.far_count, 1u)] = self;
    else a.dist[self] = nn.mean_distance(a.mean_k, a.sqrt_double);
}

template <int KMAX>
__global__ __launch_bounds__(64) void k_compose_knn_far(ComposeKnnArgs a)
{
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= *a.far_count) return;
    const int L = a.g.L;
    const int self = a.far[j];
    int ux, uy;
    unwrap(a.g, a.lin[self], ux, uy);
    const float qx = a.rec[self].x, qy = a.rec[self].y, qz = a.rec[self].z;
    // ring `last` reaches the map's farthest edge from this cell: nothing lies beyond it (last <= L - 1, the loop's hard bound)
    const int last = min(L - 1, max(max(ux, L - 1 - ux), max(uy, L - 1 - uy)));
    Nearest<KMAX> nn;
    nn.init(a.mean_k);
    bool open = true;
    for (int r = 0; r <= last && open; ++r) {
        int dx = -r, dy = -r;
        const int cells = r ? 8 * r : 1;
        for (int c = 0; c < cells; ++c) {
            const int cx = ux + dx, cy = uy + dy;
            if (cx >= 0 && cx < L && cy >= 0 && cy < L) {
                const int idx = a.grid[(size_t)cy * L + cx];
                if (idx >= 0) {
                    const float4 p = *reinterpret_cast<const float4*>(a.rec + idx);
                    nn.insert(compose_d2(qx, qy, qz, p.x, p.y, p.z));
                }
            }
            dx += ring_step_x(c, r); dy += ring_step_y(c, r);
        }
        open = !(ring_bound(a.g, ux, uy, qx, qy, r) >= nn.largest());
    }
    a.dist[self] = nn.mean_distance(a.mean_k, a.sqrt_double);
}

// ---- filter and split: class 0 road, 1 obstacle, 2 removed by the filter, 3 neither (a NaN travers; a capture holds none) --------
__device__ __forceinline__ int compose_class(const ComposeSplitArgs& a, size_t i)
{
    if (a.filter && !((double)a.dist[i] <= a.threshold)) return 2;
    const double t = (double)a.rec[i].travers;
    return t > a.travers_threshold ? 0 : (t <= a.travers_threshold ? 1 : 3);
}

// one compaction (gem_compact.hpp) over three counted classes; road and obstacle are written, each only where it has somewhere to go
struct ComposeSplit : CompactSrc {
    static constexpr int kCounted = 3, kWritten = 2;
    ComposeSplitArgs a;
    __device__ LocalRecord* out(int j) const { return j == 0 ? a.road : a.obstacle; }
    __device__ size_t size() const { return (size_t)*a.count; }
    __device__ int cls(size_t i, Item) const { return compose_class(a, i); }
    __device__ bool writes(int j) const { return out(j) != nullptr; }
    __device__ bool emit(int j, size_t i, Item, size_t o) const { out(j)[o] = a.rec[i]; return false; }
};

hipError_t launch_compose_knn(hipStream_t st, const ComposeKnnArgs& a, uint32_t n)
{
    const int L = a.g.L;
    hipError_t e;
    if ((e = hipMemsetAsync(a.grid, 0xff, (size_t)L * L * sizeof(int), st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.far_count, 0, sizeof(uint32_t), st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_compose_index, dim3((n + 255u) / 256u), dim3(256), 0, st, a);
    const unsigned tiles = (unsigned)((L + T - 1) / T);
    const unsigned far_blocks = (n + 63u) / 64u;                             // the far count stays on the device: one lane per record at most
    if (a.mean_k <= 20) {
        hipLaunchKernelGGL(k_compose_knn<20>, dim3(tiles, tiles), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_compose_knn_far<20>, dim3(far_blocks), dim3(64), 0, st, a);
    } else {
        hipLaunchKernelGGL(k_compose_knn<kComposeMaxK>, dim3(tiles, tiles), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_compose_knn_far<kComposeMaxK>, dim3(far_blocks), dim3(64), 0, st, a);
    }
    return hipGetLastError();
}

hipError_t launch_compose_split(hipStream_t st, const ComposeSplitArgs& a, uint32_t n, uint32_t* block_cnt, uint32_t* totals)
{
    return compact(st, ComposeSplit{{}, a}, n, block_cnt, totals, true, a.road || a.obstacle);
}

} // namespace gem
