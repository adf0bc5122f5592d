// gem_costmap.hip -- the two costmap_2d layers of the reference's layers/ on the device, gfx950: PointMapLayer::updateBounds
// (layers/src/pointMap_layer.cpp:55-81), ElevationMapLayer::updateBounds (layers/src/elevationMap_layer.cpp:58-81), and the pieces
// of costmap_2d they call, restated in include/gem_hip.h.
//
// The reference's loops write costmap_[index] input by input, so the LAST input of a cell decides between FREE_SPACE and
// LETHAL_OBSTACLE.  Here every input carries the stamp 2 * (its index + 1) + lethal; a cell keeps the integer maximum of its
// stamps, which is the stamp of its last input whatever the timing, and k_cost_resolve turns the low bit into the byte.  Nearly all
// of the cost is contention: the grid cloud of a capture puts some 64 inputs on each costmap cell, neighbouring lanes on the same
// one.  So a stamp is reduced before it reaches memory:
//   in the wave       a lane whose successor holds the same cell with a stamp at least as large stays silent (the successor, or a
//                     lane behind it, issues a stamp that beats this one): in input order only the last lane of a run issues
//   in the workgroup  a costmap of at most kCostLdsCells cells has a stamp grid in LDS (ds_max_u32); the workgroup's 4096
//                     consecutive inputs touch few cells, and each non-zero entry leaves with one global atomic max
//   larger costmaps   the wave-reduced stamps go to global memory directly
// The touched bounds (min / max of px, py over the accepted inputs) go wave -> workgroup (LDS) -> four global words as
// order-preserving 64-bit keys under integer min.  The reduction and the publication of the bounds are gem_cost_pass.hpp's, shared with
// ObstacleLayer and VoxelLayer; the element-wise kernels here (fill, roll, window) serve a grid of bytes or of voxel columns.  Only vector stores and atomics write memory.
#include "gem_cost_pass.hpp"

namespace gem {

struct CostInput {
    double px, py;
    bool lethal;
    uint32_t order;                     // index in the reference's loop
};

// PointMapLayer: the records of a cloud; travers > thresh is free, anything else (NaN included) lethal
struct CostPointsSrc {
    CostPointsArgs a;
    struct Item { float x, y, t; };
    __device__ size_t size() const { return a.count ? (size_t)min(*a.count, a.n) : (size_t)a.n; }
    __device__ Item load(size_t i) const { return {a.rec[i].x, a.rec[i].y, a.rec[i].travers}; }
    __device__ CostInput eval(size_t i, const Item& v) const
    {
        return {(double)v.x, (double)v.y, !((double)v.t > a.thresh), a.base + (uint32_t)i};
    }
};

// ElevationMapLayer: all L^2 cells of the capture's grid in iteration order (= linear index).  Items [0, L^2) are the cells as if
// none were kept (NaN: never below the threshold, free); items behind them are the kept cells with their traver, under the same
// order number, so a kept cell's own verdict beats its NaN twin exactly when it is lethal.
struct CostVisualSrc {
    CostVisualArgs a;
    struct Item { uint32_t k; float t; };
    __device__ size_t cells() const { return (size_t)a.g.L * a.g.L; }
    __device__ size_t size() const { return cells() + (size_t)min(*a.count, (uint32_t)cells()); }
    __device__ Item load(size_t i) const
    {
        const size_t c = cells();
        if (i < c) return {(uint32_t)i, __builtin_nanf("")};
        return {(uint32_t)a.lin[i - c], a.rec[i - c].travers};
    }
    __device__ CostInput eval(size_t, const Item& v) const
    {
        CostInput in;
        local_position(a.g, (size_t)v.k, in.px, in.py);
        in.lethal = (double)v.t < a.thresh;
        in.order = v.k;
        return in;
    }
};

// the body of a mark workgroup: inputs [4096 blockIdx.x, 4096 (blockIdx.x + 1)) of src
template <class Src, bool LDS>
__device__ __forceinline__ void cost_mark_block(const Src& src, const CostGeom& g, const CostAccum& out)
{
    extern __shared__ uint32_t s_stamp[];                               // LDS form: [cells]
    __shared__ unsigned long long s_acc[4];
    const uint32_t cells = g.sx * g.sy;
    if (LDS)
        for (uint32_t c = threadIdx.x; c < cells; c += kCostThreads) s_stamp[c] = 0u;
    if (threadIdx.x < 4) s_acc[threadIdx.x] = ~0ull;
    __syncthreads();

    const size_t n = src.size(), base = (size_t)blockIdx.x * kCostChunk;
    double lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
    constexpr int kBatch = 4;                                           // loads in flight per lane
    for (int k0 = 0; k0 < kCostItems; k0 += kBatch) {                   // workgroup-uniform trip count
        if (base + (size_t)k0 * kCostThreads >= n) break;
        typename Src::Item v[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const size_t i = base + (size_t)(k0 + k) * kCostThreads + threadIdx.x;
            if (i < n) v[k] = src.load(i);
        }
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const size_t i = base + (size_t)(k0 + k) * kCostThreads + threadIdx.x;
            uint32_t cell = 0u, stamp = 0u;                             // stamp 0: no input, or one worldToMap refused
            if (i < n) {
                const CostInput in = src.eval(i, v[k]);
                if (cost_cell(g, in.px, in.py, cell)) {
                    stamp = 2u * (in.order + 1u) + (in.lethal ? 1u : 0u);
                    lo_x = fmin(lo_x, in.px); hi_x = fmax(hi_x, in.px);
                    lo_y = fmin(lo_y, in.py); hi_y = fmax(hi_y, in.py);
                }
            }
            const uint32_t next_cell = (uint32_t)__shfl_down((int)cell, 1), next_stamp = (uint32_t)__shfl_down((int)stamp, 1);
            const bool beaten = lane_id() < 63 && next_cell == cell && next_stamp >= stamp;
            const bool issue = stamp != 0u && !beaten;
            if (issue) {
                if (LDS) atomicMax(&s_stamp[cell], stamp);
                else __hip_atomic_fetch_max(out.stamps + cell, stamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }

    cost_bounds_out(lo_x, lo_y, hi_x, hi_y, s_acc, out.acc);
    if (LDS)
        for (uint32_t c = threadIdx.x; c < cells; c += kCostThreads) {
            const uint32_t s = s_stamp[c];
            if (s) __hip_atomic_fetch_max(out.stamps + c, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
}

template <class Src, bool LDS>
__global__ __launch_bounds__(kCostThreads) void k_cost_mark(Src src, CostGeom g, CostAccum out)
{
    cost_mark_block<Src, LDS>(src, g, out);
}

// PointMapLayer over the history cloud (gem_history.hpp): workgroup b first reads the box of its 4096 records and leaves when no
// record of the block can pass worldToMap -- before it touches LDS, the stamps or the bounds words.  The rule, in double:
//   culled  <=>  !(max_x >= ox) || !(max_y >= oy) || !(min_x < ox + (sx + 1) * res) || !(min_y < oy + (sy + 1) * res)
// It never drops an accepted record.  cost_cell accepts wx only if wx >= ox, which the box's max_x then satisfies too (floats widen
// exactly), and if q = fl(fl(wx - ox) / res) < sx.  q is a double below the integer sx, so q <= sx (1 - u) with u = 2^-53, and the
// two roundings give wx - ox < sx res (1 + u).  The limit is lim = fl(ox + fl((sx + 1) res)) >= ox + (sx + 1) res (1 - u) - u |lim|,
// so wx < lim follows from u (2 sx + 1 + |lim| / res) <= 1: the extra cell absorbs every rounding as long as |lim| <= 2^51 res, which
// the host checks before it hands a box table over (cost_cull_exact; otherwise the launch culls nothing).  NaN coordinates are not
// in a box and are refused anyway; a block without a coordinate has the box {+inf, +inf, -inf, -inf} and fails the first test.
struct CostCull {
    const float4* box;                  // a box per workgroup {min_x, min_y, max_x, max_y}, or NULL: nothing is culled
    uint32_t* culled;                   // culled workgroups of this launch (one vector atomic each)
};

__device__ __forceinline__ bool cost_block_culled(const CostGeom& g, const float4& b)
{
    const double lim_x = g.ox + (double)(g.sx + 1u) * g.res, lim_y = g.oy + (double)(g.sy + 1u) * g.res;
    return !((double)b.z >= g.ox) || !((double)b.w >= g.oy) || !((double)b.x < lim_x) || !((double)b.y < lim_y);
}

template <bool LDS>
__global__ __launch_bounds__(kCostThreads) void k_cost_mark_history(CostPointsSrc src, CostGeom g, CostAccum out, CostCull c)
{
    if (c.box) {
        if (cost_block_culled(g, c.box[blockIdx.x])) {                  // workgroup-uniform
            if (threadIdx.x == 0) __hip_atomic_fetch_add(c.culled, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
    }
    cost_mark_block<CostPointsSrc, LDS>(src, g, out);
}

// four cells per thread: a touched cell takes its verdict and its stamp goes back to 0; workgroup 0 publishes the bounds words and
// resets them for the next mark
__global__ __launch_bounds__(256) void k_cost_resolve(uint32_t cells, uint32_t* __restrict__ stamps, unsigned char* __restrict__ grid,
                                                      unsigned long long* __restrict__ acc, unsigned long long* __restrict__ published)
{
    if (blockIdx.x == 0) cost_publish(acc, published);
    const uint32_t c0 = (blockIdx.x * 256u + threadIdx.x) * 4u;         // the stamp array is padded to a multiple of four words
    if (c0 >= cells) return;
    const uint4 s = *reinterpret_cast<const uint4*>(stamps + c0);
    if (!(s.x | s.y | s.z | s.w)) return;
    const uint32_t w[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (w[k] && c0 + k < cells) grid[c0 + k] = (w[k] & 1u) ? kCostLethal : kCostFree;
    *reinterpret_cast<uint4*>(stamps + c0) = make_uint4(0u, 0u, 0u, 0u);
}

// The element-wise kernels of a grid, T a byte of the costmap or a 32-bit voxel column (gem_voxlayer.hpp)
template <class T>
__global__ __launch_bounds__(256) void k_cost_fill(T* __restrict__ grid, uint32_t cells, T value)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c < cells) grid[c] = value;
}

template <class T>
__global__ __launch_bounds__(256) void k_cost_roll(const T* __restrict__ src, T* __restrict__ dst, uint32_t sx, uint32_t sy, long long cell_ox,
                                                   long long cell_oy, T value)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= sx * sy) return;
    const long long x = (long long)(c % sx) + cell_ox, y = (long long)(c / sx) + cell_oy;
    const bool in = x >= 0 && x < (long long)sx && y >= 0 && y < (long long)sy;
    dst[c] = in ? src[(size_t)y * sx + (size_t)x] : value;
}

// thread t of a launch over a window: false behind the window's last cell, else the cell's index in the grid
__device__ __forceinline__ bool cost_window_cell(uint32_t sx, const CostWindow& w, uint32_t& t, size_t& c)
{
    const uint32_t ww = (uint32_t)(w.max_i - w.min_i);
    t = blockIdx.x * 256u + threadIdx.x;
    if (t >= ww * (uint32_t)(w.max_j - w.min_j)) return false;
    c = (size_t)(w.min_j + (int)(t / ww)) * sx + (size_t)(w.min_i + (int)(t % ww));
    return true;
}

__global__ __launch_bounds__(256) void k_cost_merge(const unsigned char* __restrict__ layer, unsigned char* __restrict__ master,
                                                    uint32_t sx, CostWindow w, int mode)
{
    uint32_t t;
    size_t c;
    if (!cost_window_cell(sx, w, t, c)) return;
    const unsigned char v = layer[c];
    if (v == kCostNoInfo) return;
    if (mode == 0) { master[c] = v; return; }                           // updateWithOverwrite
    const unsigned char old = master[c];
    if (old == kCostNoInfo || old < v) master[c] = v;                   // updateWithMax
}

// PACK: the window's elements into `packed`; else the reverse
template <class T, bool PACK>
__global__ __launch_bounds__(256) void k_cost_window(T* __restrict__ grid, uint32_t sx, CostWindow w, T* __restrict__ packed)
{
    uint32_t t;
    size_t c;
    if (!cost_window_cell(sx, w, t, c)) return;
    if (PACK) packed[t] = grid[c];
    else grid[c] = packed[t];
}

template <class Src>
static hipError_t launch_mark(hipStream_t st, const Src& src, long long items, const CostGeom& g, CostAccum out)
{
    const long long nb = cost_mark_blocks(items);
    if (nb <= 0) return hipSuccess;
    if (nb > INT_MAX) return hipErrorInvalidValue;
    const uint32_t cells = g.sx * g.sy;
    if (cells <= kCostLdsCells) {
        hipLaunchKernelGGL((k_cost_mark<Src, true>), dim3((unsigned)nb), dim3(kCostThreads), cells * sizeof(uint32_t), st, src, g, out);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((k_cost_mark<Src, false>), dim3((unsigned)nb), dim3(kCostThreads), 0, st, src, g, out);
    return hipGetLastError();
}

hipError_t launch_cost_mark_points(hipStream_t st, const CostGeom& g, const CostPointsArgs& a, CostAccum out)
{
    return launch_mark(st, CostPointsSrc{a}, (long long)a.n, g, out);
}

hipError_t launch_cost_mark_history(hipStream_t st, const CostGeom& g, const CostPointsArgs& a, CostAccum out, const float4* box,
                                    uint32_t* culled)
{
    const long long nb = cost_mark_blocks((long long)a.n);
    if (nb <= 0) return hipSuccess;
    const CostPointsSrc src{a};
    const CostCull c{cost_cull_exact(g) ? box : nullptr, culled};
    const uint32_t cells = g.sx * g.sy;
    if (cells <= kCostLdsCells)
        hipLaunchKernelGGL((k_cost_mark_history<true>), dim3((unsigned)nb), dim3(kCostThreads), cells * sizeof(uint32_t), st, src, g, out, c);
    else
        hipLaunchKernelGGL((k_cost_mark_history<false>), dim3((unsigned)nb), dim3(kCostThreads), 0, st, src, g, out, c);
    return hipGetLastError();
}

hipError_t launch_cost_mark_visual(hipStream_t st, const CostGeom& g, const CostVisualArgs& a, CostAccum out)
{
    return launch_mark(st, CostVisualSrc{a}, 2ll * a.g.L * a.g.L, g, out);
}

hipError_t launch_cost_resolve(hipStream_t st, uint32_t cells, uint32_t* stamps, unsigned char* grid, unsigned long long* acc,
                               unsigned long long* published)
{
    hipLaunchKernelGGL(k_cost_resolve, dim3(cost_blocks(((uint64_t)cells + 3) / 4)), dim3(256), 0, st, cells, stamps, grid, acc, published);
    return hipGetLastError();
}

// The launchers below take elem = 1 (a byte of the costmap) or 4 (a voxel column) and nothing else; the callers pass constants.
template <class T>
static hipError_t fill_of(hipStream_t st, void* grid, uint32_t cells, uint32_t value)
{
    hipLaunchKernelGGL(k_cost_fill<T>, dim3(cost_blocks(cells)), dim3(256), 0, st, static_cast<T*>(grid), cells, (T)value);
    return hipGetLastError();
}

hipError_t launch_cost_fill(hipStream_t st, void* grid, size_t elem, uint32_t cells, uint32_t value)
{
    return elem == 4 ? fill_of<uint32_t>(st, grid, cells, value) : fill_of<unsigned char>(st, grid, cells, value);
}

template <class T>
static hipError_t roll_of(hipStream_t st, const void* src, void* dst, uint32_t sx, uint32_t sy, long long cell_ox, long long cell_oy, uint32_t value)
{
    hipLaunchKernelGGL(k_cost_roll<T>, dim3(cost_blocks((uint64_t)sx * sy)), dim3(256), 0, st, static_cast<const T*>(src), static_cast<T*>(dst), sx, sy,
                       cell_ox, cell_oy, (T)value);
    return hipGetLastError();
}

hipError_t launch_cost_roll(hipStream_t st, const void* src, void* dst, size_t elem, uint32_t sx, uint32_t sy, long long cell_ox,
                            long long cell_oy, uint32_t value)
{
    return elem == 4 ? roll_of<uint32_t>(st, src, dst, sx, sy, cell_ox, cell_oy, value) : roll_of<unsigned char>(st, src, dst, sx, sy, cell_ox, cell_oy, value);
}

hipError_t launch_cost_merge(hipStream_t st, const unsigned char* layer, unsigned char* master, uint32_t sx, CostWindow w, int mode)
{
    const uint64_t t = cost_window_cells(w);
    if (!t) return hipSuccess;
    hipLaunchKernelGGL(k_cost_merge, dim3(cost_blocks(t)), dim3(256), 0, st, layer, master, sx, w, mode);
    return hipGetLastError();
}

template <class T>
static hipError_t window_of(hipStream_t st, void* grid, uint32_t sx, CostWindow w, void* packed, bool pack)
{
    const dim3 blocks(cost_blocks(cost_window_cells(w)));
    if (pack) hipLaunchKernelGGL((k_cost_window<T, true>), blocks, dim3(256), 0, st, static_cast<T*>(grid), sx, w, static_cast<T*>(packed));
    else hipLaunchKernelGGL((k_cost_window<T, false>), blocks, dim3(256), 0, st, static_cast<T*>(grid), sx, w, static_cast<T*>(packed));
    return hipGetLastError();
}

hipError_t launch_cost_window(hipStream_t st, void* grid, size_t elem, uint32_t sx, CostWindow w, void* packed, bool pack)
{
    if (!cost_window_cells(w)) return hipSuccess;
    return elem == 4 ? window_of<uint32_t>(st, grid, sx, w, packed, pack) : window_of<unsigned char>(st, grid, sx, w, packed, pack);
}

} // namespace gem
