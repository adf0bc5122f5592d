// gem_inflate.hip -- InflationLayer's costs on the device costmap, gfx950: the squared distance of every cell to its nearest lethal
// cell, exact and truncated at the inflation radius R <= 127 cells, then the cost table.  The contract is restated in
// include/gem_hip_inflate.h.  Integer code throughout: the table comes from the host.
//
// The minimum over all seeds of dx^2 + dy^2 separates by row: with g(x, y') the distance from x to the nearest seed IN row y',
//     d2(x, y) = min over |dy| <= R of dy^2 + g(x, y + dy)^2,
// and a seed farther than R along its row cannot be within R at all, so g is only needed up to R (255: none).
//   k_inflate_seeds   a workgroup takes one word column x kInflateFlagRows rows of the seed region.  A wave's ballot over 64 bytes of a
//                     row is that row's bit word; the OR of the workgroup's words is the block's flag.  The main kernel reads the
//                     seeds from these words only, never from the grid it writes: the predicate it sees is the one before the call.
//   k_inflate         a workgroup takes a tile of 64 columns (one word column) x kInflateTileRows rows of the output region.  The
//                     flags of the blocks within R of the tile are tested first, and a tile with no seed near it leaves: on a costmap
//                     most do.  Row pass: for every row of the tile and its halo of R rows, lane l forms the 64 cells right of x (from
//                     x) and the 64 left of it out of the row's words by shifts (the words are wave-uniform), and find-first-bit
//                     gives the two distances; a second pair of words covers R >= 64.  g goes to LDS as bytes, 64 per row.  Column
//                     pass: a lane walks its column outward from dy = 0 and stops once dy^2 reaches the best so far.  Then
//                     table[d2], the NO_INFORMATION rule, and a store only where the byte changes.  Every cell belongs to one lane,
//                     which reads its old byte itself: no atomics.
//   k_inflate_reset   resetMap over a window.
// Tiles and words are aligned to multiples of 64 cells of the MAP, so a tile's own word column is bits[.., tile column].  Grids are
// flattened into blockIdx.x: a 1 x 2^30 map has more tile rows than a grid's second dimension holds.  Only vector loads and stores
// touch memory.
#include "gem_inflate.hpp"

#include <algorithm>

namespace gem {

static_assert(kInflateThreads == 256 && kInflateFlagRows % 4 == 0 && kInflateTileRows % 4 == 0, "four waves share the rows");

__global__ __launch_bounds__(kInflateThreads) void k_inflate_seeds(const unsigned char* __restrict__ grid, InflateArgs a,
                                                                   unsigned long long* __restrict__ bits, uint32_t* __restrict__ flags)
{
    __shared__ uint32_t s_any[4];
    const uint32_t wc = blockIdx.x % a.nw, fr = blockIdx.x / a.nw;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t x = (a.w0 + wc) * 64u + lane;
    const bool in_x = x >= a.seed.x0 && x < a.seed.x1;
    constexpr uint32_t kEach = kInflateFlagRows / 4;
    uint32_t any = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kEach; ++k) {
        const uint32_t y = a.seed.y0 + fr * kInflateFlagRows + wave * kEach + k;
        if (y >= a.seed.y1) break;                                      // (the same for the whole wave)
        const bool seed = in_x && grid[(size_t)y * a.sx + x] == kCostLethal;
        const unsigned long long word = __ballot(seed);
        if (lane == 0u) bits[(size_t)(y - a.seed.y0) * a.nw + wc] = word;
        any |= word != 0ull ? 1u : 0u;
    }
    if (lane == 0u) s_any[wave] = any;
    __syncthreads();
    if (threadIdx.x == 0u) flags[(size_t)fr * a.nw + wc] = s_any[0] | s_any[1] | s_any[2] | s_any[3];
}

// the words of row y (of the seed region) around tile column tw: word columns tw - 2 .. tw + 2, zero outside the seed region's
__device__ __forceinline__ unsigned long long inflate_word(const unsigned long long* __restrict__ row, const InflateArgs& a, int w)
{
    const int k = w - (int)a.w0;
    return (k >= 0 && k < (int)a.nw) ? row[k] : 0ull;
}

__global__ __launch_bounds__(kInflateThreads) void k_inflate(unsigned char* __restrict__ grid, InflateArgs a,
                                                             const unsigned long long* __restrict__ bits, const uint32_t* __restrict__ flags,
                                                             const unsigned char* __restrict__ table)
{
    __shared__ unsigned char s_g[(kInflateTileRows + 2 * kInflateMaxCells) * 64];
    const int R = (int)a.R;
    const int tw = (int)(a.ow0 + blockIdx.x % a.onw);                   // the tile's word column
    const int y0 = (int)(a.out.y0 + (blockIdx.x / a.onw) * kInflateTileRows);
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int sy0 = (int)a.seed.y0, sy1 = (int)a.seed.y1;

    // the seed rows and word columns within R of the tile
    const int ylo = max(y0 - R, sy0), yhi = min(y0 + (int)kInflateTileRows + R, sy1);
    const int wlo = max((tw * 64 - R) >> 6, (int)a.w0), whi = min((tw * 64 + 63 + R) >> 6, (int)(a.w0 + a.nw) - 1);   // (>> floors)
    if (ylo >= yhi || wlo > whi) return;
    {
        const int f0 = (ylo - sy0) / (int)kInflateFlagRows, nf = (yhi - 1 - sy0) / (int)kInflateFlagRows - f0 + 1, nwc = whi - wlo + 1;
        int found = 0;
        for (int i = (int)threadIdx.x; i < nf * nwc; i += kInflateThreads)
            found |= flags[(size_t)(f0 + i / nwc) * a.nw + (size_t)(wlo + i % nwc - (int)a.w0)] != 0u;
        if (!__syncthreads_or(found)) return;
    }

    // row pass: g of every row y0 - R + hr, hr = 0 .. rows + 2 R - 1
    const int H = (int)kInflateTileRows + 2 * R;
    const bool far = R >= 64;                                          // the first pair of words reaches 63 cells
    for (int hr = wave; hr < H; hr += 4) {
        const int y = y0 - R + hr;
        unsigned g = 255u;
        if (y >= sy0 && y < sy1) {
            const unsigned long long* row = bits + (size_t)(y - sy0) * a.nw;
            const unsigned long long w0 = inflate_word(row, a, tw), wl = inflate_word(row, a, tw - 1), wr = inflate_word(row, a, tw + 1);
            const unsigned long long wl2 = far ? inflate_word(row, a, tw - 2) : 0ull, wr2 = far ? inflate_word(row, a, tw + 2) : 0ull;
            if ((w0 | wl | wr | wl2 | wr2) != 0ull) {                   // (wave-uniform)
                // bit k of right: cell x + k; bit 63 - k of left: cell x - k
                const unsigned long long right = (w0 >> lane) | (lane ? wr << (64 - lane) : 0ull);
                const unsigned long long left = (w0 << (63 - lane)) | (lane < 63 ? wl >> (lane + 1) : 0ull);
                unsigned dr = right ? (unsigned)__builtin_ctzll(right) : 255u, dl = left ? (unsigned)__builtin_clzll(left) : 255u;
                if (far) {
                    const unsigned long long right2 = (wr >> lane) | (lane ? wr2 << (64 - lane) : 0ull);
                    const unsigned long long left2 = (wl << (63 - lane)) | (lane < 63 ? wl2 >> (lane + 1) : 0ull);
                    if (!right && right2) dr = 64u + (unsigned)__builtin_ctzll(right2);
                    if (!left && left2) dl = 64u + (unsigned)__builtin_clzll(left2);
                }
                g = min(dr, dl);
                if (g > (unsigned)R) g = 255u;
            }
        }
        s_g[hr * 64 + lane] = (unsigned char)g;
    }
    __syncthreads();

    // column pass
    const unsigned x = (unsigned)tw * 64u + (unsigned)lane;
    if (x >= a.sx) return;
    const int none = R * R + 1;
    constexpr int kEach = (int)kInflateTileRows / 4;
    for (int k = 0; k < kEach; ++k) {
        const int r = wave * kEach + k, y = y0 + r;
        if (y >= (int)a.out.y1) break;
        const unsigned char* col = s_g + (R + r) * 64 + lane;
        int best = none;
        {
            const int g = col[0];
            if (g != 255) best = g * g;
        }
        for (int dy = 1; dy <= R && dy * dy < best; ++dy) {
            const int up = col[-dy * 64], dn = col[dy * 64], g = min(up, dn);
            if (g != 255) best = min(best, dy * dy + g * g);
        }
        if (best >= none) continue;
        const unsigned char cost = table[best];
        unsigned char* cell = grid + (size_t)y * a.sx + x;
        const unsigned char old = *cell;
        unsigned char now;
        if (old == kCostNoInfo && (a.inflate_unknown ? cost > 0 : cost >= kCostInscribed)) now = cost;
        else now = old > cost ? old : cost;
        if (now != old) *cell = now;
    }
}

__global__ __launch_bounds__(kInflateThreads) void k_inflate_reset(unsigned char* __restrict__ grid, uint32_t sx, InflateBox w, unsigned char value)
{
    const size_t width = w.x1 - w.x0, n = width * (size_t)(w.y1 - w.y0), stride = (size_t)gridDim.x * kInflateThreads;
    for (size_t i = (size_t)blockIdx.x * kInflateThreads + threadIdx.x; i < n; i += stride)
        grid[(size_t)(w.y0 + i / width) * sx + (w.x0 + i % width)] = value;
}

InflateArgs inflate_args(uint32_t sx, uint32_t sy, int min_i, int min_j, int max_i, int max_j, uint32_t R, int inflate_unknown)
{
    InflateArgs a{};
    a.sx = sx; a.sy = sy; a.R = R; a.inflate_unknown = inflate_unknown ? 1 : 0;
    const long long r = (long long)R;
    auto widen = [&](long long x0, long long y0, long long x1, long long y1) {
        return InflateBox{(uint32_t)std::max(x0 - r, 0ll), (uint32_t)std::max(y0 - r, 0ll), (uint32_t)std::min(x1 + r, (long long)sx),
                          (uint32_t)std::min(y1 + r, (long long)sy)};
    };
    a.seed = widen(min_i, min_j, max_i, max_j);
    a.out = widen(a.seed.x0, a.seed.y0, a.seed.x1, a.seed.y1);
    a.w0 = a.seed.x0 / 64u; a.nw = (a.seed.x1 - 1u) / 64u - a.w0 + 1u;
    a.ow0 = a.out.x0 / 64u; a.onw = (a.out.x1 - 1u) / 64u - a.ow0 + 1u;
    return a;
}

hipError_t launch_inflate_seeds(hipStream_t st, const unsigned char* grid, const InflateArgs& a, unsigned long long* bits, uint32_t* flags)
{
    const size_t blocks = inflate_flag_rows(a) * a.nw;
    hipLaunchKernelGGL(k_inflate_seeds, dim3((unsigned)blocks), dim3(kInflateThreads), 0, st, grid, a, bits, flags);
    return hipGetLastError();
}

hipError_t launch_inflate(hipStream_t st, unsigned char* grid, const InflateArgs& a, const unsigned long long* bits, const uint32_t* flags,
                          const unsigned char* table)
{
    const size_t tile_rows = (a.out.y1 - a.out.y0 + kInflateTileRows - 1) / kInflateTileRows;
    hipLaunchKernelGGL(k_inflate, dim3((unsigned)(tile_rows * a.onw)), dim3(kInflateThreads), 0, st, grid, a, bits, flags, table);
    return hipGetLastError();
}

hipError_t launch_inflate_reset(hipStream_t st, unsigned char* grid, uint32_t sx, InflateBox w, unsigned char value)
{
    const size_t n = (size_t)(w.x1 - w.x0) * (w.y1 - w.y0);
    if (!n) return hipSuccess;
    const size_t blocks = std::min<size_t>((n + kInflateThreads - 1) / kInflateThreads, 8192);
    hipLaunchKernelGGL(k_inflate_reset, dim3((unsigned)blocks), dim3(kInflateThreads), 0, st, grid, sx, w, value);
    return hipGetLastError();
}

} // namespace gem
