// gem_frame_lean.hip -- k_frame's lean form: the kernels and their launch (launch_frame_lean, the lean branch of launch_frame).
//
// A translation unit of its own because it is built with -mllvm -amdgpu-kernarg-preload-count=14 (gem_amd/build.py), which acts on
// every kernel of a file: the leading scalar parameters of the kernels below -- the HEAD of a launch, FrameLeanHead in
// gem_frame_lean.hpp -- are in user SGPRs when a wave starts.  Before, the first phase of every workgroup was two dependent scalar
// fetches of kernel arguments (the tile / binning branch, then the words behind it), on lines the host writes for every launch, so
// every CU's scalar cache missed on them.  Now a tile block computes its tile from registers and issues the load of its count and
// its first DMA at once; the rest of the tile half is requested where the wave starts, one batch, and waited for behind those
// (frame_tile_rest, gem_frame_tile.hpp).  A binning block issues the load of its points from registers; the frame's constants
// follow behind that load as before (bin_unit_lean).
// On a device whose firmware does not preload, the 256-byte prologue the compiler puts in front of each kernel fetches the same
// words with scalar loads: the result is the same either way.
// The device code shared with the generic k_frame (gem_kernels.hip) is gem_frame_tile.hpp.  Built with -ffp-contract=off.
#include "gem_frame_tile.hpp"

#include <hip/hip_ext.h>

namespace gem {

// the head words as kernel parameters: FrameLeanHead's fields, in its order
#define GEM_FRAME_HEAD_PARAMS int nf, int T, int tiles_per_row, uint32_t tile_div, int center_tr, int center_tc, \
                              const uint32_t* bkt, uint32_t* bcount, const float4* xyzi, int B, uint32_t n
#define GEM_FRAME_HEAD_PASS   nf, T, tiles_per_row, tile_div, center_tr, center_tc, bkt, bcount, xyzi, B, n

template <int FLAGS, bool STAMPS>
__device__ __forceinline__ void frame_lean_body(GEM_FRAME_HEAD_PARAMS, const FrameLeanArgs& la)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_dyn[];
    if ((int)blockIdx.x < nf) {
        // the head from the parameters; every other word of the tile half is a load frame_tile waits for behind its first loads
        FrameLeanTile t = la.t;
        t.nf = nf; t.T = T; t.tiles_per_row = tiles_per_row; t.tile_div = tile_div; t.center_tr = center_tr; t.center_tc = center_tc;
        t.bkt = bkt; t.bcount = bcount;
        frame_tile<FLAGS, STAMPS>(t, (int)blockIdx.x, lds_dyn);
    } else {
        // a binning block issues the load of its points from the head (the frame's constants follow behind that load: bin_unit_lean)
        const int block = (int)blockIdx.x - nf;
        FrameLeanBin b = la.b;
        b.xyzi = xyzi; b.B = B; b.n = n;
        [[maybe_unused]] unsigned long long c_start = 0, r_start = 0;    // (the stamp buffer's pointer is not in the head: the start is stored behind the unit)
        if constexpr (STAMPS) { c_start = (unsigned long long)__builtin_readcyclecounter(); r_start = (unsigned long long)__builtin_amdgcn_s_memrealtime(); }
        bin_unit_lean(b, (int)(block * 4 + (threadIdx.x >> 6)));          // (the host launches this form for fast-laser frames only)
        if (block == 0 && threadIdx.x == 0) b.ctl[1] = 0u;                // (behind the unit: its pointer is not waited for in front of the points)
        if constexpr (STAMPS) {
            if (b.dbg && threadIdx.x == 0) {
                b.dbg[(size_t)block * 16] = c_start; b.dbg[(size_t)block * 16 + 15] = (unsigned long long)blockIdx.x + 1ull;
                b.dbg[(size_t)block * 16 + 12] = r_start;
                b.dbg[(size_t)block * 16 + 14] = (unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) + 1ull;      // HW_REG_XCC_ID
            }
        }
        bin_stamp_end<STAMPS>(b, block);
        // No scalar load of this half is pending where the two halves' code meets again.  The compiler lays the tile half out BEHIND
        // this one, and a load this half may have left pending into a register the tile half loads too made it put a full
        // s_waitcnt lgkmcnt(0) between the tile half's first two argument loads: a scalar round trip in front of the count's load
        // (seen in k_frame<4, true>).  Here every load is long back, so the wait is free; lgkmcnt(0) alone: 0xc07f.
        __builtin_amdgcn_s_waitcnt(0xc07f);
    }
}

#ifndef GEM_FRAME_LEAN_STAMPS
#define GEM_FRAME_LEAN_STAMPS 0
#endif
constexpr bool kFrameLeanStamps = GEM_FRAME_LEAN_STAMPS != 0;          // (build define: 1 = the production kernel carries the stamps as it did, for A/B builds)

// (the name and the template arguments of the generic form, gem_kernels.hip: LEAN = true is this one)
template <int FLAGS, bool LEAN>
__global__ __launch_bounds__(256, kFrameLeanWG) void k_frame(GEM_FRAME_HEAD_PARAMS, FrameLeanArgs la)
{
    static_assert(LEAN, "the generic form takes FuseArgs and BinArgs (gem_kernels.hip)");
    frame_lean_body<FLAGS, kFrameLeanStamps>(GEM_FRAME_HEAD_PASS, la);
}

// the lean form with the stamps of tools/frame_phases.py: what launch_frame_lean picks when the handle's stamp buffer is set
template <int FLAGS>
__global__ __launch_bounds__(256, kFrameLeanWG) void k_frame_stamped(GEM_FRAME_HEAD_PARAMS, FrameLeanArgs la) { frame_lean_body<FLAGS, true>(GEM_FRAME_HEAD_PASS, la); }

// (as in gem_kernels.hip: with a (start, stop) event pair the dispatch itself is time-stamped)
#define GEM_LAUNCH(k, grid, block, lds, st, ev, ...)                                              \
    do {                                                                                           \
        if ((ev).start || (ev).stop) hipExtLaunchKernelGGL(k, grid, block, (uint32_t)(lds), st, (ev).start, (ev).stop, 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(k, grid, block, lds, st, __VA_ARGS__);                             \
    } while (0)

hipError_t launch_frame_lean(hipStream_t st, const FuseArgs& fa, const BinArgs& ba, int attr, unsigned blocks, LaunchEvents ev)
{
    const dim3 grid(blocks), block(256);
    const FrameLeanArgs la = frame_lean_args(fa, ba);
    const FrameLeanHead h = frame_lean_head(la);
#define GEM_FRAME_HEAD_ARGS h.nf, h.T, h.tiles_per_row, h.tile_div, h.center_tr, h.center_tc, h.bkt, h.bcount, h.xyzi, h.B, h.n
    if (la.t.dbg || la.b.dbg) {                                          // the handle's stamp buffer is set: the diagnostic kernel
        if (attr == 4) GEM_LAUNCH((k_frame_stamped<4>), grid, block, kFrameLds, st, ev, GEM_FRAME_HEAD_ARGS, la);
        else           GEM_LAUNCH((k_frame_stamped<0>), grid, block, kFrameLds, st, ev, GEM_FRAME_HEAD_ARGS, la);
        return hipGetLastError();
    }
    if (attr == 4) GEM_LAUNCH((k_frame<4, true>), grid, block, kFrameLds, st, ev, GEM_FRAME_HEAD_ARGS, la);
    else           GEM_LAUNCH((k_frame<0, true>), grid, block, kFrameLds, st, ev, GEM_FRAME_HEAD_ARGS, la);
#undef GEM_FRAME_HEAD_ARGS
    return hipGetLastError();
}

} // namespace gem
