// gem_frame_pair.hip -- k_frame's pair form: one grid that runs two complete single-sweep halves (launch_frame_pair).
//
// The host holds every other call of a stream of sweeps nobody reads in between (gem_frame_pair.hpp) and this kernel carries both:
// a tile workgroup runs the whole of frame_tile for the first fused sweep, passes a barrier, and runs it again for the second; the
// binning blocks of slot 0 bin the first new sweep with its own frame constants into its own pass buffer set, those of slot 1 the
// second into another -- bin_unit_lean and frame_tile unchanged (gem_frame_tile.hpp), no new fusing logic.  One launch instead of
// two: one dispatch front, one ramp, one HIP call of the host.
// A translation unit of its own because gem_frame_lean.hip is built with kernel-argument preloading, which acts on every kernel of
// a file, and the lean kernels there are the only ones meant to preload: this kernel fetches its head with scalar loads, once per
// pair.  Nothing here waits on another workgroup; no result depends on residency or on dispatch order: the tile blocks of a launch
// read the sets the launch BEFORE binned, the binning blocks write other sets.
// Lean form only (bucket records, fast laser projection, no colours, no lowest tracking, no stamps).  Built with -ffp-contract=off.
#include "gem_frame_tile.hpp"
#include "gem_frame_pair.hpp"

#include <hip/hip_ext.h>

namespace gem {

// (the name in front of the template arguments ends in k_frame: the committed counter summaries are looked up by it)
template <int FLAGS>
__global__ __launch_bounds__(256, kFrameLeanWG) void pair_k_frame(FramePairArgs pa)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_dyn[];
    if ((int)blockIdx.x < pa.nf) {
        // Round 0, a barrier, round 1.  Every exit of frame_tile is block-uniform and its barriers are balanced on every path, so
        // all four waves meet here.  The barrier protects the LDS rows and misc, and it orders round 0's stores of the layers
        // before round 1's loads of the same cells at workgroup scope (the workgroup is on one CU).
        // (Requesting round 1's count and its first bucket lines in front of round 0, to find them in this XCD's L2 later, and
        //  leaving between the rounds when round 1's count is zero, was measured and lost: profiles/HISTORY.md.)
        frame_tile<FLAGS, false>(pa.s[0].t, (int)blockIdx.x, lds_dyn);
        __syncthreads();
        frame_tile<FLAGS, false>(pa.s[1].t, (int)blockIdx.x, lds_dyn);
    } else {
        // (a branch per slot, block-uniform: the slot's constants are scalar loads at fixed offsets of the kernel arguments)
        const int block = (int)blockIdx.x - pa.nf;
        if (block < pa.nbin[0]) {
            bin_unit_lean(pa.s[0].b, (int)(block * 4 + (threadIdx.x >> 6)));
            if (block == 0 && threadIdx.x == 0) pa.s[0].b.ctl[1] = 0u;
        } else {
            const int block1 = block - pa.nbin[0];
            bin_unit_lean(pa.s[1].b, (int)(block1 * 4 + (threadIdx.x >> 6)));
            if (block1 == 0 && threadIdx.x == 0) pa.s[1].b.ctl[1] = 0u;
        }
    }
}

// ---- the overlapping form: what the second round repeats for nothing is done once ---------------------------------------------------
// pair_k_frame's two rounds each wait for the tile's count and only then request its records: frame_tile is written to have both in
// ONE round trip, but in this kernel (no preloaded head) the compiler moves the count's first use in front of the DMA, so every
// round pays two.  Here a tile workgroup requests BOTH sweeps' counts and the first sweep's records together, first uses the
// counts behind the DMA (an empty asm statement the values pass through), and runs the two rounds from them (frame_tile's PRE
// form): the second round's DMA leaves right behind the barrier between the rounds -- no count, no wait in front of it.  Per
// pair of rounds that is two round trips and one load less; the rounds themselves, their fall-backs and the barrier between
// them are pair_k_frame's.
// (Measured and taken out, profiles/HISTORY.md: light pairs fused by one wave as one set, which loses; the head of both slots pinned
//  as one batch of scalar loads in front of the tile / binning branch, which gains nothing and doubles the scalar spills.)

// records [64 w, 64 w + 64) of the tile's bucket -> stage[64 w ..]: frame_tile's first DMA (inside the bucket whatever the count)
__device__ __forceinline__ void frame_pair_dma(const uint32_t* bkt, int tile, int w, int lane, uint4* stage)
{
    const auto* gsrc = (const __attribute__((address_space(1))) void*)(bkt + (size_t)tile * kFrameBucket * 3 + (size_t)((uint32_t)w * 64u + (uint32_t)lane) * 3);
    __builtin_amdgcn_global_load_lds(gsrc, (__attribute__((address_space(3))) void*)(stage + w * 64), 12, 0, 0);
}

// a: the first slot's tile half, b: the second's.  Both describe the same map through the same
// tile map (launch_frame_pair), so one block -> tile computation serves both.
template <int FLAGS>
__device__ __forceinline__ void frame_tile_pair(const FrameLeanTile& a, const FrameLeanTile& b, int block, unsigned char* lds_raw)
{
    constexpr int CELLS = 256, PB = kFramePB;
    uint4* stage = reinterpret_cast<uint4*>(lds_raw + CELLS * 16 + PB * 2 * 2);              // (frame_tile's layout)
    const int lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    int tr, tc;
    if (frame_tile_of(a, block, tr, tc)) {
        const int tile = tr * a.tiles_per_row + tc;
        uint32_t nAv = a.bcount[tile], nBv = b.bcount[tile];             // block-uniform, both
        frame_pair_dma(a.bkt, tile, w, lane, stage);
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(nAv), "+v"(nBv) :: "memory");             // the counts' first use: behind the DMA
#endif
        const uint32_t nA = (uint32_t)__builtin_amdgcn_readfirstlane((int)nAv), nB = (uint32_t)__builtin_amdgcn_readfirstlane((int)nBv);
        frame_tile<FLAGS, false, true>(a, block, lds_raw, nA);
        __syncthreads();                                                 // (pair_k_frame's: the LDS rows, and the first round's stores before the second's loads)
        frame_pair_dma(b.bkt, tile, w, lane, stage);
        frame_tile<FLAGS, false, true>(b, block, lds_raw, nB);
    }
}

template <int FLAGS>
__global__ __launch_bounds__(256, kFrameLeanWG) void pairov_k_frame(FramePairArgs pa)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_dyn[];
    if ((int)blockIdx.x < pa.nf) {
        frame_tile_pair<FLAGS>(pa.s[0].t, pa.s[1].t, (int)blockIdx.x, lds_dyn);
    } else {                                                             // the binning half: pair_k_frame's
        const int block = (int)blockIdx.x - pa.nf;
        if (block < pa.nbin[0]) {
            bin_unit_lean(pa.s[0].b, (int)(block * 4 + (threadIdx.x >> 6)));
            if (block == 0 && threadIdx.x == 0) pa.s[0].b.ctl[1] = 0u;
        } else {
            const int block1 = block - pa.nbin[0];
            bin_unit_lean(pa.s[1].b, (int)(block1 * 4 + (threadIdx.x >> 6)));
            if (block1 == 0 && threadIdx.x == 0) pa.s[1].b.ctl[1] = 0u;
        }
    }
}

#define GEM_LAUNCH(k, grid, block, lds, st, ev, ...)                                              \
    do {                                                                                           \
        if ((ev).start || (ev).stop) hipExtLaunchKernelGGL(k, grid, block, (uint32_t)(lds), st, (ev).start, (ev).stop, 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(k, grid, block, lds, st, __VA_ARGS__);                             \
    } while (0)

// fuse[0 .. nfuse) in order || bin[0 .. nbin), each into its own set; at most two of either, at least one of both together
// overlap: the overlapping kernel where it applies -- two sweeps to fuse, into the same map through the same tile map
// (frame_pair_same_map, gem_frame_pair.hpp); pair_k_frame otherwise
hipError_t launch_frame_pair(hipStream_t st, const FuseArgs* const* fuse, int nfuse, const BinArgs* const* bin, int nbin, LaunchEvents ev, bool overlap)
{
    if (nfuse < 0 || nfuse > 2 || nbin < 0 || nbin > 2 || nfuse + nbin == 0) return hipErrorInvalidValue;
    FramePairArgs pa{};
    const FuseArgs no_fuse{};
    const BinArgs no_bin{};
    for (int s = 0; s < 2; ++s) {
        pa.s[s] = frame_lean_args(s < nfuse ? *fuse[s] : no_fuse, s < nbin ? *bin[s] : no_bin);
        if (s >= nfuse) { pa.s[s].t.T = 0; pa.s[s].t.nf = 0; }           // (frame_tile leaves at once: no rank is below T)
        if (s >= nbin) pa.s[s].b.B = 0;
        pa.nbin[s] = (pa.s[s].b.B + 3) / 4;
        if (pa.s[s].t.nf > pa.nf) pa.nf = pa.s[s].t.nf;
    }
    const dim3 grid((unsigned)(pa.nf + pa.nbin[0] + pa.nbin[1])), block(256);
    if (grid.x == 0) return hipSuccess;
    if (overlap && nfuse == 2 && frame_pair_same_map(*fuse[0], *fuse[1])) GEM_LAUNCH((pairov_k_frame<0>), grid, block, kFrameLds, st, ev, pa);
    else GEM_LAUNCH((pair_k_frame<0>), grid, block, kFrameLds, st, ev, pa);
    return hipGetLastError();
}

} // namespace gem
