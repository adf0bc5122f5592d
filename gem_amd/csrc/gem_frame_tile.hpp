// gem_frame_tile.hpp -- the device code both forms of k_frame share (internal header): the bucket form's stores, the lean binning
// unit, the cycle stamps, and frame_tile -- one workgroup fusing one tile's bucket.  gem_kernels.hip holds the generic k_frame,
// gem_frame_lean.hip the lean one (a translation unit of its own: it is built with kernel-argument preloading, a flag that acts
// on every kernel of a file).  Device code only; built with -ffp-contract=off (see gem_device.hpp).
#pragma once

#include "gem_kernels.hpp"
#include "gem_frame_lean.hpp"
#include "gem_frame_sort.hpp"
#include "gem_wave.hpp"

#include <type_traits>

namespace gem {

// A binned record: {height, variance, cell in tile | colour flag << 31, index of the point}.  The last word is only read when colours are
// fused (ATTR != 0): without them the records are 12 bytes -- a quarter less to write, to read back and to stage through the LDS.
struct __attribute__((packed, aligned(4))) Rec3 { uint32_t x, y, z; };
__device__ __forceinline__ void rec_store3(uint4* rec, size_t i, uint32_t x, uint32_t y, uint32_t z)
{
    *reinterpret_cast<Rec3*>(reinterpret_cast<uint32_t*>(rec) + i * 3) = Rec3{x, y, z};
}

// k_frame's binning waves raise their issue priority (s_setprio) behind the issue of the load of their points.  Eight workgroups
// share a CU and a SIMD issues for the highest level first; the binning blocks come last in block order, a binning wave is ~130
// vector instructions and two memory round trips, and at the tiles' level it waited its turn behind tile waves most of which have a
// microsecond of slack.  Measured (profiles/HISTORY.md, last section): a binning block's mean life 2.6 -> 2.0 us, the last one's end
// 4.8 -> 3.8 us of a stamped launch, the C2 step 5.95 -> 5.75 us.  Levels for the tiles' waves by their record count were measured
// as well: alone no gain, with this one inside the noise, left out.  (Only the order of the levels counts: any value above the
// tiles' 0 is the same.)  The lean form only (bin_unit_lean): the same line in bin_unit cost the generic k_frame four more scalar
// spills (10 -> 14).
#ifndef GEM_FRAME_BIN_PRIO
#define GEM_FRAME_BIN_PRIO 3
#endif
constexpr int kFrameBinPrio = GEM_FRAME_BIN_PRIO;                       // (build define: 0 = the binning waves at the tiles' level, for A/B builds)

// the bucket form's stores (A: BinArgs or FrameLeanBin): the wave's points grouped by tile, stable in lane (= input) order
template <class A>
__device__ __forceinline__ void bucket_store(const A& a, bool valid, uint32_t tile, uint32_t cl, uint32_t src, float hh, float vv)
{
    const int lane = lane_id();
    const uint64_t peers = wave_peers_few(valid, tile, a.tile_bits);
    const uint64_t lt = lanemask_lt();
    const uint32_t rank = (uint32_t)__popcll(peers & lt);
    const uint32_t cnt = (uint32_t)__popcll(peers);
    const bool leader = valid && rank == 0;
    uint32_t old = 0;
    if (leader) old = atomicAdd(&a.bcount[tile], cnt);
    old = (uint32_t)__shfl((int)old, valid ? (__ffsll((unsigned long long)peers) - 1) : lane, 64);
    if (valid) {
        const uint32_t pos = old + rank, z = cl | (src << 8);
        if (pos < (uint32_t)kFrameBucket) rec_store3(reinterpret_cast<uint4*>(a.bkt), (size_t)tile * kFrameBucket + pos, __float_as_uint(hh), __float_as_uint(vv), z);
        else a.spill[src] = make_uint4(__float_as_uint(hh), __float_as_uint(vv), z, tile);
    }
}

// STAMPS = false (k_frame's lean production form): no stamp code at all, a.dbg is not read
template <bool STAMPS = true, class A>
__device__ __forceinline__ void bin_stamp_begin(const A& a, int block)
{
    if constexpr (!STAMPS) return;
    else if (a.dbg && threadIdx.x == 0) {
        a.dbg[(size_t)block * 16] = (unsigned long long)__builtin_readcyclecounter(); a.dbg[(size_t)block * 16 + 15] = (unsigned long long)blockIdx.x + 1ull;
        a.dbg[(size_t)block * 16 + 12] = (unsigned long long)__builtin_amdgcn_s_memrealtime();
        a.dbg[(size_t)block * 16 + 14] = (unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) + 1ull;      // HW_REG_XCC_ID
    }
}
template <bool STAMPS = true, class A>
__device__ __forceinline__ void bin_stamp_end(const A& a, int block)
{
    if constexpr (!STAMPS) return;
    else if (a.dbg && threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        a.dbg[(size_t)block * 16 + 1] = (unsigned long long)__builtin_readcyclecounter(); a.dbg[(size_t)block * 16 + 13] = (unsigned long long)__builtin_amdgcn_s_memrealtime();
    }
}

// The lean form's arguments beyond the preloaded head are pinned in scalar registers at ONE place per path (a tile: frame_tile_rest,
// behind its first vector loads; a binning unit: behind the load of its points): an empty asm statement the value has to pass
// through in an SGPR.  Left alone the compiler sinks every argument load into the block that first uses it and a wave waits out a
// scalar-cache round trip per block; pinned, the loads of one path are one batch of wide s_load and one wait.
// (A pointer that went through the statement is a global one all the same: the cast says so, or its accesses would be flat ones.)
#if defined(__HIP_DEVICE_COMPILE__)
#define GEM_PIN(x) asm volatile("" : "+s"(x))
#define GEM_PIN_PTR(p) do { uintptr_t u_ = reinterpret_cast<uintptr_t>(p); asm volatile("" : "+s"(u_)); (p) = (decltype(p))(__attribute__((address_space(1))) std::remove_pointer_t<decltype(p)>*)u_; } while (0)
#else
#define GEM_PIN(x) (void)(x)
#define GEM_PIN_PTR(p) (void)(p)
#endif

// k_frame's lean form: one unit of a single fast-laser sweep without colours (the host has checked that: frame_launch_lean) into the
// buckets, from the lean argument block -- the generic projection, its doubles and the two thirds of FrameConst only it reads are
// not carried.  The point count is a word here (a single sweep), the arithmetic is bin_unit's.
__device__ __forceinline__ void bin_unit_lean(const FrameLeanBin& a, int unit)
{
    constexpr int TS = 4, TE = 16;
    if (unit >= a.B) return;                               // whole wave leaves together
    const uint32_t i = (uint32_t)unit * 64u + (uint32_t)lane_id();
    const float4 p = a.xyzi[i < a.n ? i : 0u];
    if constexpr (kFrameBinPrio != 0) __builtin_amdgcn_s_setprio(kFrameBinPrio);     // (above the tiles' waves, behind the issue of the load)
    // the frame's constants arrive while the load of the points is in flight: one batch, no scalar load is waited for behind it
    FrameLeanBin f = a;
    GEM_PIN(f.keep_sentinel); GEM_PIN(f.tile_bits); GEM_PIN(f.tiles_per_row); GEM_PIN(f.filter_on); GEM_PIN_PTR(f.bkt); GEM_PIN_PTR(f.bcount);
#pragma unroll
    for (int k = 0; k < 12; ++k) GEM_PIN(f.T[k]);
    GEM_PIN(f.lower_f); GEM_PIN(f.upper_f); GEM_PIN(f.fbx); GEM_PIN(f.fby); GEM_PIN(f.fband); GEM_PIN(f.fplane);
    GEM_PIN(f.cx); GEM_PIN(f.cy); GEM_PIN(f.sx); GEM_PIN(f.sy); GEM_PIN(f.L); GEM_PIN(f.res); GEM_PIN(f.row0); GEM_PIN(f.row1);
    GEM_PIN(f.beam_a); GEM_PIN(f.beam_c); GEM_PIN(f.t2); GEM_PIN(f.Js[0]); GEM_PIN(f.Js[1]);
    int row, col; float hh, vv;
    const bool valid = project_bin_laser_fast(f, p.x, p.y, p.z, i < a.n, f.keep_sentinel != 0, row, col, hh, vv);
    uint32_t tile = (uint32_t)((row >> TS) * f.tiles_per_row + (col >> TS));
    uint32_t cl = (uint32_t)(((row & (TE - 1)) << TS) | (col & (TE - 1)));
    if (!valid) { tile = 0; cl = 0; }
    bucket_store(f, valid, tile, cl, i, hh, vv);
}

constexpr int kRankMax    = 7;           // fast path: records per cell and batch

constexpr int kFramePB = kFrameBucket;              // records per tile the fast path holds in LDS
constexpr int kFrameSpec = 256;                     // records requested before the count is known: one per thread
#ifndef GEM_FRAME_SIZED_SORT
#define GEM_FRAME_SIZED_SORT 1
#endif
constexpr bool kFrameSizedSort = GEM_FRAME_SIZED_SORT != 0;          // (build define: 0 = every wave runs the 8-key network, for A/B builds)
#ifndef GEM_FRAME_RANK_ONE
#define GEM_FRAME_RANK_ONE 1
#endif
#ifndef GEM_FRAME_LIGHT
#define GEM_FRAME_LIGHT 1
#endif
constexpr bool kFrameLight = GEM_FRAME_LIGHT != 0;                   // (build define: 0 = every tile takes the cell-centric path, for A/B builds)
constexpr bool kFrameRankOne = GEM_FRAME_RANK_ONE != 0;             // (build define: 0 = every tile ranks kFramePB / 256 slots per thread, for A/B builds)
constexpr int kFrameWG = 6;                         // workgroups per CU the register budget is set for
// LDS: rank rows [256] x 8 u16 | generic lists head / tail [256][4] u16 (aliased), cell of a slot [PB] u16, next [PB] u16, stage [PB] x 16 B, misc
constexpr size_t kFrameLds = 256 * 16 + kFramePB * 2 * 2 + kFramePB * 16 + 16;

// LEAN: the form the HOST picks per launch while no tile of the handle has needed frame_tile's slow path (gem_capi_pipeline.cpp,
// frame_launch_lean).  It carries the bucket form only -- frame_tile for the tile blocks (its slow path included, so the form is
// right for any input, only slow for heavy tiles), bucket binning that does not read ctl[0] and sets ctl[1] = 0 -- and so fits
// the budget of kFrameLeanWG workgroups per CU: at most 64 VGPRs, at most 80 SGPRs (the CU admits min(8, 800 / (sgprs rounded up
// to 16 + 16)) blocks of four waves), kFrameLds of LDS.  With 1472 + 512 workgroups of a C2 frame and 2048 slots every block is
// resident from the start; nothing in the kernel depends on that.  The generic form (LEAN = false) is the kernel as it was.
#ifndef GEM_FRAME_LEAN_WG
#define GEM_FRAME_LEAN_WG 8
#endif
constexpr int kFrameLeanWG = GEM_FRAME_LEAN_WG;                         // (build define: 6 tells "lean" and "eight per CU" apart on the GPU)
static_assert(kFrameLeanWG >= 1 && kFrameLeanWG <= 8 && (size_t)kFrameLeanWG * kFrameLds <= 160 * 1024, "kFrameLeanWG lean workgroups fit the CU's LDS");

// A: FuseArgs (the generic form), or FrameLeanTile (the lean form's own argument block, gem_frame_lean.hpp).
// STAMPS: the cycle stamps of tools/frame_phases.py (a.dbg, thread 0) are compiled in -- the generic form and k_frame_stamped; the
// lean production kernel carries none of it: no a.dbg, no stamp counter, no tid == 0 masks kept alive for them.
// one step of the reference's recurrence (GPU:480-531) on a cell's registers; !live leaves them as they are
template <bool LOWEST>
__device__ __forceinline__ void frame_chain_step(float& ce, float& cs, float& lw, float h, float v, bool live, float mahal, float var_floor)
{
    float e2 = ce, s2 = cs;
    (void)fuse_step(e2, s2, h, v, mahal, var_floor);
    const bool fl = live && (!LOWEST || h != -1.0f);                     // GPU:482 (only LOWEST passes carry such records)
    ce = fl ? e2 : ce; cs = fl ? s2 : cs;
    if constexpr (LOWEST) { const float l2 = lowest_step(lw, h, v); lw = live ? l2 : lw; }
}

// The lean form hands frame_tile its HEAD alone in registers (gem_frame_lean.hpp, FrameLeanHead: the words of the block -> tile map,
// the bucket and its count -- preloaded into scalar registers where the wave starts, gem_frame_lean.hip) and every other word of the
// tile half as a load in flight: frame_tile_rest is where those are waited for, ONE batch, behind the issue of the count's load
// and the first DMA.  (The generic form's arguments are one object, fetched as the compiler sees fit.)
template <int FLAGS, bool STAMPS>
__device__ __forceinline__ void frame_tile_rest(FrameLeanTile& t)
{
    if constexpr (STAMPS) GEM_PIN_PTR(t.dbg);
    GEM_PIN_PTR(t.elevation); GEM_PIN_PTR(t.variance); if constexpr ((FLAGS & 4) != 0) { GEM_PIN_PTR(t.lowest); GEM_PIN(t.start0); GEM_PIN(t.start1); }
    GEM_PIN(t.L); GEM_PIN(t.row0); GEM_PIN(t.row1);
    GEM_PIN(t.n_pending); GEM_PIN(t.pending[0]); GEM_PIN(t.pending[1]); GEM_PIN(t.pending[2]); GEM_PIN(t.pending[3]);
    GEM_PIN(t.dense); GEM_PIN(t.mahal); GEM_PIN(t.var_floor);
}

// PRE (the pair kernel's overlapping form, gem_frame_pair.hip): the caller has loaded the count and issued this wave's first DMA
// itself -- exactly the two requests below -- and hands the count in; every other instantiation is the code it was.
template <int FLAGS, bool STAMPS, bool PRE = false, class A>
__device__ __forceinline__ void frame_tile(const A& args, int block, unsigned char* lds_raw, [[maybe_unused]] uint32_t nrec_pre = 0u)
{
    constexpr bool LOWEST = (FLAGS & 4) != 0;
    constexpr bool LEAN = std::is_same_v<A, FrameLeanTile>;
    constexpr int TS = 4, TE = 16, CELLS = 256, NT = 256, NW = 4, PB = kFramePB;
    constexpr uint32_t NIL = 0xffffu;
    static_assert(PB % 64 == 0 && PB % NT == 0 && kFrameSpec == NT && PB <= 1024, "geometry");
    uint16_t* rowp  = reinterpret_cast<uint16_t*>(lds_raw);                // fast path: rows[CELLS] of 8 u16 {slot 0..6, count}
    uint16_t* head  = rowp;                                                // slow path: head / tail [CELLS][NW]
    uint16_t* tail  = head + CELLS * NW;
    uint16_t* scell = reinterpret_cast<uint16_t*>(lds_raw + CELLS * 16);   // [PB] slow path: cell of a slot, NIL = no record
    uint16_t* nxt   = scell + PB;                                          // [PB]
    uint4*    stage = reinterpret_cast<uint4*>(nxt + PB);                  // [PB] {h, var, cell | index << 8, -}
    uint32_t* misc  = reinterpret_cast<uint32_t*>(stage + PB);             // [0] fast-path overflow, [1] next window

    const int tid = (int)threadIdx.x, lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);              // (uniform: the LDS base of a DMA goes to M0)
    // the lean form: a copy, whose words beyond the head are loads in flight until frame_tile_rest (below) pins them
    std::conditional_t<LEAN, A, const A&> a = args;
    int tr, tc;
    if (!frame_tile_of(a, block, tr, tc)) return;
    const int tile = tr * a.tiles_per_row + tc;
    const int row_base = tr << TS, col_base = tc << TS;
    int L = a.L;
    [[maybe_unused]] int dbg_k = 0;
#define GEM_STAMP() do { if constexpr (STAMPS) { if (a.dbg && tid == 0) a.dbg[(size_t)tile * 16 + dbg_k++] = (unsigned long long)__builtin_readcyclecounter(); } } while (0)
#define GEM_STAMP_END() do { if constexpr (STAMPS) { if (a.dbg && tid == 0) { \
        a.dbg[(size_t)tile * 16 + 13] = (unsigned long long)__builtin_amdgcn_s_memrealtime(); \
        a.dbg[(size_t)tile * 16 + 15] = (unsigned long long)block + 1ull; \
        a.dbg[(size_t)tile * 16 + 14] = (unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) + 1ull;      /* HW_REG_XCC_ID: the XCD's clock is its own */ \
    } } } while (0)
    // (the lean form's stamp buffer is not in the head: its start stamps are taken here and stored behind frame_tile_rest)
    [[maybe_unused]] unsigned long long c_start = 0, r_start = 0;
    if constexpr (!LEAN) {
        GEM_STAMP();                                                     // 0: start
        if constexpr (STAMPS) { if (a.dbg && tid == 0) a.dbg[(size_t)tile * 16 + 12] = (unsigned long long)__builtin_amdgcn_s_memrealtime(); }   // (100 MHz, one clock for the chip)
    } else if constexpr (STAMPS) {
        c_start = (unsigned long long)__builtin_readcyclecounter(); r_start = (unsigned long long)__builtin_amdgcn_s_memrealtime();
    }

    // ---- one round trip: the count, the first kFrameSpec records of the bucket and the tile ------------------
    uint32_t nrec;                                                       // block-uniform
    if constexpr (PRE) nrec = nrec_pre; else nrec = a.bcount[tile];
    const uint32_t* const bkt = a.bkt + (size_t)tile * kFrameBucket * 3;
    auto dma = [&](uint32_t k0) {                                        // records [k0, k0 + 64) -> stage[k0 ..]: lane l's 12 bytes land at 16 l
        const auto* gsrc = (const __attribute__((address_space(1))) void*)(bkt + (size_t)(k0 + (uint32_t)lane) * 3);
        auto* ldst = (__attribute__((address_space(3))) void*)(stage + k0);
        __builtin_amdgcn_global_load_lds(gsrc, ldst, 12, 0, 0);
    };
    if constexpr (!PRE) dma((uint32_t)w * 64u);                          // (inside the bucket whatever the count: kFrameSpec <= kFrameBucket)

    // ---- the lean form: every word beyond the head, requested where the wave started, is waited for here, one batch
    if constexpr (LEAN) { frame_tile_rest<FLAGS, STAMPS>(a); L = a.L; }
    if constexpr (STAMPS && LEAN) {
        if (a.dbg && tid == 0) { a.dbg[(size_t)tile * 16 + dbg_k++] = c_start; a.dbg[(size_t)tile * 16 + 12] = r_start; }   // 0: start
    }

    // ---- LIGHT PATH (lean form): the count decides before any cell load is issued.  An empty tile leaves here; a tile of at
    //      most 64 records is fused by wave 0 alone, one lane per RECORD instead of one thread per cell -- two thirds of a C2
    //      sweep's tile workgroups hold 24 records in 21 of their 256 cells.  dense (queued increments, a dirty floor) touches
    //      every cell and keeps the general path.
    if constexpr (LEAN && kFrameLight) {
        if (!a.dense && nrec <= 64u) {                                   // block-uniform; every branch on nrec, w and over below is wave-uniform
            bool over = false;
            if (nrec == 0) {
                GEM_STAMP();
            } else if (w != 0) {
                __syncthreads();                                         // the one barrier of a light tile: waves 1-3 learn the verdict
                over = __builtin_amdgcn_readfirstlane((int)misc[2]) != 0;
            } else {
                // all records of the tile are the 64 slots this wave's own DMA brought: its own vmcnt, no barrier
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                bool on = (uint32_t)lane < nrec;
                const uint32_t z = stage[on ? lane : 0].z;
                const uint32_t cell = z & 0xffu, idx = z >> 8;
                const int row = row_base + (int)(cell >> TS), col = col_base + (int)(cell & (TE - 1));
                on = on && row < a.row1 && row >= a.row0 && col < L;     // (the binning keeps no other record: a guard, not a case)
                size_t g = 0, gl = 0;
                if (on) {
                    g = (size_t)row * L + col;
                    if constexpr (LOWEST) {                              // (the geographic cell, as the general path computes it)
                        int gr = row - a.start0, gc = col - a.start1;
                        gr += gr < 0 ? L : 0; gc += gc < 0 ? L : 0;
                        gl = (size_t)gr * L + gc;
                    }
                }
                // the second round trip: the record's cell (off lanes read cell 0; duplicate addresses among lanes are fine)
                float ce = a.elevation[g], cs = a.variance[g], lw = 0.0f;
                if constexpr (LOWEST) lw = a.lowest[gl];
                GEM_STAMP();                                             // 1: records arrived, cell loads issued
                // ... and while those are in flight: the lanes of a cell, and the verdict (a cell above kRankMax: as before)
                const uint64_t peers = wave_peers(on, cell, 2 * TS);
                over = __ballot(__popcll(peers) > kRankMax) != 0;
                if (lane == 0) misc[2] = over ? 1u : 0u;                 // (misc[0] / [1] are the general path's: it resets them unsynchronised)
                __syncthreads();
                if (!over) {                                             // wave-uniform
                    GEM_STAMP();                                         // 2: grouped, verdict known
                    // rank = peers with a smaller point index (the bucket is in reservation order); the group's lowest lane owns the cell
                    uint32_t rank = 0;
                    for (uint64_t m = peers & ~(1ull << lane); __ballot(m != 0) != 0; m &= m - 1) {      // wave-uniform: the largest group - 1 rounds
                        const int j = m != 0 ? __ffsll((unsigned long long)m) - 1 : lane;
                        const uint32_t other = (uint32_t)__builtin_amdgcn_ds_bpermute(j << 2, (int)idx);
                        rank += (m != 0 && other < idx) ? 1u : 0u;
                    }
                    // the rank rows hand the records over in index order (written and read by this wave alone: LDS is in order per wave)
                    if (on) rowp[cell * 8 + rank] = (uint16_t)lane;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    const bool owner = on && (peers & lanemask_lt()) == 0;
                    const uint32_t n = owner ? (uint32_t)__popcll(peers) : 0u;
                    const uint4 rw = *reinterpret_cast<const uint4*>(rowp + cell * 8);
                    const uint32_t p[kRankMax] = {rw.x & 0xffffu, rw.x >> 16, rw.y & 0xffffu, rw.y >> 16, rw.z & 0xffffu, rw.z >> 16, rw.w & 0xffffu};
                    GEM_STAMP();                                         // 3: ranked
                    const float ce0 = ce, cs0 = cs;
#pragma unroll
                    for (int i = 0; i < kRankMax; ++i) {
                        if (__ballot((uint32_t)i < n) == 0) break;       // wave-uniform
                        const uint32_t sl = (uint32_t)i < n ? p[i] : 0u; // slot 0 is always a valid address
                        frame_chain_step<LOWEST>(ce, cs, lw, __uint_as_float(stage[sl].x), __uint_as_float(stage[sl].y), (uint32_t)i < n, a.mahal, a.var_floor);
                    }
                    GEM_STAMP();                                         // 4: cells arrived, chains done
                    if (cs < a.var_floor) cs = a.var_floor;
                    if (owner) {
                        if (__float_as_uint(ce) != __float_as_uint(ce0)) a.elevation[g] = ce;
                        if (__float_as_uint(cs) != __float_as_uint(cs0)) a.variance[g] = cs;
                        if constexpr (LOWEST) a.lowest[gl] = lw;         // (the general path rewrites the untouched cells with what it read)
                    }
                    if (lane == 0) a.bcount[tile] = 0u;                  // consumed (behind the barrier: every wave has its copy of the count)
                    GEM_STAMP();                                         // 5: stores issued
                    GEM_STAMP_END();
                }
            }
            if (!over) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); return; }    // (no LDS DMA outlives the workgroup)
            // a cell of more than kRankMax records: all four waves go on into the general path, which ranks, overflows and reports
            dbg_k = 1;
        }
    }

    const int c = tid;
    const int row = row_base + (c >> TS), col = col_base + (c & (TE - 1));
    const bool owned = row < a.row1 && row >= a.row0 && col < L;
    float ce, cs, lw = 0.0f;
    {   // unconditional loads (clamped address): cells outside the map or the strip read cell 0 and are never written back
        const size_t g = owned ? (size_t)row * L + col : 0;
        ce = a.elevation[g]; cs = a.variance[g];
        if constexpr (LOWEST) {
            // map_lowest is indexed by the GEOGRAPHIC cell (GPU:430 PointsToIndex), not by the circular-buffer cell
            int gr = row - a.start0, gc = col - a.start1;
            gr += gr < 0 ? L : 0; gc += gc < 0 ? L : 0;
            lw = a.lowest[owned ? (size_t)gr * L + gc : 0];
        }
    }
    const float ce0 = ce, cs0 = cs;                                      // as loaded: only cells that changed are written back
    reinterpret_cast<uint4*>(rowp)[tid] = make_uint4(0, 0, 0, 0);        // rank rows start with count 0
    if (tid == 0) misc[0] = 0u;
    GEM_STAMP();                                                         // 1: loads issued
    if (nrec == 0 && !a.dense) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); return; }    // (no LDS DMA outlives the workgroup)
    const bool fits = nrec <= (uint32_t)PB;
    if (fits && nrec > (uint32_t)kFrameSpec)                             // block-uniform: the rest of a heavy tile (a second round trip)
        for (uint32_t k0 = (uint32_t)kFrameSpec + (uint32_t)w * 64u; k0 < nrec; k0 += NW * 64u) dma(k0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    GEM_STAMP();                                                         // 2: records and tile arrived
    // consumed: the count is zero again for the pass after next (behind the barrier: every wave has its copy of the count)
    if (tid == 0 && nrec != 0) a.bcount[tile] = 0u;

    // queued Mapvar_update increments (GPU:540-547), before the first record
    if constexpr (LEAN) {                                                // (static indices: the four words stay scalar registers)
#pragma unroll
        for (int k = 0; k < kMaxPending; ++k) if (k < a.n_pending && cs != kInitVariance) cs += a.pending[k];
    } else {
        for (int k = 0; k < a.n_pending; ++k) if (cs != kInitVariance) cs += a.pending[k];
    }

    bool slow = !fits;
    if (fits) {
        // ---- ranks: PB / NT slots per thread, all cell reads, then all rank atomics, then all row writes in flight together
        constexpr int RK = PB / NT;
        auto ranks = [&](auto rounds) {
            constexpr int R = decltype(rounds)::value;
            uint32_t rcell[R], rold[R];
#pragma unroll
            for (int r = 0; r < R; ++r) { const uint32_t k = (uint32_t)(tid + r * NT); rcell[r] = k < nrec ? (stage[k].z & 0xffu) : 0u; }
#pragma unroll
            for (int r = 0; r < R; ++r) { const uint32_t k = (uint32_t)(tid + r * NT); rold[r] = 0; if (k < nrec) rold[r] = atomicAdd(reinterpret_cast<uint32_t*>(rowp) + rcell[r] * 4 + 3, 0x10000u); }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint32_t k = (uint32_t)(tid + r * NT);
                if (k < nrec) { const uint32_t rk = rold[r] >> 16; if (rk < (uint32_t)kRankMax) rowp[rcell[r] * 8 + rk] = (uint16_t)k; else misc[0] = 1u; }
            }
        };
        if (kFrameRankOne && nrec <= (uint32_t)NT) ranks(std::integral_constant<int, 1>{});     // block-uniform: one slot per thread (about 1240 of a C2 sweep's 1330 live tiles)
        else ranks(std::integral_constant<int, RK>{});
        __syncthreads();
        GEM_STAMP();                                                     // 3: ranked
        slow = misc[0] != 0;                                             // block-uniform
    }
    if (!slow) {
        // ---- owner: sort <= 7 keys (point index << 10 | slot), run the chain from registers.  Sized by the WAVE's largest count
        //      (ballots: wave-uniform branches): most waves of a LiDAR sweep hold at most two records per cell (gem_frame_sort.hpp)
        const uint4 rw = *reinterpret_cast<const uint4*>(rowp + tid * 8);
        const uint32_t n = rw.w >> 16;
        const uint32_t p[kRankMax] = {rw.x & 0xffffu, rw.x >> 16, rw.y & 0xffffu, rw.y >> 16, rw.z & 0xffffu, rw.z >> 16, rw.w & 0xffffu};
        auto chain = [&](float h, float v, bool live) { frame_chain_step<LOWEST>(ce, cs, lw, h, v, live, a.mahal, a.var_floor); };
        // N keys for a wave whose largest count is in [NMIN, min(N, kRankMax)]: entries at or beyond a lane's n stay ~0 and sort
        // behind its live keys, all of which are among the first N -- the order the full network gives
        auto owner = [&](auto size, auto least) {
            constexpr int N = decltype(size)::value, NMIN = decltype(least)::value, M = N < kRankMax ? N : kRankMax;
            uint32_t k[N];                                               // ~0 = no record
#pragma unroll
            for (int i = 0; i < N; ++i) k[i] = 0xffffffffu;
#pragma unroll
            for (int i = 0; i < M; ++i) {
                if (i >= NMIN && __ballot((uint32_t)i < n) == 0) break;  // wave-uniform
                const uint32_t sl = (uint32_t)i < n ? p[i] : 0u;         // slot 0 is always a valid address
                if ((uint32_t)i < n) k[i] = ((stage[sl].z >> 8) << 10) | sl;
            }
            frame_sort_keys<N>(k);
            float hh[M], vv[M];
#pragma unroll
            for (int i = 0; i < M; ++i) {
                if (i >= NMIN && __ballot((uint32_t)i < n) == 0) break;  // wave-uniform
                const uint32_t sl = (uint32_t)i < n ? (k[i] & 1023u) : 0u;
                hh[i] = __uint_as_float(stage[sl].x); vv[i] = __uint_as_float(stage[sl].y);
            }
#pragma unroll
            for (int i = 0; i < M; ++i) {
                if (i >= NMIN && __ballot((uint32_t)i < n) == 0) break;  // wave-uniform
                chain(hh[i], vv[i], (uint32_t)i < n);
            }
        };
        static_assert(frame_sort_size(2) == 2 && frame_sort_size(3) == 4 && frame_sort_size(4) == 4 && frame_sort_size(5) == 8, "the classes below");
        if (!kFrameSizedSort) {
            owner(std::integral_constant<int, 8>{}, std::integral_constant<int, 0>{});
        } else if (__ballot(n > 0u) == 0) {
            // no record in this wave's 64 cells: nothing to do (the queued increments are in cs already)
        } else if (__ballot(n > 1u) == 0) {                              // largest count 1: the record is the row's first entry, no key
            const uint32_t sl = n != 0u ? p[0] : 0u;
            chain(__uint_as_float(stage[sl].x), __uint_as_float(stage[sl].y), n != 0u);
        } else if (__ballot(n > 2u) == 0) {
            owner(std::integral_constant<int, 2>{}, std::integral_constant<int, 2>{});
        } else if (__ballot(n > 4u) == 0) {
            owner(std::integral_constant<int, 4>{}, std::integral_constant<int, 3>{});
        } else {
            owner(std::integral_constant<int, 8>{}, std::integral_constant<int, 5>{});
        }
    } else {
        // ---- slow path: windows [lo, lo + PB) of point indices, in order.  It re-reads the tile's records per window (and the
        //      whole spill arena when the bucket overflowed): the pass buffer set is switched to the descriptor form for good
        //      (frame_form), so a stream pays this once per buffer set
        if (tid == 0) {
            a.ctl[0] = 1u;
            // ... and the host is told (a word of pinned memory it reads before every launch: it stops picking k_frame's lean form)
            if (a.form_seen) __hip_atomic_store(a.form_seen, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        const uint32_t nb = min(nrec, (uint32_t)kFrameBucket);
        const uint32_t nspill = fits ? 0u : frame_spill_slots(a);
        const uint64_t lt = lanemask_lt();
        uint32_t lo = 0;
        for (;;) {                                                       // block-uniform
            const uint32_t hi = lo + (uint32_t)PB;
            reinterpret_cast<uint4*>(head)[tid] = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);   // head + tail: 4 KB
            for (int k = tid; k < PB; k += NT) scell[k] = (uint16_t)NIL;
            if (tid == 0) misc[1] = 0xffffffffu;
            __syncthreads();
            uint32_t next = 0xffffffffu;
            auto take = [&](uint32_t x, uint32_t y, uint32_t z) -> bool {
                const uint32_t idx = z >> 8;
                if (idx >= lo && idx < hi) { stage[idx - lo] = make_uint4(x, y, z, 0u); scell[idx - lo] = (uint16_t)(z & 0xffu); return true; }
                if (idx >= hi) next = min(next, idx);
                return false;
            };
            for (uint32_t k = (uint32_t)tid; k < nb; k += NT) (void)take(bkt[k * 3], bkt[k * 3 + 1], bkt[k * 3 + 2]);
            for (uint32_t j = (uint32_t)tid; j < nspill; j += NT) {
                const uint4 r = a.spill[j];
                if (r.w == (uint32_t)tile && take(r.x, r.y, r.z)) a.spill[j].w = kSpillFree;   // taken: the slot is free for the pass after next
            }
            if (next != 0xffffffffu) atomicMin(&misc[1], next);
            __syncthreads();
            {   // wave w appends slots [w PB / NW, (w + 1) PB / NW) to its own list of each cell, 64 consecutive slots per step
                constexpr uint32_t per = PB / NW;
                for (uint32_t kc = (uint32_t)w * per; kc < (uint32_t)(w + 1) * per; kc += 64) {
                    const uint32_t sl = kc + (uint32_t)lane;
                    const uint32_t cell = scell[sl];
                    const bool on = cell != NIL;
                    const uint64_t peers = wave_peers(on, cell, 2 * TS);
                    const uint64_t above = lane == 63 ? 0ull : (peers & (~0ull << (lane + 1)));
                    if (on) {
                        nxt[sl] = above ? (uint16_t)(sl + (uint32_t)(__ffsll((unsigned long long)above) - 1 - lane)) : (uint16_t)NIL;
                        const uint32_t hx = cell * NW + (uint32_t)w;
                        if ((peers & lt) == 0) {                         // first of its group: link behind the wave's list of this cell
                            if (head[hx] == NIL) head[hx] = (uint16_t)sl;
                            else nxt[tail[hx]] = (uint16_t)sl;
                        }
                        if (above == 0) tail[hx] = (uint16_t)sl;
                    }
                }
            }
            __syncthreads();
            {   // walk list(wave 0), list(wave 1), ... of this thread's cell
                const uint2 hv = *reinterpret_cast<const uint2*>(head + c * NW);
                const uint32_t hd[NW] = {hv.x & 0xffffu, hv.x >> 16, hv.y & 0xffffu, hv.y >> 16};
                uint32_t ww = 0, cur = NIL;
#pragma unroll
                for (int x = NW - 1; x >= 0; --x) if (hd[x] != NIL) { cur = hd[x]; ww = (uint32_t)x; }
                while (__ballot(cur != NIL) != 0) {                      // wave-uniform
                    const bool live = cur != NIL;
                    const uint32_t sl = live ? cur : 0u;
                    const float h = __uint_as_float(stage[sl].x), v = __uint_as_float(stage[sl].y);
                    uint32_t nx = nxt[sl];
                    if (live && nx == NIL) {                             // end of this wave's list: the next non-empty one
                        uint32_t nw_ = NW;
#pragma unroll
                        for (int x = NW - 1; x >= 0; --x) if ((uint32_t)x > ww && hd[x] != NIL) { nx = hd[x]; nw_ = (uint32_t)x; }
                        ww = nw_;
                    }
                    float e2 = ce, s2 = cs;
                    (void)fuse_step(e2, s2, h, v, a.mahal, a.var_floor);
                    const bool fl = live && (!LOWEST || h != -1.0f);     // GPU:482
                    ce = fl ? e2 : ce; cs = fl ? s2 : cs;
                    if constexpr (LOWEST) { const float l2 = lowest_step(lw, h, v); lw = live ? l2 : lw; }
                    cur = live ? nx : NIL;
                }
            }
            const uint32_t nlo = misc[1];
            __syncthreads();                                             // every thread has read misc[1] and left the lists
            if (nlo == 0xffffffffu) break;
            lo = nlo;
        }
    }
    GEM_STAMP();                                                         // 4: chains done

    // ---- variance floor at the end of every Fuse (GPU:533-534), then the single write-back of the tile
    if (cs < a.var_floor) cs = a.var_floor;
    if (owned) {
        // (recomputed here: the address of the tile's read, kept alive across the body, costs registers of the 80-VGPR budget)
        int cc = tid;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(cc));
#endif
        const size_t g = (size_t)(row_base + (cc >> TS)) * L + col_base + (cc & (TE - 1));
        if (__float_as_uint(ce) != __float_as_uint(ce0)) a.elevation[g] = ce;
        if (__float_as_uint(cs) != __float_as_uint(cs0)) a.variance[g] = cs;
        if constexpr (LOWEST) {
            int gr = row_base + (cc >> TS) - a.start0, gc = col_base + (cc & (TE - 1)) - a.start1;
            gr += gr < 0 ? L : 0; gc += gc < 0 ? L : 0;
            a.lowest[(size_t)gr * L + gc] = lw;
        }
    }
    GEM_STAMP();                                                         // 5: stores issued
    GEM_STAMP_END();
#undef GEM_STAMP_END
#undef GEM_STAMP
}

} // namespace gem
