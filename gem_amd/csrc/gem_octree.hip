// gem_octree.hip -- octomap::ColorOcTree insertion (updateNode + integrateNodeColor per record, updateInnerOccupancy) and the
// fullMapToMsg byte stream on the device, gfx950.  The contract is in include/gem_hip.h (gem_octree_build); the launch structure in
// gem_octree.hpp; tests/octree_ref.py states the same twice (build_literal, and build_array which is this file in Python).
//
// What makes it parallel.  (1) A leaf's value is a function of its number of hits alone (prune and expand copy values), so the
// kernels carry the saturating count and look value and blend factor up in two host-built tables.  (2) A node k levels above the
// leaves can collapse only while all 8^k leaves under it exist, so the prune / expand history of a leaf -- which its colour does
// depend on -- is confined to its largest aligned block of leaves that are all hit (k*).  The records are sorted stably by Morton
// key, and every such block replays its own records in input order: the same colours as the sequential loop.
//
// Colours are kept as r | g << 8 | b << 16 (0xffffff: not set), the three bytes as the stream has them; a stream node is a uint2:
// the value's bits, colour | child mask << 24.
#include "gem_octree.hpp"

#include <algorithm>

namespace gem {

namespace {

using u64 = unsigned long long;
constexpr u64 kNoKey = ~0ull;

__device__ __forceinline__ u64 spread3(uint32_t v)              // bit i of a 16-bit value to bit 3 i
{
    u64 x = v;
    x = (x | x << 16) & 0x0000ff0000ffull;
    x = (x | x << 8) & 0x00f00f00f00full;
    x = (x | x << 4) & 0x0c30c30c30c3ull;
    x = (x | x << 2) & 0x249249249249ull;
    return x;
}

// k = (int)floor(rf * (double)coord) + 32768, valid iff 0 <= k < 65536; a non-finite coordinate has none
__device__ __forceinline__ bool axis_key(float coord, double rf, uint32_t& k)
{
    const double f = floor(rf * (double)coord);
    const bool ok = __builtin_isfinite(coord) && f >= -32768.0 && f < 32768.0;
    k = ok ? (uint32_t)((int)f + 32768) : 0u;
    return ok;
}

__device__ __forceinline__ uint32_t rgb_of(uint32_t bgra)        // PCL's b g r a bytes -> r | g << 8 | b << 16
{
    return ((bgra >> 16) & 255u) | (bgra & 0xff00u) | ((bgra & 255u) << 16);
}

// integrateNodeColor on a node whose value belongs to p: each channel (uint8_t)((double)prev * p + (double)c * (0.99 - p))
__device__ __forceinline__ uint32_t oct_blend(uint32_t col, uint32_t rgb, double p)
{
    if (col == kOctWhite) return rgb;
    const double q = 0.99 - p;
    uint32_t out = 0u;
#pragma unroll
    for (int s = 0; s < 24; s += 8) {
        const double v = (double)((col >> s) & 255u) * p + (double)((rgb >> s) & 255u) * q;
        out |= ((uint32_t)(int)v & 255u) << s;
    }
    return out;
}

// getAverageChildColor from sums packed r | g << 16 | b << 32 | count << 48 (count >= 1)
__device__ __forceinline__ u64 pack_sum(bool set, uint32_t col)
{
    return set ? ((u64)(col & 255u) | (u64)((col >> 8) & 255u) << 16 | (u64)((col >> 16) & 255u) << 32 | 1ull << 48) : 0ull;
}
__device__ __forceinline__ uint32_t mean_of(u64 acc)
{
    const uint32_t c = (uint32_t)(acc >> 48);
    return ((uint32_t)(acc & 0xffffu) / c) | (((uint32_t)(acc >> 16) & 0xffffu) / c) << 8 | (((uint32_t)(acc >> 32) & 0xffffu) / c) << 16;
}

__device__ __forceinline__ const u64* sorted_key(const OctArgs& a) { return a.key[(a.st->npass - 1u) & 1u]; }
__device__ __forceinline__ const uint32_t* sorted_src(const OctArgs& a) { return a.src[(a.st->npass - 1u) & 1u]; }

// v summed over the workgroup into heads[blockIdx.x]; in the last workgroup to arrive heads becomes its exclusive prefix and the
// total is returned through *total (true there only)
__device__ __forceinline__ bool sum_then_scan(uint32_t v, uint32_t* heads, uint32_t* ticket, uint32_t* total)
{
    __shared__ uint32_t s_scan[16];
    __shared__ uint32_t s_last;
    uint32_t tot;
    block_exclusive_scan<kOctThreads>(v, s_scan, &tot);
    if (threadIdx.x == 0) heads[blockIdx.x] = tot;
    const int nb = (int)gridDim.x;
    if (!last_arrival(ticket, nb, &s_last)) return false;
    uint32_t carry = 0u;
    for (int b0 = 0; b0 < nb; b0 += kOctThreads) {        // workgroup-uniform trip count
        const int i = b0 + (int)threadIdx.x;
        const uint32_t x = i < nb ? heads[i] : 0u;
        uint32_t t;
        const uint32_t ex = block_exclusive_scan<kOctThreads>(x, s_scan, &t);
        if (i < nb) heads[i] = carry + ex;
        carry += t;
    }
    *total = carry;
    return true;
}

} // namespace

// ---- keys, validity, varying bits, histogram of digit 0 -----------------------------------------------------------------------
__global__ __launch_bounds__(kLsdThreads) void k_oct_keys(OctArgs a)
{
    __shared__ uint32_t s_h[kLsdBins];
    __shared__ uint32_t s_scan[16];
    __shared__ uint32_t s_last;
    for (int d = threadIdx.x; d < kLsdBins; d += kLsdThreads) s_h[d] = 0u;
    __syncthreads();
    u64 o = 0ull, n_and = kNoKey;
    uint32_t cnt = 0u;
#pragma unroll
    for (int k = 0; k < kLsdItems; ++k) {
        const long long i = lsd_pos(k);
        if (i < a.n) {
            const float4 p = *reinterpret_cast<const float4*>(a.in + i);
            uint32_t kx, ky, kz;
            const bool okx = axis_key(p.x, a.rf, kx), oky = axis_key(p.y, a.rf, ky), okz = axis_key(p.z, a.rf, kz);
            u64 key = kNoKey;
            if (okx && oky && okz) {
                key = spread3(kx) | spread3(ky) << 1 | spread3(kz) << 2;
                o |= key; n_and &= key; ++cnt;
                atomicAdd(&s_h[(uint32_t)key & (kLsdBins - 1)], 1u);
            }
            a.key_in[i] = key;
        }
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        o |= __shfl_xor(o, s); n_and &= __shfl_xor(n_and, s); cnt += __shfl_xor(cnt, s);
    }
    if (lane_id() == 0 && cnt) {
        atomicOr(&a.st->acc_or, o); atomicAnd(&a.st->acc_and, n_and); atomicAdd(&a.st->acc_valid, cnt);
    }
    __syncthreads();
    reinterpret_cast<uint4*>(a.hist[0])[(size_t)blockIdx.x * (kLsdBins / 4) + threadIdx.x] = reinterpret_cast<const uint4*>(s_h)[threadIdx.x];
    if (!last_arrival(&a.st->ticket[0], a.nb, &s_last)) return;
    if (threadIdx.x == 0) {
        OctState* st = a.st;
        const u64 vo = __hip_atomic_load(&st->acc_or, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const u64 va = __hip_atomic_load(&st->acc_and, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t S = __hip_atomic_load(&st->acc_valid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&st->acc_or, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&st->acc_and, kNoKey, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&st->acc_valid, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const u64 vary = S ? (vo & ~va) : 0ull;                       // the bits above the highest varying one are the same in every key
        const int bits = vary ? 64 - __clzll((long long)vary) : 0;
        const int np = (bits + kLsdDigit - 1) / kLsdDigit;
        st->npass = (uint32_t)(np < 1 ? 1 : (np > kOctMaxPasses ? kOctMaxPasses : np));
        st->S = S;
        st->nleaves = 0u; st->nblk[0] = st->nblk[1] = st->nblk[2] = 0u; st->fb_leaves = 0u; st->fb_points = 0u;
        st->nnodes = 0u; st->n_leaf_nodes = 0u; st->n_pruned = 0u;
    }
    lsd_scan_hist(a.hist[0], a.nb, s_scan);
}

// ---- the stable LSD passes the varying bits need --------------------------------------------------------------------------------
template <int PASS>
__global__ __launch_bounds__(kLsdThreads) void k_oct_scatter(OctArgs a)
{
    const uint32_t np = a.st->npass;
    if ((uint32_t)PASS >= np) return;                                   // (uniform over the grid)
    const uint32_t S = a.st->S;
    auto load = [&](long long j, u64& key, uint32_t& src) -> bool {
        if constexpr (PASS == 0) {
            src = (uint32_t)j;
            key = j < a.n ? a.key_in[j] : kNoKey;
            return key != kNoKey;
        } else {
            const bool valid = j < (long long)S;
            key = valid ? a.key[(PASS - 1) & 1][j] : 0ull;
            src = valid ? a.src[(PASS - 1) & 1][j] : 0u;
            return valid;
        }
    };
    lsd_scatter_pass<u64, (PASS + 1 < kOctMaxPasses)>(kLsdDigit * PASS, (uint32_t)PASS + 1u < np, load, a.key[PASS & 1], a.src[PASS & 1], a.hist[PASS & 1],
                          a.hist[(PASS + 1) & 1], &a.st->ticket[1 + PASS], a.nb);
}

// ---- leaves ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kOctThreads) void k_oct_heads(OctArgs a)
{
    const uint32_t S = a.st->S;
    const u64* key = sorted_key(a);
    const uint32_t j = blockIdx.x * (uint32_t)kOctThreads + threadIdx.x;
    const bool head = j < S && (j == 0u || key[j - 1] != key[j]);
    uint32_t total;
    if (!sum_then_scan(head ? 1u : 0u, a.heads, &a.st->ticket[6], &total)) return;
    if (threadIdx.x == 0) { a.st->nleaves = total; a.leaf_start[total] = S; }
}

__global__ __launch_bounds__(kOctThreads) void k_oct_leaves(OctArgs a)
{
    __shared__ uint32_t s_scan[16];
    const uint32_t S = a.st->S;
    const u64* key = sorted_key(a);
    const uint32_t j = blockIdx.x * (uint32_t)kOctThreads + threadIdx.x;
    const bool head = j < S && (j == 0u || key[j - 1] != key[j]);
    uint32_t tot;
    const uint32_t li = a.heads[blockIdx.x] + block_exclusive_scan<kOctThreads>(head ? 1u : 0u, s_scan, &tot);
    if (head) { a.leaf_key[li] = key[j]; a.leaf_start[li] = j; }
}

// ---- k*, the block lists, the k* = 0 walk ---------------------------------------------------------------------------------------
// The leaf keys are sorted and distinct, so the aligned block of 8^k leaves around leaf i is all there iff the leaf (key - base)
// places in front of i is the block's first key and the one 8^k - 1 places behind that is its last.
__global__ __launch_bounds__(kOctThreads) void k_oct_kstar(OctArgs a)
{
    const uint32_t nl = a.st->nleaves;
    const uint32_t i = blockIdx.x * (uint32_t)kOctThreads + threadIdx.x;
    if (i >= nl) return;
    const u64 key = a.leaf_key[i];
    int ks = 0;
#pragma unroll
    for (int k = 1; k <= 3; ++k) {
        const u64 sz = 1ull << (3 * k);
        const u64 base = key & ~(sz - 1ull);
        const u64 back = key - base;
        if (ks != k - 1 || back > (u64)i) break;
        const u64 j = (u64)i - back;
        if (j + sz - 1ull < (u64)nl && a.leaf_key[j] == base && a.leaf_key[j + sz - 1ull] == base + sz - 1ull) ks = k;
    }
    a.kstar[i] = (uint8_t)ks;
    const uint32_t s = a.leaf_start[i], e = a.leaf_start[i + 1];
    if (ks == 0) {                                                      // nothing around this leaf can collapse: count and colour
        const uint32_t* src = sorted_src(a);
        uint32_t cnt = 0u, col = kOctWhite;
        for (uint32_t j = s; j < e; ++j) {
            const uint32_t rgb = rgb_of(a.in[src[j]].bgra);
            cnt = min(cnt + 1u, a.sat);
            col = oct_blend(col, rgb, a.p_tab[cnt]);
        }
        a.term[i] = OctTerm{col, cnt};
    } else if (ks == 1) {
        if ((key & 7ull) == 0ull) a.blk[0][atomicAdd(&a.st->nblk[0], 1u)] = i;
    } else if (ks == 2) {
        if ((key & 63ull) == 0ull) a.blk[1][atomicAdd(&a.st->nblk[1], 1u)] = i;
    } else {                                                            // the host finishes these; a well-formed placeholder meanwhile
        a.term[i] = OctTerm{kOctWhite, 0u};
        atomicAdd(&a.st->fb_leaves, 1u);
        atomicAdd(&a.st->fb_points, e - s);
        if ((key & 511ull) == 0ull) atomicAdd(&a.st->nblk[2], 1u);
    }
}

// ---- the block walkers ----------------------------------------------------------------------------------------------------------
// A lane per leaf; the eight lanes of an octet share a level-1 node (M, kept in every lane of the octet), the wave a level-2 node
// (T, in every lane).  <false>: eight k* = 1 blocks per wave, each octet merges its own eight segments by input position and T is
// not there (the block's level-2 parent lacks a leaf and never collapses).  <true>: one k* = 2 block per wave, one record per step.
// Every shuffle and ballot is executed by the whole wave; what a step changes is predicated.
template <bool WAVE>
__global__ __launch_bounds__(64) void k_oct_walk(OctArgs a)
{
    const uint32_t nblk = a.st->nblk[WAVE ? 1 : 0];
    const uint32_t* list = a.blk[WAVE ? 1 : 0];
    const uint32_t* src = sorted_src(a);
    const int lane = (int)threadIdx.x, o = lane >> 3, q = lane & 7, first = lane & ~7;
    const uint32_t items = WAVE ? nblk : (nblk + 7u) / 8u;
    const uint32_t sat = a.sat;
    for (uint32_t it = blockIdx.x; it < items; it += gridDim.x) {
        const uint32_t bi = WAVE ? it : it * 8u + (uint32_t)o;
        const bool have = bi < nblk;
        const uint32_t li = have ? list[bi] + (uint32_t)(WAVE ? lane : q) : 0u;
        uint32_t cur = have ? a.leaf_start[li] : 0u;
        const uint32_t end = have ? a.leaf_start[li + 1] : 0u;
        uint32_t hp = cur < end ? src[cur] : ~0u;                        // input position of the segment's head
        bool Lex = false, Mex = false, Mch = false, Tex = false, Tch = false;
        uint32_t Lcnt = 0u, Lcol = kOctWhite, Mcnt = 0u, Mcol = kOctWhite, Tcnt = 0u, Tcol = kOctWhite;
        for (;;) {
            uint32_t m = hp;
            m = min(m, (uint32_t)__shfl_xor((int)m, 1)); m = min(m, (uint32_t)__shfl_xor((int)m, 2)); m = min(m, (uint32_t)__shfl_xor((int)m, 4));
            if (WAVE) { m = min(m, (uint32_t)__shfl_xor((int)m, 8)); m = min(m, (uint32_t)__shfl_xor((int)m, 16)); m = min(m, (uint32_t)__shfl_xor((int)m, 32)); }
            if (__ballot(m != ~0u) == 0ull) break;
            const bool act = m != ~0u;                                   // this lane's group has a record this step
            const uint64_t ob = __ballot(act && hp == m);
            int ol = lane;                                               // the lane whose segment the record heads
            if (act) ol = WAVE ? __ffsll((unsigned long long)ob) - 1 : first + __ffs((int)((ob >> first) & 0xffull)) - 1;
            const bool in_oct = act && (ol >> 3) == o;
            const bool owner = act && ol == lane;
            const uint32_t rgb = act ? rgb_of(a.in[m].bgra) : 0u;
            // search(key): T pruned, else the octet's M pruned, else the leaf
            const bool oLex = (__ballot(Lex) >> ol) & 1ull;
            const uint32_t oLcnt = (uint32_t)__shfl((int)Lcnt, ol);
            const bool aMex = (__ballot(Mex) >> ol) & 1ull, aMch = (__ballot(Mch) >> ol) & 1ull;
            const uint32_t aMcnt = (uint32_t)__shfl((int)Mcnt, ol);
            bool found = false;
            uint32_t scnt = 0u;
            if (WAVE && Tex && !Tch) { found = true; scnt = Tcnt; }
            else if (aMex && !aMch) { found = true; scnt = aMcnt; }
            else if (aMex && oLex) { found = true; scnt = oLcnt; }
            const bool upd = act && !(found && scnt >= sat);             // updateNode's early return
            // updateNodeRecurs, downwards
            bool freshT = false, freshM = false;
            if (WAVE && upd && !Tex) { Tex = true; Tch = false; Tcnt = 0u; Tcol = kOctWhite; freshT = true; }
            if (upd && !aMex) {
                if (WAVE && !Tch && !freshT) { Mex = true; Mch = false; Mcnt = Tcnt; Mcol = Tcol; }          // expand T: every octet
                else { freshM = true; if (in_oct) { Mex = true; Mch = false; Mcnt = 0u; Mcol = kOctWhite; } }
            }
            if (WAVE && upd) Tch = true;
            if (upd && in_oct) {
                if (!oLex) {
                    if (!Mch && !freshM) { Lex = true; Lcnt = Mcnt; Lcol = Mcol; }                           // expand M: every lane of the octet
                    else if (owner) { Lex = true; Lcnt = 0u; Lcol = kOctWhite; }
                }
                Mch = true;
                if (owner) Lcnt = min(Lcnt + 1u, sat);
            }
            // ... and back up: pruneNode at M, then at T
            const uint32_t c0 = (uint32_t)__shfl((int)Lcnt, first), col0 = (uint32_t)__shfl((int)Lcol, first);
            const uint64_t eqb = __ballot(Lex && Lcnt == c0);
            const bool pruneM = upd && in_oct && ((eqb >> first) & 0xffull) == 0xffull;
            u64 acc = pack_sum(Lex && Lcol != kOctWhite, Lcol);
            acc += __shfl_xor(acc, 1); acc += __shfl_xor(acc, 2); acc += __shfl_xor(acc, 4);
            if (pruneM) { Mcnt = c0; Mcol = col0 != kOctWhite ? mean_of(acc) : col0; Mch = false; Lex = false; }
            if (WAVE) {
                const bool any = __ballot(pruneM) != 0ull;
                const uint32_t m0c = (uint32_t)__shfl((int)Mcnt, 0), m0col = (uint32_t)__shfl((int)Mcol, 0);
                const uint64_t okb = __ballot(Mex && !Mch && Mcnt == m0c);
                u64 tacc = pack_sum(q == 0 && Mex && Mcol != kOctWhite, Mcol);
                tacc += __shfl_xor(tacc, 8); tacc += __shfl_xor(tacc, 16); tacc += __shfl_xor(tacc, 32);
                tacc = __shfl(tacc, 0);
                if (any && okb == ~0ull) { Tcnt = m0c; Tcol = m0col != kOctWhite ? mean_of(tacc) : m0col; Tch = false; Mex = false; }
            }
            // integrateNodeColor: search again
            if (act) {
                if (WAVE && Tex && !Tch) Tcol = oct_blend(Tcol, rgb, a.p_tab[Tcnt]);
                else if (in_oct) {
                    if (!Mch) Mcol = oct_blend(Mcol, rgb, a.p_tab[Mcnt]);
                    else if (owner) Lcol = oct_blend(Lcol, rgb, a.p_tab[Lcnt]);
                }
            }
            if (owner) { ++cur; hp = cur < end ? src[cur] : ~0u; }
        }
        if (have) {
            OctTerm t{kOctWhite | kOctDead << 24, 0u};
            if (WAVE && Tex && !Tch) { if (lane == 0) t = OctTerm{Tcol | 2u << 24, Tcnt}; }
            else if (Mex && !Mch) { if (q == 0) t = OctTerm{Mcol | 1u << 24, Mcnt}; }
            else t = OctTerm{Lcol, Lcnt};
            a.term[li] = t;
        }
    }
}

// ---- nodes per leaf, the stream ---------------------------------------------------------------------------------------------------
// Pre-order = the nodes ordered by (first leaf under them, depth): a terminal introduces its path from the first depth at which its
// key leaves the previous leaf's (a covered leaf in front of it shares its block's prefix, so it serves as well as the block's base).
__global__ __launch_bounds__(kOctThreads) void k_oct_count(OctArgs a)
{
    const uint32_t nl = a.st->nleaves;
    const uint32_t i = blockIdx.x * (uint32_t)kOctThreads + threadIdx.x;
    uint32_t nn = 0u, level = kOctDead;
    if (i < nl) {
        level = a.term[i].col_level >> 24;
        if (level != kOctDead) {
            int d0 = 0;
            if (i > 0u) {
                const u64 x = a.leaf_key[i] ^ a.leaf_key[i - 1];
                d0 = kOctDepth - (63 - __clzll((long long)x)) / 3;
            }
            a.d0[i] = (uint8_t)d0;
            nn = (uint32_t)(kOctDepth - (int)level - d0 + 1);
        }
        a.off[i] = nn;
    }
    const uint32_t nleaf = (uint32_t)__popcll(__ballot(level == 0u)), npr = (uint32_t)__popcll(__ballot(level != 0u && level != kOctDead));
    if (lane_id() == 0) {
        if (nleaf) atomicAdd(&a.st->n_leaf_nodes, nleaf);
        if (npr) atomicAdd(&a.st->n_pruned, npr);
    }
    uint32_t total;
    if (!sum_then_scan(nn, a.heads, &a.st->ticket[7], &total)) return;
    if (threadIdx.x == 0) a.st->nnodes = total;
}

__global__ __launch_bounds__(kOctThreads) void k_oct_emit(OctArgs a)
{
    __shared__ uint32_t s_scan[16];
    const uint32_t nl = a.st->nleaves;
    const uint32_t i = blockIdx.x * (uint32_t)kOctThreads + threadIdx.x;
    const uint32_t nn = i < nl ? a.off[i] : 0u;
    uint32_t tot;
    const uint32_t at = a.heads[blockIdx.x] + block_exclusive_scan<kOctThreads>(nn, s_scan, &tot);
    if (i >= nl) return;
    a.off[i] = at;
    if (nn == 0u) return;
    const OctTerm t = a.term[i];
    const long long leaf_at = (long long)at + nn - 1u;                 // the terminal is the last node of its path
    if (leaf_at < a.out_cap) a.out[leaf_at] = make_uint2(__float_as_uint(a.f_tab[t.cnt]), t.col_level & 0x00ffffffu);
}

// one depth of updateInnerOccupancy: the inner nodes at depth d, each from its children at depth d + 1 (already in the stream)
__global__ __launch_bounds__(kOctThreads) void k_oct_inner(OctArgs a, int d)
{
    const uint32_t nl = a.st->nleaves;
    const uint32_t i = blockIdx.x * (uint32_t)kOctThreads + threadIdx.x;
    if (i >= nl) return;
    const uint32_t level = a.term[i].col_level >> 24;
    if (level == kOctDead) return;
    const int d0 = (int)a.d0[i];
    if (d < d0 || d >= kOctDepth - (int)level) return;
    const int sh = 3 * (kOctDepth - 1 - d);
    const u64 prefix = a.leaf_key[i] >> (sh + 3);
    float v = 0.0f;
    uint32_t sr = 0u, sg = 0u, sb = 0u, cs = 0u, mask = 0u;
    // the node's leaves are the (at most 8^(16 - d)) leaves from i on: nothing is searched beyond them
    const u64 span = sh + 3 < 32 ? 1ull << (sh + 3) : (u64)nl;
    const uint32_t end = (uint32_t)min((u64)nl, (u64)i + span);
    uint32_t lo_i = i;
    for (uint32_t c = 0u; c < 8u; ++c) {
        const u64 lo = ((prefix << 3) | (u64)c) << sh;
        uint32_t l = lo_i, r = end;                                     // the first leaf with key >= lo
        while (l < r) {
            const uint32_t mid = l + ((r - l) >> 1);
            if (a.leaf_key[mid] < lo) l = mid + 1u; else r = mid;
        }
        lo_i = l;
        if (l >= nl || a.leaf_key[l] >= lo + (1ull << sh)) continue;
        const long long at = (long long)a.off[l] + (d + 1 - (int)a.d0[l]);
        const uint2 node = at < a.out_cap ? a.out[at] : make_uint2(0u, kOctWhite);
        const float cv = __uint_as_float(node.x);
        v = mask ? fmaxf(v, cv) : cv;
        mask |= 1u << c;
        const uint32_t col = node.y & 0x00ffffffu;
        if (col != kOctWhite) { sr += col & 255u; sg += (col >> 8) & 255u; sb += col >> 16; ++cs; }
    }
    const uint32_t col = cs ? (sr / cs) | (sg / cs) << 8 | (sb / cs) << 16 : kOctWhite;
    const long long at = (long long)a.off[i] + (d - d0);
    if (at < a.out_cap) a.out[at] = make_uint2(__float_as_uint(v), col | mask << 24);
}

hipError_t launch_octree_front(hipStream_t st, const OctArgs& a)
{
    if (a.n <= 0 || a.nb <= 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.nb), block(kLsdThreads);
    const dim3 g1((unsigned)((a.n + kOctThreads - 1) / kOctThreads)), b1(kOctThreads);
    hipLaunchKernelGGL(k_oct_keys, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_oct_scatter<0>, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_oct_scatter<1>, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_oct_scatter<2>, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_oct_scatter<3>, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_oct_scatter<4>, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_oct_heads, g1, b1, 0, st, a);
    hipLaunchKernelGGL(k_oct_leaves, g1, b1, 0, st, a);
    hipLaunchKernelGGL(k_oct_kstar, g1, b1, 0, st, a);
    // the block counts stay on the device: n records make at most n / 64 items of either kind (eight 2^3 blocks or one 4^3 block of
    // leaves that each hold a record), the waves stride over the list, and a wave without an item reads the count and leaves
    const unsigned waves = (unsigned)std::min<long long>(kOctWalkWaves, a.n / 64 + 1);
    hipLaunchKernelGGL(k_oct_walk<false>, dim3(waves), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_oct_walk<true>, dim3(waves), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_octree_back(hipStream_t st, const OctArgs& a)
{
    if (a.n <= 0) return hipErrorInvalidValue;
    const dim3 g1((unsigned)((a.n + kOctThreads - 1) / kOctThreads)), b1(kOctThreads);
    hipLaunchKernelGGL(k_oct_count, g1, b1, 0, st, a);
    hipLaunchKernelGGL(k_oct_emit, g1, b1, 0, st, a);
    for (int d = kOctDepth - 1; d >= 0; --d) hipLaunchKernelGGL(k_oct_inner, g1, b1, 0, st, a, d);
    return hipGetLastError();
}

} // namespace gem
