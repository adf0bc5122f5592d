// gem_navquad.hpp -- the quadratic potential of include/gem_hip_navquad.h (internal header): THE cell update, written once for the
// host compiler and the device -- the per-byte table word, the exact quotient without a divide, the increment and T(n) -- then the
// host twin's relaxation (plain C++, no device) and the round launcher of gem_navquad.hip.  Compiles without HIP too: the quotient is
// checked exhaustively on its own (tests/cpp/navquad_check.cpp).  Integer results only; the one float is an estimate that a remainder
// test corrects.
#pragma once

#include "gem_navpath.hpp"

#include <cstdint>
#include <cstring>
#include <queue>
#include <utility>
#include <vector>

namespace gem {

constexpr int kNavQuadMaxWeight = 462;                              // 10046 * 462^2 < 2^31: the numerator fits 31 bits
constexpr int kNavQuadPasses = 3;                                   // in-tile passes a round allows a tile (DESIGN 7w has the measurement)
constexpr int kNavQuadHfBits = 9;                                  // 462 < 2^9
constexpr unsigned kNavQuadHfMask = (1u << kNavQuadHfBits) - 1u;
static_assert(kNavQuadMaxWeight <= (int)kNavQuadHfMask, "a weight fits the table word's low bits");
static_assert(10046ll * kNavQuadMaxWeight * kNavQuadMaxWeight < (1ll << 31), "the numerator needs no 64-bit arithmetic");

GEM_NAV_HD float navquad_as_float(unsigned u) { float f; memcpy(&f, &u, sizeof f); return f; }
GEM_NAV_HD unsigned navquad_as_bits(float f) { unsigned u; memcpy(&u, &f, sizeof u); return u; }
// a * b for operands below 2^24: the full-rate 24-bit multiplier on the device
GEM_NAV_HD unsigned navquad_mul24(unsigned a, unsigned b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return a * b;
#endif
}

// The table word of a weight hf in 1 .. 462: the float 1 / (10000 * hf) with its nine lowest mantissa bits replaced by hf itself; 0 for
// an impassable byte.  ONE word a cell gives the update the weight and a reciprocal good to 2^-14, and the remainder test below
// makes the quotient exact whatever those bits hold.
GEM_NAV_HD unsigned navquad_word(int hf)
{
    if (hf <= 0) return 0u;
    const float rcp = 1.0f / (float)(10000 * hf);
    return (navquad_as_bits(rcp) & ~kNavQuadHfMask) | (unsigned)hf;
}

// floor((-2301 dc^2 + 5307 dc hf + 7040 hf^2) / (10000 hf)) for 0 <= dc < hf <= 462, `word` = navquad_word(hf): a float estimate
// (the numerator is below 2^31, the quotient at most hf, so the estimate's error is far below 1) and one correction step either way
// against the remainder.  No divide.
GEM_NAV_HD int navquad_quot(unsigned word, unsigned dc)
{
    const unsigned hf = word & kNavQuadHfMask;
    const unsigned slope = navquad_mul24(hf, 5307u) - navquad_mul24(dc, 2301u);       // dc < hf: positive, below 2^22
    const unsigned num = navquad_mul24(navquad_mul24(hf, hf), 7040u) + navquad_mul24(dc, slope);
    const unsigned den = navquad_mul24(hf, 10000u);
    int q = (int)((float)num * navquad_as_float(word));
    const int rem = (int)(num - navquad_mul24((unsigned)q, den));       // the difference in 32 bits, then signed: |rem| < 2 * den < 2^24
    q += rem < 0 ? -1 : (rem >= (int)den ? 1 : 0);
    return q;
}

// inc(hf, dc) of the contract: hf at dc >= hf, else the quotient clamped into 1 .. hf
GEM_NAV_HD int navquad_inc(unsigned word, unsigned dc)
{
    const int hf = (int)(word & kNavQuadHfMask);
    if (dc >= (unsigned)hf) return hf;
    const int q = navquad_quot(word, dc);
    return q < 1 ? 1 : (q > hf ? hf : q);
}

// T(n): the four neighbours' potentials (UNREACHED for one off the map, impassable or unreached) and the cell's table word; UNREACHED
// for an impassable cell or one without a reached neighbour.  Only lanes with dc < hf take the quotient's path.
GEM_NAV_HD int navquad_update(unsigned word, int left, int right, int up, int down)
{
    const int h = left < right ? left : right, v = up < down ? up : down;
    const int ta = h < v ? h : v, tc = h < v ? v : h;
    const int hf = (int)(word & kNavQuadHfMask);
    if (hf == 0 || ta == kNavUnreached) return kNavUnreached;
    const unsigned gap = (unsigned)(tc - ta);                           // tc >= ta >= 0
    const unsigned dc = tc == kNavUnreached || gap > (unsigned)hf ? (unsigned)hf : gap;
    return ta + navquad_inc(word, dc);                                  // <= ta + hf: at or below the linear potential, no overflow
}

// The host twin's potential: chaotic relaxation in an order unlike the kernel's -- a binary heap keyed by potential; a cell that was
// lowered is pushed (again), a popped cell re-evaluates its four neighbours, an entry that a smaller one overtook is dropped.  Values
// only fall from UNREACHED, and when the heap is empty every cell has been evaluated since its neighbours last changed: a fixed point,
// and by monotonicity the greatest (include/gem_hip_navquad.h).  `w` has 256 weights in 0 .. 462.
inline void navquad_potential_host(const unsigned char* grid, int sx, int sy, const int* w, bool outline, int start, int* pot)
{
    const long long cells = (long long)sx * sy;
    for (long long i = 0; i < cells; ++i) pot[i] = kNavUnreached;
    if (start < 0) return;
    unsigned tab[256];
    for (int c = 0; c < 256; ++c) tab[c] = navquad_word(w[c]);
    auto word = [&](int x, int y) -> unsigned {
        if (outline && (x == 0 || y == 0 || x == sx - 1 || y == sy - 1)) return 0u;
        return tab[grid[(size_t)y * sx + x]];
    };
    auto at = [&](int x, int y) { return x >= 0 && y >= 0 && x < sx && y < sy ? pot[(size_t)y * sx + x] : kNavUnreached; };
    using Item = std::pair<int, int>;                                   // potential, cell
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    pot[start] = 0;
    heap.push({0, start});
    const int dx[4] = {-1, 1, 0, 0}, dy[4] = {0, 0, -1, 1};
    while (!heap.empty()) {
        const Item it = heap.top();
        heap.pop();
        if (it.first != pot[it.second]) continue;
        const int cx = it.second % sx, cy = it.second / sx;
        for (int k = 0; k < 4; ++k) {
            const int x = cx + dx[k], y = cy + dy[k];
            if (x < 0 || y < 0 || x >= sx || y >= sy) continue;
            const int n = y * sx + x;
            if (n == start) continue;                                   // the source stays 0
            const int t = navquad_update(word(x, y), at(x - 1, y), at(x + 1, y), at(x, y - 1), at(x, y + 1));
            if (t < pot[n]) { pot[n] = t; heap.push({t, n}); }
        }
    }
}

#if defined(__HIPCC__)
struct NavArgs;
hipError_t launch_navquad_round(hipStream_t st, const NavArgs& a);
#endif

} // namespace gem
