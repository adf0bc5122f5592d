// gem_navpath.hpp -- GridPath::getPath of the global-plan contract (include/gem_hip_navplan.h), written once for the host compiler and
// the device: the scan order of the eight neighbours, the key whose integer minimum is "the smallest potential, strict < keeps the
// first", and the sequential walk.  The host twin (gem_navplan_host) runs nav_grid_path as it stands; k_nav_finish (gem_navplan.hip)
// takes the same order and key with one neighbour per lane, and its walk is the loop below with the scan replaced by a wave minimum.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GEM_NAV_HD __host__ __device__ __forceinline__
#else
#define GEM_NAV_HD inline
#endif

namespace gem {

constexpr int kNavUnreached = 0x7fffffff;                           // GEM_NAV_UNREACHED
constexpr unsigned long long kNavNoKey = ~0ull;                     // a neighbour off the map

// neighbour k = 0 .. 7 in the library's order: xd = -1, 0, 1 outer, yd = -1, 0, 1 inner, (0, 0) skipped
GEM_NAV_HD int nav_xd(int k) { const int j = k + (k >= 4); return j / 3 - 1; }
GEM_NAV_HD int nav_yd(int k) { const int j = k + (k >= 4); return j % 3 - 1; }
// potential * 8 + scan order: the minimum over the neighbours is the first smallest one
GEM_NAV_HD unsigned long long nav_key(int pot, int k) { return ((unsigned long long)(unsigned)pot << 3) | (unsigned)k; }

// The walk from the goal back to the start over a converged potential.  Cells are linear, y * sx + x; both lie on the map.  Writes the
// visited cells, goal first, to rev[0 .. min(n, cap)) (rev may be NULL) and returns n, the path's cell count; 0: the goal is unreached.
// Every step goes to a strictly smaller potential (a reached non-start cell has a 4-neighbour smaller by its weight), so the walk
// visits no cell twice: the loop is bounded by the cell count, and says so.
GEM_NAV_HD long long nav_grid_path(const int* pot, int sx, int sy, int start, int goal, int* rev, long long cap)
{
    if (pot[goal] == kNavUnreached) return 0;
    const long long cells = (long long)sx * sy;
    long long n = 0;
    int c = goal;
    for (long long step = 0; c != start && step < cells - 1; ++step) {
        if (rev && n < cap) rev[n] = c;
        ++n;
        const int cx = c % sx, cy = c / sx;
        unsigned long long best = kNavNoKey;
        for (int k = 0; k < 8; ++k) {
            const int x = cx + nav_xd(k), y = cy + nav_yd(k);
            if (x < 0 || y < 0 || x >= sx || y >= sy) continue;
            const unsigned long long key = nav_key(pot[y * sx + x], k);
            if (key < best) best = key;
        }
        if (best == kNavNoKey) break;                                   // (a 1 x 1 map has no neighbour; c == start there anyway)
        const int k = (int)(best & 7ull);
        c =(cy + nav_yd(k)) * sx + cx + nav_xd(k);
    }
    if (rev && n < cap) rev[n] = c;
    return n + 1;
}

} // namespace gem
