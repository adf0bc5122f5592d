// gem_navgrad.hip -- paths on the last plan's potential for a batch of goals (include/gem_hip_navpath.h): one wave64 per goal, one
// wave per workgroup, every goal's walk in flight at once.  A walk is a serial chain of dependent loads; what a launch hides is the
// latency of one chain behind the others'.
//
//   GRADIENT   a step of the walk (nav_walk_step, gem_navgrad.hpp) can read only the 4 x 4 block P(cx - 1 .. cx + 2, cy - 1 .. cy + 2).
//              Sixteen lanes load one cell each, predicated for the map's edge (lanes 16 .. 63 repeat them: no divergence, the same
//              cache lines); the block is handed round with v_readlane, so it lies in SCALAR registers, and every lane does the step's
//              arithmetic redundantly on uniform values.  A step is one load round trip and the step's chain; lane 0 stores the point.
//   GRID       the grid path's scan with one neighbour per lane and a minimum over groups of eight lanes, as k_nav_finish does.
// The potential is read, never written; no LDS.
#include "gem_navgrad.hpp"

#include <hip/hip_runtime.h>

namespace gem {

__global__ __launch_bounds__(64) void k_nav_paths(NavPathArgs a)
{
    const int g = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (g >= a.n_goals) return;
    const int gx = a.goals[2 * g], gy = a.goals[2 * g + 1];
    float* pts = a.pts ? a.pts + (size_t)g * (size_t)a.max_points * 2 : nullptr;
    int status = 0, n = 0, goal_pot = kNavUnreached;
    const bool on = gx >= 0 && gy >= 0 && gx < a.sx && gy < a.sy;
    if (on) goal_pot = a.pot[(size_t)gy * (size_t)a.sx + (size_t)gx];
    if (!on) status = GEM_NAVPATH_OFF_MAP;
    else if (goal_pot == kNavUnreached) status = GEM_NAVPATH_UNREACHED;
    else if (a.form == GEM_NAVPATH_GRID) {
        int cx = gx, cy = gy;
        const int k = lane & 7;                                         // lanes 8 .. 63 repeat lanes 0 .. 7
        const int xd = nav_xd(k), yd = nav_yd(k);
        while (!status) {                                               // (bounded by max_points)
            if (n >= a.max_points) { status = GEM_NAVPATH_CAP; break; }
            if (lane == 0 && pts) { pts[2 * (size_t)n] = (float)cx; pts[2 * (size_t)n + 1] = (float)cy; }
            ++n;
            if (cx == a.sx0 && cy == a.sy0) { status = GEM_NAVPATH_FOUND; break; }
            const int x = cx + xd, y = cy + yd;
            const bool in = x >= 0 && y >= 0 && x < a.sx && y < a.sy;
            const int p = a.pot[in ? (size_t)y * (size_t)a.sx + (size_t)x : (size_t)0];
            unsigned long long key = in ? nav_key(p, k) : kNavNoKey;
#pragma unroll
            for (int off = 1; off < 8; off <<= 1) {
                const unsigned long long o = __shfl_xor(key, off, 8);
                key = o < key ? o : key;
            }
            const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)key);      // (every group of eight holds the same key)
            const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(key >> 32));
            if ((lo & hi) == 0xffffffffu) { status = GEM_NAVPATH_HIGH; break; }
            const int kb = (int)(lo & 7u);
            cx += nav_xd(kb); cy += nav_yd(kb);
        }
    } else {
        NavWalk w = nav_walk_begin(gx, gy);
        const int i = (lane & 3) - 1, j = ((lane >> 2) & 3) - 1;        // lanes 16 .. 63 repeat lanes 0 .. 15
        while (!status) {                                               // (bounded by max_points: every pass that goes on appends a point)
            const int x = w.cx + i, y = w.cy + j;
            const bool in = x >= 0 && y >= 0 && x < a.sx && y < a.sy;
            const int v = in ? a.pot[(size_t)y * (size_t)a.sx + (size_t)x] : kNavUnreached;
            int B[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) B[c] = __builtin_amdgcn_readlane(v, c);
            float px = 0.f, py = 0.f;
            bool emit = false;
            const int at = w.n;
            status = nav_walk_step(w, B, a.sx0, a.sy0, a.max_points, px, py, emit);
            if (emit && lane == 0 && pts) { pts[2 * (size_t)at] = px; pts[2 * (size_t)at + 1] = py; }
        }
        n = w.n;
    }
    if (lane == 0) {
        gem_navpath_result r{};
        r.status = status; r.n_points = n;
        r.goal_cell[0] = on ? gx : -1; r.goal_cell[1] = on ? gy : -1;
        r.goal_potential = goal_pot;
        a.res[g] = r;
    }
}

hipError_t launch_nav_paths(hipStream_t st, const NavPathArgs& a)
{
    hipLaunchKernelGGL(k_nav_paths, dim3((unsigned)a.n_goals), dim3(64), 0, st, a);
    return hipGetLastError();
}

} // namespace gem
