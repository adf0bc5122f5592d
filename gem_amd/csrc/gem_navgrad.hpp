// gem_navgrad.hpp -- paths on a plan's potential for a batch of goals (include/gem_hip_navpath.h; internal header): the arithmetic of
// GradientPath::getPath that the kernel (gem_navgrad.hip) and its host twin share -- the gradient of a cell G, the interpolation L and
// ONE STEP of the walk over the 4 x 4 block of potentials a step can read -- the grid form's neighbour scan, the host twin itself
// (plain C++, no device) and the kernel's argument block.  Compiles without HIP too: the host twin is run on its own under the
// sanitizers (tests/cpp/navpath_check.cpp).  Build with -ffp-contract=off: every operation below is rounded on its own.
#pragma once

#include "../../include/gem_hip.h"
#include "gem_navpath.hpp"

#include <cmath>

namespace gem {

constexpr int kNavPathMaxGoals = 1024;
constexpr int kNavPathMaxPoints = 1 << 20;
constexpr long long kNavPathMaxTotal = 1ll << 24;                   // n_goals * max_points
constexpr int kNavPathMaxSize = 1 << 24;                            // a cell coordinate is exact in a float below it

struct NavVec { float x, y; };

// G of a cell whose potential cv is not high, from its four neighbours' (UNREACHED off the map).  Differences in int32, then converted.
GEM_NAV_HD NavVec nav_grad(int cv, int left, int right, int up, int down)
{
    float gx = 0.f, gy = 0.f;
    if (left != kNavUnreached) gx += (float)(left - cv);
    if (right != kNavUnreached) gx += (float)(cv - right);
    if (up != kNavUnreached) gy += (float)(up - cv);
    if (down != kNavUnreached) gy += (float)(cv - down);
    const float n = sqrtf(gx * gx + gy * gy);
    if (!(n > 0.f)) return NavVec{0.f, 0.f};
    const float r = (float)(1.0 / (double)n);
    return NavVec{r * gx, r * gy};
}

// what the C++ expression (1.0 - t) * a + t * b over floats evaluates to: t * b is a float product, the rest is double
GEM_NAV_HD float nav_lerp(float t, float a, float b) { return (float)((1.0 - (double)t) * (double)a + (double)(t * b)); }

// the walk's state: the cell, the offset inside it, the list's length and its last two points (the float == test of the oscillation
// needs the third from last only when the next one is appended)
struct NavWalk {
    int cx, cy;
    float dx, dy;
    int n;
    float ax, ay, bx, by;               // the last point | the one before it
};

GEM_NAV_HD NavWalk nav_walk_begin(int gx, int gy) { return NavWalk{gx, gy, 0.f, 0.f, 0, 0.f, 0.f, 0.f, 0.f}; }

// One iteration of the walk.  B is the block P(cx - 1 .. cx + 2, cy - 1 .. cy + 2), row-major: B[(j + 1) * 4 + (i + 1)] = P(cx + i,
// cy + j), read at the walk's cell as it is on entry.  Returns 0 to go on or the final status; *emit says whether (px, py) is a new
// point of the list (w.n counts it already).  Every index into B is a constant: on the device the block stays in scalar registers.
GEM_NAV_HD int nav_walk_step(NavWalk& w, const int* B, int sx0, int sy0, int max_points, float& px, float& py, bool& emit)
{
    emit = false;
    if (w.n >= max_points) return GEM_NAVPATH_CAP;
    const float nx = (float)w.cx + w.dx, ny = (float)w.cy + w.dy;
    emit = true;
    if (fabs((double)nx - (double)sx0) < 0.5 && fabs((double)ny - (double)sy0) < 0.5) {
        px = (float)sx0; py = (float)sy0;
        ++w.n;
        return GEM_NAVPATH_FOUND;
    }
    px = nx; py = ny;
    const bool osc = w.n >= 2 && nx == w.bx && ny == w.by;          // the new point against the third from last
    w.bx = w.ax; w.by = w.ay; w.ax = nx; w.ay = ny;
    ++w.n;
    const int U = kNavUnreached;
    const bool high = B[0] == U || B[1] == U || B[2] == U || B[4] == U || B[5] == U || B[6] == U || B[8] == U || B[9] == U || B[10] == U;
    if (high || osc) {
        // the smallest of the eight neighbours, row-major, strict <; c itself stays when none is smaller
        int bp = B[5], bi = 0, bj = 0;
        if (B[0] < bp) { bp = B[0]; bi = -1; bj = -1; }
        if (B[1] < bp) { bp = B[1]; bi = 0; bj = -1; }
        if (B[2] < bp) { bp = B[2]; bi = 1; bj = -1; }
        if (B[4] < bp) { bp = B[4]; bi = -1; bj = 0; }
        if (B[6] < bp) { bp = B[6]; bi = 1; bj = 0; }
        if (B[8] < bp) { bp = B[8]; bi = -1; bj = 1; }
        if (B[9] < bp) { bp = B[9]; bi = 0; bj = 1; }
        if (B[10] < bp) { bp = B[10]; bi = 1; bj = 1; }
        w.cx += bi; w.cy += bj;
        w.dx = 0.f; w.dy = 0.f;
        return bp == U ? GEM_NAVPATH_HIGH : 0;
    }
    // the four cells' gradients: all four cells lie in the 3 x 3 block just tested, so none is high
    const NavVec g00 = nav_grad(B[5], B[4], B[6], B[1], B[9]);
    const NavVec g10 = nav_grad(B[6], B[5], B[7], B[2], B[10]);
    const NavVec g01 = nav_grad(B[9], B[8], B[10], B[5], B[13]);
    const NavVec g11 = nav_grad(B[10], B[9], B[11], B[6], B[14]);
    const float x1 = nav_lerp(w.dx, g00.x, g10.x), x2 = nav_lerp(w.dx, g01.x, g11.x), x = nav_lerp(w.dy, x1, x2);
    const float y1 = nav_lerp(w.dx, g00.y, g10.y), y2 = nav_lerp(w.dx, g01.y, g11.y), y = nav_lerp(w.dy, y1, y2);
    if (x == 0.f && y == 0.f) return GEM_NAVPATH_ZERO_GRADIENT;
    const float ss = 0.5f / sqrtf(x * x + y * y);
    w.dx += x * ss;
    w.dy += y * ss;
    if (w.dx > 1.f) { ++w.cx; w.dx -= 1.f; }
    if (w.dx < -1.f) { --w.cx; w.dx += 1.f; }
    if (w.dy > 1.f) { ++w.cy; w.dy -= 1.f; }
    if (w.dy < -1.f) { --w.cy; w.dy += 1.f; }
    return 0;
}

// P(x, y): pot on the map, UNREACHED off it
inline int nav_pot_at(const int* pot, int sx, int sy, int x, int y)
{
    return x >= 0 && y >= 0 && x < sx && y < sy ? pot[(size_t)y * (size_t)sx + (size_t)x] : kNavUnreached;
}

// The host twin of one goal (gem_navpath_host behind its argument checks): plain C++, the step above as it stands.
inline void navpath_walk_host(const int* pot, int sx, int sy, int sx0, int sy0, int gx, int gy, int form, int max_points, float* out_pts,
                              gem_navpath_result* out)
{
    *out = gem_navpath_result{};
    out->goal_cell[0] = out->goal_cell[1] = -1;
    out->goal_potential = kNavUnreached;
    if (gx < 0 || gy < 0 || gx >= sx || gy >= sy) { out->status = GEM_NAVPATH_OFF_MAP; return; }
    out->goal_cell[0] = gx; out->goal_cell[1] = gy;
    out->goal_potential = nav_pot_at(pot, sx, sy, gx, gy);
    if (out->goal_potential == kNavUnreached) { out->status = GEM_NAVPATH_UNREACHED; return; }
    int status = 0, n = 0;
    if (form == GEM_NAVPATH_GRID) {
        int cx = gx, cy = gy;
        while (!status) {
            if (n >= max_points) { status = GEM_NAVPATH_CAP; break; }
            if (out_pts) { out_pts[2 * (size_t)n] = (float)cx; out_pts[2 * (size_t)n + 1] = (float)cy; }
            ++n;
            if (cx == sx0 && cy == sy0) { status = GEM_NAVPATH_FOUND; break; }
            unsigned long long best = kNavNoKey;
            for (int k = 0; k < 8; ++k) {
                const int x = cx + nav_xd(k), y = cy + nav_yd(k);
                if (x < 0 || y < 0 || x >= sx || y >= sy) continue;
                const unsigned long long key = nav_key(pot[(size_t)y * (size_t)sx + (size_t)x], k);
                if (key < best) best = key;
            }
            if (best == kNavNoKey) { status = GEM_NAVPATH_HIGH; break; }   // (a 1 x 1 map whose cell is not the start: nowhere to go)
            const int k = (int)(best & 7ull);
            cx += nav_xd(k); cy += nav_yd(k);
        }
    } else {
        NavWalk w = nav_walk_begin(gx, gy);
        while (!status) {
            int B[16];
            for (int j = 0; j < 4; ++j)
                for (int i = 0; i < 4; ++i) B[j * 4 + i] = nav_pot_at(pot, sx, sy, w.cx + i - 1, w.cy + j - 1);
            float px = 0.f, py = 0.f;
            bool emit = false;
            const int at = w.n;
            status = nav_walk_step(w, B, sx0, sy0, max_points, px, py, emit);
            if (emit && out_pts) { out_pts[2 * (size_t)at] = px; out_pts[2 * (size_t)at + 1] = py; }
        }
        n = w.n;
    }
    out->status = status;
    out->n_points = n;
}

// the kernel's argument block
struct NavPathArgs {
    const int* pot;                     // [sy][sx], read only
    const int* goals;                   // [n_goals][2]: (x, y), (-1, -1) off the map
    float* pts;                         // [n_goals][max_points][2], may be NULL
    gem_navpath_result* res;            // [n_goals]
    int sx, sy;
    int sx0, sy0;                       // the plan's start cell, (-1, -1) off the map
    int form, max_points;
    int n_goals;
};

#if defined(__HIPCC__)
hipError_t launch_nav_paths(hipStream_t st, const NavPathArgs& a);
#endif

} // namespace gem
