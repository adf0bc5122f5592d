// The host restatement of the path contract on its own (include/gem_hip_navpath.h): gem_amd/csrc/gem_navgrad.hpp -- G, L, one step of the
// gradient walk, the grid form and the host twin of one goal -- compiled by a plain C++ compiler, without HIP and without the library.  A
// stand-alone program, so that it can be built with -fsanitize=address,undefined: potentials of small maps (1 x 1, 2 x 2, 3 x 3, 7 x 5 with a
// wall, 24 x 17 with pseudo-random weights) in heap arrays of exactly size_x * size_y ints, EVERY cell a goal -- the border cells among
// them, where the x + 2 and y + 2 reads leave the map -- and point buffers of exactly max_points pairs (a write past either is a heap
// overflow).  A few answers are derived by hand.
#include "../../gem_amd/csrc/gem_navgrad.hpp"

#include <cstdio>
#include <queue>
#include <utility>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

// the potential of gem_hip_navplan.h by a binary-heap Dijkstra: w per cell, 0 = impassable
static std::vector<int> potential(const std::vector<int>& w, int sx, int sy, int start)
{
    std::vector<int> pot((size_t)sx * sy, GEM_NAV_UNREACHED);
    using Item = std::pair<int, int>;
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    pot[start] = 0;
    heap.push({0, start});
    const int dx[4] = {-1, 1, 0, 0}, dy[4] = {0, 0, -1, 1};
    while (!heap.empty()) {
        const Item it = heap.top();
        heap.pop();
        if (it.first != pot[it.second]) continue;
        for (int k = 0; k < 4; ++k) {
            const int x = it.second % sx + dx[k], y = it.second / sx + dy[k];
            if (x < 0 || y < 0 || x >= sx || y >= sy) continue;
            const int n = y * sx + x;
            if (n == start || w[n] <= 0) continue;
            if (it.first + w[n] < pot[n]) { pot[n] = it.first + w[n]; heap.push({pot[n], n}); }
        }
    }
    return pot;
}

static long long walked = 0;

// every cell of the map and a ring of cells off it as goals, both forms, two caps
static void every_goal(const std::vector<int>& pot, int sx, int sy, int sx0, int sy0)
{
    using namespace gem;
    for (int form = 0; form < 2; ++form)
        for (int cap : {2, 7, 4 * (sx + sy) + 8})
            for (int gy = -1; gy <= sy; ++gy)
                for (int gx = -1; gx <= sx; ++gx) {
                    std::vector<float> pts(2 * (size_t)cap, -1.f);
                    gem_navpath_result r;
                    navpath_walk_host(pot.data(), sx, sy, sx0, sy0, gx, gy, form, cap, pts.data(), &r);
                    const bool on = gx >= 0 && gy >= 0 && gx < sx && gy < sy;
                    CHECK(r.status >= GEM_NAVPATH_FOUND && r.status <= GEM_NAVPATH_CAP && r.n_points >= 0 && r.n_points <= cap);
                    CHECK((r.status == GEM_NAVPATH_OFF_MAP) == !on);
                    if (!on) { CHECK(r.n_points == 0 && r.goal_cell[0] == -1 && r.goal_potential == GEM_NAV_UNREACHED); continue; }
                    CHECK(r.goal_cell[0] == gx && r.goal_cell[1] == gy && r.goal_potential == pot[(size_t)gy * sx + gx]);
                    CHECK((r.status == GEM_NAVPATH_UNREACHED) == (r.goal_potential == GEM_NAV_UNREACHED));
                    if (r.status == GEM_NAVPATH_UNREACHED) { CHECK(r.n_points == 0); continue; }
                    CHECK(r.n_points >= 1 && pts[0] == (float)gx && pts[1] == (float)gy);             // goal first
                    if (r.status == GEM_NAVPATH_FOUND) CHECK(pts[2 * (size_t)r.n_points - 2] == (float)sx0 && pts[2 * (size_t)r.n_points - 1] == (float)sy0);
                    if (r.status == GEM_NAVPATH_CAP) CHECK(r.n_points == cap);
                    for (size_t i = 2 * (size_t)r.n_points; i < pts.size(); ++i) CHECK(pts[i] == -1.f);   // nothing behind the list
                    // the same walk without a point buffer answers the same
                    gem_navpath_result q;
                    navpath_walk_host(pot.data(), sx, sy, sx0, sy0, gx, gy, form, cap, nullptr, &q);
                    CHECK(q.status == r.status && q.n_points == r.n_points);
                    walked += r.n_points;
                }
}

int main()
{
    using namespace gem;
    const int U = GEM_NAV_UNREACHED;
    // G and L by hand
    {
        const NavVec g = nav_grad(100, 150, 50, U, 100);                  // gx = 50 + 50, gy = 0
        CHECK(g.x == 1.f && g.y == 0.f);
        const NavVec d = nav_grad(100, 103, 97, 104, 96);                 // (6, 8) / 10
        CHECK(d.x == (float)(1.0 / 10.0) * 6.f && d.y == (float)(1.0 / 10.0) * 8.f);
        const NavVec z = nav_grad(7, U, U, U, U);
        CHECK(z.x == 0.f && z.y == 0.f);
        CHECK(nav_lerp(0.f, 3.f, 9.f) == 3.f && nav_lerp(1.f, 3.f, 9.f) == 9.f && nav_lerp(0.25f, 4.f, 8.f) == 5.f);
    }
    // 1 x 1, 2 x 2, 3 x 3: uniform weights
    for (int s = 1; s <= 3; ++s) {
        const std::vector<int> w((size_t)s * s, 50);
        for (int start = 0; start < s * s; ++start) every_goal(potential(w, s, s, start), s, s, start % s, start / s);
    }
    // 7 x 5 with a wall in column 3 over rows 1 .. 3 (tests/cpp/navplan_check.cpp): the grid path from (5, 1) by hand
    {
        std::vector<int> w(35, 50);
        for (int y = 1; y < 4; ++y) w[y * 7 + 3] = 0;
        const std::vector<int> pot = potential(w, 7, 5, 1 * 7 + 1);
        CHECK(pot[1 * 7 + 5] == 300 && pot[2 * 7 + 3] == U);
        every_goal(pot, 7, 5, 1, 1);
        std::vector<float> pts(2 * 5);
        gem_navpath_result r;
        navpath_walk_host(pot.data(), 7, 5, 1, 1, 5, 1, GEM_NAVPATH_GRID, 5, pts.data(), &r);
        const float want[10] = {5, 1, 4, 0, 3, 0, 2, 1, 1, 1};
        CHECK(r.status == GEM_NAVPATH_FOUND && r.n_points == 5);
        for (int i = 0; i < 10; ++i) CHECK(pts[i] == want[i]);
        navpath_walk_host(pot.data(), 7, 5, 1, 1, 5, 1, GEM_NAVPATH_GRID, 4, pts.data(), &r);
        CHECK(r.status == GEM_NAVPATH_CAP && r.n_points == 4);
        // the gradient walk from (2, 1), the start's neighbour: its own point, then the start
        navpath_walk_host(pot.data(), 7, 5, 1, 1, 2, 1, GEM_NAVPATH_GRADIENT, 5, pts.data(), &r);
        CHECK(r.status == GEM_NAVPATH_FOUND && r.n_points >= 2 && pts[0] == 2.f && pts[1] == 1.f);
    }
    // 24 x 17, weights 50 + 3 * byte from a linear congruential generator, one cell in seven blocked, no outline
    {
        const int sx = 24, sy = 17;
        std::vector<int> w((size_t)sx * sy);
        unsigned s = 12345u;
        for (int& v : w) { s = s * 1664525u + 1013904223u; const unsigned b = (s >> 16) % 68u; s = s * 1664525u + 1013904223u; v = (s >> 16) % 7u == 0 ? 0 : 50 + 3 * (int)b; }
        every_goal(potential(w, sx, sy, 9 * sx + 11), sx, sy, 11, 9);
        every_goal(potential(w, sx, sy, 0), sx, sy, 0, 0);
    }
    // a constant block: ZERO_GRADIENT after one point
    {
        std::vector<int> pot(81, 700);
        pot[0] = 0;
        gem_navpath_result r;
        navpath_walk_host(pot.data(), 9, 9, 0, 0, 5, 4, GEM_NAVPATH_GRADIENT, 50, nullptr, &r);
        CHECK(r.status == GEM_NAVPATH_ZERO_GRADIENT && r.n_points == 1);
    }
    if (fails) { std::printf("FAILED\n"); return 1; }
    std::printf("%lld points walked\nok\n", walked);
    return 0;
}
