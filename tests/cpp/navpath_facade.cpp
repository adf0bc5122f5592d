// The path side of the C++ facade (gem.hpp): gem::NavPaths and gem::Costmap::navPaths.  Without a GPU ("0") it checks the library's host
// twin on the 7 x 5 map of navplan_check.cpp against an answer derived by hand and shows that the facade compiles and links; with one
// ("1") the batch on the device must give the same grid path as navPlanTo, a gradient path that ends at the start, and leave the plan alone.
#include "gem/gem.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

using gem::Costmap;
using gem::FootprintPoint;

int main(int argc, char** argv)
{
    // 7 x 5, a wall in column 3 over rows 1 .. 3, no outline, every free cell costs 50; start (1, 1)
    std::vector<unsigned char> g(35, 0);
    for (int y = 1; y < 4; ++y) g[y * 7 + 3] = Costmap::LETHAL_OBSTACLE;
    const std::vector<int> w = gem::NavPlan::weights();
    {
        std::vector<int> pot(35, -1);
        gem_navplan_status st{};
        const int s[2] = {1, 1}, e[2] = {5, 1}, off[2] = {7, 1}, wall[2] = {3, 2};
        CHECK(gem_navplan_host(g.data(), 7, 5, w.data(), 0, s, s, pot.data(), nullptr, 0, &st) == GEM_OK);
        float pts[10];
        gem_navpath_result r{};
        CHECK(gem_navpath_host(pot.data(), 7, 5, s, e, GEM_NAVPATH_GRID, 5, pts, &r) == GEM_OK);
        const float want[10] = {5, 1, 4, 0, 3, 0, 2, 1, 1, 1};             // goal first: (5, 1) (4, 0) (3, 0) (2, 1) and the start
        CHECK(r.status == GEM_NAVPATH_FOUND && r.n_points == 5 && r.goal_potential == 300 && r.goal_cell[0] == 5 && r.goal_cell[1] == 1);
        for (int i = 0; i < 10; ++i) CHECK(pts[i] == want[i]);
        CHECK(gem_navpath_host(pot.data(), 7, 5, s, off, GEM_NAVPATH_GRADIENT, 5, pts, &r) == GEM_OK && r.status == GEM_NAVPATH_OFF_MAP && r.n_points == 0);
        CHECK(gem_navpath_host(pot.data(), 7, 5, s, wall, GEM_NAVPATH_GRADIENT, 5, pts, &r) == GEM_OK && r.status == GEM_NAVPATH_UNREACHED);
        CHECK(gem_navpath_host(pot.data(), 7, 5, s, e, 2, 5, pts, &r) == GEM_ERR_INVALID && gem_navpath_host(pot.data(), 7, 5, s, e, 1, 1, pts, &r) == GEM_ERR_INVALID);
    }
    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;
    if (!expect_gpu) {
        std::printf(fails ? "FAILED\n" : "OK (no GPU: built)\n");
        return fails ? 1 : 0;
    }
    gem::ElevationMap map(32, 0.1f);
    {
        Costmap cm(map, 7, 5, 0.5, -1.0, 2.0, Costmap::FREE_SPACE);
        cm.write(0, 0, 7, 5, g);
        auto at = [](int x, int y) { return FootprintPoint{-1.0 + (x + 0.5) * 0.5, 2.0 + (y + 0.5) * 0.5}; };
        bool threw = false;
        try { cm.navPaths({at(5, 1)}); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                             // no plan yet
        const gem::NavPlan p = cm.navPlan(at(1, 1), at(1, 1), {}, false);
        CHECK(p.found);
        const std::vector<int> pot = cm.potential();
        const std::vector<FootprintPoint> goals{at(5, 1), at(6, 4), at(3, 2), at(9, 9), at(1, 1)};
        const gem::NavPaths grid = cm.navPaths(goals, GEM_NAVPATH_GRID, 64), grad = cm.navPaths(goals);
        CHECK(grid.paths.size() == 5 && grid.found(0) && grid.found(1) && grid.found(4) && grid.results[2].status == GEM_NAVPATH_UNREACHED &&
              grid.results[3].status == GEM_NAVPATH_OFF_MAP && grid.paths[2].empty() && grid.paths[4].size() == 1);
        CHECK(grad.found(0) && grad.found(1) && grad.found(4) && grad.results[2].status == GEM_NAVPATH_UNREACHED && grad.results[3].status == GEM_NAVPATH_OFF_MAP);
        for (int i : {0, 1}) {                                                    // start first, goal last, both forms
            CHECK(grad.paths[i].front().x == at(1, 1).x && grad.paths[i].front().y == at(1, 1).y);
            CHECK(grad.paths[i].back().x == goals[i].x && grad.paths[i].back().y == goals[i].y);
            CHECK(grad.paths[i].size() >= grid.paths[i].size());                      // half-cell steps
        }
        CHECK(cm.potential() == pot);                                              // the potential is as it was
        for (int i : {0, 1}) {
            const gem::NavPlan q = cm.navPlanTo(goals[i]);
            CHECK(q.found && q.path.size() == grid.paths[i].size());
            for (size_t k = 0; k < q.path.size() && k < grid.paths[i].size(); ++k)
                CHECK(q.path[k].x == grid.paths[i][k].x && q.path[k].y == grid.paths[i][k].y);
        }
        for (int bad : {0, 1, (1 << 20) + 1, 1 << 30}) {                          // refused before anything is sized by it
            threw = false;
            try { cm.navPaths(goals, GEM_NAVPATH_GRID, bad); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
            CHECK(threw);
        }
        threw = false;
        try { cm.navPaths(std::vector<FootprintPoint>(1025, at(1, 1)), GEM_NAVPATH_GRID, 16); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
        threw = false;
        try { cm.navPaths({}); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
        threw = false;
        try { cm.navPaths(goals, 7); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
        cm.updateOrigin(-0.5, 2.0);                                               // the map moved: the plan is stale
        threw = false;
        try { cm.navPaths(goals); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
