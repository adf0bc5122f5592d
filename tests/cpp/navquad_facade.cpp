// The quadratic plan through the C++ facade (gem.hpp): gem::Costmap::navPlanQuadratic.  Without a GPU ("0") it checks the library's
// host twin, gem_navquad_host, on an open 8 x 8 map of uniform weight 50 against potentials derived by hand (0 50 100 150 / 50 85 127
// 171 / ...: tests/test_navquad_cpu.py has the table), its weight limit, and shows that the facade compiles and
// links; with one ("1") the device's plan must equal the twin's, the linear plan must replace it and the other way round, and navPaths /
// navPlanTo must run on it.
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
    std::vector<unsigned char> g(64, 0);
    std::vector<int> w(256, 50);
    std::vector<int> twin(64, -1), lin(64, -1), cells(64, -1);
    gem_navplan_status hst{};
    const int s[2] = {0, 0}, e[2] = {3, 3};
    CHECK(gem_navquad_host(g.data(), 8, 8, w.data(), 0, s, e, twin.data(), cells.data(), 64, &hst) == GEM_OK);
    const int want[16] = {0, 50, 100, 150, 50, 85, 127, 171, 100, 127, 162, 201, 150, 171, 201, 236};
    for (int y = 0; y < 4; ++y)
        for (int x = 0; x < 4; ++x) CHECK(twin[y * 8 + x] == want[y * 4 + x]);
    CHECK(hst.found == 1 && hst.n_path == 4 && hst.goal_potential == 236 && cells[0] == 0 && cells[3] == 3 * 8 + 3);
    CHECK(gem_navplan_host(g.data(), 8, 8, w.data(), 0, s, e, lin.data(), nullptr, 0, &hst) == GEM_OK && lin[3 * 8 + 3] == 300);
    w[7] = 462;
    CHECK(gem_navquad_host(g.data(), 8, 8, w.data(), 0, s, e, nullptr, nullptr, 0, &hst) == GEM_OK);
    w[7] = 463;
    CHECK(gem_navquad_host(g.data(), 8, 8, w.data(), 0, s, e, nullptr, nullptr, 0, &hst) == GEM_ERR_INVALID);
    CHECK(gem_navplan_host(g.data(), 8, 8, w.data(), 0, s, e, nullptr, nullptr, 0, &hst) == GEM_OK);       // the linear plan has no such limit
    CHECK(gem_navquad_host(g.data(), 8, 8, w.data(), 2, s, e, nullptr, nullptr, 0, &hst) == GEM_ERR_INVALID);
    w[7] = 50;
    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;
    if (!expect_gpu) {
        std::printf(fails ? "FAILED\n" : "OK (no GPU: built)\n");
        return fails ? 1 : 0;
    }
    gem::ElevationMap map(32, 0.1f);
    {
        Costmap cm(map, 8, 8, 0.5, -1.0, 2.0, Costmap::FREE_SPACE);
        cm.write(0, 0, 8, 8, g);
        auto at = [](int x, int y) { return FootprintPoint{-1.0 + (x + 0.5) * 0.5, 2.0 + (y + 0.5) * 0.5}; };
        const gem::NavPlan q = cm.navPlanQuadratic(at(0, 0), at(3, 3), w, false);
        CHECK(q.found && q.path.size() == 4 && q.status.goal_potential == 236);
        CHECK(q.path.front().x == at(0, 0).x && q.path.back().y == at(3, 3).y);
        CHECK(cm.potential() == twin);
        const gem::NavPlan to = cm.navPlanTo(at(2, 1));                            // another goal on the quadratic potential
        CHECK(to.found && to.status.goal_potential == 127);
        const gem::NavPaths grad = cm.navPaths({at(3, 3), at(7, 5)});
        CHECK(grad.paths.size() == 2 && grad.found(0) && grad.results[0].goal_potential == 236 && grad.results[1].goal_potential != GEM_NAV_UNREACHED);
        const gem::NavPlan l = cm.navPlan(at(0, 0), at(3, 3), w, false);           // the linear plan replaces it
        CHECK(l.found && l.status.goal_potential == 300 && cm.potential() == lin);
        const gem::NavPlan q2 = cm.navPlanQuadratic(at(0, 0), at(3, 3), w, false); // and the other way round
        CHECK(q2.status.goal_potential == 236 && cm.potential() == twin);
        std::vector<int> big = w;
        big[0] = 463;
        bool threw = false;
        try { cm.navPlanQuadratic(at(0, 0), at(3, 3), big, false); } catch (const gem::Error& err) { threw = err.code() == GEM_ERR_INVALID; }
        CHECK(threw && cm.potential() == twin);                                   // refused, the last plan unchanged
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
