// The global-plan side of the C++ facade (gem.hpp): gem::NavPlan::weights, gem::Costmap::navPlan / potential.  Without a GPU ("0") it
// checks the host-only weight table and the host twin against an answer derived by hand and shows that the facade compiles and links;
// with one ("1") the device plan on the same 7 x 5 map must equal it.
#include "gem/gem.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

using gem::Costmap;
using gem::FootprintPoint;
using gem::NavPlan;

int main(int argc, char** argv)
{
    const int U = GEM_NAV_UNREACHED;
    // 7 x 5, a wall in column 3 over rows 1 .. 3, no outline, every free cell costs 50; start (1, 1), goal (5, 1)
    std::vector<unsigned char> g(35, 0);
    for (int y = 1; y < 4; ++y) g[y * 7 + 3] = Costmap::LETHAL_OBSTACLE;
    const std::vector<int> want{100, 50,  100, 150, 200, 250, 300,     //
                                50,  0,   50,  U,   250, 300, 350,     //
                                100, 50,  100, U,   300, 350, 400,     //
                                150, 100, 150, U,   350, 400, 450,     //
                                200, 150, 200, 250, 300, 350, 400};
    // from (5, 1) the first smallest neighbour in scan order is (4, 0), then (3, 0), then (2, 1), then the start
    const std::vector<int> want_cells{1 * 7 + 1, 1 * 7 + 2, 0 * 7 + 3, 0 * 7 + 4, 1 * 7 + 5};
    const std::vector<int> w = NavPlan::weights();
    {
        CHECK(w.size() == 256 && w[0] == 50 && w[1] == 53 && w[67] == 251 && w[68] == 252 && w[251] == 252 && w[252] == 0 && w[253] == 0 &&
              w[254] == 0 && w[255] == 252);
        CHECK(NavPlan::weights(50, 3.0, 253, false)[255] == 0);
        bool threw = false;
        try { NavPlan::weights(50, 2.5); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
        std::vector<int> pot(35, -1), cells(35, -1);
        gem_navplan_status st{};
        const int s[2] = {1, 1}, e[2] = {5, 1};
        CHECK(gem_navplan_host(g.data(), 7, 5, w.data(), 0, s, e, pot.data(), cells.data(), 35, &st) == GEM_OK);
        CHECK(pot == want && st.found == 1 && st.n_path == 5 && st.goal_potential == 300 && st.rounds == 0 && st.chunks == 0);
        cells.resize(5);
        CHECK(cells == want_cells);
        CHECK(gem_navplan_host(g.data(), 7, 5, w.data(), 0, s, e, nullptr, cells.data(), 4, &st) == GEM_ERR_INVALID && st.n_path == 5);
        CHECK(gem_navplan_host(g.data(), 7, 5, w.data(), GEM_NAV_OUTLINE, s, e, pot.data(), nullptr, 0, &st) == GEM_OK && st.found == 0 &&
              st.n_path == 0 && st.goal_potential == U && pot[2 * 7 + 2] == 100 && pot[0] == U);
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
        bool threw = false;
        try { cm.potential(); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                             // no plan yet
        const NavPlan p = cm.navPlan({-1.0 + 1.5 * 0.5, 2.0 + 1.5 * 0.5}, {-1.0 + 5.5 * 0.5, 2.0 + 1.5 * 0.5}, {}, false);
        CHECK(p.found && p.status.n_path == 5 && p.status.goal_potential == 300 && p.status.chunks >= 1 && p.path.size() == 5);
        CHECK(p.status.start_cell[0] == 1 && p.status.start_cell[1] == 1 && p.status.goal_cell[0] == 5 && p.status.goal_cell[1] == 1);
        for (size_t i = 0; i < p.path.size() && i < want_cells.size(); ++i)
            CHECK(p.path[i].x == -1.0 + (want_cells[i] % 7 + 0.5) * 0.5 && p.path[i].y == 2.0 + (want_cells[i] / 7 + 0.5) * 0.5);
        CHECK(cm.potential() == want);
        const NavPlan q = cm.navPlan({-1.0 + 1.5 * 0.5, 2.0 + 1.5 * 0.5}, {-1.0 + 5.5 * 0.5, 2.0 + 1.5 * 0.5});     // the outline closes the way round
        CHECK(!q.found && q.path.empty() && q.status.goal_potential == U);
        cm.updateOrigin(-0.5, 2.0);                                               // the map moved: the plan is stale
        threw = false;
        try { cm.potential(); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
