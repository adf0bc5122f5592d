// The frontier side of the C++ facade (gem.hpp): gem::Frontier, gem::FrontierSearch, gem::Costmap::frontiers / readFrontiers / navPlanTo.
// Without a GPU ("0") it checks the host twin against an answer derived by hand and shows that the facade compiles and links; with
// one ("1") the device search on the same 7 x 5 map must equal it, and navPlanTo must equal a plan to the same goal.
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
    // 7 x 5, every free cell costs 50, the start at (1, 1), no outline; unknown: (3, 1) and (4, 2), which touch by a corner -- one
    // frontier -- and the far column x = 6, another.  Potentials by hand: |x - 1| + |y - 1| steps of 50 where the way is free.
    std::vector<unsigned char> g(35, 0);
    g[1 * 7 + 3] = g[2 * 7 + 4] = Costmap::NO_INFORMATION;
    for (int y = 0; y < 5; ++y) g[y * 7 + 6] = Costmap::NO_INFORMATION;
    const std::vector<int> w = NavPlan::weights(50, 3.0, 253, false);
    std::vector<int> pot(35, -1);
    gem_navplan_status nst{};
    const int s[2] = {1, 1};
    CHECK(gem_navplan_host(g.data(), 7, 5, w.data(), 0, s, s, pot.data(), nullptr, 0, &nst) == GEM_OK);
    CHECK(pot[1 * 7 + 2] == 50 && pot[1 * 7 + 3] == GEM_NAV_UNREACHED && pot[0 * 7 + 3] == 150 && pot[1 * 7 + 5] == 300 && pot[6] == GEM_NAV_UNREACHED);
    // frontier one: cells 10 and 18, doors of (3, 1): (2, 1) at 50; root 10, size 2, sums 7 and 3.  Frontier two: the column, root 6,
    // size 5, sums 30 and 10, cheapest door (5, 0) at 250 = cell 5.
    const gem_frontier_params prm{0.0, 1.0, 1.0};
    std::vector<int> labels(35, -7);
    std::vector<gem_frontier> rec(4);
    gem_frontier_status st{};
    CHECK(gem_frontiers_host(g.data(), pot.data(), 7, 5, 0.5, &prm, labels.data(), rec.data(), 4, &st) == GEM_OK);
    CHECK(st.n_cells == 7 && st.n_frontiers == 2 && st.n_kept == 2 && st.best == 1 && st.rounds == 0 && st.chunks == 0);
    CHECK(rec[0].root == 6 && rec[0].size == 5 && rec[0].sum_x == 30 && rec[0].sum_y == 10 && rec[0].access_potential == 250 && rec[0].access_cell == 5);
    CHECK(rec[1].root == 10 && rec[1].size == 2 && rec[1].sum_x == 7 && rec[1].sum_y == 3 && rec[1].access_potential == 50 && rec[1].access_cell == 9);
    CHECK(rec[0].cost == 250.0 - 2.5 && rec[1].cost == 50.0 - 1.0 && st.best_frontier.root == 10 && st.best_frontier.cost == 49.0);
    CHECK(labels[10] == 10 && labels[18] == 10 && labels[6] == 6 && labels[34] == 6 && labels[0] == -1 && labels[11] == -1);
    CHECK(gem_frontiers_host(g.data(), pot.data(), 7, 5, 0.5, &prm, nullptr, rec.data(), 1, &st) == GEM_ERR_INVALID && st.n_kept == 2);
    gem::Frontier f;
    f.record = rec[1]; f.originX = -1.0; f.originY = 2.0; f.resolution = 0.5;
    CHECK(f.centroid().x == -1.0 + (3.5 + 0.5) * 0.5 && f.centroid().y == 2.0 + (1.5 + 0.5) * 0.5);

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
        try { cm.frontiers(); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                             // no plan yet
        const FootprintPoint robot{-1.0 + 1.5 * 0.5, 2.0 + 1.5 * 0.5};
        cm.navPlan(robot, robot, w, false);
        threw = false;
        try { cm.readFrontiers(); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                             // no search yet
        const gem::FrontierSearch fs = cm.frontiers(0.0, 1.0, 1.0);
        CHECK(fs.found && fs.status.n_cells == 7 && fs.status.n_frontiers == 2 && fs.status.n_kept == 2 && fs.status.best == 1 && fs.status.chunks >= 1);
        CHECK(fs.best.record.root == 10 && fs.best.record.size == 2 && fs.best.record.access_cell == 9 && fs.best.record.cost == 49.0);
        CHECK(fs.best.centroid().x == f.centroid().x && fs.best.centroid().y == f.centroid().y);
        std::vector<int> dev_labels;
        const std::vector<gem::Frontier> kept = cm.readFrontiers(&dev_labels);
        CHECK(dev_labels == labels && kept.size() == 2 && kept[0].record.root == 6 && kept[0].record.sum_x == 30 && kept[0].record.cost == 247.5 &&
              kept[1].record.root == 10);
        // on to the winner's access cell, (2, 1): the walk alone, and the same answer as a plan to that goal
        const FootprintPoint goal{-1.0 + 2.5 * 0.5, 2.0 + 1.5 * 0.5};
        const NavPlan p = cm.navPlanTo(goal);
        CHECK(p.found && p.status.n_path == 2 && p.status.goal_potential == 50 && p.status.chunks == 1 && p.path.size() == 2);
        CHECK(p.status.goal_cell[0] == 2 && p.status.goal_cell[1] == 1 && p.path.size() == 2 && p.path[1].x == goal.x && p.path[1].y == goal.y);
        CHECK(cm.potential() == pot);
        CHECK(cm.readFrontiers().size() == 2);                                    // the potential is unchanged: the search stands
        const NavPlan q = cm.navPlan(robot, goal, w, false);
        CHECK(q.found && q.path.size() == p.path.size() && q.status.goal_potential == 50);
        threw = false;
        try { cm.readFrontiers(); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                             // a new plan: the search is stale
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
