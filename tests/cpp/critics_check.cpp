// The best-trajectory side of the C++ facade (gem.hpp): gem::Critic, gem::BestTrajectory, gem::selectTrajectory and
// gem::Costmap::prepareMapGridFront / mapGridFront / bestTrajectory.  Without a GPU ("0") it checks the host-only combination and shows
// that the facade compiles and links; with one ("1") it runs against hand-derived answers on the 5 x 5 map of mapgrid_check.cpp.
#include "gem/gem.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

using gem::BestTrajectory;
using gem::Costmap;
using gem::Critic;
using gem::FootprintPoint;
using gem::FootprintPose;

static_assert(sizeof(gem_critic) == 32 && sizeof(gem_best_trajectory) == 32, "both are 32 bytes");

int main(int argc, char** argv)
{
    {   // three critics over four trajectories; the middle one has scale 0 and is never read
        const std::vector<Critic> critics{Critic::external(2.0, 0), Critic::external(0.0, 1), Critic::external(1.0, 2)};
        const std::vector<double> scores{1.0, 0.5, -2.0, 0.5,      //
                                         -1.0, -1.0, -1.0, -1.0,   //
                                         0.0, 1.0, 5.0, 1.0};
        std::vector<double> totals;
        const BestTrajectory b = gem::selectTrajectory(critics, scores, &totals);
        CHECK(totals == (std::vector<double>{2.0, 2.0, -2.0, 2.0}));
        CHECK(b.valid() && b.index == 0 && b.cost == 2.0 && b.n_valid == 3 && b.reserved == 0);      // a three-way tie: the smallest index
        const BestTrajectory none = gem::selectTrajectory({Critic::external(1.0, 0)}, {-1.0, std::numeric_limits<double>::quiet_NaN()});
        CHECK(!none.valid() && none.index == -1 && none.cost == -1.0 && none.n_valid == 0);
        const BestTrajectory empty = gem::selectTrajectory({Critic::external(1.0, 0)}, {});
        CHECK(empty.index == -1 && empty.cost == -1.0 && empty.n_valid == 0);
        for (double bad : {-1.0, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()}) {
            bool threw = false;
            try { gem::selectTrajectory({Critic::external(bad, 0)}, {1.0}); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
            CHECK(threw);
        }
        const Critic o = Critic::obstacle(0.01, GEM_CRITIC_CENTRE_COST), g = Critic::mapGrid(24.0, GEM_CRITIC_GRID_FRONT, 0.325, GEM_MAPGRID_SUM);
        CHECK(o.kind == GEM_CRITIC_OBSTACLE && o.flags == GEM_CRITIC_CENTRE_COST && o.scale == 0.01);
        CHECK(g.kind == GEM_CRITIC_MAPGRID && g.grid == GEM_CRITIC_GRID_FRONT && g.xshift == 0.325 && g.flags == GEM_MAPGRID_SUM && g.scale == 24.0);
    }
    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;
    if (!expect_gpu) {
        std::printf(fails ? "FAILED\n" : "OK (no GPU: built)\n");
        return fails ? 1 : 0;
    }
    gem::ElevationMap map(32, 0.1f);
    {
        Costmap cm(map, 5, 5, 1.0, 0.0, 0.0, Costmap::FREE_SPACE);
        std::vector<unsigned char> g(25, 0);
        for (int y = 0; y < 4; ++y) g[y * 5 + 2] = Costmap::LETHAL_OBSTACLE;      // a wall in column 2 with its gap in row 4
        cm.write(0, 0, 5, 5, g);
        cm.prepareMapGrid({{0.5, 0.5}});                                          // path and goal from the cell (0, 0)
        const std::vector<Critic> critics{Critic::obstacle(0.5), Critic::mapGrid(2.0, GEM_CRITIC_GRID_PATH, 0.0, GEM_MAPGRID_STOP_ON_FAILURE),
                                          Critic::mapGrid(0.5, GEM_CRITIC_GRID_FRONT), Critic::external(1.0, 0)};
        // four trajectories of two poses: to the far corner | from the wall | off the map | one cell up
        const std::vector<FootprintPose> poses{FootprintPose::fromYaw(0.5, 0.5, 0.0), FootprintPose::fromYaw(4.5, 4.5, 0.0),
                                               FootprintPose::fromYaw(2.5, 1.5, 0.0), FootprintPose::fromYaw(1.5, 1.5, 0.0),
                                               FootprintPose::fromYaw(1.5, 1.5, 0.0), FootprintPose::fromYaw(5.5, 1.5, 0.0),
                                               FootprintPose::fromYaw(0.5, 0.5, 0.0), FootprintPose::fromYaw(0.5, 1.5, 0.0)};
        const std::vector<double> ext{0.25, 0.0, 0.0, 3.0};
        bool threw = false;
        try { cm.bestTrajectory(critics, poses, 2, {}, ext); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                             // the FRONT grid was never prepared
        cm.prepareMapGridFront({{4.5, 4.5}});                                     // the far corner, through the gap
        const Costmap::MapGrid front = cm.mapGridFront();
        CHECK(front.started && front.goalX == 4 && front.goalY == 4 && front.dist[0] == 8 && front.dist[1 * 5 + 0] == 7 && front.dist[24] == 0);
        CHECK(cm.mapGrid(Costmap::PathGrid).dist[24] == 8);                       // PATH is as it was
        std::vector<double> totals;
        // t0: 0 + 2 * 8 + 0.5 * 0 + 0.25 | t1: the centre on the wall, -1 | t2: the second pose off the map, -3 | t3: 0 + 2 * 1 + 0.5 * 7 + 3
        BestTrajectory b = cm.bestTrajectory(critics, poses, 2, {}, ext, {}, &totals);
        CHECK(totals == (std::vector<double>{16.25, -1.0, -3.0, 8.5}));
        CHECK(b.index == 3 && b.cost == 8.5 && b.n_valid == 2);
        // one pose of t2 and t3: t2 = 2 * 2 + 0.5 * 6 + 0, t3 = 2 * 0 + 0.5 * 8 + 3: a tie, the smaller index wins
        b = cm.bestTrajectory(critics, poses, 2, {}, ext, {2, 2, 1, 1}, &totals);
        CHECK(totals == (std::vector<double>{16.25, -1.0, 7.0, 7.0}));
        CHECK(b.index == 2 && b.cost == 7.0 && b.n_valid == 3);
        threw = false;
        try { cm.bestTrajectory(critics, poses, 2, {}, ext, {2, 2, 0, 1}); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                             // a length of 0 in host memory is refused
        b = cm.bestTrajectory({Critic::obstacle(1.0)}, {poses[2], poses[5]}, 1, {});
        CHECK(!b.valid() && b.cost == -1.0 && b.n_valid == 0);                    // all rejected
        b = cm.bestTrajectory({Critic::obstacle(1.0)}, {}, 2, {});
        CHECK(b.index == -1 && b.n_valid == 0);                                   // no trajectories
        cm.updateOrigin(1.0, 0.0);                                                // the map moved: the grids are stale
        threw = false;
        try { cm.mapGridFront(); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
