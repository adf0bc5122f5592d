// The rollout side of the C++ facade (gem.hpp): gem::RolloutConfig, gem::RolloutPlan, gem::RolloutBest, gem::rolloutHost and
// gem::Costmap::rolloutBest.  Without a GPU ("0") it checks the plan, the host twin and the pick on a case with known answers and shows
// that the facade compiles and links; with one ("1") rolloutBest -- the candidates and the pick on the device -- must answer exactly
// what the host twin gives over the bytes and grids read back from the same costmap.
#include "gem/gem.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

using gem::Costmap;
using gem::FootprintPoint;
using gem::RolloutBest;
using gem::RolloutConfig;
using gem::RolloutPlan;
using gem::RolloutState;

static_assert(sizeof(gem_rollout_config) == 240 && sizeof(struct gem_rollout_plan) == 2368 && sizeof(gem_rollout_best) == 64, "the sizes the header states");

int main(int argc, char** argv)
{
    const std::vector<FootprintPoint> spec{{-0.07, -0.05}, {-0.07, 0.05}, {0.07, 0.05}, {0.07, -0.05}};
    {   // a free 40 x 40 map at 0.1: PATH is the row distance to row 20, GOAL the Manhattan distance to cell (35, 20).  From the centre of
        // cell (10, 20) heading along the row at 0.5 m/s the fastest straight candidate ends in cell (15, 20): 0.6 * 0 + 20 * 0.8 = 16.
        const gem_costmap_config geom{40, 40, 0.1, 0.0, 0.0, 0};
        std::vector<unsigned char> bytes(1600, 0);
        std::vector<int> path(1600), goal(1600);
        for (int y = 0; y < 40; ++y)
            for (int x = 0; x < 40; ++x) { path[y * 40 + x] = std::abs(y - 20); goal[y * 40 + x] = std::abs(x - 35) + std::abs(y - 20); }
        RolloutConfig cfg;
        const RolloutState s{{1.05, 2.05, 0.0}, {0.5, 0.0, 0.0}};
        const RolloutPlan plan(cfg, s);
        CHECK(plan.n_vx == 3 && plan.n_vth == 20 && plan.off_b == 62 && plan.off_c == 82 && plan.off_d == 86 && plan.n_cand == 87 && plan.max_steps == 20);     // 0.5 * 1 / 0.025
        CHECK(plan.min_x == 0.375 && plan.max_x == 0.5 && plan.dvx == 0.0625 && plan.lists[2] == 0.5 && plan.state_flags == 0);
        const gem::Rollout r = gem::rolloutHost(plan, s, geom, bytes, path, goal, spec, 0, true);
        CHECK(r.best.index == 40 && r.best.stage == 1 && r.best.cost == 16.0 && r.best.raw_cost == 16.0 && r.best.xv == 0.5 && r.best.yv == 0.0 && r.best.thetav == 0.0);
        CHECK(r.steps[40] == 20 && r.cost[40] == 16.0 && r.ahead[40] == 17 && r.poses.size() == 87u * 20u);     // 1.525 + 0.325 = 1.85: cell 18
        CHECK(r.poses[40 * 20 + 19].x > 1.524 && r.poses[40 * 20 + 19].x < 1.526 && r.poses[40 * 20 + 19].cos_th == 1.0);
        CHECK(r.cost[62] == 20.0 && r.steps[86] == 4);                                                        // in place: 25 * 0.8 | backing up 0.1 m
        const RolloutBest again = plan.pick(0, r.cost, r.ahead);
        CHECK(std::memcmp(&again, &r.best, 64) == 0);
        // escaping: no phase A; every rotation stuck, every strafe stuck: the backward candidate
        const RolloutPlan esc(cfg, s, GEM_ROLLOUT_ESCAPING | GEM_ROLLOUT_STUCK_LEFT | GEM_ROLLOUT_STUCK_RIGHT | GEM_ROLLOUT_STUCK_LEFT_STRAFE | GEM_ROLLOUT_STUCK_RIGHT_STRAFE);
        CHECK(esc.off_b == 0 && esc.n_cand == 25);
        const gem::Rollout back = gem::rolloutHost(esc, s, geom, bytes, path, goal, spec);
        CHECK(back.best.index == 24 && back.best.stage == 3 && back.best.xv == -0.1 && back.best.cost == back.best.raw_cost && back.best.cost >= 0);
        bool threw = false;
        try { plan.pick(GEM_ROLLOUT_ESCAPING, r.cost, r.ahead); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                             // the plan was not made for an escaping robot
        threw = false;
        const RolloutState moved{{1.05, 2.05, 0.0}, {0.3, 0.0, 0.0}};
        try { gem::rolloutHost(plan, moved, geom, bytes, path, goal, spec); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                             // ... nor for this velocity
        cfg.vx_samples = 1;
        threw = false;
        try { RolloutPlan bad(cfg, s); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                             // the library divides by zero there
    }
    const bool expect_gpu = argc > 1 && std::atoi(argv[1]) != 0;
    if (!expect_gpu) {
        std::printf(fails ? "FAILED\n" : "OK (no GPU: built)\n");
        return fails ? 1 : 0;
    }
    gem::ElevationMap map(32, 0.1f);
    {
        Costmap cm(map, 40, 40, 0.1, 0.0, 0.0, Costmap::FREE_SPACE);
        std::vector<unsigned char> g(1600, 0);
        for (int i = 0; i < 1600; ++i) g[i] = static_cast<unsigned char>((i * 37) % 200);
        for (int y = 0; y < 18; ++y) g[y * 40 + 30] = Costmap::LETHAL_OBSTACLE;    // a wall to the right of the start, open above row 18
        cm.write(0, 0, 40, 40, g);
        cm.prepareMapGrid({{1.05, 1.05}, {3.55, 3.55}});
        RolloutConfig cfg;
        cfg.max_vel_x = 1.2; cfg.sim_time = 1.5;
        const RolloutState s{{2.35, 1.05, 0.3}, {0.9, 0.0, 0.1}};
        const RolloutPlan plan(cfg, s);
        const gem::Rollout want = gem::rolloutHost(plan, s, cm.geometry(), cm.read(0, 0, 40, 40), cm.mapGrid(Costmap::PathGrid).dist,
                                                   cm.mapGrid(Costmap::GoalGrid).dist, spec, GEM_FOOTPRINT_INSCRIBED_LETHAL);
        int legal = 0;
        for (double c : want.cost) legal += c >= 0;
        CHECK(legal > 0 && legal < plan.n_cand);                                  // some run into the wall
        std::vector<double> cost;
        std::vector<int> ahead;
        const RolloutBest got = cm.rolloutBest(plan, s, 0, spec, GEM_FOOTPRINT_INSCRIBED_LETHAL, &cost, &ahead);
        CHECK(std::memcmp(&got, &want.best, 64) == 0 && got.stage >= 1 && got.stage <= 3);
        CHECK(cost.size() == want.cost.size() && std::memcmp(cost.data(), want.cost.data(), cost.size() * sizeof(double)) == 0 && ahead == want.ahead);
        const RolloutBest again = cm.rolloutBest(plan, s, 0, spec, GEM_FOOTPRINT_INSCRIBED_LETHAL);       // without the arrays
        CHECK(std::memcmp(&again, &want.best, 64) == 0);
        bool threw = false;
        try { cm.rolloutBest(plan, s, GEM_ROLLOUT_STUCK_LEFT, spec); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                             // a plan made for other state flags
        cm.rollTo(2.5, 2.5);
        cm.rollTo(2.9, 2.1);
        threw = false;
        try { cm.rolloutBest(plan, s, 0, spec); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                             // the grids are stale
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
