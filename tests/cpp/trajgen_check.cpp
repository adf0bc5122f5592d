// The trajectory-generation side of the C++ facade (gem.hpp): gem::TrajectoryLimits, gem::TrajectoryConfig, gem::TrajectoryPlan,
// gem::generateTrajectories and gem::Costmap::dwaBest.  Without a GPU ("0") it checks the host twin on cases with known answers and
// shows that the facade compiles and links; with one ("1") dwaBest -- generation and critics on the device -- must answer exactly what
// the host twin's trajectories give through bestTrajectory's host form.
#include "gem/gem.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

using gem::BestTrajectory;
using gem::Costmap;
using gem::Critic;
using gem::FootprintPoint;
using gem::TrajectoryConfig;
using gem::TrajectoryLimits;
using gem::TrajectoryPlan;
using gem::TrajectoryState;

static_assert(sizeof(gem_trajgen_limits) == 88 && sizeof(gem_trajgen_config) == 64 && sizeof(gem_dwa_plan) == 1200, "the sizes the header states");

int main(int argc, char** argv)
{
    {   // one sample, straight ahead at 0.5 m/s from the origin: by time, 2 s in steps of 0.25 s -> 8 poses, 0.125 m apart (all exact)
        TrajectoryLimits lim;
        lim.max_vel_x = lim.min_vel_x = 0.5; lim.max_vel_y = lim.min_vel_y = 0.0; lim.acc_lim_theta = 0.0;
        lim.min_vel_trans = -1.0; lim.max_vel_trans = -1.0;
        TrajectoryConfig cfg;
        cfg.sim_time = 2.0; cfg.sim_granularity = 0.25; cfg.discretize_by_time = 1; cfg.vsamples[0] = cfg.vsamples[1] = cfg.vsamples[2] = 1;
        cfg.oscillation_flags = GEM_OSC_FORWARD_NEG_ONLY;
        const TrajectoryState s{{0.f, 0.f, 0.f}, {0.5f, 0.f, 0.f}};
        const TrajectoryPlan plan(lim, cfg, s);
        CHECK(plan.n_x == 1 && plan.n_y == 1 && plan.n_th == 1 && plan.n_traj == 1 && plan.max_steps == 8);
        CHECK(plan.list(0) == std::vector<float>{0.5f} && plan.list(2) == std::vector<float>{0.f});
        const gem::Trajectories t = gem::generateTrajectories(plan, s);
        CHECK(t.posesPerTrajectory == 8 && t.length == std::vector<int>{8} && t.poses.size() == 8);
        for (int i = 0; i < 8 && i < static_cast<int>(t.poses.size()); ++i)
            CHECK(t.poses[i].x == 0.125 * i && t.poses[i].y == 0.0 && t.poses[i].cos_th == 1.0 && t.poses[i].sin_th == 0.0);
        CHECK(t.ext == (std::vector<double>{-5.0, 0.0}));                          // forward although only backward is allowed | no rotation
        CHECK(t.velocity == (std::vector<float>{0.5f, 0.f, 0.f}) && plan.velocity(s, 0) == (std::array<float, 3>{0.5f, 0.f, 0.f}));
        bool threw = false;
        try { plan.velocity(s, 1); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
        threw = false;
        try { gem::generateTrajectories(plan, s, 7); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);                                                             // fewer slots than the plan's max_steps
        cfg.sim_time = 0.0;
        threw = false;
        try { TrajectoryPlan bad(lim, cfg, s); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
        // a quarter turn to the left: the heading after the last step is pi / 2 within float32, the path bends to +y
        cfg.sim_time = 2.0;
        const TrajectoryState turn{{0.f, 0.f, 0.f}, {0.5f, 0.f, 0.78539816f}};
        const TrajectoryPlan arc(lim, cfg, turn);
        const gem::Trajectories a = gem::generateTrajectories(arc, turn, 9);
        CHECK(a.length == std::vector<int>{8} && a.poses.size() == 9 && a.poses[7].y > 0.3 && a.poses[7].sin_th > 0.97 && a.ext[1] == double(0.78539816f));
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
        for (int y = 0; y < 18; ++y) g[y * 40 + 30] = Costmap::LETHAL_OBSTACLE;    // a wall to the right of the start, open above row 18
        cm.write(0, 0, 40, 40, g);
        cm.prepareMapGrid({{1.05, 1.05}, {3.55, 3.55}});
        const std::vector<FootprintPoint> spec{{-0.07, -0.05}, {-0.07, 0.05}, {0.07, 0.05}, {0.07, -0.05}};
        const std::vector<Critic> critics{Critic::external(1.0, 0), Critic::obstacle(0.01), Critic::mapGrid(32.0, GEM_CRITIC_GRID_PATH),
                                          Critic::mapGrid(24.0, GEM_CRITIC_GRID_GOAL), Critic::external(0.5, 1)};
        TrajectoryLimits lim;
        lim.max_vel_x = 1.2; lim.max_vel_trans = 1.5; lim.min_vel_trans = -1.0;     // every sample is generated: the host form refuses a length of 0
        TrajectoryConfig cfg;
        cfg.vsamples[0] = 7; cfg.vsamples[1] = 3; cfg.vsamples[2] = 11;
        cfg.oscillation_flags = GEM_OSC_ROT_POS_ONLY;
        const TrajectoryState s{{1.55f, 1.05f, 0.4f}, {0.9f, 0.f, 0.1f}};
        const TrajectoryPlan plan(lim, cfg, s);
        const int T = plan.max_steps + 2;
        const gem::Trajectories tw = gem::generateTrajectories(plan, s, T);
        bool all = true;
        for (int n : tw.length) all = all && n >= 1;
        CHECK(all && plan.n_traj == 7 * 3 * 12 && plan.max_steps > 8);
        std::vector<double> want_totals, totals;
        const BestTrajectory want = cm.bestTrajectory(critics, tw.poses, T, spec, tw.ext, tw.length, &want_totals);
        const BestTrajectory got = cm.dwaBest(critics, plan, s, T, spec, &totals);
        CHECK(want.valid() && want.n_valid > 0 && want.n_valid < plan.n_traj);      // some run into the wall or turn the forbidden way
        CHECK(got.index == want.index && got.n_valid == want.n_valid && std::memcmp(&got.cost, &want.cost, sizeof(double)) == 0 && got.reserved == 0);
        CHECK(totals.size() == want_totals.size() && std::memcmp(totals.data(), want_totals.data(), totals.size() * sizeof(double)) == 0);
        const std::array<float, 3> cmd = plan.velocity(s, got.index);
        CHECK(cmd[0] == tw.velocity[3 * got.index] && cmd[1] == tw.velocity[3 * got.index + 1] && cmd[2] == tw.velocity[3 * got.index + 2]);
        const BestTrajectory again = cm.dwaBest(critics, plan, s, T, spec);           // without totals
        CHECK(again.index == want.index && again.n_valid == want.n_valid);
        bool threw = false;
        try { cm.dwaBest(critics, plan, s, plan.max_steps - 1, spec); } catch (const gem::Error& e) { threw = e.code() == GEM_ERR_INVALID; }
        CHECK(threw);
    }
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
