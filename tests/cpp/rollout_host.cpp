// The host restatement of the rollout contract on its own: gem_amd/csrc/gem_rollout.hpp and gem_sincos.hpp compiled by a plain C++
// compiler, without HIP and without the library.  A stand-alone program, so that it can be built with -fsanitize=address,undefined: it
// walks plans of every shape through plan, the trajectories and the pick with buffers of exactly the size the contract states (a write
// past a slot is a heap overflow), over maps whose edges and blocked cells the candidates run into, refuses what must be refused, and
// checks a few known answers.
#include "../../gem_amd/csrc/gem_rollout.hpp"

#include <cstdio>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main()
{
    using namespace gem;
    const gem_rollout_config base{1.0, 0.025, 0.025, 0.05, 0.6, 0.8, 0.01, 0.325, 0.5, 0.1, 1.0, -1.0, 0.4, -0.1, 2.5, 2.5, 3.2, 0.0, 0.0,
                                  3, 20, 1, 1, 0, 4, {-0.3, -0.1, 0.1, 0.3, 0.0, 0.0, 0.0, 0.0}};
    // a 23 x 17 map at 0.1 with a seeded pattern of costs, lethal, inscribed and unknown cells; PATH / GOAL with OB and UN cells among them
    const unsigned sx = 23, sy = 17;
    const gem_costmap_config geom{sx, sy, 0.1, -0.4, 0.3, 0};
    std::vector<unsigned char> bytes(sx * sy);
    std::vector<int> path(sx * sy), goal(sx * sy);
    unsigned long long seed = 12345;
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(seed >> 33); };
    for (unsigned i = 0; i < sx * sy; ++i) {
        const unsigned r = next() % 100;
        bytes[i] = r < 4 ? 254 : (r < 7 ? 253 : (r < 9 ? 255 : (unsigned char)(next() % 253)));
        path[i] = r >= 95 ? (int)(sx * sy) + (int)(r & 1) : (int)(next() % 60);
        goal[i] = r >= 93 && r < 95 ? (int)(sx * sy) + 1 : (int)(next() % 60);
    }
    const double specs[3][8] = {{0}, {0.12, 0.0, -0.08, 0.08, -0.08, -0.08, 0, 0}, {-0.17, -0.11, -0.17, 0.11, 0.17, 0.11, 0.17, -0.11}};
    const int spec_n[3] = {0, 3, 4};
    long long legal = 0, minus1 = 0, minus2 = 0, recorded = 0;
    int stages[4] = {0, 0, 0, 0};
    for (int state = 0; state < 32; state += 3)
        for (int nx = 2; nx <= 8; nx += 3)
            for (int nth = 2; nth <= 20; nth += 9)
                for (int k = 0; k < 6; ++k) {
                    gem_rollout_config cfg = base;
                    cfg.vx_samples = nx; cfg.vtheta_samples = nth; cfg.dwa = k & 1; cfg.holonomic_robot = (k >> 1) & 1; cfg.final_goal_valid = k == 5;
                    cfg.final_goal_x = 0.9; cfg.final_goal_y = 1.1;
                    const double pos[3] = {-0.35 + 0.37 * k, 0.4 + 0.25 * k, -3.0 + 1.1 * k}, vel[3] = {0.1 * k, 0.0, 0.3 - 0.1 * k};
                    RolloutPlan plan;
                    CHECK(rollout_plan_host(&cfg, pos, vel, state, &plan) == GEM_OK);
                    CHECK(plan.n_cand == plan.off_d + 1 && plan.max_steps >= 1 && plan.max_steps <= GEM_ROLLOUT_MAX_STEPS && rollout_call_ok(&plan, pos, vel, state));
                    const size_t n = (size_t)plan.n_cand;
                    std::vector<double> cost(n);
                    std::vector<int> ahead(n), steps(n);
                    std::vector<gem_footprint_pose> poses(n * (size_t)plan.max_steps);
                    gem_rollout_best best, again;
                    const int s = k % 3;
                    CHECK(rollout_host(&plan, pos, vel, &geom, bytes.data(), path.data(), goal.data(), spec_n[s] ? specs[s] : nullptr, spec_n[s], k & 1,
                                       cost.data(), ahead.data(), steps.data(), poses.data(), &best) == GEM_OK);
                    CHECK(rollout_pick_checked(&plan, state, cost.data(), ahead.data(), &again) == GEM_OK && std::memcmp(&best, &again, sizeof best) == 0);
                    CHECK(best.stage >= 1 && best.stage <= 3 && best.index >= 0 && best.index < plan.n_cand && (best.stage == 3) == (best.index == plan.off_d));
                    ++stages[best.stage];
                    for (size_t c = 0; c < n; ++c) {
                        CHECK(steps[c] >= 0 && steps[c] <= plan.max_steps && (cost[c] >= 0 || cost[c] == -1.0 || cost[c] == -2.0));
                        CHECK(cost[c] >= 0 || ahead[c] == -1);
                        legal += cost[c] >= 0; minus1 += cost[c] == -1.0; minus2 += cost[c] == -2.0; recorded += steps[c];
                    }
                    RolloutPlan other = plan;
                    other.max_steps += 1;
                    CHECK(rollout_host(&other, pos, vel, &geom, bytes.data(), path.data(), goal.data(), nullptr, 0, 0, cost.data(), ahead.data(), steps.data(),
                                       nullptr, &best) == GEM_ERR_INVALID);
                }
    CHECK(legal > 1000 && minus1 > 1000 && minus2 > 100 && recorded > 10000 && stages[1] > 0 && stages[3] > 0);
    {   // the limits: 128 + 128 list values fit, 129 + 128 do not, and nothing is written past the plan
        gem_rollout_config cfg = base;
        const double pos[3] = {0.0, 0.0, 0.0}, vel[3] = {0.2, 0.0, 0.1};
        RolloutPlan plan;
        cfg.vx_samples = 128; cfg.vtheta_samples = 128;
        CHECK(rollout_plan_host(&cfg, pos, vel, 0, &plan) == GEM_OK && plan.n_cand == 128 * 128 + 2 + 128 + 4 + 1);
        plan.n_cand = -9;
        cfg.vx_samples = 129;
        CHECK(rollout_plan_host(&cfg, pos, vel, 0, &plan) == GEM_ERR_INVALID && plan.n_cand == -9);
        cfg.vx_samples = 2147483647;
        CHECK(rollout_plan_host(&cfg, pos, vel, 0, &plan) == GEM_ERR_INVALID);
        cfg = base; cfg.sim_granularity = 1e-5;
        CHECK(rollout_plan_host(&cfg, pos, vel, 0, &plan) == GEM_ERR_INVALID);     // more than GEM_ROLLOUT_MAX_STEPS steps
        cfg = base; cfg.sim_granularity = 1e-300;
        CHECK(rollout_plan_host(&cfg, pos, vel, 0, &plan) == GEM_ERR_INVALID);     // a step count beyond int
        cfg = base; cfg.occdist_scale = -0.0;
        CHECK(rollout_plan_host(&cfg, pos, vel, 0, &plan) == GEM_ERR_INVALID);
    }
    {   // known answers: the steps rule on both sides of a half, the floor of one, the clamped velocity update
        RolloutParams p{};
        p.sim_time = 1.0; p.gran = 0.125; p.ang_gran = 0.125;
        CHECK(rollout_steps(p, 0.3125, 0.0, 0.0) == 3 && rollout_steps(p, std::nextafter(0.3125, 0.0), 0.0, 0.0) == 2 && rollout_steps(p, 0.0, 0.0, 0.0) == 1);
        p.sim_time = 2.0;
        CHECK(rollout_steps(p, 0.0, 0.0, -0.3125) == 3 && rollout_steps(p, 0.0, 0.3125, 0.0) == 5);           // no sim_time in the angular term
        CHECK(rollout_new_velocity(0.5, 0.2, 1.0, 0.1) == 0.2 + 1.0 * 0.1 && rollout_new_velocity(0.5, 0.45, 1.0, 0.1) == 0.5);
        CHECK(rollout_new_velocity(-0.5, 0.2, 1.0, 0.1) == 0.2 - 1.0 * 0.1 && rollout_new_velocity(0.2, 0.2, 1.0, 0.1) == 0.2);
        CHECK(rollout_limited(0.1, 0.4) == 0.4 && rollout_limited(-0.1, 0.4) == -0.4 && rollout_limited(0.7, 0.4) == 0.7 && rollout_limited(0.0, 0.4) == -0.4);
    }
    std::printf(fails ? "FAILED\n" : "ok\n");
    return fails ? 1 : 0;
}
