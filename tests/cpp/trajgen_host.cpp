// The host restatement of the trajectory-generation contract on its own: gem_amd/csrc/gem_trajgen.hpp and gem_sincos.hpp compiled by a
// plain C++ compiler, without HIP and without the library.  A stand-alone program, so that it can be built with
// -fsanitize=address,undefined: it walks plans of every shape through plan, generate and velocity with buffers of exactly the size the
// contract states (a write past a slot is a heap overflow), refuses what must be refused, and checks a few known answers.
#include "../../gem_amd/csrc/gem_trajgen.hpp"

#include <cstdio>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main()
{
    using namespace gem;
    gem_trajgen_limits lim{0.55, 0.0, 0.1, -0.1, 1.0, 0.4, 0.55, 0.1, 2.5, 2.5, 3.2};
    long long poses_written = 0;
    for (int dwa = 0; dwa < 2; ++dwa)
        for (int by_time = 0; by_time < 2; ++by_time)
            for (int nx = -1; nx <= 9; nx += 2)
                for (int nth = 1; nth <= 21; nth += 5) {
                    gem_trajgen_config cfg{1.7, 0.025, 0.1, 0.05, dwa, by_time, !dwa, 21, {nx, 3, nth}, 0};
                    const float pos[3] = {1.f, 2.f, 3.1f}, vel[3] = {0.2f, 0.05f, -0.1f}, goal[2] = {3.f, 3.5f};
                    gem_dwa_plan plan;
                    CHECK(trajgen_plan_host(&lim, &cfg, pos, vel, goal, &plan) == GEM_OK);
                    CHECK(trajgen_plan_ok(plan) && plan.n_x + plan.n_y + plan.n_th <= GEM_TRAJGEN_MAX_LIST);
                    const int T = plan.max_steps > 0 ? plan.max_steps : 1;
                    const size_t n = static_cast<size_t>(plan.n_traj);
                    std::vector<gem_footprint_pose> poses(n * static_cast<size_t>(T));
                    std::vector<int> len(n);
                    std::vector<double> ext(2 * n);
                    std::vector<float> v(3 * n);
                    CHECK(trajgen_generate_host(&plan, pos, vel, poses.data(), len.data(), ext.data(), v.data(), T) == GEM_OK);
                    if (plan.max_steps > 1) CHECK(trajgen_generate_host(&plan, pos, vel, poses.data(), len.data(), ext.data(), v.data(), T - 1) == GEM_ERR_INVALID);
                    for (size_t t = 0; t < n; ++t) {
                        CHECK(len[t] >= 0 && len[t] <= T);
                        poses_written += len[t];
                        float w[3];
                        CHECK(trajgen_velocity_host(&plan, vel, static_cast<long long>(t), w) == GEM_OK && w[0] == v[3 * t] && w[1] == v[3 * t + 1] && w[2] == v[3 * t + 2]);
                        CHECK(ext[t] == 0.0 || ext[t] == -5.0);
                        CHECK(ext[n + t] == std::fabs(static_cast<double>(v[3 * t + 2])));
                    }
                    float w[3];
                    CHECK(trajgen_velocity_host(&plan, vel, plan.n_traj, w) == GEM_ERR_INVALID && trajgen_velocity_host(&plan, vel, -1, w) == GEM_ERR_INVALID);
                }
    CHECK(poses_written > 10000);
    {   // the list limit: 100 + 101 + 57 values do not fit, and nothing is written past the plan
        gem_trajgen_config cfg{1.7, 0.025, 0.1, 0.05, 1, 0, 0, 0, {100, 100, 56}, 0};
        const float pos[3] = {0.f, 0.f, 0.f}, vel[3] = {0.2f, 0.f, 0.1f}, goal[2] = {0.f, 0.f};
        gem_dwa_plan plan;
        plan.n_traj = -9;
        CHECK(trajgen_plan_host(&lim, &cfg, pos, vel, goal, &plan) == GEM_ERR_INVALID && plan.n_traj == -9);
        cfg.vsamples[0] = 2147483647;
        CHECK(trajgen_plan_host(&lim, &cfg, pos, vel, goal, &plan) == GEM_ERR_INVALID);
    }
    {   // the cosine: exact at 0, the quadrants' signs, the identity within a few ulps up to the contract's bound
        double s, c;
        gem_sincos(0.0, s, c);
        CHECK(s == 0.0 && c == 1.0);
        for (int i = -4000; i <= 4000; ++i) {
            const double t = i * 0.0502654824574;                    // up to +-64 pi
            gem_sincos(t, s, c);
            CHECK(std::fabs(s * s + c * c - 1.0) < 1e-15 && std::fabs(s - std::sin(t)) <= 0x1p-52 && std::fabs(c - std::cos(t)) <= 0x1p-52);
        }
    }
    std::printf(fails ? "FAILED\n" : "ok\n");
    return fails ? 1 : 0;
}
