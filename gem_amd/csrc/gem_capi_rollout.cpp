// gem_capi_rollout.cpp -- the entry points of include/gem_hip_rollout.h: the host-only gem_rollout_plan / _host / _pick (the twin of
// the kernels, gem_rollout.hpp) and gem_costmap_rollout_best / _device.  The kernels are in gem_rollout.hip.
//
// Everything is checked on the host before anything is enqueued or written: the plan is made again from the call's own arguments and
// compared byte for byte, the PATH and GOAL grids pass critics_prepare's test (prepared, and in the costmap's present generation).
// The plan's lists, the start state, the parameters and the footprint spec travel in the kernel arguments.  The candidates' costs and
// `ahead` (Costmaps::ro_cost, ro_ahead) and the host form's answer (ro_best) come from ensure() and only grow: a second identical
// call allocates nothing.
#include "gem_costmap_host.hpp"
#include "gem_footprint.hpp"
#include "gem_rollout.hpp"

namespace {

static_assert(sizeof(gem_rollout_config) == 240 && sizeof(RolloutPlan) == 2368 && sizeof(gem_rollout_best) == 64, "the sizes the header states");
static_assert(sizeof(RolloutBest) == sizeof(gem_rollout_best), "the answer is a RolloutBest");
static_assert(kRolloutMaxList == GEM_ROLLOUT_MAX_LIST && kRolloutMaxYVels == GEM_ROLLOUT_MAX_Y_VELS && kRolloutMaxSteps == GEM_ROLLOUT_MAX_STEPS &&
              kRolloutMaxVertices == GEM_FOOTPRINT_MAX_VERTICES, "the kernels' constants are the headers'");
static_assert(kRolloutEscaping == GEM_ROLLOUT_ESCAPING && kRolloutStuckLeft == GEM_ROLLOUT_STUCK_LEFT && kRolloutStuckRight == GEM_ROLLOUT_STUCK_RIGHT &&
              kRolloutStuckLeftStrafe == GEM_ROLLOUT_STUCK_LEFT_STRAFE && kRolloutStuckRightStrafe == GEM_ROLLOUT_STUCK_RIGHT_STRAFE &&
              kRolloutStateBits == (GEM_ROLLOUT_ESCAPING | GEM_ROLLOUT_STUCK_LEFT | GEM_ROLLOUT_STUCK_RIGHT | GEM_ROLLOUT_STUCK_LEFT_STRAFE |
                                    GEM_ROLLOUT_STUCK_RIGHT_STRAFE), "rollout_pick_tail tests these bits");
static_assert(sizeof(CostGeom) + sizeof(FootSpec) + sizeof(RolloutArgs) <= 4096, "the kernel arguments");

int rollout_best(gem_handle* h, int id, const char* what, const RolloutPlan* plan, const double pos[3], const double vel[3], int state,
                 const double* spec_xy, int n_vertices, int flags, double* out_cost, int* out_ahead, gem_rollout_best* out_best, bool on_device)
{
    auto bad = [&](const char* why) { return fail(h, GEM_ERR_INVALID, (std::string(what) + ": " + why).c_str()); };
    int rc;
    CostMap* found;
    if ((rc = costmap_find(h, id, what, &found))) return rc;
    CostMap& m = *found;
    if (!out_best) return bad("out_best is NULL");
    if (state & ~kRolloutStateBits) return bad("unknown state flag bits");
    if (!rollout_spec_ok(spec_xy, n_vertices, flags)) return bad("0 .. 32 vertices and not NULL, every coordinate finite, no flag but GEM_FOOTPRINT_INSCRIBED_LETHAL");
    if (!rollout_call_ok(plan, pos, vel, state))
        return bad("a NULL argument, or a plan that gem_rollout_plan does not make from this configuration, pos, vel and state flags");
    for (int slot = 0; slot < 2; ++slot) {
        if (!m.mg_gen[slot]) return bad("the PATH or the GOAL grid was never prepared");
        if (m.mg_gen[slot] != m.gen) return bad("the PATH or the GOAL grid was prepared before the costmap last rolled or was observed");
    }
    auto& cm = h->costmap;
    const size_t nc = (size_t)plan->n_cand;
    if ((rc = ensure(h, cm.ro_cost, nc * sizeof(double))) || (rc = ensure(h, cm.ro_ahead, nc * sizeof(int)))) return rc;
    if (!on_device && (rc = ensure(h, cm.ro_best, sizeof(RolloutBest)))) return rc;
    FootSpec spec{};
    for (int i = 0; i < 2 * n_vertices; ++i) spec.xy[i] = spec_xy[i];
    spec.n = n_vertices;
    RolloutArgs a{};
    a.grid = grid_of(m);
    a.path = static_cast<const int*>(m.mg_dist[0].p); a.goal = static_cast<const int*>(m.mg_dist[1].p);
    a.cost = on_device && out_cost ? out_cost : static_cast<double*>(cm.ro_cost.p);
    a.ahead = on_device && out_ahead ? out_ahead : static_cast<int*>(cm.ro_ahead.p);
    a.out_best = on_device ? reinterpret_cast<RolloutBest*>(out_best) : static_cast<RolloutBest*>(cm.ro_best.p);
    a.p = rollout_params(*plan, pos, vel, state, flags);
    std::memcpy(a.lists, plan->lists, sizeof a.lists);
    GEM_HIP(h, launch_rollout(h->stream, geom_of(m), spec, a, plan->max_steps));
    if (on_device) return GEM_OK;
    HostXfer down[3] = {{out_best, cm.ro_best.p, sizeof(RolloutBest)}, {nullptr, nullptr, 0}, {nullptr, nullptr, 0}};
    int n_down = 1;
    if (out_cost) down[n_down++] = HostXfer{out_cost, cm.ro_cost.p, nc * sizeof(double)};
    if (out_ahead) down[n_down++] = HostXfer{out_ahead, cm.ro_ahead.p, nc * sizeof(int)};
    return download_arrays(h, down, n_down, 0);
}

} // namespace

extern "C" {

int gem_rollout_plan(const gem_rollout_config* config, const double pos[3], const double vel[3], int state_flags, struct gem_rollout_plan* out)
{
    return rollout_plan_host(config, pos, vel, state_flags, out);
}

int gem_rollout_host(const struct gem_rollout_plan* plan, const double pos[3], const double vel[3], const gem_costmap_config* geometry,
                     const unsigned char* bytes, const int* path, const int* goal, const double* spec_xy, int n_vertices, int flags,
                     double* out_cost, int* out_ahead, int* out_steps, gem_footprint_pose* out_poses, gem_rollout_best* out_best)
{
    return rollout_host(plan, pos, vel, geometry, bytes, path, goal, spec_xy, n_vertices, flags, out_cost, out_ahead, out_steps, out_poses, out_best);
}

int gem_rollout_pick(const struct gem_rollout_plan* plan, int state_flags, const double* cost, const int* ahead, gem_rollout_best* out_best)
{
    return rollout_pick_checked(plan, state_flags, cost, ahead, out_best);
}

int gem_costmap_rollout_best(gem_handle* h, int id, const struct gem_rollout_plan* plan, const double pos[3], const double vel[3], int state_flags,
                             const double* spec_xy, int n_vertices, int flags, double* out_cost, int* out_ahead, gem_rollout_best* out_best)
{
    GEM_ENTRY("gem_costmap_rollout_best");
    return rollout_best(h, id, "gem_costmap_rollout_best", plan, pos, vel, state_flags, spec_xy, n_vertices, flags, out_cost, out_ahead, out_best, false);
}

int gem_costmap_rollout_best_device(gem_handle* h, int id, const struct gem_rollout_plan* plan, const double pos[3], const double vel[3],
                                    int state_flags, const double* spec_xy, int n_vertices, int flags, double* d_out_cost, int* d_out_ahead,
                                    gem_rollout_best* d_out_best)
{
    GEM_ENTRY("gem_costmap_rollout_best_device");
    return rollout_best(h, id, "gem_costmap_rollout_best_device", plan, pos, vel, state_flags, spec_xy, n_vertices, flags, d_out_cost, d_out_ahead,
                        d_out_best, true);
}

} // extern "C"
