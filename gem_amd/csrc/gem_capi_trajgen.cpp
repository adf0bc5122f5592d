// gem_capi_trajgen.cpp -- the entry points of include/gem_hip_trajgen.h: the host-only gem_trajgen_plan / _generate / _velocity (the
// twin of the kernel, gem_trajgen.hpp), gem_trajgen_generate_device, and gem_costmap_dwa_best / _device, which generates into arenas
// of the handle and runs the critics of gem_capi_critics.cpp on them.  The kernel is in gem_trajgen.hip.
//
// Everything is checked on the host before anything is enqueued or written.  The plan's lists, the start state and the parameters
// travel in the kernel arguments.  The generated poses, lengths and external columns (Costmaps::tg_pose, tg_len, tg_ext) come from
// ensure() and only grow: a second identical call allocates nothing.
#include "gem_capi_internal.hpp"
#include "gem_critics.hpp"
#include "gem_trajgen.hpp"

namespace {

static_assert(sizeof(gem_trajgen_limits) == 88 && sizeof(gem_trajgen_config) == 64 && sizeof(gem_dwa_plan) == 1200, "the sizes the header states");
static_assert(sizeof(gem_footprint_pose) == sizeof(FootPose), "a pose is a FootPose");
static_assert(kTrajgenMaxList == GEM_TRAJGEN_MAX_LIST && kTrajgenMaxPoses == 2147483646ll, "the kernel's constants are the headers'");
static_assert(kTrajgenOscBits == (GEM_OSC_FORWARD_POS_ONLY | GEM_OSC_FORWARD_NEG_ONLY | GEM_OSC_STRAFE_POS_ONLY | GEM_OSC_STRAFE_NEG_ONLY |
                                  GEM_OSC_ROT_POS_ONLY | GEM_OSC_ROT_NEG_ONLY), "trajgen_oscillation tests these bits");

TrajgenArgs args_of(const gem_dwa_plan& pl, const float pos[3], const float vel[3], int T)
{
    TrajgenArgs a{};
    a.n_traj = pl.n_traj; a.T = T;
    a.p = trajgen_params(pl, pos, vel);
    std::memcpy(a.lists, pl.samples, sizeof a.lists);
    return a;
}

int dwa_best(gem_handle* h, int id, const char* what, const gem_critic* critics, int n_critics, const gem_dwa_plan* plan, const float pos[3],
             const float vel[3], int T, const double* spec_xy, int n_vertices, double* out_total, gem_best_trajectory* out_best, bool on_device)
{
    if (!trajgen_call_ok(plan, pos, vel, T))
        return fail(h, GEM_ERR_INVALID, (std::string(what) + ": a plan, start state or poses_per_traj that gem_trajgen_generate refuses").c_str());
    CriticsCall c{what, critics, n_critics, nullptr, nullptr, plan->n_traj, T, spec_xy, n_vertices, nullptr, 2, out_total, out_best, true, true};
    CriticsArgs ca{};
    FootSpec spec{};
    CostGeom geom{};
    int rc;
    if ((rc = critics_prepare(h, id, c, ca, spec, geom))) return rc;
    auto& cm = h->costmap;
    const size_t nt = (size_t)plan->n_traj;
    if ((rc = ensure(h, cm.tg_pose, nt * (size_t)T * sizeof(FootPose))) || (rc = ensure(h, cm.tg_len, nt * sizeof(int))) ||
        (rc = ensure(h, cm.tg_ext, 2 * nt * sizeof(double)))) return rc;
    if (!on_device) {
        if ((rc = ensure(h, cm.cr_best, sizeof(CriticsBest)))) return rc;
        if (out_total && (rc = ensure(h, cm.cr_total, nt * sizeof(double)))) return rc;
    }
    TrajgenArgs ta = args_of(*plan, pos, vel, T);
    ta.poses = static_cast<gem_footprint_pose*>(cm.tg_pose.p); ta.traj_len = static_cast<int*>(cm.tg_len.p);
    ta.ext = static_cast<double*>(cm.tg_ext.p); ta.vel_out = nullptr;
    ca.poses = static_cast<const FootPose*>(cm.tg_pose.p); ca.traj_len = static_cast<const int*>(cm.tg_len.p);
    ca.ext = static_cast<const double*>(cm.tg_ext.p);
    if (on_device) {
        ca.out_total = out_total; ca.out_best = reinterpret_cast<CriticsBest*>(out_best);
    } else {
        ca.out_total = out_total && nt ? static_cast<double*>(cm.cr_total.p) : nullptr;
        ca.out_best = static_cast<CriticsBest*>(cm.cr_best.p);
    }
    GEM_HIP(h, launch_trajgen(h->stream, ta));
    GEM_HIP(h, launch_critics(h->stream, geom, spec, ca));
    if (on_device) return GEM_OK;
    HostXfer down[2] = {{out_best, cm.cr_best.p, sizeof(CriticsBest)}, {out_total, cm.cr_total.p, nt * sizeof(double)}};
    return download_arrays(h, down, ca.out_total ? 2 : 1, 0);
}

} // namespace

extern "C" {

int gem_trajgen_plan(const gem_trajgen_limits* limits, const gem_trajgen_config* config, const float pos[3], const float vel[3],
                     const float goal[2], gem_dwa_plan* out)
{
    return trajgen_plan_host(limits, config, pos, vel, goal, out);
}

int gem_trajgen_generate(const gem_dwa_plan* plan, const float pos[3], const float vel[3], gem_footprint_pose* poses, int* traj_len,
                         double* ext, float* out_vel, int poses_per_traj)
{
    return trajgen_generate_host(plan, pos, vel, poses, traj_len, ext, out_vel, poses_per_traj);
}

int gem_trajgen_velocity(const gem_dwa_plan* plan, const float vel[3], long long index, float out_vel[3])
{
    return trajgen_velocity_host(plan, vel, index, out_vel);
}

int gem_trajgen_sincos(const double* angles, long long n, double* out_sin, double* out_cos)
{
    if (n < 0 || (n > 0 && (!angles || !out_sin || !out_cos))) return GEM_ERR_INVALID;
    for (long long i = 0; i < n; ++i) gem_sincos(angles[i], out_sin[i], out_cos[i]);
    return GEM_OK;
}

int gem_trajgen_generate_device(gem_handle* h, const gem_dwa_plan* plan, const float pos[3], const float vel[3], gem_footprint_pose* d_poses,
                                int* d_traj_len, double* d_ext, float* d_vel, int poses_per_traj)
{
    GEM_ENTRY("gem_trajgen_generate_device");
    if (h->tp_x) return fail(h, GEM_ERR_INVALID, "gem_trajgen_generate_device: not on a handle with a communicator");
    if (!trajgen_call_ok(plan, pos, vel, poses_per_traj))
        return fail(h, GEM_ERR_INVALID, "gem_trajgen_generate_device: a plan gem_trajgen_plan did not make, a start state that is not finite, poses_per_traj "
                                        "outside 1 .. 2^20 or below the plan's max_steps, more than 2^31 - 2 pose slots, or |theta| beyond 64 pi");
    if (plan->n_traj > 0 && (!d_poses || !d_traj_len || !d_ext)) return fail(h, GEM_ERR_INVALID, "gem_trajgen_generate_device: a NULL array with a non-zero count");
    TrajgenArgs a = args_of(*plan, pos, vel, poses_per_traj);
    a.poses = d_poses; a.traj_len = d_traj_len; a.ext = d_ext; a.vel_out = d_vel;
    GEM_HIP(h, launch_trajgen(h->stream, a));
    return GEM_OK;
}

int gem_costmap_dwa_best(gem_handle* h, int id, const gem_critic* critics, int n_critics, const gem_dwa_plan* plan, const float pos[3],
                         const float vel[3], int poses_per_traj, const double* spec_xy, int n_vertices, double* out_total,
                         gem_best_trajectory* out_best)
{
    GEM_ENTRY("gem_costmap_dwa_best");
    return dwa_best(h, id, "gem_costmap_dwa_best", critics, n_critics, plan, pos, vel, poses_per_traj, spec_xy, n_vertices, out_total, out_best, false);
}

int gem_costmap_dwa_best_device(gem_handle* h, int id, const gem_critic* critics, int n_critics, const gem_dwa_plan* plan, const float pos[3],
                                const float vel[3], int poses_per_traj, const double* spec_xy, int n_vertices, double* d_out_total,
                                gem_best_trajectory* d_out_best)
{
    GEM_ENTRY("gem_costmap_dwa_best_device");
    return dwa_best(h, id, "gem_costmap_dwa_best_device", critics, n_critics, plan, pos, vel, poses_per_traj, spec_xy, n_vertices, d_out_total,
                    d_out_best, true);
}

} // extern "C"
