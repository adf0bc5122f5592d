// gem_capi_footprint.cpp -- the footprint entry points of include/gem_hip_footprint.h: clearing the robot's footprint out of a layer
// (updateFootprint + setConvexPolygonCost) and CostmapModel::footprintCost for batches of poses and whole trajectories.  The kernels
// are in gem_footprint.hip.
//
// The specification travels in the kernel arguments.  gem_costmap_clear_footprint computes the transformed vertices, the touched
// bounds, the vertex cells and `ok` on the host in plain C++ (it knows the geometry after rolling) and only enqueues the fill.  The
// host-array forms of the scoring calls stage their poses and results in Costmaps::fp_pose / fp_cost / fp_traj, which come from
// ensure(): gem_debug_get("arena_allocations") counts them, and a loop that has reached its sizes allocates nothing.
#include "gem_costmap_host.hpp"
#include "gem_footprint.hpp"

namespace {

constexpr long long kMaxPoses = 2147483646ll;                       // 2^31 - 2
constexpr int kMaxPosesPerTraj = 1 << 20;
constexpr int kKnownFlags = GEM_FOOTPRINT_INSCRIBED_LETHAL | GEM_FOOTPRINT_SUM;
static_assert(sizeof(gem_footprint_pose) == 32 && sizeof(FootPose) == 32, "a pose is four packed doubles");
static_assert(kFootMaxVertices == GEM_FOOTPRINT_MAX_VERTICES, "the kernels' vertex limit is the header's");

int check_spec(gem_handle* h, const char* what, const double* spec_xy, int n_vertices, FootSpec* out)
{
    if (n_vertices < 0 || n_vertices > kFootMaxVertices || (n_vertices > 0 && !spec_xy))
        return fail(h, GEM_ERR_INVALID, (std::string(what) + ": 0 .. 32 vertices, and not NULL").c_str());
    *out = FootSpec{};
    for (int i = 0; i < 2 * n_vertices; ++i) {
        if (!std::isfinite(spec_xy[i])) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": a spec coordinate is not finite").c_str());
        out->xy[i] = spec_xy[i];
    }
    out->n = n_vertices;
    return GEM_OK;
}

struct ScoreCall {
    const char* what;
    const gem_footprint_pose* poses;
    long long n_traj;
    int T;
    int* pose_cost;                     // nullable
    int* traj_cost;
    bool on_device;
};

int score(gem_handle* h, int id, const ScoreCall& c, const double* spec_xy, int n_vertices, int flags)
{
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, c.what, &m))) return rc;
    if (c.T < 1 || c.T > kMaxPosesPerTraj) return fail(h, GEM_ERR_INVALID, (std::string(c.what) + ": poses_per_traj outside 1 .. 2^20").c_str());
    if (c.n_traj < 0 || c.n_traj > kMaxPoses / c.T) return fail(h, GEM_ERR_INVALID, (std::string(c.what) + ": a negative count, or more than 2^31 - 2 poses").c_str());
    if (flags & ~kKnownFlags) return fail(h, GEM_ERR_INVALID, (std::string(c.what) + ": unknown flag bits").c_str());
    FootSpec spec;
    if ((rc = check_spec(h, c.what, spec_xy, n_vertices, &spec))) return rc;
    if (c.n_traj > 0 && (!c.poses || !c.traj_cost)) return fail(h, GEM_ERR_INVALID, (std::string(c.what) + ": a NULL array with a non-zero count").c_str());
    if (c.n_traj == 0) return GEM_OK;

    const size_t n_poses = (size_t)c.n_traj * (size_t)c.T;
    FootScoreArgs a{};
    a.n_traj = c.n_traj; a.T = c.T;
    a.inscribed_lethal = (flags & GEM_FOOTPRINT_INSCRIBED_LETHAL) ? 1 : 0;
    a.sum = (flags & GEM_FOOTPRINT_SUM) ? 1 : 0;
    if (c.on_device) {
        a.poses = reinterpret_cast<const FootPose*>(c.poses); a.pose_cost = c.pose_cost; a.traj_cost = c.traj_cost;
        GEM_HIP(h, launch_foot_score(h->stream, geom_of(*m), grid_of(*m), spec, a));
        return GEM_OK;
    }
    auto& cm = h->costmap;
    if ((rc = ensure(h, cm.fp_pose, n_poses * sizeof(FootPose))) || (rc = ensure(h, cm.fp_traj, (size_t)c.n_traj * sizeof(int)))) return rc;
    if (c.pose_cost && (rc = ensure(h, cm.fp_cost, n_poses * sizeof(int)))) return rc;
    HostXfer up{const_cast<gem_footprint_pose*>(c.poses), cm.fp_pose.p, n_poses * sizeof(FootPose)};
    if ((rc = upload_arrays(h, &up, 1))) return rc;
    a.poses = static_cast<const FootPose*>(cm.fp_pose.p);
    a.pose_cost = c.pose_cost ? static_cast<int*>(cm.fp_cost.p) : nullptr;
    a.traj_cost = static_cast<int*>(cm.fp_traj.p);
    GEM_HIP(h, launch_foot_score(h->stream, geom_of(*m), grid_of(*m), spec, a));
    HostXfer down[2] = {{c.traj_cost, cm.fp_traj.p, (size_t)c.n_traj * sizeof(int)}, {c.pose_cost, cm.fp_cost.p, n_poses * sizeof(int)}};
    return download_arrays(h, down, c.pose_cost ? 2 : 1, 0);
}

} // namespace

extern "C" {

int gem_costmap_clear_footprint(gem_handle* h, int id, const gem_footprint_pose* pose, const double* spec_xy, int n_vertices,
                                double bounds[4], int* out_ok)
{
    GEM_ENTRY("gem_costmap_clear_footprint");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_clear_footprint", &m))) return rc;
    FootSpec spec;
    if ((rc = check_spec(h, "gem_costmap_clear_footprint", spec_xy, n_vertices, &spec))) return rc;
    if (!pose || !std::isfinite(pose->x) || !std::isfinite(pose->y) || !std::isfinite(pose->cos_th) || !std::isfinite(pose->sin_th))
        return fail(h, GEM_ERR_INVALID, "gem_costmap_clear_footprint: the pose is NULL or not finite");
    const FootPose P{pose->x, pose->y, pose->cos_th, pose->sin_th};
    const CostGeom g = geom_of(*m);
    FootCells c{};
    c.n = spec.n;
    c.min_x = c.min_y = ~0u;
    bool on_map = true;
    for (int i = 0; i < spec.n; ++i) {
        double wx, wy;
        foot_vertex(P, spec.xy[2 * i], spec.xy[2 * i + 1], wx, wy);
        if (bounds) {                                                   // touch(): *min_x = std::min(px, *min_x), ...
            bounds[0] = std::min(wx, bounds[0]); bounds[1] = std::min(wy, bounds[1]);
            bounds[2] = std::max(wx, bounds[2]); bounds[3] = std::max(wy, bounds[3]);
        }
        uint32_t mx = 0u, my = 0u;
        if (!cost_cell_xy(g, wx, wy, mx, my)) { on_map = false; continue; }
        c.x[i] = mx; c.y[i] = my;
        c.min_x = std::min(c.min_x, mx); c.max_x = std::max(c.max_x, mx);
        c.min_y = std::min(c.min_y, my); c.max_y = std::max(c.max_y, my);
    }
    if (out_ok) *out_ok = (spec.n < 3 || on_map) ? 1 : 0;
    if (spec.n < 3 || !on_map) return GEM_OK;                           // setConvexPolygonCost: nothing to fill / returns false
    GEM_HIP(h, launch_foot_clear(h->stream, grid_of(*m), g.sx, g.sy, c));
    return GEM_OK;
}

int gem_costmap_footprint_cost(gem_handle* h, int id, const gem_footprint_pose* poses, long long n, const double* spec_xy,
                               int n_vertices, int flags, int* out_cost)
{
    GEM_ENTRY("gem_costmap_footprint_cost");
    return score(h, id, ScoreCall{"gem_costmap_footprint_cost", poses, n, 1, nullptr, out_cost, false}, spec_xy, n_vertices, flags);
}

int gem_costmap_footprint_cost_device(gem_handle* h, int id, const gem_footprint_pose* d_poses, long long n, const double* spec_xy,
                                      int n_vertices, int flags, int* d_out_cost)
{
    GEM_ENTRY("gem_costmap_footprint_cost_device");
    return score(h, id, ScoreCall{"gem_costmap_footprint_cost_device", d_poses, n, 1, nullptr, d_out_cost, true}, spec_xy, n_vertices, flags);
}

int gem_costmap_score_trajectories(gem_handle* h, int id, const gem_footprint_pose* poses, long long n_traj, int poses_per_traj,
                                   const double* spec_xy, int n_vertices, int flags, int* out_pose_cost, int* out_traj_cost)
{
    GEM_ENTRY("gem_costmap_score_trajectories");
    return score(h, id, ScoreCall{"gem_costmap_score_trajectories", poses, n_traj, poses_per_traj, out_pose_cost, out_traj_cost, false},
                 spec_xy, n_vertices, flags);
}

int gem_costmap_score_trajectories_device(gem_handle* h, int id, const gem_footprint_pose* d_poses, long long n_traj, int poses_per_traj,
                                          const double* spec_xy, int n_vertices, int flags, int* d_out_pose_cost, int* d_out_traj_cost)
{
    GEM_ENTRY("gem_costmap_score_trajectories_device");
    return score(h, id, ScoreCall{"gem_costmap_score_trajectories_device", d_poses, n_traj, poses_per_traj, d_out_pose_cost, d_out_traj_cost, true},
                 spec_xy, n_vertices, flags);
}

} // extern "C"
