// gem_capi_critics.cpp -- the best-trajectory entry points of include/gem_hip_critics.h: gem_costmap_best_trajectory / _device and the
// host-only gem_critics_select.  The kernels are in gem_critics.hip; the FRONT grid's entries are with the other grids in
// gem_capi_mapgrid.cpp.  critics_prepare -- the checks and the argument block -- is shared with gem_costmap_dwa_best (gem_capi_trajgen.cpp).
//
// Everything is checked on the host before anything is enqueued or written.  The critic list and the footprint spec travel in the
// kernel arguments.  The first pass's candidates (Costmaps::cr_cand) and the host-array form's staging (cr_pose, cr_len, cr_ext,
// cr_total, cr_best) come from ensure() and only grow: gem_debug_get("arena_allocations") counts them, and a second identical call
// allocates nothing.
#include "gem_costmap_host.hpp"
#include "gem_critics.hpp"

#include <cmath>
#include <cstring>

namespace {

constexpr long long kMaxPoses = 2147483646ll;                       // 2^31 - 2
constexpr int kMaxPosesPerTraj = 1 << 20;
constexpr int kObstacleFlags = GEM_FOOTPRINT_INSCRIBED_LETHAL | GEM_FOOTPRINT_SUM | GEM_CRITIC_CENTRE_COST;
constexpr int kMapGridFlags = GEM_MAPGRID_STOP_ON_FAILURE | GEM_MAPGRID_SUM;
static_assert(sizeof(gem_critic) == 32 && sizeof(CriticDev) == 32, "a critic is 32 bytes");
static_assert(sizeof(gem_best_trajectory) == 32 && sizeof(CriticsBest) == 32, "the result is 32 bytes");
static_assert(kCriticsMax == GEM_CRITIC_MAX && kCriticObstacle == GEM_CRITIC_OBSTACLE && kCriticMapGrid == GEM_CRITIC_MAPGRID &&
              kCriticExternal == GEM_CRITIC_EXTERNAL && kCriticCentreCost == GEM_CRITIC_CENTRE_COST, "the kernel's constants are the header's");
static_assert(GEM_CRITIC_GRID_PATH == GEM_MAPGRID_PATH && GEM_CRITIC_GRID_GOAL == GEM_MAPGRID_GOAL, "the first two grids are the MapGrid calls'");
static_assert(GEM_FOOTPRINT_INSCRIBED_LETHAL == 1 && GEM_FOOTPRINT_SUM == 2 && GEM_MAPGRID_STOP_ON_FAILURE == 1 && GEM_MAPGRID_SUM == 2,
              "k_critics tests these bits");

// the combination of one trajectory over the scores the caller holds: SimpleScoredSamplingPlanner::scoreTrajectory without its early exit
double combine(const gem_critic* c, int n_critics, const double* scores, long long n_traj, long long t)
{
    double total = 0.0;
    for (int k = 0; k < n_critics; ++k) {
        if (c[k].scale == 0.0) continue;
        double s = scores[(long long)k * n_traj + t];
        if (s < 0.0) { total = s; break; }
        if (s != 0.0) s = s * c[k].scale;
        total = total + s;
    }
    return total;
}

bool scale_ok(double s) { return std::isfinite(s) && s >= 0.0; }

using Call = CriticsCall;

int bad(gem_handle* h, const Call& c, const char* why) { return fail(h, GEM_ERR_INVALID, (std::string(c.what) + ": " + why).c_str()); }

} // namespace

// the checks of a best-trajectory call, the candidates' arena and the kernel's argument block with everything but the caller's arrays
int gemi::critics_prepare(gem_handle* h, int id, const CriticsCall& c, CriticsArgs& a, FootSpec& spec, CostGeom& geom)
{
    int rc;
    CostMap* found;
    if ((rc = costmap_find(h, id, c.what, &found))) return rc;
    CostMap& m = *found;
    if (c.n_critics < 1 || c.n_critics > GEM_CRITIC_MAX || !c.critics) return bad(h, c, "1 .. GEM_CRITIC_MAX critics, and not NULL");
    if (c.T < 1 || c.T > kMaxPosesPerTraj) return bad(h, c, "poses_per_traj outside 1 .. 2^20");
    if (c.n_traj < 0 || c.n_traj > kMaxPoses / c.T) return bad(h, c, "a negative count, or more than 2^31 - 2 poses");
    if (c.n_ext < 0) return bad(h, c, "a negative column count");
    if (!c.out_best) return bad(h, c, "out_best is NULL");
    if (c.n_traj > 0 && !c.poses && !c.own_arrays) return bad(h, c, "a NULL array with a non-zero count");

    a = CriticsArgs{};
    spec = FootSpec{};
    int obstacles = 0;
    for (int k = 0; k < c.n_critics; ++k) {
        const gem_critic& q = c.critics[k];
        CriticDev& d = a.c[k];
        if (!scale_ok(q.scale)) return bad(h, c, "a scale negative or not finite");
        d.kind = q.kind; d.flags = q.flags; d.scale = q.scale;
        if (q.kind == GEM_CRITIC_OBSTACLE) {
            if (q.flags & ~kObstacleFlags) return bad(h, c, "unknown flag bits of an OBSTACLE critic");
            if (++obstacles > 1) return bad(h, c, "more than one OBSTACLE critic");
            if (c.n_vertices < 0 || c.n_vertices > kFootMaxVertices || (c.n_vertices > 0 && !c.spec_xy)) return bad(h, c, "0 .. 32 vertices, and not NULL");
            for (int i = 0; i < 2 * c.n_vertices; ++i) {
                if (!std::isfinite(c.spec_xy[i])) return bad(h, c, "a spec coordinate is not finite");
                spec.xy[i] = c.spec_xy[i];
            }
            spec.n = c.n_vertices;
        } else if (q.kind == GEM_CRITIC_MAPGRID) {
            if (q.flags & ~kMapGridFlags) return bad(h, c, "unknown flag bits of a MAPGRID critic");
            const int slot = q.grid == GEM_CRITIC_GRID_PATH ? 0 : (q.grid == GEM_CRITIC_GRID_GOAL ? 1 : (q.grid == GEM_CRITIC_GRID_FRONT ? 2 : -1));
            if (slot < 0) return bad(h, c, "a MAPGRID critic's grid is GEM_CRITIC_GRID_PATH, _GOAL or _FRONT");
            if (!std::isfinite(q.xshift)) return bad(h, c, "xshift not finite");
            if (!m.mg_gen[slot]) return bad(h, c, "a critic's grid was never prepared");
            if (m.mg_gen[slot] != m.gen) return bad(h, c, "a critic's grid was prepared before the costmap last rolled or was observed");
            d.grid = slot; d.xshift = q.xshift;
        } else if (q.kind == GEM_CRITIC_EXTERNAL) {
            if (q.flags) return bad(h, c, "unknown flag bits of an EXTERNAL critic");
            if (q.column < 0 || q.column >= c.n_ext) return bad(h, c, "an EXTERNAL critic's column outside 0 .. n_ext_columns - 1");
            if (c.n_traj > 0 && !c.ext && !c.own_arrays) return bad(h, c, "a NULL array with a non-zero count");
            d.column = q.column;
        } else {
            return bad(h, c, "an unknown kind of critic");
        }
    }
    if (!c.on_device && c.traj_len)
        for (long long t = 0; t < c.n_traj; ++t)
            if (c.traj_len[t] < 1 || c.traj_len[t] > c.T) return bad(h, c, "a length outside 1 .. poses_per_traj");

    auto& cm = h->costmap;
    if ((rc = ensure(h, cm.cr_cand, (size_t)kCriticsMaxBlocks * sizeof(CriticsCandidate)))) return rc;
    a.grid = grid_of(m);
    for (int s = 0; s < 3; ++s) a.dist[s] = static_cast<const int*>(m.mg_dist[s].p);
    a.cand = static_cast<CriticsCandidate*>(cm.cr_cand.p);
    a.n_traj = c.n_traj; a.T = c.T; a.n_critics = c.n_critics;
    geom = geom_of(m);
    return GEM_OK;
}

namespace {

int best(gem_handle* h, int id, const Call& c)
{
    CriticsArgs a{};
    FootSpec spec{};
    CostGeom geom{};
    int rc;
    if ((rc = critics_prepare(h, id, c, a, spec, geom))) return rc;
    auto& cm = h->costmap;
    if (c.on_device) {
        a.poses = reinterpret_cast<const FootPose*>(c.poses); a.traj_len = c.traj_len; a.ext = c.ext;
        a.out_total = c.out_total; a.out_best = reinterpret_cast<CriticsBest*>(c.out_best);
        GEM_HIP(h, launch_critics(h->stream, geom, spec, a));
        return GEM_OK;
    }
    const size_t nt = (size_t)c.n_traj, pose_bytes = nt * (size_t)c.T * sizeof(FootPose);
    const size_t ext_bytes = c.ext ? (size_t)c.n_ext * nt * sizeof(double) : 0;
    if ((rc = ensure(h, cm.cr_best, sizeof(CriticsBest))) || (rc = ensure(h, cm.cr_pose, pose_bytes)) || (rc = ensure(h, cm.cr_ext, ext_bytes))) return rc;
    if (c.traj_len && (rc = ensure(h, cm.cr_len, nt * sizeof(int)))) return rc;
    if (c.out_total && (rc = ensure(h, cm.cr_total, nt * sizeof(double)))) return rc;
    HostXfer up[3];
    int n_up = 0;
    if (nt) up[n_up++] = HostXfer{const_cast<gem_footprint_pose*>(c.poses), cm.cr_pose.p, pose_bytes};
    if (nt && ext_bytes) up[n_up++] = HostXfer{const_cast<double*>(c.ext), cm.cr_ext.p, ext_bytes};
    if (nt && c.traj_len) up[n_up++] = HostXfer{const_cast<int*>(c.traj_len), cm.cr_len.p, nt * sizeof(int)};
    if (n_up && (rc = upload_arrays(h, up, n_up))) return rc;
    a.poses = static_cast<const FootPose*>(cm.cr_pose.p);
    a.traj_len = c.traj_len && nt ? static_cast<const int*>(cm.cr_len.p) : nullptr;
    a.ext = static_cast<const double*>(cm.cr_ext.p);
    a.out_total = c.out_total && nt ? static_cast<double*>(cm.cr_total.p) : nullptr;
    a.out_best = static_cast<CriticsBest*>(cm.cr_best.p);
    GEM_HIP(h, launch_critics(h->stream, geom, spec, a));
    HostXfer down[2] = {{c.out_best, cm.cr_best.p, sizeof(CriticsBest)}, {c.out_total, cm.cr_total.p, nt * sizeof(double)}};
    return download_arrays(h, down, a.out_total ? 2 : 1, 0);
}

} // namespace

extern "C" {

int gem_costmap_best_trajectory(gem_handle* h, int id, const gem_critic* critics, int n_critics, const gem_footprint_pose* poses,
                                const int* traj_len, long long n_traj, int poses_per_traj, const double* spec_xy, int n_vertices,
                                const double* ext, int n_ext_columns, double* out_total, gem_best_trajectory* out_best)
{
    GEM_ENTRY("gem_costmap_best_trajectory");
    return best(h, id, Call{"gem_costmap_best_trajectory", critics, n_critics, poses, traj_len, n_traj, poses_per_traj, spec_xy, n_vertices,
                            ext, n_ext_columns, out_total, out_best, false});
}

int gem_costmap_best_trajectory_device(gem_handle* h, int id, const gem_critic* critics, int n_critics, const gem_footprint_pose* d_poses,
                                       const int* d_traj_len, long long n_traj, int poses_per_traj, const double* spec_xy, int n_vertices,
                                       const double* d_ext, int n_ext_columns, double* d_out_total, gem_best_trajectory* d_out_best)
{
    GEM_ENTRY("gem_costmap_best_trajectory_device");
    return best(h, id, Call{"gem_costmap_best_trajectory_device", critics, n_critics, d_poses, d_traj_len, n_traj, poses_per_traj, spec_xy,
                            n_vertices, d_ext, n_ext_columns, d_out_total, d_out_best, true});
}

int gem_critics_select(const gem_critic* critics, int n_critics, const double* scores, long long n_traj, double* out_total,
                       gem_best_trajectory* out_best)
{
    if (n_critics < 1 || n_critics > GEM_CRITIC_MAX || !critics || !out_best || n_traj < 0 || (n_traj > 0 && !scores)) return GEM_ERR_INVALID;
    for (int k = 0; k < n_critics; ++k) if (!scale_ok(critics[k].scale)) return GEM_ERR_INVALID;
    gem_best_trajectory b{-1, 0, -1.0, 0};
    for (long long t = 0; t < n_traj; ++t) {                            // findBestTrajectory: strict <, in generation order
        const double total = combine(critics, n_critics, scores, n_traj, t);
        if (out_total) out_total[t] = total;
        if (total >= 0.0) {
            ++b.n_valid;
            if (b.cost < 0.0 || total < b.cost) { b.cost = total; b.index = t; }
        }
    }
    *out_best = b;
    return GEM_OK;
}

} // extern "C"
