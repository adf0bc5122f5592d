// gem_capi_mapgrid.cpp -- the MapGrid entry points of include/gem_hip_mapgrid.h: adjustPlanResolution (host only), the path and goal
// distance grids of a costmap and MapGridCostFunction::scoreTrajectory.  The kernels are in gem_mapgrid.hip.
//
// gem_costmap_mapgrid_prepare adjusts the plan and applies worldToMap on the host in plain C++ (it knows the geometry after rolling)
// and only enqueues.  The cells travel in pinned host memory that the distance kernel reads over the link: two buffers take turns
// (Costmaps::mg_pin), each guarded by an event recorded behind the launch that reads it, so a call waits at most for the launch two
// prepares back and never for the stream's other work.  The grids and their status words live with the costmap (Map::mg_dist,
// mg_status), the host-array forms of the scoring calls stage in Costmaps::mg_pose / mg_traj; all come from ensure() and only grow:
// gem_debug_get("arena_allocations") counts them, and a second identical call allocates nothing.  A grid is valid while the
// costmap's generation (new at create and at every roll that moves it) is the one it was prepared in.
//
// gem_costmap_mapgrid_prepare_tiled / _prepare_front_tiled fill the same slots on a costmap of any size with the tile rounds of
// gem_mapgrid_tiled.hip; they wait (prepare_tiled below), and share everything up to the launches with the capped form (stage).
//
// A costmap has three grid slots: path, goal and front (the goal grid of DWA's front plan, include/gem_hip_critics.h).  prepare() and
// read() below work on slots; the public `which` of the MapGrid calls still admits PATH | GOAL only, and the front slot is reached
// through gem_costmap_mapgrid_prepare_front / _read_front and by gem_costmap_best_trajectory (gem_capi_critics.cpp).
#include "gem_costmap_host.hpp"
#include "gem_mapgrid.hpp"
#include "gem_mapgrid_tiled.hpp"
#include "gem_rounds.hpp"

#include <cmath>
#include <cstring>

namespace {

constexpr long long kMaxPoses = 2147483646ll;                       // 2^31 - 2
constexpr int kMaxPosesPerTraj = 1 << 20;
constexpr int kKnownFlags = GEM_MAPGRID_STOP_ON_FAILURE | GEM_MAPGRID_SUM;
constexpr int kBoth = GEM_MAPGRID_PATH | GEM_MAPGRID_GOAL;              // what the public `which` admits
constexpr int kSlots = 3, kFrontSlot = 2;                           // path | goal | front (gem_hip_critics.h): the front grid has entries of its own
static_assert(kMapGridMaxWords == GEM_MAPGRID_MAX_WORDS, "the kernel's LDS limit is the header's");
static_assert(sizeof(gem_footprint_pose) == sizeof(FootPose), "a pose is four packed doubles");

bool fits(const CostMap& m) { return (unsigned long long)mapgrid_row_words(m.cfg.size_x) * m.cfg.size_y <= kMapGridMaxWords; }

// MapGrid::adjustPlanResolution.  Returns the adjusted plan's point count and writes the first `cap` points to out (NULL: none);
// -1: a coordinate or a step count that is not usable, or more than `limit` points.
long long adjust_plan(const double* plan, long long n, double resolution, double* out, long long cap, long long limit)
{
    if (n == 0) return 0;
    long long count = 0;
    auto put = [&](double x, double y) {
        if (out && count < cap) { out[2 * count] = x; out[2 * count + 1] = y; }
        ++count;
    };
    for (long long i = 0; i < 2 * n; ++i) if (!std::isfinite(plan[i])) return -1;
    double last_x = plan[0], last_y = plan[1];
    put(last_x, last_y);
    const double min_sq_resolution = resolution * resolution;
    for (long long i = 1; i < n; ++i) {
        const double loop_x = plan[2 * i], loop_y = plan[2 * i + 1];
        const double sqdist = (loop_x - last_x) * (loop_x - last_x) + (loop_y - last_y) * (loop_y - last_y);
        if (sqdist > min_sq_resolution) {
            const double q = std::ceil(std::sqrt(sqdist) / resolution);
            if (!(q < 2147483648.0)) return -1;                         // (also an overflowed sqdist)
            const int steps = (int)q;
            if (count + steps > limit) return -1;
            const double deltax = (loop_x - last_x) / steps, deltay = (loop_y - last_y) / steps;
            for (int j = 1; j < steps; ++j) put(last_x + j * deltax, last_y + j * deltay);
        }
        put(loop_x, loop_y);
        if (count > limit) return -1;
        last_x = loop_x; last_y = loop_y;
    }
    return count;
}

// exactly one grid -> its slot
int slot_of(int which_one) { return which_one == GEM_MAPGRID_PATH ? 0 : (which_one == GEM_MAPGRID_GOAL ? 1 : -1); }

int usable_slot(gem_handle* h, CostMap& m, int slot, const char* what)
{
    if (!m.mg_gen[slot]) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": the grid was never prepared").c_str());
    if (m.mg_gen[slot] != m.gen) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": the grid was prepared before the costmap last rolled or was observed").c_str());
    return GEM_OK;
}

int usable_grid(gem_handle* h, CostMap& m, int which_one, const char* what, int* slot)
{
    *slot = slot_of(which_one);
    if (*slot < 0) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": which_one is GEM_MAPGRID_PATH or GEM_MAPGRID_GOAL").c_str());
    return usable_slot(h, m, *slot, what);
}

struct ScoreCall {
    const char* what;
    const gem_footprint_pose* poses;
    long long n_traj;
    int T;
    long long* out;
    bool on_device;
};

int score(gem_handle* h, int id, int which_one, const ScoreCall& c, double xshift, int flags)
{
    int rc, slot;
    CostMap* m;
    if ((rc = costmap_find(h, id, c.what, &m))) return rc;
    if (c.T < 1 || c.T > kMaxPosesPerTraj) return fail(h, GEM_ERR_INVALID, (std::string(c.what) + ": poses_per_traj outside 1 .. 2^20").c_str());
    if (c.n_traj < 0 || c.n_traj > kMaxPoses / c.T) return fail(h, GEM_ERR_INVALID, (std::string(c.what) + ": a negative count, or more than 2^31 - 2 poses").c_str());
    if (flags & ~kKnownFlags) return fail(h, GEM_ERR_INVALID, (std::string(c.what) + ": unknown flag bits").c_str());
    if (!std::isfinite(xshift)) return fail(h, GEM_ERR_INVALID, (std::string(c.what) + ": xshift not finite").c_str());
    if ((rc = usable_grid(h, *m, which_one, c.what, &slot))) return rc;
    if (c.n_traj > 0 && (!c.poses || !c.out)) return fail(h, GEM_ERR_INVALID, (std::string(c.what) + ": a NULL array with a non-zero count").c_str());
    if (c.n_traj == 0) return GEM_OK;

    MapGridScoreArgs a{};
    a.dist = static_cast<const int*>(m->mg_dist[slot].p);
    a.n_traj = c.n_traj; a.T = c.T; a.xshift = xshift;
    a.stop_on_failure = (flags & GEM_MAPGRID_STOP_ON_FAILURE) ? 1 : 0;
    a.sum = (flags & GEM_MAPGRID_SUM) ? 1 : 0;
    if (c.on_device) {
        a.poses = reinterpret_cast<const FootPose*>(c.poses); a.out = c.out;
        GEM_HIP(h, launch_mapgrid_score(h->stream, geom_of(*m), a));
        return GEM_OK;
    }
    auto& cm = h->costmap;
    const size_t n_poses = (size_t)c.n_traj * (size_t)c.T;
    if ((rc = ensure(h, cm.mg_pose, n_poses * sizeof(FootPose))) || (rc = ensure(h, cm.mg_traj, (size_t)c.n_traj * sizeof(long long)))) return rc;
    HostXfer up{const_cast<gem_footprint_pose*>(c.poses), cm.mg_pose.p, n_poses * sizeof(FootPose)};
    if ((rc = upload_arrays(h, &up, 1))) return rc;
    a.poses = static_cast<const FootPose*>(cm.mg_pose.p);
    a.out = static_cast<long long*>(cm.mg_traj.p);
    GEM_HIP(h, launch_mapgrid_score(h->stream, geom_of(*m), a));
    HostXfer down{c.out, cm.mg_traj.p, (size_t)c.n_traj * sizeof(long long)};
    return download_arrays(h, &down, 1, 0);
}

// What the capped and the tiled prepare share up to their launches: the checks, the adjusted plan, the slots' grids and status words,
// and this call's turn of the pinned cells, filled.  `slots` is a mask of slots (bit 0 path | 1 goal | 2 front), at most two of them.
struct Staged {
    CostMap* m = nullptr;
    CostGeom g{};
    size_t cells = 0;
    int turn = 0;
    int n_grids = 0;
    MapGridArgs a{};                    // grid, cells, n, the sizes, and per requested grid dist / status / goal
};

int stage(gem_handle* h, int id, const char* what, const double* plan_xy, long long n, int slots, bool capped, Staged& s)
{
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, what, &m))) return rc;
    if (n < 0 || (n > 0 && !plan_xy)) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": a negative count, or a NULL plan with a non-zero count").c_str());
    if (capped && !fits(*m)) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": ceil(size_x / 64) * size_y above GEM_MAPGRID_MAX_WORDS").c_str());
    auto& cm = h->costmap;
    const CostGeom g = geom_of(*m);
    const long long count = adjust_plan(plan_xy, n, g.res, nullptr, 0, GEM_MAPGRID_MAX_POINTS);
    if (count < 0) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": a plan coordinate not finite, or an adjusted plan above GEM_MAPGRID_MAX_POINTS").c_str());
    cm.mg_plan.resize((size_t)count * 2);
    adjust_plan(plan_xy, n, g.res, cm.mg_plan.data(), count, GEM_MAPGRID_MAX_POINTS);

    // the grids and status words; then this call's turn of the pinned cells
    const size_t cells = (size_t)g.sx * g.sy;
    for (int k = 0; k < kSlots; ++k)
        if ((slots & (1 << k)) && (rc = ensure(h, m->mg_dist[k], cells * sizeof(int)))) return rc;
    if ((rc = ensure(h, m->mg_status, kSlots * kMapGridStatusWords * sizeof(int)))) return rc;
    const int turn = (int)(cm.mg_turn & 1u);
    if (!cm.mg_ev[turn]) GEM_HIP(h, hipEventCreateWithFlags(&cm.mg_ev[turn], hipEventDisableTiming));
    if (cm.mg_ev_pending[turn]) { GEM_HIP(h, hipEventSynchronize(cm.mg_ev[turn])); cm.mg_ev_pending[turn] = false; }
    const size_t bytes = std::max<size_t>((size_t)count, 1) * sizeof(int);
    if (bytes > cm.mg_pin_cap[turn]) {
        if (cm.mg_pin[turn]) GEM_HIP(h, hipHostFree(cm.mg_pin[turn]));
        cm.mg_pin[turn] = nullptr; cm.mg_pin_cap[turn] = 0;
        const size_t want = bytes + bytes / 4 + 4096;
        GEM_HIP(h, hipHostMalloc(&cm.mg_pin[turn], want, hipHostMallocDefault));
        cm.mg_pin_cap[turn] = want;
    }
    int* pin = static_cast<int*>(cm.mg_pin[turn]);
    for (long long i = 0; i < count; ++i) {
        uint32_t cell = 0u;
        pin[i] = cost_cell(g, cm.mg_plan[2 * i], cm.mg_plan[2 * i + 1], cell) ? (int)cell : -1;
    }
    ++cm.mg_turn;

    s.m = m; s.g = g; s.cells = cells; s.turn = turn;
    MapGridArgs& a = s.a;
    a = MapGridArgs{};
    a.grid = grid_of(*m); a.cells = pin; a.n = (int)count;
    a.sx = g.sx; a.sy = g.sy; a.nw = mapgrid_row_words(g.sx);
    int ng = 0;
    for (int k = 0; k < kSlots; ++k) {
        if (!(slots & (1 << k))) continue;
        a.dist[ng] = static_cast<int*>(m->mg_dist[k].p);
        a.status[ng] = static_cast<int*>(m->mg_status.p) + k * kMapGridStatusWords;
        a.goal[ng] = k != 0;                                             // the front grid is a goal grid of its own plan
        ++ng;
    }
    s.n_grids = ng;
    return GEM_OK;
}

// gem_costmap_mapgrid_prepare and _prepare_front behind their own checks of `which`: one launch of the LDS search, only enqueued
int prepare(gem_handle* h, int id, const char* what, const double* plan_xy, long long n, int slots)
{
    Staged s;
    if (const int rc = stage(h, id, what, plan_xy, n, slots, true, s)) return rc;
    auto& cm = h->costmap;
    const MapGridArgs& a = s.a;
    GEM_HIP(h, launch_mapgrid_fill(h->stream, a.dist[0], s.n_grids == 2 ? a.dist[1] : nullptr, (uint32_t)s.cells, (int)s.cells + 1));
    GEM_HIP(h, launch_mapgrid_distance(h->stream, a, s.n_grids));
    GEM_HIP(h, hipEventRecord(cm.mg_ev[s.turn], h->stream));
    cm.mg_ev_pending[s.turn] = true;
    for (int k = 0; k < kSlots; ++k) if (slots & (1 << k)) s.m->mg_gen[k] = s.m->gen;
    return GEM_OK;
}

// gem_costmap_mapgrid_prepare_tiled and _prepare_front_tiled: the same grids in the same slots by the tile rounds of
// gem_mapgrid_tiled.hip, on a costmap of any size.  The call WAITS: fill, seed, then CHUNKS of rounds, each closed by k_mgt_close, which
// answers through pinned words; the host loop and its bound are run_tile_rounds' (gem_rounds.hpp), a chunk is tiles_x + tiles_y rounds
// (gem_debug_set "mapgrid_chunk" sets another length), exactly as gem_costmap_navplan drives its potential.  The rim pass follows the
// converged close.  The slots' generations are 0 from before the first launch until then: a failure in between leaves "never
// prepared", not a half-relaxed grid.  The first close has waited for the seed kernel, so the pinned cells need no event.
int prepare_tiled(gem_handle* h, int id, const char* what, const double* plan_xy, long long n, int slots, gem_mapgrid_tiled_status* st)
{
    int rc;
    Staged s;
    if ((rc = stage(h, id, what, plan_xy, n, slots, false, s))) return rc;
    auto& cm = h->costmap;
    CostMap* m = s.m;
    MapGridTiledArgs a{};
    a.grid = s.a.grid; a.cells = s.a.cells; a.n = s.a.n;
    a.sx = (int)s.g.sx; a.sy = (int)s.g.sy; a.ntx = nav_tiles(a.sx); a.nty = nav_tiles(a.sy);
    a.n_grids = s.n_grids;
    for (int k = 0; k < 2; ++k) { a.dist[k] = s.a.dist[k]; a.status[k] = s.a.status[k]; a.goal[k] = s.a.goal[k]; }
    const size_t nt = (size_t)a.ntx * a.nty;
    if ((rc = ensure(h, m->mg_act, 2 * 2 * nt * sizeof(int)))) return rc;
    if (!cm.mgt_pin) GEM_HIP(h, hipHostMalloc(&cm.mgt_pin, kMgtPinWords * sizeof(int), hipHostMallocDefault));
    a.act = static_cast<int*>(m->mg_act.p);
    a.pin = static_cast<int*>(cm.mgt_pin);
    volatile int* pin = a.pin;
    for (int i = 0; i < kMgtPinWords; ++i) pin[i] = 0;

    for (int k = 0; k < kSlots; ++k) if (slots & (1 << k)) m->mg_gen[k] = 0;     // (a failure below leaves no grid to read)
    GEM_HIP(h, launch_mapgrid_fill(h->stream, a.dist[0], a.n_grids == 2 ? a.dist[1] : nullptr, (uint32_t)s.cells, (int)s.cells + 1));
    GEM_HIP(h, launch_mgt_seed(h->stream, a));
    RoundsResult rr;
    rc = run_tile_rounds(
        (long long)s.cells, h->mapgrid_chunk > 0 ? h->mapgrid_chunk : (long long)a.ntx + a.nty,
        [&](int round) -> int {
            a.round = round;
            GEM_HIP(h, launch_mgt_round(h->stream, a));
            return GEM_OK;
        },
        [&](int round, bool& converged) -> int {
            a.round = round;
            GEM_HIP(h, launch_mgt_close(h->stream, a));
            GEM_HIP(h, hipStreamSynchronize(h->stream));
            converged = pin[kMgtConverged] != 0;
            return GEM_OK;
        },
        rr);
    if (rc) return rc;
    if (!rr.converged) return fail(h, GEM_ERR_HIP, (std::string(what) + ": the distances did not converge within their bound").c_str());
    GEM_HIP(h, launch_mgt_rim(h->stream, a));
    for (int k = 0; k < kSlots; ++k) if (slots & (1 << k)) m->mg_gen[k] = m->gen;
    if (st) {
        st->started = pin[kMgtStarted];
        st->goal_cell[0] = pin[kMgtGoalX]; st->goal_cell[1] = pin[kMgtGoalY];
        st->rounds = pin[kMgtRounds];
        st->chunks = rr.chunks;
    }
    return GEM_OK;
}

int read(gem_handle* h, int id, const char* what, int slot, int* out, int* out_started, int out_goal_cell[2])
{
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, what, &m))) return rc;
    if ((rc = usable_slot(h, *m, slot, what))) return rc;
    int st[kMapGridStatusWords] = {};
    HostXfer d[2] = {{st, static_cast<int*>(m->mg_status.p) + slot * kMapGridStatusWords, sizeof(st)},
                     {out, m->mg_dist[slot].p, (size_t)m->cfg.size_x * m->cfg.size_y * sizeof(int)}};
    if ((rc = download_arrays(h, d, out ? 2 : 1, 0))) return rc;
    if (out_started) *out_started = st[kMapGridStarted];
    if (out_goal_cell) { out_goal_cell[0] = st[kMapGridGoalX]; out_goal_cell[1] = st[kMapGridGoalY]; }
    return GEM_OK;
}

} // namespace

extern "C" {

int gem_mapgrid_adjust_plan(const double* plan_xy, long long n, double resolution, double* out_xy, long long cap, long long* out_n)
{
    if (n < 0 || (n > 0 && !plan_xy) || !std::isfinite(resolution) || !(resolution > 0.0) || (out_xy && cap < 0)) return GEM_ERR_INVALID;
    const long long count = adjust_plan(plan_xy, n, resolution, out_xy, out_xy ? cap : 0, GEM_MAPGRID_MAX_POINTS);
    if (count < 0) return GEM_ERR_INVALID;
    if (out_n) *out_n = count;
    return out_xy && cap < count ? GEM_ERR_INVALID : GEM_OK;
}

int gem_costmap_mapgrid_prepare(gem_handle* h, int id, const double* plan_xy, long long n, int which)
{
    GEM_ENTRY("gem_costmap_mapgrid_prepare");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_mapgrid_prepare", &m))) return rc;
    if (!(which & kBoth) || (which & ~kBoth)) return fail(h, GEM_ERR_INVALID, "gem_costmap_mapgrid_prepare: which is a mask of GEM_MAPGRID_PATH | GEM_MAPGRID_GOAL");
    return prepare(h, id, "gem_costmap_mapgrid_prepare", plan_xy, n, which);      // (the public bits are the slots' bits)
}

int gem_costmap_mapgrid_prepare_front(gem_handle* h, int id, const double* plan_xy, long long n)
{
    GEM_ENTRY("gem_costmap_mapgrid_prepare_front");
    return prepare(h, id, "gem_costmap_mapgrid_prepare_front", plan_xy, n, 1 << kFrontSlot);
}

int gem_costmap_mapgrid_prepare_tiled(gem_handle* h, int id, const double* plan_xy, long long n, int which, gem_mapgrid_tiled_status* st)
{
    GEM_ENTRY("gem_costmap_mapgrid_prepare_tiled");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_mapgrid_prepare_tiled", &m))) return rc;
    if (!(which & kBoth) || (which & ~kBoth)) return fail(h, GEM_ERR_INVALID, "gem_costmap_mapgrid_prepare_tiled: which is a mask of GEM_MAPGRID_PATH | GEM_MAPGRID_GOAL");
    return prepare_tiled(h, id, "gem_costmap_mapgrid_prepare_tiled", plan_xy, n, which, st);
}

int gem_costmap_mapgrid_prepare_front_tiled(gem_handle* h, int id, const double* plan_xy, long long n, gem_mapgrid_tiled_status* st)
{
    GEM_ENTRY("gem_costmap_mapgrid_prepare_front_tiled");
    return prepare_tiled(h, id, "gem_costmap_mapgrid_prepare_front_tiled", plan_xy, n, 1 << kFrontSlot, st);
}

int gem_costmap_mapgrid_read(gem_handle* h, int id, int which_one, int* out, int* out_started, int out_goal_cell[2])
{
    GEM_ENTRY("gem_costmap_mapgrid_read");
    int rc, slot;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_mapgrid_read", &m))) return rc;
    if ((rc = usable_grid(h, *m, which_one, "gem_costmap_mapgrid_read", &slot))) return rc;
    return read(h, id, "gem_costmap_mapgrid_read", slot, out, out_started, out_goal_cell);
}

int gem_costmap_mapgrid_read_front(gem_handle* h, int id, int* out, int* out_started, int out_goal_cell[2])
{
    GEM_ENTRY("gem_costmap_mapgrid_read_front");
    return read(h, id, "gem_costmap_mapgrid_read_front", kFrontSlot, out, out_started, out_goal_cell);
}

int gem_costmap_mapgrid_score(gem_handle* h, int id, int which_one, const gem_footprint_pose* poses, long long n_traj, int poses_per_traj,
                              double xshift, int flags, long long* out_traj)
{
    GEM_ENTRY("gem_costmap_mapgrid_score");
    return score(h, id, which_one, ScoreCall{"gem_costmap_mapgrid_score", poses, n_traj, poses_per_traj, out_traj, false}, xshift, flags);
}

int gem_costmap_mapgrid_score_device(gem_handle* h, int id, int which_one, const gem_footprint_pose* d_poses, long long n_traj,
                                     int poses_per_traj, double xshift, int flags, long long* d_out_traj)
{
    GEM_ENTRY("gem_costmap_mapgrid_score_device");
    return score(h, id, which_one, ScoreCall{"gem_costmap_mapgrid_score_device", d_poses, n_traj, poses_per_traj, d_out_traj, true}, xshift, flags);
}

} // extern "C"
