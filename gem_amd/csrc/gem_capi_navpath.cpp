// gem_capi_navpath.cpp -- the entry points of include/gem_hip_navpath.h: paths on the last plan's potential for a batch of goals, grid
// or gradient.  The kernel is in gem_navgrad.hip; the walk's arithmetic and the host twin of one goal are in gem_navgrad.hpp.
//
// The goals are mapped with worldToMap on the host (it knows the geometry after rolling) and handed over as cells; the start cell is
// the last plan's.  One launch, one wave per goal.  The goal cells, and for the waiting form the points and the results, live with
// the costmap (Map::np_*) in arenas from ensure() that only grow: a second identical call allocates nothing.  Nothing of the plan is
// written: not the potential, not the costmap's last path or status, not the frontier search.
#include "gem_costmap_host.hpp"
#include "gem_navgrad.hpp"

#include <cmath>
#include <string>
#include <vector>

namespace {

static_assert(sizeof(gem_navpath_result) == 32, "the result is 32 bytes on both sides");

bool form_ok(int form) { return form == GEM_NAVPATH_GRID || form == GEM_NAVPATH_GRADIENT; }

int paths(gem_handle* h, int id, const char* what, const double* goals_xy, int n_goals, int form, int max_points, float* out_pts,
          gem_navpath_result* out, bool on_device)
{
    auto bad = [&](const char* reason) { return fail(h, GEM_ERR_INVALID, (std::string(what) + ": " + reason).c_str()); };
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, what, &m))) return rc;
    if (!goals_xy || !out) return bad("NULL goals or results");
    if (n_goals < 1 || n_goals > kNavPathMaxGoals) return bad("n_goals outside 1 .. 1024");
    if (max_points < 2 || max_points > kNavPathMaxPoints) return bad("max_points outside 2 .. 2^20");
    if ((long long)n_goals * max_points > kNavPathMaxTotal) return bad("n_goals * max_points above 2^24");
    if (!form_ok(form)) return bad("an unknown form");
    for (int i = 0; i < 2 * n_goals; ++i)
        if (!std::isfinite(goals_xy[i])) return bad("a coordinate not finite");
    const CostGeom g = geom_of(*m);
    if (g.sx >= (uint32_t)kNavPathMaxSize || g.sy >= (uint32_t)kNavPathMaxSize) return bad("size_x or size_y of 2^24 or more");
    if ((rc = costmap_plan_fresh(h, *m, what))) return rc;

    const size_t n_pts = (size_t)n_goals * (size_t)max_points * 2;
    if ((rc = ensure(h, m->np_goal, (size_t)n_goals * 2 * sizeof(int)))) return rc;
    if (!on_device) {
        if ((rc = ensure(h, m->np_res, (size_t)n_goals * sizeof(gem_navpath_result)))) return rc;
        if (out_pts && (rc = ensure(h, m->np_pts, n_pts * sizeof(float)))) return rc;
    }
    auto& cells = h->costmap.np_cells;
    cells.resize((size_t)n_goals * 2);
    for (int i = 0; i < n_goals; ++i) {
        uint32_t mx = 0u, my = 0u;
        const bool on = cost_cell_xy(g, goals_xy[2 * i], goals_xy[2 * i + 1], mx, my);
        cells[2 * (size_t)i] = on ? (int)mx : -1;
        cells[2 * (size_t)i + 1] = on ? (int)my : -1;
    }
    HostXfer up{cells.data(), m->np_goal.p, cells.size() * sizeof(int)};
    if ((rc = upload_arrays(h, &up, 1))) return rc;

    NavPathArgs a{};
    a.pot = static_cast<const int*>(m->nav_pot.p);
    a.goals = static_cast<const int*>(m->np_goal.p);
    a.pts = on_device ? out_pts : (out_pts ? static_cast<float*>(m->np_pts.p) : nullptr);
    a.res = on_device ? out : static_cast<gem_navpath_result*>(m->np_res.p);
    a.sx = (int)g.sx; a.sy = (int)g.sy;
    a.sx0 = m->nav_last.start_cell[0]; a.sy0 = m->nav_last.start_cell[1];
    a.form = form; a.max_points = max_points; a.n_goals = n_goals;
    GEM_HIP(h, launch_nav_paths(h->stream, a));
    if (on_device) return GEM_OK;
    HostXfer down[2] = {{out, m->np_res.p, (size_t)n_goals * sizeof(gem_navpath_result)}, {out_pts, m->np_pts.p, n_pts * sizeof(float)}};
    return download_arrays(h, down, out_pts ? 2 : 1, 0);
}

} // namespace

extern "C" {

int gem_navpath_host(const int* pot, int size_x, int size_y, const int start_cell[2], const int goal_cell[2], int form, int max_points,
                     float* out_pts, gem_navpath_result* out)
{
    if (!pot || !start_cell || !goal_cell || !out || size_x < 1 || size_y < 1 || size_x >= kNavPathMaxSize || size_y >= kNavPathMaxSize ||
        max_points < 2 || max_points > kNavPathMaxPoints || !form_ok(form))
        return GEM_ERR_INVALID;
    navpath_walk_host(pot, size_x, size_y, start_cell[0], start_cell[1], goal_cell[0], goal_cell[1], form, max_points, out_pts, out);
    return GEM_OK;
}

int gem_costmap_navplan_paths(gem_handle* h, int id, const double* goals_xy, int n_goals, int form, int max_points, float* out_pts,
                              gem_navpath_result* out)
{
    GEM_ENTRY("gem_costmap_navplan_paths");
    return paths(h, id, "gem_costmap_navplan_paths", goals_xy, n_goals, form, max_points, out_pts, out, false);
}

int gem_costmap_navplan_paths_device(gem_handle* h, int id, const double* goals_xy, int n_goals, int form, int max_points, float* d_out_pts,
                                     gem_navpath_result* d_out)
{
    GEM_ENTRY("gem_costmap_navplan_paths_device");
    return paths(h, id, "gem_costmap_navplan_paths_device", goals_xy, n_goals, form, max_points, d_out_pts, d_out, true);
}

} // extern "C"
