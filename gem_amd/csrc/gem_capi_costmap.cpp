// gem_capi_costmap.cpp -- the costmap-layer entry points of include/gem_hip.h (PointMapLayer and ElevationMapLayer of the
// reference's layers/, with the pieces of costmap_2d they call restated there).  The kernels are in gem_costmap.hip.
//
// State (gem_handle::Costmaps):
//   a costmap      two byte grids (a roll writes the other one and they swap) and a stamp word per cell, all-zero between calls;
//                  with voxels attached (gem_capi_voxlayer.cpp) two grids of 32-bit columns that reset and roll with the bytes
//   small          the bounds words of a mark (four accumulated by the mark kernels, four published by the resolve pass)
//   in, win        a host cloud of gem_costmap_mark_points on the device | the packed window of gem_costmap_read / _write
// gem_costmap_mark_history reads the history cloud (gem_handle::History, gem_capi_history.cpp) and its box table where they lie.
// A mark is its mark launches followed by one resolve launch on the handle's stream; the inputs that already live on the device
// (the capture, the submap stack) are read where they are, a capture's record count from its device word.  Every device buffer comes
// from ensure(), so gem_debug_get("arena_allocations") counts it.
// Also here: what the layers share on the host -- read_bounds and read_window / write_window under the four read and write entry
// points of the bytes and the columns (gem_costmap_host.hpp), and stage_observations, obs_params_common and touch of ObstacleLayer
// and VoxelLayer (gem_observe_host.hpp).
#include "gem_observe_host.hpp"
#include "gem_voxlayer.hpp"

#include <algorithm>

namespace {

constexpr size_t kRec = sizeof(LocalRecord);
constexpr long long kMaxInputs = 2147483646ll;                      // 2^31 - 2: the stamp 2 * (i + 1) + 1 fits 32 bits

unsigned long long* acc_words(gem_handle* h) { return static_cast<unsigned long long*>(h->costmap.small.p); }
CostAccum accum_of(gem_handle* h, CostMap& m) { return CostAccum{static_cast<uint32_t*>(m.stamps.p), acc_words(h)}; }

int invalid(gem_handle* h, const char* what, const char* reason) { return fail(h, GEM_ERR_INVALID, (std::string(what) + ": " + reason).c_str()); }
int usable(gem_handle* h, const char* what) { return h->tp_x ? invalid(h, what, "not on a handle with a communicator") : GEM_OK; }

// the resolve pass behind a mark's launches, then the caller's bounds merged with the touched ones
int finish_mark(gem_handle* h, CostMap& m, double bounds[4])
{
    unsigned long long* acc = acc_words(h);
    GEM_HIP(h, launch_cost_resolve(h->stream, cells_of(m), static_cast<uint32_t*>(m.stamps.p), grid_of(m), acc, acc + 4));
    return read_bounds(h, bounds);
}

int mark_records(gem_handle* h, CostMap& m, const LocalRecord* d_rec, long long n, double thresh, double bounds[4])
{
    if (n > 0) {
        CostPointsArgs a{d_rec, nullptr, (uint32_t)n, 0u, thresh};
        GEM_HIP(h, launch_cost_mark_points(h->stream, geom_of(m), a, accum_of(h, m)));
    }
    return finish_mark(h, m, bounds);
}

int check_cloud(gem_handle* h, const char* what, const void* points, long long n, double thresh)
{
    if (n < 0 || n > kMaxInputs || (n > 0 && !points)) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": bad cloud").c_str());
    if (!std::isfinite(thresh)) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": travers_thresh not finite").c_str());
    return GEM_OK;
}

// the last capture: its records, linear indices, device count word (Local::small holds the two slots' counts first) and geometry
bool capture_of(gem_handle* h, CostVisualArgs* v)
{
    const auto& lc = h->local;
    if (!lc.enabled || lc.cur < 0) return false;
    const auto& s = lc.slot[lc.cur];
    v->rec = static_cast<const LocalRecord*>(s.rec.p); v->lin = static_cast<const int*>(s.lin.p);
    v->count = static_cast<const uint32_t*>(lc.small.p) + lc.cur;
    v->g = LocalGeom{s.off, s.res, s.px, s.py, h->L, s.sx, s.sy};
    return true;
}

// Costmap2D::updateOrigin (costmap_2d.cpp), restated in include/gem_hip.h
int update_origin(gem_handle* h, CostMap& m, double new_ox, double new_oy, const char* what)
{
    if (!std::isfinite(new_ox) || !std::isfinite(new_oy)) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": origin not finite").c_str());
    const double qx = (new_ox - m.cfg.origin_x) / m.cfg.resolution, qy = (new_oy - m.cfg.origin_y) / m.cfg.resolution;
    if (!(qx > -2147483649.0 && qx < 2147483648.0 && qy > -2147483649.0 && qy < 2147483648.0))
        return fail(h, GEM_ERR_INVALID, (std::string(what) + ": the step's cell count does not fit an int").c_str());
    const int cell_ox = (int)qx, cell_oy = (int)qy;
    if (cell_ox == 0 && cell_oy == 0) return GEM_OK;
    const double ox = m.cfg.origin_x + cell_ox * m.cfg.resolution, oy = m.cfg.origin_y + cell_oy * m.cfg.resolution;
    if (!std::isfinite(ox) || !std::isfinite(oy)) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": origin not finite").c_str());
    GEM_HIP(h, launch_cost_roll(h->stream, grid_of(m), m.grid[1 - m.act].p, 1, m.cfg.size_x, m.cfg.size_y, cell_ox, cell_oy, m.cfg.default_value));
    m.act = 1 - m.act;
    if (m.has_vox) {                                                    // VoxelLayer::updateOrigin: the columns move with the bytes
        GEM_HIP(h, launch_cost_roll(h->stream, columns_of(m), m.vox[1 - m.vox_act].p, 4, m.cfg.size_x, m.cfg.size_y, cell_ox, cell_oy, kVoxUnknown));
        m.vox_act = 1 - m.vox_act;
    }
    m.cfg.origin_x = ox; m.cfg.origin_y = oy;
    m.gen = ++h->costmap.generation;                                    // the distance grids of gem_costmap_mapgrid_prepare are stale now
    return GEM_OK;
}

void free_map(CostMap& m)
{
    for (Arena* a : {&m.grid[0], &m.grid[1], &m.stamps, &m.infl_table, &m.mg_dist[0], &m.mg_dist[1], &m.mg_dist[2], &m.mg_status, &m.mg_act,
                     &m.nav_pot, &m.nav_act, &m.nav_path, &m.nav_status, &m.np_goal, &m.np_res, &m.np_pts,
                     &m.fr_label, &m.fr_index, &m.fr_act, &m.fr_rec, &m.fr_out, &m.fr_words, &m.vox[0], &m.vox[1]}) {
        if (a->p) hipFree(a->p);
        a->p = nullptr; a->cap = 0;
    }
    m = CostMap{};
}

} // namespace

namespace gemi {

int costmap_find(gem_handle* h, int id, const char* what, CostMap** out)
{
    if (const int rc = usable(h, what)) return rc;
    if (id < 0 || id >= gem_handle::Costmaps::kMax || !h->costmap.map[id].used) return invalid(h, what, "no such costmap");
    *out = &h->costmap.map[id];
    return GEM_OK;
}

int costmap_plan_fresh(gem_handle* h, const CostMap& m, const char* what)
{
    if (!m.nav_gen) return invalid(h, what, "no plan was made");
    if (m.nav_gen != m.gen) return invalid(h, what, "the plan was made before the costmap last rolled or was observed");
    return GEM_OK;
}

int costmap_search_fresh(gem_handle* h, const CostMap& m, const char* what)
{
    if (!m.fr_gen) return invalid(h, what, "no search was made, or a plan was made since");
    if (m.fr_gen != m.gen) return invalid(h, what, "the search was made before the costmap last rolled or was observed");
    return GEM_OK;
}

bool geometry_ok(const gem_costmap_config* c)
{
    return c && c->size_x != 0 && c->size_y != 0 && (long long)c->size_x * c->size_y <= kMaxCells && std::isfinite(c->resolution) &&
           c->resolution > 0.0 && std::isfinite(c->origin_x) && std::isfinite(c->origin_y);
}

bool window_ok(const CostMap& m, int min_i, int min_j, int max_i, int max_j)
{
    return min_i >= 0 && min_j >= 0 && min_i <= max_i && min_j <= max_j && (long long)max_i <= (long long)m.cfg.size_x &&
           (long long)max_j <= (long long)m.cfg.size_y;
}

int read_window(gem_handle* h, CostMap& m, const char* what, void* grid, size_t elem, CostWindow win, void* out, size_t row_stride)
{
    if (!window_ok(m, win.min_i, win.min_j, win.max_i, win.max_j)) return invalid(h, what, "window outside the map");
    const size_t w = (size_t)(win.max_i - win.min_i), rows = (size_t)(win.max_j - win.min_j), bytes = w * rows * elem;
    if (!w || !rows) return GEM_OK;
    if (!out || row_stride < w) return invalid(h, what, "null output or a row stride below the window's width");
    int rc;
    void* src = grid;
    if (!(w == m.cfg.size_x && rows == m.cfg.size_y)) {                 // a partial window is packed on the device first
        if ((rc = ensure(h, h->costmap.win, bytes))) return rc;
        GEM_HIP(h, launch_cost_window(h->stream, grid, elem, m.cfg.size_x, win, h->costmap.win.p, true));
        src = h->costmap.win.p;
    }
    if (row_stride == w) {
        HostXfer d{out, src, bytes};
        return download_arrays(h, &d, 1, 0);
    }
    std::vector<unsigned char>& tmp = h->costmap.host_rows;             // packed rows, then out at the caller's stride
    tmp.resize(bytes);
    HostXfer d{tmp.data(), src, bytes};
    if ((rc = download_arrays(h, &d, 1, 0))) return rc;
    for (size_t r = 0; r < rows; ++r) memcpy(static_cast<unsigned char*>(out) + r * row_stride * elem, tmp.data() + r * w * elem, w * elem);
    return GEM_OK;
}

int write_window(gem_handle* h, CostMap& m, const char* what, void* grid, size_t elem, CostWindow win, const void* in, size_t row_stride)
{
    if (!window_ok(m, win.min_i, win.min_j, win.max_i, win.max_j)) return invalid(h, what, "window outside the map");
    const size_t w = (size_t)(win.max_i - win.min_i), rows = (size_t)(win.max_j - win.min_j), bytes = w * rows * elem;
    if (!w || !rows) return GEM_OK;
    if (!in || row_stride < w) return invalid(h, what, "null input or a row stride below the window's width");
    int rc;
    if ((rc = ensure(h, h->costmap.win, bytes))) return rc;
    if (row_stride != w) {                                              // the caller's rows, packed
        std::vector<unsigned char>& tmp = h->costmap.host_rows;
        tmp.resize(bytes);
        for (size_t r = 0; r < rows; ++r) memcpy(tmp.data() + r * w * elem, static_cast<const unsigned char*>(in) + r * row_stride * elem, w * elem);
        in = tmp.data();
    }
    HostXfer x{const_cast<void*>(in), h->costmap.win.p, bytes};
    if ((rc = upload_arrays(h, &x, 1))) return rc;
    GEM_HIP(h, launch_cost_window(h->stream, grid, elem, m.cfg.size_x, win, h->costmap.win.p, false));
    return GEM_OK;
}

int stage_observations(gem_handle* h, const ObserveCall& c, const void* points[GEM_OBS_MAX])
{
    auto& in = h->costmap.in;
    size_t host_bytes = 0, at[GEM_OBS_MAX];
    for (int k = 0; k < c.n_obs; ++k) {
        at[k] = host_bytes;
        host_bytes += ((size_t)c.obs[k].n * c.obs[k].point_step + 255) / 256 * 256;
    }
    int rc;
    if (!c.on_device && host_bytes && (rc = ensure(h, in, host_bytes))) return rc;
    HostXfer up[GEM_OBS_MAX];
    int n_up = 0;
    for (int k = 0; k < c.n_obs; ++k) {
        points[k] = c.on_device ? c.obs[k].points : static_cast<const unsigned char*>(in.p) + at[k];
        if (!c.on_device && c.obs[k].n > 0)
            up[n_up++] = HostXfer{const_cast<void*>(c.obs[k].points), const_cast<void*>(points[k]), (size_t)c.obs[k].n * c.obs[k].point_step};
    }
    return n_up ? upload_arrays(h, up, n_up) : GEM_OK;
}

ObsParams obs_params_common(const CostGeom& g, const gem_observation& o, const void* points, double layer_max_h)
{
    ObsParams p{};
    p.points = static_cast<const unsigned char*>(points);
    p.n = (uint32_t)o.n; p.step = o.point_step;
    p.ox = o.origin[0]; p.oy = o.origin[1]; p.oz = o.origin[2];
    p.sq_obstacle_range = o.obstacle_range * o.obstacle_range;
    p.raytrace_range = o.raytrace_range;
    p.min_h = o.min_obstacle_height; p.max_h = o.max_obstacle_height; p.layer_max_h = layer_max_h;
    p.cell_range = obs_cell_distance(o.raytrace_range, g.res);
    p.marking = (o.flags & GEM_OBS_MARKING) ? 1 : 0;
    return p;
}

void touch(double bounds[4], double x, double y)
{
    if (!bounds) return;
    bounds[0] = obs_std_min(x, bounds[0]); bounds[1] = obs_std_min(y, bounds[1]);
    bounds[2] = obs_std_max(x, bounds[2]); bounds[3] = obs_std_max(y, bounds[3]);
}

// A mark used to merge with `bounds[k] < v ? bounds[k] : v` and `v < bounds[2 + k] ? bounds[2 + k] : v`; obs_std_min(v, bounds[k]) and
// obs_std_max(v, bounds[2 + k]), which the observes used, expand to these very expressions, so the two agree for every input, NaN
// and signed zeros included: a NaN in bounds is replaced (both comparisons are false), and of two zeros the decoded one stays.
int read_bounds(gem_handle* h, double bounds[4])
{
    if (!bounds) return GEM_OK;
    unsigned long long w[4];
    HostXfer d{w, acc_words(h) + 4, sizeof(w)};
    if (const int rc = download_arrays(h, &d, 1, 0)) return rc;
    double v;
    for (int k = 0; k < 2; ++k) {
        if (cost_key_decode(w[k], false, &v)) bounds[k] = obs_std_min(v, bounds[k]);
        if (cost_key_decode(w[2 + k], true, &v)) bounds[2 + k] = obs_std_max(v, bounds[2 + k]);
    }
    return GEM_OK;
}

void costmap_free(gem_handle* h)
{
    auto& c = h->costmap;
    if (h->stream) hipStreamSynchronize(h->stream);
    for (auto& m : c.map) free_map(m);
    for (Arena* a : {&c.small, &c.in, &c.win, &c.fp_pose, &c.fp_cost, &c.fp_traj, &c.infl_bits, &c.infl_flags, &c.mg_pose, &c.mg_traj,
                     &c.cr_cand, &c.cr_pose, &c.cr_len, &c.cr_ext, &c.cr_total, &c.cr_best,
                     &c.tg_pose, &c.tg_len, &c.tg_ext, &c.ro_cost, &c.ro_ahead, &c.ro_best, &c.nav_w, &c.fr_blocks, &c.ob_bits, &c.ob_rays, &c.ob_cnt, &c.vx_marks, &c.vx_touched, &c.vx_rays}) {
        if (a->p) hipFree(a->p);
        a->p = nullptr; a->cap = 0;
    }
    if (c.nav_pin) hipHostFree(c.nav_pin);
    c.nav_pin = nullptr;
    if (c.fr_pin) hipHostFree(c.fr_pin);
    c.fr_pin = nullptr;
    if (c.mgt_pin) hipHostFree(c.mgt_pin);
    c.mgt_pin = nullptr;
    for (int k = 0; k < 2; ++k) {
        if (c.mg_pin[k]) hipHostFree(c.mg_pin[k]);
        if (c.mg_ev[k]) hipEventDestroy(c.mg_ev[k]);
        c.mg_pin[k] = nullptr; c.mg_pin_cap[k] = 0; c.mg_ev[k] = nullptr; c.mg_ev_pending[k] = false;
    }
}

} // namespace gemi

extern "C" {

int gem_costmap_create(gem_handle* h, const gem_costmap_config* cfg, int* out_id)
{
    GEM_ENTRY("gem_costmap_create");
    int rc;
    if ((rc = usable(h, "gem_costmap_create"))) return rc;
    if (!cfg || !out_id) return fail(h, GEM_ERR_INVALID, "gem_costmap_create: null argument");
    if (cfg->size_x == 0 || cfg->size_y == 0 || (long long)cfg->size_x * cfg->size_y > kMaxCells)
        return fail(h, GEM_ERR_INVALID, "gem_costmap_create: size zero or above 2^30 cells");
    if (!std::isfinite(cfg->resolution) || !(cfg->resolution > 0.0) || !std::isfinite(cfg->origin_x) || !std::isfinite(cfg->origin_y))
        return fail(h, GEM_ERR_INVALID, "gem_costmap_create: resolution not finite and positive, or origin not finite");
    auto& c = h->costmap;
    int id = 0;
    while (id < gem_handle::Costmaps::kMax && c.map[id].used) ++id;
    if (id == gem_handle::Costmaps::kMax) return fail(h, GEM_ERR_INVALID, "gem_costmap_create: every costmap of the handle is in use");
    CostMap& m = c.map[id];
    const size_t cells = (size_t)cfg->size_x * cfg->size_y, stamp_bytes = (cells + 3) / 4 * 16;
    if (!c.small.p) {
        if ((rc = ensure(h, c.small, 64))) return rc;
        GEM_HIP(h, hipMemsetAsync(c.small.p, 0xff, 64, h->stream));            // no input accepted yet
    }
    if ((rc = ensure(h, m.grid[0], cells)) || (rc = ensure(h, m.grid[1], cells)) || (rc = ensure(h, m.stamps, stamp_bytes))) {
        free_map(m);
        return rc;
    }
    m.cfg = *cfg; m.act = 0;
    m.gen = ++c.generation;
    GEM_HIP(h, hipMemsetAsync(m.stamps.p, 0, stamp_bytes, h->stream));
    GEM_HIP(h, launch_cost_fill(h->stream, grid_of(m), 1, (uint32_t)cells, m.cfg.default_value));
    m.used = true;
    *out_id = id;
    return GEM_OK;
}

int gem_costmap_destroy(gem_handle* h, int id)
{
    GEM_ENTRY("gem_costmap_destroy");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_destroy", &m))) return rc;
    GEM_HIP(h, hipStreamSynchronize(h->stream));
    free_map(*m);
    return GEM_OK;
}

int gem_costmap_geometry(gem_handle* h, int id, gem_costmap_config* out)
{
    GEM_ENTRY("gem_costmap_geometry");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_geometry", &m))) return rc;
    if (!out) return fail(h, GEM_ERR_INVALID, "gem_costmap_geometry: null argument");
    *out = m->cfg;
    return GEM_OK;
}

int gem_costmap_reset(gem_handle* h, int id)
{
    GEM_ENTRY("gem_costmap_reset");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_reset", &m))) return rc;
    GEM_HIP(h, launch_cost_fill(h->stream, grid_of(*m), 1, cells_of(*m), m->cfg.default_value));
    if (m->has_vox) GEM_HIP(h, launch_cost_fill(h->stream, columns_of(*m), 4, cells_of(*m), kVoxUnknown));      // VoxelLayer::resetMaps
    return GEM_OK;
}

int gem_costmap_update_origin(gem_handle* h, int id, double new_origin_x, double new_origin_y)
{
    GEM_ENTRY("gem_costmap_update_origin");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_update_origin", &m))) return rc;
    return update_origin(h, *m, new_origin_x, new_origin_y, "gem_costmap_update_origin");
}

int gem_costmap_roll_to(gem_handle* h, int id, double robot_x, double robot_y)
{
    GEM_ENTRY("gem_costmap_roll_to");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_roll_to", &m))) return rc;
    // getSizeInMetersX() = (size_x - 1 + 0.5) * resolution (costmap_2d.cpp)
    const double mx = (m->cfg.size_x - 1 + 0.5) * m->cfg.resolution, my = (m->cfg.size_y - 1 + 0.5) * m->cfg.resolution;
    return update_origin(h, *m, robot_x - mx / 2, robot_y - my / 2, "gem_costmap_roll_to");
}

int gem_costmap_mark_points(gem_handle* h, int id, const void* points, long long n, double travers_thresh, double bounds[4])
{
    GEM_ENTRY("gem_costmap_mark_points");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_mark_points", &m))) return rc;
    if ((rc = check_cloud(h, "gem_costmap_mark_points", points, n, travers_thresh))) return rc;
    if (n > 0) {
        if ((rc = ensure(h, h->costmap.in, (size_t)n * kRec))) return rc;
        HostXfer x{const_cast<void*>(points), h->costmap.in.p, (size_t)n * kRec};
        if ((rc = upload_arrays(h, &x, 1))) return rc;
    }
    return mark_records(h, *m, static_cast<const LocalRecord*>(h->costmap.in.p), n, travers_thresh, bounds);
}

int gem_costmap_mark_points_device(gem_handle* h, int id, const void* d_points, long long n, double travers_thresh, double bounds[4])
{
    GEM_ENTRY("gem_costmap_mark_points_device");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_mark_points_device", &m))) return rc;
    if ((rc = check_cloud(h, "gem_costmap_mark_points_device", d_points, n, travers_thresh))) return rc;
    return mark_records(h, *m, static_cast<const LocalRecord*>(d_points), n, travers_thresh, bounds);
}

int gem_costmap_mark_grid_cloud(gem_handle* h, int id, double travers_thresh, double bounds[4])
{
    GEM_ENTRY("gem_costmap_mark_grid_cloud");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_mark_grid_cloud", &m))) return rc;
    if (!std::isfinite(travers_thresh)) return fail(h, GEM_ERR_INVALID, "gem_costmap_mark_grid_cloud: travers_thresh not finite");
    CostVisualArgs cap{};
    if (!capture_of(h, &cap)) return fail(h, GEM_ERR_INVALID, "gem_costmap_mark_grid_cloud: the local map is not enabled or has no capture");
    CostPointsArgs a{cap.rec, cap.count, (uint32_t)h->cells, 0u, travers_thresh};
    GEM_HIP(h, launch_cost_mark_points(h->stream, geom_of(*m), a, accum_of(h, *m)));
    return finish_mark(h, *m, bounds);
}

int gem_costmap_mark_global(gem_handle* h, int id, int index, double travers_thresh, double bounds[4])
{
    GEM_ENTRY("gem_costmap_mark_global");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_mark_global", &m))) return rc;
    if (!std::isfinite(travers_thresh)) return fail(h, GEM_ERR_INVALID, "gem_costmap_mark_global: travers_thresh not finite");
    auto& g = h->global;
    if (!g.enabled) return fail(h, GEM_ERR_INVALID, "gem_costmap_mark_global: the submap stack is not enabled (gem_global_enable)");
    const int S = (int)g.cnt.size();
    if (index < -1 || index >= S) return fail(h, GEM_ERR_INVALID, "gem_costmap_mark_global: index out of range");
    const int first = index < 0 ? 0 : index, last = index < 0 ? S : index + 1;
    long long total = 0;
    for (int s = first; s < last; ++s) total += g.cnt[s];
    if (total > kMaxInputs) return fail(h, GEM_ERR_INVALID, "gem_costmap_mark_global: more than 2^31 - 2 records");
    long long at = 0;
    for (int s = first; s < last; ++s) {                                // stack order is input order: the submaps' indices follow each other
        if (!g.cnt[s]) continue;
        CostPointsArgs a{static_cast<const LocalRecord*>(g.stack[g.act].p) + g.off[s], nullptr, (uint32_t)g.cnt[s], (uint32_t)at, travers_thresh};
        GEM_HIP(h, launch_cost_mark_points(h->stream, geom_of(*m), a, accum_of(h, *m)));
        at += g.cnt[s];
    }
    return finish_mark(h, *m, bounds);
}

// PointMapLayer over the history cloud where it lies (gem_hip_history.h): one launch, a workgroup per block of the box table
int gem_costmap_mark_history(gem_handle* h, int id, double travers_thresh, double bounds[4])
{
    GEM_ENTRY("gem_costmap_mark_history");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_mark_history", &m))) return rc;
    if (!std::isfinite(travers_thresh)) return fail(h, GEM_ERR_INVALID, "gem_costmap_mark_history: travers_thresh not finite");
    auto& hs = h->history;
    if (!hs.enabled) return fail(h, GEM_ERR_INVALID, "gem_costmap_mark_history: the history is not enabled (gem_history_enable)");
    if (hs.len > kMaxInputs) return fail(h, GEM_ERR_INVALID, "gem_costmap_mark_history: more than 2^31 - 2 records");
    uint32_t* culled = static_cast<uint32_t*>(hs.small.p);
    GEM_HIP(h, hipMemsetAsync(culled, 0, 4, h->stream));
    if (hs.len > 0) {
        CostPointsArgs a{static_cast<const LocalRecord*>(hs.log[hs.act].p), nullptr, (uint32_t)hs.len, 0u, travers_thresh};
        GEM_HIP(h, launch_cost_mark_history(h->stream, geom_of(*m), a, accum_of(h, *m),
                                            h->history_cull ? static_cast<const float4*>(hs.box.p) : nullptr, culled));
    }
    return finish_mark(h, *m, bounds);
}

int gem_costmap_mark_visual(gem_handle* h, int id, double travers_thresh, double bounds[4])
{
    GEM_ENTRY("gem_costmap_mark_visual");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_mark_visual", &m))) return rc;
    if (!std::isfinite(travers_thresh)) return fail(h, GEM_ERR_INVALID, "gem_costmap_mark_visual: travers_thresh not finite");
    CostVisualArgs a{};
    if (!capture_of(h, &a)) return fail(h, GEM_ERR_INVALID, "gem_costmap_mark_visual: the local map is not enabled or has no capture");
    a.thresh = travers_thresh;
    GEM_HIP(h, launch_cost_mark_visual(h->stream, geom_of(*m), a, accum_of(h, *m)));
    return finish_mark(h, *m, bounds);
}

int gem_costmap_merge(gem_handle* h, int id, int master_id, int min_i, int min_j, int max_i, int max_j, int mode)
{
    GEM_ENTRY("gem_costmap_merge");
    int rc;
    CostMap *m, *master;
    if ((rc = costmap_find(h, id, "gem_costmap_merge", &m)) || (rc = costmap_find(h, master_id, "gem_costmap_merge", &master))) return rc;
    if (m->cfg.size_x != master->cfg.size_x || m->cfg.size_y != master->cfg.size_y)
        return fail(h, GEM_ERR_INVALID, "gem_costmap_merge: the two costmaps differ in size");
    if (!window_ok(*m, min_i, min_j, max_i, max_j)) return fail(h, GEM_ERR_INVALID, "gem_costmap_merge: window outside the map");
    if (mode != 0 && mode != 1) return fail(h, GEM_ERR_INVALID, "gem_costmap_merge: mode is 0 (overwrite) or 1 (max)");
    if (m == master) return GEM_OK;                                      // either rule leaves a map merged onto itself as it is
    GEM_HIP(h, launch_cost_merge(h->stream, grid_of(*m), grid_of(*master), m->cfg.size_x, CostWindow{min_i, min_j, max_i, max_j}, mode));
    return GEM_OK;
}

int gem_costmap_read(gem_handle* h, int id, int min_i, int min_j, int max_i, int max_j, unsigned char* out, size_t row_stride)
{
    GEM_ENTRY("gem_costmap_read");
    CostMap* m;
    if (const int rc = costmap_find(h, id, "gem_costmap_read", &m)) return rc;
    return read_window(h, *m, "gem_costmap_read", grid_of(*m), 1, CostWindow{min_i, min_j, max_i, max_j}, out, row_stride);
}

int gem_costmap_write(gem_handle* h, int id, int min_i, int min_j, int max_i, int max_j, const unsigned char* in, size_t row_stride)
{
    GEM_ENTRY("gem_costmap_write");
    CostMap* m;
    if (const int rc = costmap_find(h, id, "gem_costmap_write", &m)) return rc;
    return write_window(h, *m, "gem_costmap_write", grid_of(*m), 1, CostWindow{min_i, min_j, max_i, max_j}, in, row_stride);
}

} // extern "C"
