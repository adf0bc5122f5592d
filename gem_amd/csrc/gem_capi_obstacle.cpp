// gem_capi_obstacle.cpp -- the ObstacleLayer entry points of include/gem_hip_obstacle.h: gem_costmap_observe / _observe_device (the
// kernels are in gem_obstacle.hip) and the host twin gem_obstacle_host, which runs the same per-record and per-ray functions
// (gem_obstacle.hpp) in a plain sequential loop, raytraceLine cell by cell.
//
// State (gem_handle::Costmaps): ob_bits, the end-cell and mark bitmaps, all-zero between calls (the kernels clear what they consume);
// ob_rays, the ray list; ob_cnt, the compaction's block counts and total; `in`, the host clouds of gem_costmap_observe behind each
// other (stage_observations of gem_observe_host.hpp).  All come from ensure(), so gem_debug_get("arena_allocations") counts them.  Per observation the call enqueues its pass, then
// (clearing) the compaction and the walk -- or with "obstacle_direct" the walk per record --; behind the last observation one launch
// applies the marks.  Clears and marks commute with nothing in between them, so the stream's order is all the ordering there is.
#include "gem_observe_host.hpp"
#include "gem_compact.hpp"
#include "gem_obstacle.hpp"

#include <algorithm>

namespace {

constexpr long long kMaxRecords = 2147483646ll;                     // 2^31 - 2
static_assert(sizeof(gem_observation) == 80, "gem_observation is 80 bytes");
static_assert(kObsMax == GEM_OBS_MAX && kObsMarking == GEM_OBS_MARKING && kObsClearing == GEM_OBS_CLEARING, "the kernels' constants are the header's");

} // namespace

// the checks of the header's last paragraph that do not need a handle: NULL, or the reason
const char* gemi::check_observations(const gem_observation* obs, int n_obs, double layer_max_h)
{
    if (n_obs < 0 || n_obs > GEM_OBS_MAX || (n_obs > 0 && !obs)) return "0 .. 8 observations, and not NULL";
    if (std::isnan(layer_max_h)) return "layer_max_obstacle_height is NaN";
    long long total = 0;
    for (int k = 0; k < n_obs; ++k) {
        const gem_observation& o = obs[k];
        if (o.n < 0 || o.n > kMaxRecords || (total += o.n) > kMaxRecords) return "a negative count, or more than 2^31 - 2 records";
        if (o.point_step < 12u || (o.point_step & 3u)) return "point_step below 12 or no multiple of 4";
        if (!o.flags || (o.flags & ~(unsigned)(GEM_OBS_MARKING | GEM_OBS_CLEARING))) return "flags empty or with unknown bits";
        if (!std::isfinite(o.origin[0]) || !std::isfinite(o.origin[1]) || !std::isfinite(o.origin[2])) return "an origin is not finite";
        if (!(o.obstacle_range >= 0.0) || !(o.raytrace_range >= 0.0)) return "a range is negative or NaN";
        if (!(o.min_obstacle_height <= o.max_obstacle_height)) return "a height is NaN, or min_obstacle_height > max_obstacle_height";
        if (o.n > 0 && !o.points) return "NULL points with a non-zero count";
    }
    return nullptr;
}

namespace {

// the host's part of an observation: the origin's cell, the map's far edges, the cell range
ObsParams params_of(const CostGeom& g, const gem_observation& o, const void* points, double layer_max_h)
{
    ObsParams p = obs_params_common(g, o, points, layer_max_h);
    p.end_x = g.ox + g.sx * g.res; p.end_y = g.oy + g.sy * g.res;
    p.clearing = ((o.flags & GEM_OBS_CLEARING) && cost_cell_xy(g, p.ox, p.oy, p.x0, p.y0)) ? 1 : 0;
    return p;
}

int observe(gem_handle* h, int id, const ObserveCall& c, double bounds[4])
{
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, c.what, &m))) return rc;
    if (const char* why = check_observations(c.obs, c.n_obs, c.layer_max_h)) return fail(h, GEM_ERR_INVALID, (std::string(c.what) + ": " + why).c_str());
    if (c.n_obs == 0) return GEM_OK;

    const CostGeom g = geom_of(*m);
    const uint32_t cells = cells_of(*m), words = obs_words(cells);
    auto& cm = h->costmap;
    const void* points[GEM_OBS_MAX];
    const size_t max_n = longest_observation(c);
    const size_t nb = (size_t)compact_blocks((long long)cells);
    if ((rc = ensure_zeroed(h, cm.ob_bits, 2 * (size_t)words * sizeof(uint32_t))) || (rc = ensure(h, cm.ob_rays, std::max<size_t>(max_n, 1) * sizeof(uint32_t))) ||
        (rc = ensure(h, cm.ob_cnt, (nb + 1) * sizeof(uint32_t))))
        return rc;
    if ((rc = stage_observations(h, c, points))) return rc;

    unsigned long long* acc = static_cast<unsigned long long*>(cm.small.p);
    ObsScratch s{};
    s.end_bits = static_cast<uint32_t*>(cm.ob_bits.p); s.mark_bits = s.end_bits + words;
    s.rays = static_cast<uint32_t*>(cm.ob_rays.p);
    s.block_cnt = static_cast<uint32_t*>(cm.ob_cnt.p); s.total = s.block_cnt + nb;
    s.acc = acc;
    m->gen = ++cm.generation;                                           // the grid changes: plans, searches and distance grids made before are stale
    for (int k = 0; k < c.n_obs; ++k) {
        const ObsParams p = params_of(g, c.obs[k], points[k], c.layer_max_h);
        if (p.clearing) touch(bounds, p.ox, p.oy);
        if (p.n == 0u || !(p.clearing || p.marking)) continue;
        GEM_HIP(h, launch_obs_pass(h->stream, g, p, s, h->obstacle_direct));
        if (!p.clearing) continue;
        if (h->obstacle_direct) GEM_HIP(h, launch_obs_walk_records(h->stream, g, p, s, grid_of(*m)));
        else GEM_HIP(h, launch_obs_walk_cells(h->stream, g, p, s, grid_of(*m)));
    }
    GEM_HIP(h, launch_obs_apply(h->stream, cells, s.mark_bits, grid_of(*m), acc, acc + 4));
    return read_bounds(h, bounds);
}

} // namespace

extern "C" {

int gem_costmap_observe(gem_handle* h, int id, const gem_observation* obs, int n_obs, double layer_max_obstacle_height, double bounds[4])
{
    GEM_ENTRY("gem_costmap_observe");
    return observe(h, id, ObserveCall{"gem_costmap_observe", obs, n_obs, layer_max_obstacle_height, false}, bounds);
}

int gem_costmap_observe_device(gem_handle* h, int id, const gem_observation* obs, int n_obs, double layer_max_obstacle_height, double bounds[4])
{
    GEM_ENTRY("gem_costmap_observe_device");
    return observe(h, id, ObserveCall{"gem_costmap_observe_device", obs, n_obs, layer_max_obstacle_height, true}, bounds);
}

// the contract, record by record and cell by cell: every clearing observation, then every marking one
int gem_obstacle_host(unsigned char* grid, const gem_costmap_config* geom, const gem_observation* obs, int n_obs, double layer_max_obstacle_height,
                      double bounds[4])
{
    if (!grid || !geometry_ok(geom)) return GEM_ERR_INVALID;
    if (check_observations(obs, n_obs, layer_max_obstacle_height)) return GEM_ERR_INVALID;
    const CostGeom g{geom->origin_x, geom->origin_y, geom->resolution, geom->size_x, geom->size_y};
    for (int pass = 0; pass < 2; ++pass)                                // 0: clearing, 1: marking
        for (int k = 0; k < n_obs; ++k) {
            const ObsParams p = params_of(g, obs[k], obs[k].points, layer_max_obstacle_height);
            if (pass == 0 ? !p.clearing : !p.marking) continue;
            if (pass == 0) touch(bounds, p.ox, p.oy);
            for (size_t i = 0; i < (size_t)p.n; ++i) {
                float r[3];
                memcpy(r, p.points + i * p.step, sizeof(r));
                const double wx = (double)r[0], wy = (double)r[1], wz = (double)r[2];
                if (!obs_in_window(p, wz)) continue;
                if (pass == 0) {
                    uint32_t x1, y1;
                    double ex, ey;
                    if (!obs_clear_record(g, p, wx, wy, x1, y1, ex, ey)) continue;
                    const uint32_t end = obs_ray_end((int)p.x0, (int)p.y0, (int)x1, (int)y1, p.cell_range);
                    for (uint32_t c = 0; c <= end; ++c) {
                        uint32_t cx, cy;
                        obs_line_cell<unsigned long long>((int)p.x0, (int)p.y0, (int)x1, (int)y1, c, cx, cy);
                        grid[(size_t)cy * g.sx + cx] = kCostFree;
                    }
                    touch(bounds, ex, ey);
                } else {
                    uint32_t cell;
                    if (!obs_mark_record(g, p, wx, wy, wz, cell)) continue;
                    grid[cell] = kCostLethal;
                    touch(bounds, wx, wy);
                }
            }
        }
    return GEM_OK;
}

} // extern "C"
