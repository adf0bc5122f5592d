// gem_capi_voxlayer.cpp -- the VoxelLayer entry points of include/gem_hip_voxlayer.h: the voxel columns of a costmap
// (gem_costmap_voxels_create / _destroy / _read / _write), gem_costmap_voxel_observe / _observe_device (the kernels are in
// gem_voxlayer.hip) and the host twin gem_voxlayer_host, which runs the same per-record and per-ray functions (gem_voxlayer.hpp) in
// plain sequential loops, raytraceLine voxel by voxel, and the same byte rule per cell.
//
// State: a costmap's two column grids (gem_handle::Costmaps::Map::vox; gem_capi_costmap.cpp resets, rolls and frees them with the
// bytes); Costmaps::vx_marks and vx_touched, all-zero between calls (the apply kernel clears what it consumes); vx_rays, the ray list;
// `in`, the host clouds behind each other; `win`, the packed window of a read or a write.  All come from ensure(), so
// gem_debug_get("arena_allocations") counts them.  Per observation the call enqueues its pass and (clearing) its walk; behind the last
// one launch applies the byte rule.  With mark_threshold above 0 and bounds asked for, the marking clouds are read once more behind it.
#include "gem_costmap_host.hpp"
#include "gem_voxlayer.hpp"

#include <algorithm>

namespace {

constexpr long long kMaxCells = 1ll << 30;

bool config_ok(const gem_voxel_config* c)
{
    return c && c->size_z >= 1u && c->size_z <= 16u && std::isfinite(c->z_resolution) && c->z_resolution > 0.0 && std::isfinite(c->origin_z) &&
           c->unknown_threshold <= 16u && c->mark_threshold <= 16u;
}

VoxGeom vox_of(const gem_voxel_config& c) { return VoxGeom{c.origin_z, c.z_resolution, c.size_z, c.unknown_threshold, c.mark_threshold}; }

// the host's part of an observation: the map's far edges by getSizeInMeters, the cell range, the sensor's voxel coordinates
VoxParams params_of(const CostGeom& g, const VoxGeom& v, const gem_observation& o, const void* points, double layer_max_h)
{
    VoxParams p{};
    p.o.points = static_cast<const unsigned char*>(points);
    p.o.n = (uint32_t)o.n; p.o.step = o.point_step;
    p.o.ox = o.origin[0]; p.o.oy = o.origin[1]; p.o.oz = o.origin[2];
    p.o.sq_obstacle_range = o.obstacle_range * o.obstacle_range;
    p.o.raytrace_range = o.raytrace_range;
    p.o.min_h = o.min_obstacle_height; p.o.max_h = o.max_obstacle_height; p.o.layer_max_h = layer_max_h;
    p.o.end_x = g.ox + (g.sx - 1 + 0.5) * g.res; p.o.end_y = g.oy + (g.sy - 1 + 0.5) * g.res;
    p.o.cell_range = obs_cell_distance(o.raytrace_range, g.res);
    p.o.marking = (o.flags & GEM_OBS_MARKING) ? 1 : 0;
    p.o.clearing = ((o.flags & GEM_OBS_CLEARING) && vox_cell_float(g, v, p.o.ox, p.o.oy, p.o.oz, p.fx0, p.fy0, p.fz0)) ? 1 : 0;
    p.mark_touches = v.mark_thr == 0u ? 1 : 0;
    return p;
}

void touch(double bounds[4], double x, double y)
{
    if (!bounds) return;
    bounds[0] = obs_std_min(x, bounds[0]); bounds[1] = obs_std_min(y, bounds[1]);
    bounds[2] = obs_std_max(x, bounds[2]); bounds[3] = obs_std_max(y, bounds[3]);
}

bool window_ok(const CostMap& m, int min_i, int min_j, int max_i, int max_j)
{
    return min_i >= 0 && min_j >= 0 && min_i <= max_i && min_j <= max_j && (long long)max_i <= (long long)m.cfg.size_x &&
           (long long)max_j <= (long long)m.cfg.size_y;
}

int find_with_voxels(gem_handle* h, int id, const char* what, CostMap** m)
{
    if (const int rc = costmap_find(h, id, what, m)) return rc;
    if (!(*m)->has_vox) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": the costmap has no voxels attached").c_str());
    return GEM_OK;
}

struct ObserveCall {
    const char* what;
    const gem_observation* obs;
    int n_obs;
    double layer_max_h;
    bool on_device;
};

int observe(gem_handle* h, int id, const ObserveCall& c, double bounds[4])
{
    int rc;
    CostMap* m;
    if ((rc = find_with_voxels(h, id, c.what, &m))) return rc;
    if (const char* why = check_observations(c.obs, c.n_obs, c.layer_max_h)) return fail(h, GEM_ERR_INVALID, (std::string(c.what) + ": " + why).c_str());
    if (c.n_obs == 0) return GEM_OK;

    const CostGeom g = geom_of(*m);
    const VoxGeom v = vox_of(m->vox_cfg);
    const uint32_t cells = cells_of(*m);
    auto& cm = h->costmap;
    size_t max_n = 0, host_bytes = 0, at[GEM_OBS_MAX];
    for (int k = 0; k < c.n_obs; ++k) {
        max_n = std::max(max_n, (size_t)c.obs[k].n);
        at[k] = host_bytes;
        host_bytes += ((size_t)c.obs[k].n * c.obs[k].point_step + 255) / 256 * 256;
    }
    if ((rc = ensure_zeroed(h, cm.vx_marks, (size_t)cells * sizeof(uint32_t))) || (rc = ensure_zeroed(h, cm.vx_touched, (size_t)cells)) ||
        (rc = ensure(h, cm.vx_rays, std::max<size_t>(max_n, 1) * sizeof(unsigned long long))))
        return rc;
    if (!c.on_device && host_bytes) {
        if ((rc = ensure(h, cm.in, host_bytes))) return rc;
        HostXfer up[GEM_OBS_MAX];
        int n_up = 0;
        for (int k = 0; k < c.n_obs; ++k)
            if (c.obs[k].n > 0)
                up[n_up++] = HostXfer{const_cast<void*>(c.obs[k].points), static_cast<unsigned char*>(cm.in.p) + at[k], (size_t)c.obs[k].n * c.obs[k].point_step};
        if (n_up && (rc = upload_arrays(h, up, n_up))) return rc;
    }

    unsigned long long* acc = static_cast<unsigned long long*>(cm.small.p);
    VoxScratch s{};
    s.columns = columns_of(*m);
    s.marks = static_cast<uint32_t*>(cm.vx_marks.p); s.touched = static_cast<unsigned char*>(cm.vx_touched.p);
    s.rays = static_cast<unsigned long long*>(cm.vx_rays.p);
    s.acc = acc;
    m->gen = ++cm.generation;                                           // the grid changes: plans, searches and distance grids made before are stale
    VoxParams params[GEM_OBS_MAX];
    bool late = false;                                                  // marks touch behind the apply: mark_threshold above 0, bounds asked for
    for (int k = 0; k < c.n_obs; ++k) {
        const gem_observation& o = c.obs[k];
        const void* points = c.on_device ? o.points : static_cast<const unsigned char*>(cm.in.p) + at[k];
        const VoxParams& p = params[k] = params_of(g, v, o, points, c.layer_max_h);
        if (p.o.n == 0u || !(p.o.clearing || p.o.marking)) continue;
        GEM_HIP(h, launch_vox_pass(h->stream, g, v, p, s));
        if (p.o.clearing) GEM_HIP(h, launch_vox_walk(h->stream, g, v, p, s));
        if (p.o.marking && !p.mark_touches && bounds) late = true;
    }
    GEM_HIP(h, launch_vox_apply(h->stream, g, v, s, grid_of(*m), !late, acc + 4));
    if (late) {
        for (int k = 0; k < c.n_obs; ++k)
            if (params[k].o.n > 0u && params[k].o.marking) GEM_HIP(h, launch_vox_mark_bounds(h->stream, g, v, params[k], s));
        GEM_HIP(h, launch_vox_publish(h->stream, acc, acc + 4));
    }
    if (!bounds) return GEM_OK;
    unsigned long long w[4];
    HostXfer d{w, acc + 4, sizeof(w)};
    if ((rc = download_arrays(h, &d, 1, 0))) return rc;
    double val;
    for (int k = 0; k < 2; ++k) {
        if (cost_key_decode(w[k], false, &val)) bounds[k] = obs_std_min(val, bounds[k]);
        if (cost_key_decode(w[2 + k], true, &val)) bounds[2 + k] = obs_std_max(val, bounds[2 + k]);
    }
    return GEM_OK;
}

} // namespace

extern "C" {

int gem_costmap_voxels_create(gem_handle* h, int id, const gem_voxel_config* cfg)
{
    GEM_ENTRY("gem_costmap_voxels_create");
    int rc;
    CostMap* m;
    if ((rc = costmap_find(h, id, "gem_costmap_voxels_create", &m))) return rc;
    if (!config_ok(cfg))
        return fail(h, GEM_ERR_INVALID, "gem_costmap_voxels_create: size_z outside 1 .. 16, z_resolution not finite and positive, origin_z not finite, or a threshold above 16");
    if (m->has_vox) return fail(h, GEM_ERR_INVALID, "gem_costmap_voxels_create: the costmap has voxels attached");
    const size_t bytes = (size_t)cells_of(*m) * sizeof(uint32_t);
    if ((rc = ensure(h, m->vox[0], bytes)) || (rc = ensure(h, m->vox[1], bytes))) return rc;
    m->vox_act = 0;
    GEM_HIP(h, launch_vox_fill(h->stream, columns_of(*m), cells_of(*m)));
    m->vox_cfg = *cfg;
    m->has_vox = true;
    return GEM_OK;
}

int gem_costmap_voxels_destroy(gem_handle* h, int id)
{
    GEM_ENTRY("gem_costmap_voxels_destroy");
    int rc;
    CostMap* m;
    if ((rc = find_with_voxels(h, id, "gem_costmap_voxels_destroy", &m))) return rc;
    GEM_HIP(h, hipStreamSynchronize(h->stream));
    for (Arena* a : {&m->vox[0], &m->vox[1]}) {
        if (a->p) hipFree(a->p);
        a->p = nullptr; a->cap = 0;
    }
    m->has_vox = false;
    return GEM_OK;
}

int gem_costmap_voxels_read(gem_handle* h, int id, int min_i, int min_j, int max_i, int max_j, unsigned* out, size_t row_stride_words)
{
    GEM_ENTRY("gem_costmap_voxels_read");
    int rc;
    CostMap* m;
    if ((rc = find_with_voxels(h, id, "gem_costmap_voxels_read", &m))) return rc;
    if (!window_ok(*m, min_i, min_j, max_i, max_j)) return fail(h, GEM_ERR_INVALID, "gem_costmap_voxels_read: window outside the map");
    const size_t w = (size_t)(max_i - min_i), rows = (size_t)(max_j - min_j);
    if (!w || !rows) return GEM_OK;
    if (!out || row_stride_words < w) return fail(h, GEM_ERR_INVALID, "gem_costmap_voxels_read: null output or a row stride below the window's width");
    const bool whole = w == m->cfg.size_x && rows == m->cfg.size_y;
    const uint32_t* src = columns_of(*m);
    if (!whole) {                                                        // a partial window is packed on the device first
        if ((rc = ensure(h, h->costmap.win, w * rows * sizeof(uint32_t)))) return rc;
        GEM_HIP(h, launch_vox_window(h->stream, columns_of(*m), m->cfg.size_x, CostWindow{min_i, min_j, max_i, max_j}, static_cast<uint32_t*>(h->costmap.win.p)));
        src = static_cast<const uint32_t*>(h->costmap.win.p);
    }
    if (row_stride_words == w) {
        HostXfer d{out, const_cast<uint32_t*>(src), w * rows * sizeof(uint32_t)};
        return download_arrays(h, &d, 1, 0);
    }
    std::vector<unsigned char>& tmp = h->costmap.host_rows;             // packed rows, then out at the caller's stride
    tmp.resize(w * rows * sizeof(uint32_t));
    HostXfer d{tmp.data(), const_cast<uint32_t*>(src), w * rows * sizeof(uint32_t)};
    if ((rc = download_arrays(h, &d, 1, 0))) return rc;
    for (size_t r = 0; r < rows; ++r) memcpy(out + r * row_stride_words, tmp.data() + r * w * sizeof(uint32_t), w * sizeof(uint32_t));
    return GEM_OK;
}

int gem_costmap_voxels_write(gem_handle* h, int id, int min_i, int min_j, int max_i, int max_j, const unsigned* in, size_t row_stride_words)
{
    GEM_ENTRY("gem_costmap_voxels_write");
    int rc;
    CostMap* m;
    if ((rc = find_with_voxels(h, id, "gem_costmap_voxels_write", &m))) return rc;
    if (!window_ok(*m, min_i, min_j, max_i, max_j)) return fail(h, GEM_ERR_INVALID, "gem_costmap_voxels_write: window outside the map");
    const size_t w = (size_t)(max_i - min_i), rows = (size_t)(max_j - min_j);
    if (!w || !rows) return GEM_OK;
    if (!in || row_stride_words < w) return fail(h, GEM_ERR_INVALID, "gem_costmap_voxels_write: null input or a row stride below the window's width");
    if ((rc = ensure(h, h->costmap.win, w * rows * sizeof(uint32_t)))) return rc;
    const void* src = in;
    if (row_stride_words != w) {
        std::vector<unsigned char>& tmp = h->costmap.host_rows;
        tmp.resize(w * rows * sizeof(uint32_t));
        for (size_t r = 0; r < rows; ++r) memcpy(tmp.data() + r * w * sizeof(uint32_t), in + r * row_stride_words, w * sizeof(uint32_t));
        src = tmp.data();
    }
    HostXfer x{const_cast<void*>(src), h->costmap.win.p, w * rows * sizeof(uint32_t)};
    if ((rc = upload_arrays(h, &x, 1))) return rc;
    GEM_HIP(h, launch_vox_unpack(h->stream, static_cast<const uint32_t*>(h->costmap.win.p), m->cfg.size_x, CostWindow{min_i, min_j, max_i, max_j},
                                 columns_of(*m)));
    return GEM_OK;
}

int gem_costmap_voxel_observe(gem_handle* h, int id, const gem_observation* obs, int n_obs, double layer_max_obstacle_height, double bounds[4])
{
    GEM_ENTRY("gem_costmap_voxel_observe");
    return observe(h, id, ObserveCall{"gem_costmap_voxel_observe", obs, n_obs, layer_max_obstacle_height, false}, bounds);
}

int gem_costmap_voxel_observe_device(gem_handle* h, int id, const gem_observation* obs, int n_obs, double layer_max_obstacle_height, double bounds[4])
{
    GEM_ENTRY("gem_costmap_voxel_observe_device");
    return observe(h, id, ObserveCall{"gem_costmap_voxel_observe_device", obs, n_obs, layer_max_obstacle_height, true}, bounds);
}

// the contract as a set function: every clearing observation's rays voxel by voxel, every marking observation's accepted marks into a
// word per cell, the byte rule per cell, then the marks' touches
int gem_voxlayer_host(unsigned char* grid, unsigned* columns, const gem_costmap_config* geom, const gem_voxel_config* voxels,
                      const gem_observation* obs, int n_obs, double layer_max_obstacle_height, double bounds[4])
{
    if (!grid || !columns || !geom || geom->size_x == 0 || geom->size_y == 0 || (long long)geom->size_x * geom->size_y > kMaxCells ||
        !std::isfinite(geom->resolution) || !(geom->resolution > 0.0) || !std::isfinite(geom->origin_x) || !std::isfinite(geom->origin_y))
        return GEM_ERR_INVALID;
    if (!config_ok(voxels) || check_observations(obs, n_obs, layer_max_obstacle_height)) return GEM_ERR_INVALID;
    const CostGeom g{geom->origin_x, geom->origin_y, geom->resolution, geom->size_x, geom->size_y};
    const VoxGeom v = vox_of(*voxels);
    const size_t cells = (size_t)g.sx * g.sy;
    std::vector<uint32_t> marks(cells, 0u);
    std::vector<unsigned char> touched(cells, 0);
    for (int pass = 0; pass < 3; ++pass) {                              // 0: clearing, 1: marking, 2: the marks' touches behind the byte rule
        if (pass == 2)
            for (size_t c = 0; c < cells; ++c) {
                unsigned char byte;
                if (vox_cell_byte(v, columns[c], marks[c], touched[c] != 0, &byte)) grid[c] = byte;
                columns[c] |= marks[c];
            }
        for (int k = 0; k < n_obs; ++k) {
            const VoxParams p = params_of(g, v, obs[k], obs[k].points, layer_max_obstacle_height);
            if (pass == 0 ? !p.o.clearing : !p.o.marking) continue;
            for (size_t i = 0; i < (size_t)p.o.n; ++i) {
                float r[3];
                memcpy(r, p.o.points + i * p.o.step, sizeof(r));
                const double wx = (double)r[0], wy = (double)r[1], wz = (double)r[2];
                if (!obs_in_window(p.o, wz)) continue;
                if (pass == 0) {
                    unsigned long long ray;
                    double ex, ey;
                    if (!vox_clear_record(g, v, p, wx, wy, wz, ray, ex, ey)) continue;
                    const uint32_t cell = (uint32_t)ray & 0x3FFFFFFFu, z1 = (uint32_t)(ray >> 30) & 15u, end = (uint32_t)(ray >> 34);
                    const VoxLine line = vox_line((int)p.fx0, (int)p.fy0, (int)p.fz0, (int)(cell % g.sx), (int)(cell / g.sx), (int)z1);
                    for (uint32_t s = 0; s <= end; ++s) {
                        uint32_t cx, cy, cz;
                        vox_line_voxel<unsigned long long>(line, s, cx, cy, cz);
                        const size_t c = (size_t)cy * g.sx + cx;
                        columns[c] &= ~vox_mask(cz);
                        touched[c] = 1;
                    }
                    touch(bounds, ex, ey);
                } else {
                    uint32_t cell, z;
                    if (!vox_mark_record(g, v, p, wx, wy, wz, cell, z)) continue;
                    if (pass == 1) marks[cell] |= vox_mask(z);
                    else if (!vox_below(vox_marked(columns[cell]), v.mark_thr)) touch(bounds, wx, wy);
                }
            }
        }
    }
    return GEM_OK;
}

} // extern "C"
