// gem_capi_voxlayer.cpp -- the VoxelLayer entry points of include/gem_hip_voxlayer.h: the voxel columns of a costmap
// (gem_costmap_voxels_create / _destroy / _read / _write), gem_costmap_voxel_observe / _observe_device (the kernels are in
// gem_voxlayer.hip) and the host twin gem_voxlayer_host, which runs the same per-record and per-ray functions (gem_voxlayer.hpp) in
// plain sequential loops, raytraceLine voxel by voxel, and the same byte rule per cell.
//
// State: a costmap's two column grids (gem_handle::Costmaps::Map::vox; gem_capi_costmap.cpp resets, rolls and frees them with the
// bytes); Costmaps::vx_marks and vx_touched, all-zero between calls (the apply kernel clears what it consumes); vx_rays, the ray list;
// `in`, the host clouds behind each other; `win`, the packed window of a read or a write (stage_observations of gem_observe_host.hpp, read_window and
// write_window of gem_costmap_host.hpp).  All come from ensure(), so
// gem_debug_get("arena_allocations") counts them.  Per observation the call enqueues its pass and (clearing) its walk; behind the last
// one launch applies the byte rule.  With mark_threshold above 0 and bounds asked for, the marking clouds are read once more behind it.
#include "gem_observe_host.hpp"
#include "gem_voxlayer.hpp"

#include <algorithm>

namespace {

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
    p.o = obs_params_common(g, o, points, layer_max_h);
    p.o.end_x = g.ox + (g.sx - 1 + 0.5) * g.res; p.o.end_y = g.oy + (g.sy - 1 + 0.5) * g.res;
    p.o.clearing = ((o.flags & GEM_OBS_CLEARING) && vox_cell_float(g, v, p.o.ox, p.o.oy, p.o.oz, p.fx0, p.fy0, p.fz0)) ? 1 : 0;
    p.mark_touches = v.mark_thr == 0u ? 1 : 0;
    return p;
}

int find_with_voxels(gem_handle* h, int id, const char* what, CostMap** m)
{
    if (const int rc = costmap_find(h, id, what, m)) return rc;
    if (!(*m)->has_vox) return fail(h, GEM_ERR_INVALID, (std::string(what) + ": the costmap has no voxels attached").c_str());
    return GEM_OK;
}

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
    const void* points[GEM_OBS_MAX];
    const size_t max_n = longest_observation(c);
    if ((rc = ensure_zeroed(h, cm.vx_marks, (size_t)cells * sizeof(uint32_t))) || (rc = ensure_zeroed(h, cm.vx_touched, (size_t)cells)) ||
        (rc = ensure(h, cm.vx_rays, std::max<size_t>(max_n, 1) * sizeof(unsigned long long))))
        return rc;
    if ((rc = stage_observations(h, c, points))) return rc;

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
        const VoxParams& p = params[k] = params_of(g, v, c.obs[k], points[k], c.layer_max_h);
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
    return read_bounds(h, bounds);
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
    GEM_HIP(h, launch_cost_fill(h->stream, columns_of(*m), 4, cells_of(*m), kVoxUnknown));
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
    CostMap* m;
    if (const int rc = find_with_voxels(h, id, "gem_costmap_voxels_read", &m)) return rc;
    return read_window(h, *m, "gem_costmap_voxels_read", columns_of(*m), sizeof(uint32_t), CostWindow{min_i, min_j, max_i, max_j}, out, row_stride_words);
}

int gem_costmap_voxels_write(gem_handle* h, int id, int min_i, int min_j, int max_i, int max_j, const unsigned* in, size_t row_stride_words)
{
    GEM_ENTRY("gem_costmap_voxels_write");
    CostMap* m;
    if (const int rc = find_with_voxels(h, id, "gem_costmap_voxels_write", &m)) return rc;
    return write_window(h, *m, "gem_costmap_voxels_write", columns_of(*m), sizeof(uint32_t), CostWindow{min_i, min_j, max_i, max_j}, in, row_stride_words);
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
    if (!grid || !columns || !geometry_ok(geom) || !config_ok(voxels) || check_observations(obs, n_obs, layer_max_obstacle_height)) return GEM_ERR_INVALID;
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
