// gem_costmap_host.hpp -- what the costmap family's translation units (gem_capi_costmap / _inflate / _footprint / _mapgrid / _critics /
// _rollout / _navplan / _frontier / _obstacle / _voxlayer .cpp) share on the host: the lookup of a costmap by id, its
// geometry and grids, the staleness checks of a plan and of a frontier search, the read-back of the touched bounds and a window
// of a grid read or written (what ObstacleLayer and VoxelLayer share beyond that is in gem_observe_host.hpp).  Host
// only; the functions are defined in gem_capi_costmap.cpp unless stated.
#pragma once

#include "gem_capi_internal.hpp"
#include "gem_costmap.hpp"

namespace gemi {

using CostMap = gem_handle::Costmaps::Map;

constexpr long long kMaxCells = 1ll << 30;                         // of a costmap

inline unsigned char* grid_of(CostMap& m) { return static_cast<unsigned char*>(m.grid[m.act].p); }
inline uint32_t cells_of(const CostMap& m) { return m.cfg.size_x * m.cfg.size_y; }
inline CostGeom geom_of(const CostMap& m) { return CostGeom{m.cfg.origin_x, m.cfg.origin_y, m.cfg.resolution, m.cfg.size_x, m.cfg.size_y}; }
// the active one of a costmap's two grids of voxel columns, a uint32_t per cell (NULL without voxels attached: Map::has_vox)
inline uint32_t* columns_of(CostMap& m) { return static_cast<uint32_t*>(m.vox[m.vox_act].p); }

// Each fails with GEM_ERR_INVALID and "<what>: <reason>", or returns GEM_OK.
// not on a handle with a communicator, and `id` names a costmap in use
int costmap_find(gem_handle* h, int id, const char* what, CostMap** out);
// the last plan (nav_gen) / the last frontier search (fr_gen) was made, and in the costmap's present generation
int costmap_plan_fresh(gem_handle* h, const CostMap& m, const char* what);
int costmap_search_fresh(gem_handle* h, const CostMap& m, const char* what);

// a geometry a costmap can have (gem_costmap_create's checks): what the host twins of the layers accept
bool geometry_ok(const gem_costmap_config* c);
// cells [min_i, max_i) x [min_j, max_j) lie in the map (an empty window does)
bool window_ok(const CostMap& m, int min_i, int min_j, int max_i, int max_j);
// A window of one of the map's grids (`grid`: elements of `elem` bytes, 1 or 4) to or from the caller's rows, row_stride in elements.
// A partial window goes through Costmaps::win, packed on the device; a wider stride through Costmaps::host_rows.
int read_window(gem_handle* h, CostMap& m, const char* what, void* grid, size_t elem, CostWindow w, void* out, size_t row_stride);
int write_window(gem_handle* h, CostMap& m, const char* what, void* grid, size_t elem, CostWindow w, const void* in, size_t row_stride);

// the checks of gem_hip_obstacle.h's last paragraph that do not need a handle (gem_capi_obstacle.cpp): NULL, or the reason
const char* check_observations(const gem_observation* obs, int n_obs, double layer_max_h);
// the four published bounds words of the call just enqueued (Costmaps::small + 4) merged into the caller's bounds as touch() of costmap_layer.cpp would
int read_bounds(gem_handle* h, double bounds[4]);

} // namespace gemi
