// gem_costmap_host.hpp -- what the costmap family's translation units (gem_capi_costmap / _inflate / _footprint / _mapgrid / _critics /
// _navplan / _frontier / _obstacle / _voxlayer .cpp) share on the host: the lookup of a costmap by id, its geometry and grid, and the staleness checks of a plan
// and of a frontier search.  Host only; the functions are defined in gem_capi_costmap.cpp.
#pragma once

#include "gem_capi_internal.hpp"
#include "gem_costmap.hpp"

namespace gemi {

using CostMap = gem_handle::Costmaps::Map;

inline unsigned char* grid_of(CostMap& m) { return static_cast<unsigned char*>(m.grid[m.act].p); }
inline uint32_t cells_of(const CostMap& m) { return m.cfg.size_x * m.cfg.size_y; }
inline CostGeom geom_of(const CostMap& m) { return CostGeom{m.cfg.origin_x, m.cfg.origin_y, m.cfg.resolution, m.cfg.size_x, m.cfg.size_y}; }

// Each fails with GEM_ERR_INVALID and "<what>: <reason>", or returns GEM_OK.
// not on a handle with a communicator, and `id` names a costmap in use
int costmap_find(gem_handle* h, int id, const char* what, CostMap** out);
// the last plan (nav_gen) / the last frontier search (fr_gen) was made, and in the costmap's present generation
int costmap_plan_fresh(gem_handle* h, const CostMap& m, const char* what);
int costmap_search_fresh(gem_handle* h, const CostMap& m, const char* what);
// the checks of gem_hip_obstacle.h's last paragraph that do not need a handle (gem_capi_obstacle.cpp): NULL, or the reason
const char* check_observations(const gem_observation* obs, int n_obs, double layer_max_h);
// the active one of a costmap's two grids of voxel columns, a uint32_t per cell (NULL without voxels attached: Map::has_vox)
inline uint32_t* columns_of(CostMap& m) { return static_cast<uint32_t*>(m.vox[m.vox_act].p); }

} // namespace gemi
