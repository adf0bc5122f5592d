// gem_observe_host.hpp -- what the two layers that take observations (gem_capi_obstacle.cpp, gem_capi_voxlayer.cpp) share on the host.
// Host only; the functions are defined in gem_capi_costmap.cpp.
#pragma once

#include "gem_costmap_host.hpp"
#include "gem_obstacle.hpp"

namespace gemi {

// one call of an observe entry point (ObstacleLayer's or VoxelLayer's)
struct ObserveCall {
    const char* what;
    const gem_observation* obs;
    int n_obs;
    double layer_max_h;
    bool on_device;
};
// the records of the call's longest observation: what the layers size their ray lists by, before they stage
inline size_t longest_observation(const ObserveCall& c)
{
    size_t n = 0;
    for (int k = 0; k < c.n_obs; ++k) n = c.obs[k].n > (long long)n ? (size_t)c.obs[k].n : n;
    return n;
}
// The clouds of a call where the kernels read them: the caller's device pointers, or the host clouds uploaded behind each other into
// Costmaps::in (each rounded to 256 bytes, one upload_arrays for all).  Behind the layer's own ensure()s, as the launch order was.
int stage_observations(gem_handle* h, const ObserveCall& c, const void* points[GEM_OBS_MAX]);
// the fields of ObsParams that ObstacleLayer and VoxelLayer fill alike: everything but end_x / end_y, the origin's cell and `clearing`
ObsParams obs_params_common(const CostGeom& g, const gem_observation& o, const void* points, double layer_max_h);
// touch() of costmap_layer.cpp: *min = std::min(p, *min), *max = std::max(p, *max); nothing with bounds NULL
void touch(double bounds[4], double x, double y);

} // namespace gemi
