"""ctypes binding of libgem_hip.so (the C ABI declared in include/gem_hip.h).

There is no CPU fallback: if the library is missing it is built with hipcc; if it cannot be
loaded, or no HIP device is present at gem_create time, the error is raised to the caller.
"""
from __future__ import annotations

import ctypes as C
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_longlong, c_uint32, c_void_p

from . import build as _build

GEM_OK = 0

# layers / layouts / models (include/gem_hip.h)
LAYER_ELEVATION, LAYER_VARIANCE, LAYER_INTENSITY, LAYER_TRAVER, LAYER_LOWEST, \
    LAYER_COLOR_R, LAYER_COLOR_G, LAYER_COLOR_B, LAYER_ROUGH, LAYER_SLOPE = range(10)
LAYOUT_STORAGE_ROWMAJOR, LAYOUT_GRIDMAP_COLMAJOR_NAN = 0, 1
MODEL_LASER, MODEL_STRUCTURED_LIGHT, MODEL_STEREO, MODEL_PERFECT = range(4)
CLEAN_NONE, CLEAN_REMOVE_NAN, CLEAN_PASSTHROUGH_Z = range(3)
COMPOSE_SQRT_DOUBLE = 1
COST_FREE_SPACE, COST_LETHAL_OBSTACLE, COST_NO_INFORMATION = 0, 254, 255
COSTMAP_OVERWRITE, COSTMAP_MAX = 0, 1
VOXEL_FIELD_NONE, VOXEL_FIELD_X, VOXEL_FIELD_Y, VOXEL_FIELD_Z, VOXEL_FIELD_INTENSITY = range(5)
DEPTH_U16, DEPTH_F32 = 0, 1
FOOTPRINT_MAX_VERTICES = 32
FOOTPRINT_INSCRIBED_LETHAL, FOOTPRINT_SUM = 1, 2
COST_INSCRIBED_INFLATED_OBSTACLE = 253
INFLATE_MAX_CELLS = 127
COLOR_NONE, COLOR_BGR8, COLOR_RGB8 = range(3)


class MapConfig(C.Structure):
    _fields_ = [("length", c_int), ("resolution", c_float), ("mahalanobis_threshold", c_float),
                ("variance_floor", c_float), ("obstacle_threshold", c_float),
                ("strip_row0", c_int), ("strip_rows", c_int), ("device", c_int)]


class VoxelParams(C.Structure):
    """gem_voxel_params: one pcl::VoxelGrid stage."""
    _fields_ = [("leaf", c_float * 3), ("field", c_int), ("limit_min", c_double), ("limit_max", c_double),
                ("limit_negative", c_int), ("reserved", c_int)]


class ComposeParams(C.Structure):
    """gem_compose_params: the outlier filter and split of gem_local_compose."""
    _fields_ = [("mean_k", c_int), ("stddev_mul", c_double), ("travers_threshold", c_double), ("flags", c_int)]


class OctreeParams(C.Structure):
    """gem_octree_params: a ColorOcTree's resolution and (0 = octomap's defaults) its hit probability and clamps."""
    _fields_ = [("resolution", c_double), ("prob_hit", c_double), ("clamp_min", c_double), ("clamp_max", c_double), ("flags", c_int)]


class OctreeStats(C.Structure):
    """gem_octree_stats"""
    _fields_ = [("points_in", c_longlong), ("points_keyed", c_longlong), ("leaves_depth16", c_longlong), ("pruned_leaves", c_longlong),
                ("nodes", c_longlong), ("bytes", c_longlong), ("coupled_blocks", c_longlong * 3), ("fallback_points", c_longlong)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "coupled_blocks"}
        d["coupled_blocks"] = [int(v) for v in self.coupled_blocks]
        return d


class CostmapConfig(C.Structure):
    """gem_costmap_config: a costmap's geometry and the value of a cell nothing has written."""
    _fields_ = [("size_x", C.c_uint), ("size_y", C.c_uint), ("resolution", c_double), ("origin_x", c_double), ("origin_y", c_double),
                ("default_value", C.c_ubyte)]


class InflationParams(C.Structure):
    """gem_inflation_params: InflationLayer's parameters (cost_scaling_factor is the library's weight_)."""
    _fields_ = [("inflation_radius", c_double), ("inscribed_radius", c_double), ("cost_scaling_factor", c_double), ("inflate_unknown", c_int)]


class FootprintPose(C.Structure):
    """gem_footprint_pose: a pose with the cosine and sine of its heading (the kernels hold no transcendental)."""
    _fields_ = [("x", c_double), ("y", c_double), ("cos_th", c_double), ("sin_th", c_double)]


class RejectFilter(C.Structure):
    _fields_ = [("enabled", c_int), ("box_x", c_float), ("box_y", c_float), ("band_y", c_float), ("plane_y", c_float)]


class FrameParams(C.Structure):
    _fields_ = [("T", c_float * 16), ("lower", c_double), ("upper", c_double), ("sensor_model", c_int),
                ("sensor_params", c_double * 8), ("sensor_jacobian", c_float * 3),
                ("rotation_variance", c_float * 9), ("C_SB_T", c_float * 9), ("P_mul_C_BM_T", c_float * 3),
                ("B_r_BS_skew", c_float * 9), ("filter", RejectFilter), ("original_width", c_int)]


class Camera(C.Structure):
    _fields_ = [("lidar_to_image", c_double * 12), ("width", c_int), ("height", c_int)]


class CleanParams(C.Structure):
    _fields_ = [("mode", c_int), ("z_min", c_float), ("z_max", c_float)]


class DepthImage(C.Structure):
    """gem_depth_image: a depth image's geometry, format and pinhole intrinsics (+ the format of its registered colour image)."""
    _fields_ = [("width", c_int), ("height", c_int), ("format", c_int), ("row_stride", C.c_size_t),
                ("fx", c_double), ("fy", c_double), ("cx", c_double), ("cy", c_double),
                ("depth_unit", c_float), ("intensity", c_float), ("color_format", c_int), ("color_row_stride", C.c_size_t)]


class Stats(C.Structure):
    _fields_ = [("points_in", c_longlong), ("points_binned", c_longlong), ("cells_touched", c_longlong),
                ("ms_bin", c_float), ("ms_fuse", c_float), ("launches_bin", c_int), ("launches_fuse", c_int),
                ("ms_frame", c_float), ("launches_frame", c_int),
                ("ms_sort", c_float * 6), ("launches_sort", c_int), ("ms_walk", c_float), ("launches_walk", c_int)]


# every symbol include/gem_hip.h declares: (restype, argtypes)
SIGNATURES = {
    "gem_abi_version": (c_int, []),
    "gem_create": (c_int, [POINTER(MapConfig), POINTER(c_void_p)]),
    "gem_destroy": (None, [c_void_p]),
    "gem_last_error": (c_char_p, [c_void_p]),
    "gem_set_stream": (c_int, [c_void_p, c_void_p]),
    "gem_synchronize": (c_int, [c_void_p]),
    "gem_wait_event": (c_int, [c_void_p, c_void_p]),
    "gem_move": (c_int, [c_void_p, POINTER(c_float), POINTER(c_float), POINTER(c_int), POINTER(c_float)]),
    "gem_get_pose": (c_int, [c_void_p, POINTER(c_float), POINTER(c_int)]),
    "gem_process_points": (c_int, [c_void_p, POINTER(FrameParams), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gem_fuse": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gem_add": (c_int, [c_void_p, POINTER(FrameParams), c_int, c_void_p, c_void_p, c_void_p]),
    "gem_add_device": (c_int, [c_void_p, POINTER(FrameParams), c_int, c_void_p, c_void_p, c_void_p]),
    "gem_add_batch_device": (c_int, [c_void_p, c_int, POINTER(FrameParams), c_void_p, POINTER(c_longlong), POINTER(c_float)]),
    "gem_add_batch": (c_int, [c_void_p, c_int, POINTER(FrameParams), POINTER(c_void_p), POINTER(c_int), POINTER(c_float)]),
    "gem_mapvar_update": (c_int, [c_void_p, c_float]),
    "gem_get_layer": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "gem_set_layer": (c_int, [c_void_p, c_int, c_void_p]),
    "gem_layer_device_ptr": (c_int, [c_void_p, c_int, POINTER(c_void_p)]),
    "gem_map_feature": (c_int, [c_void_p] + [c_void_p] * 9),
    "gem_map_optmove": (c_int, [c_void_p, POINTER(c_float), c_float, POINTER(c_float)]),
    "gem_map_closeloop": (c_int, [c_void_p, POINTER(c_float), c_float]),
    "gem_set_lowest_tracking": (c_int, [c_void_p, c_int]),
    "gem_add_aos": (c_int, [c_void_p, POINTER(FrameParams), c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int]),
    "gem_raytracing": (c_int, [c_void_p]),
    "gem_set_timing": (c_int, [c_void_p, c_int]),
    "gem_set_counting": (c_int, [c_void_p, c_int]),
    "gem_get_stats": (c_int, [c_void_p, POINTER(Stats), c_int]),
    "gem_comm_unique_id": (c_int, [c_void_p]),
    "gem_comm_init": (c_int, [c_void_p, c_void_p, c_int, c_int]),
    "gem_allgather_layers": (c_int, [c_void_p, c_int]),
    "gem_colorize": (c_int, [c_void_p, POINTER(Camera), c_int, c_void_p, c_void_p, C.c_size_t, c_void_p]),
    "gem_colorize_device": (c_int, [c_void_p, POINTER(Camera), c_int, c_void_p, c_void_p, C.c_size_t, c_void_p]),
    "gem_show": (c_int, [c_void_p, c_double, c_double, POINTER(c_double), c_void_p, c_void_p, c_void_p, POINTER(c_int), c_void_p]),
    "gem_comm_init_tiles": (c_int, [c_void_p, c_void_p, c_int, c_int]),
    "gem_reserve": (c_int, [c_void_p, c_longlong, c_int, c_int]),
    "gem_get_strip": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    "gem_add_sharded_device": (c_int, [c_void_p, c_int, POINTER(FrameParams), c_void_p, POINTER(c_longlong), c_int, c_int, c_int, POINTER(c_float)]),
    "gem_shard_sort_device": (c_int, [c_void_p, c_int, POINTER(FrameParams), c_void_p, POINTER(c_longlong), c_int, c_int, c_int, c_int, POINTER(c_int),
                                      POINTER(c_uint32), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p)]),
    "gem_shard_fuse_device": (c_int, [c_void_p, c_int, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_uint32), POINTER(c_void_p), POINTER(c_uint32),
                                      c_int, POINTER(c_float)]),
    "gem_clean_params_for_model": (c_int, [c_int, c_double, c_double, POINTER(CleanParams)]),
    "gem_clean_device": (c_int, [c_void_p, POINTER(CleanParams), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gem_add_raw": (c_int, [c_void_p, POINTER(FrameParams), POINTER(CleanParams), c_int, c_void_p, c_void_p]),
    "gem_add_raw_device": (c_int, [c_void_p, POINTER(FrameParams), POINTER(CleanParams), c_int, c_void_p, c_void_p]),
    "gem_add_aos_raw": (c_int, [c_void_p, POINTER(FrameParams), POINTER(CleanParams), c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int]),
    "gem_process_points_raw": (c_int, [c_void_p, POINTER(FrameParams), POINTER(CleanParams), c_int, c_void_p, c_void_p, c_void_p,
                                       POINTER(c_int), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gem_voxel_device": (c_int, [c_void_p, POINTER(VoxelParams), c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gem_add_voxel": (c_int, [c_void_p, POINTER(FrameParams), POINTER(VoxelParams), c_int, c_int, c_void_p, c_void_p]),
    "gem_add_voxel_device": (c_int, [c_void_p, POINTER(FrameParams), POINTER(VoxelParams), c_int, c_int, c_void_p, c_void_p]),
    "gem_depth_constants": (c_int, [POINTER(DepthImage), POINTER(c_float)]),
    "gem_depth_unproject_device": (c_int, [c_void_p, POINTER(DepthImage), c_void_p, c_void_p, POINTER(CleanParams), c_void_p, c_void_p]),
    "gem_add_depth": (c_int, [c_void_p, POINTER(FrameParams), POINTER(DepthImage), c_void_p, c_void_p, POINTER(CleanParams),
                              POINTER(VoxelParams), c_int]),
    "gem_add_depth_device": (c_int, [c_void_p, POINTER(FrameParams), POINTER(DepthImage), c_void_p, c_void_p, POINTER(CleanParams),
                                     POINTER(VoxelParams), c_int]),
    "gem_local_enable": (c_int, [c_void_p, c_longlong]),
    "gem_local_capture": (c_int, [c_void_p, c_double, c_double, POINTER(c_double)]),
    "gem_local_keep_previous": (c_int, [c_void_p]),
    "gem_local_grid_cloud": (c_int, [c_void_p, c_void_p, POINTER(c_int)]),
    "gem_local_spill": (c_int, [c_void_p, POINTER(c_float), POINTER(c_float), c_void_p, POINTER(c_int), POINTER(c_int)]),
    "gem_local_export": (c_int, [c_void_p, c_void_p, c_longlong, POINTER(c_longlong), c_int]),
    "gem_local_size": (c_int, [c_void_p, POINTER(c_longlong)]),
    "gem_local_compose": (c_int, [c_void_p, POINTER(ComposeParams), c_void_p, c_void_p, POINTER(c_int), POINTER(c_double)]),
    "gem_local_compose_distances": (c_int, [c_void_p, POINTER(ComposeParams), c_void_p, POINTER(c_int)]),
    "gem_octree_build": (c_int, [c_void_p, c_int, POINTER(OctreeParams), c_void_p, c_longlong, POINTER(OctreeStats)]),
    "gem_octree_build_device": (c_int, [c_void_p, c_int, POINTER(OctreeParams), c_void_p, c_longlong, POINTER(OctreeStats)]),
    "gem_local_compose_octrees": (c_int, [c_void_p, POINTER(ComposeParams), POINTER(OctreeParams), POINTER(OctreeParams), POINTER(c_int),
                                          POINTER(c_double), POINTER(OctreeStats)]),
    "gem_octree_read": (c_int, [c_void_p, c_int, c_void_p, C.c_size_t, POINTER(C.c_size_t)]),
    "gem_global_enable": (c_int, [c_void_p, c_longlong]),
    "gem_global_push_local": (c_int, [c_void_p, c_int, POINTER(c_int)]),
    "gem_global_push": (c_int, [c_void_p, c_void_p, c_longlong, POINTER(c_int)]),
    "gem_global_loop_closure": (c_int, [c_void_p, c_int, POINTER(c_float), POINTER(c_float), c_float, c_double, POINTER(c_longlong)]),
    "gem_global_export": (c_int, [c_void_p, c_int, c_void_p, c_longlong, POINTER(c_longlong)]),
    "gem_global_count": (c_int, [c_void_p, POINTER(c_int)]),
    "gem_costmap_create": (c_int, [c_void_p, POINTER(CostmapConfig), POINTER(c_int)]),
    "gem_costmap_destroy": (c_int, [c_void_p, c_int]),
    "gem_costmap_geometry": (c_int, [c_void_p, c_int, POINTER(CostmapConfig)]),
    "gem_costmap_reset": (c_int, [c_void_p, c_int]),
    "gem_costmap_update_origin": (c_int, [c_void_p, c_int, c_double, c_double]),
    "gem_costmap_roll_to": (c_int, [c_void_p, c_int, c_double, c_double]),
    "gem_costmap_mark_points": (c_int, [c_void_p, c_int, c_void_p, c_longlong, c_double, POINTER(c_double)]),
    "gem_costmap_mark_points_device": (c_int, [c_void_p, c_int, c_void_p, c_longlong, c_double, POINTER(c_double)]),
    "gem_costmap_mark_grid_cloud": (c_int, [c_void_p, c_int, c_double, POINTER(c_double)]),
    "gem_costmap_mark_global": (c_int, [c_void_p, c_int, c_int, c_double, POINTER(c_double)]),
    "gem_costmap_mark_visual": (c_int, [c_void_p, c_int, c_double, POINTER(c_double)]),
    "gem_costmap_merge": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "gem_costmap_read": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, C.c_size_t]),
    "gem_costmap_write": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, C.c_size_t]),
}
# include/gem_hip_history.h (the history cloud; gem_hip.h includes it)
HISTORY_SIGNATURES = {
    "gem_history_enable": (c_int, [c_void_p, c_longlong]),
    "gem_history_append": (c_int, [c_void_p, c_void_p, c_longlong]),
    "gem_history_append_device": (c_int, [c_void_p, c_void_p, c_longlong]),
    "gem_history_reset_from_global": (c_int, [c_void_p]),
    "gem_history_clear": (c_int, [c_void_p]),
    "gem_history_size": (c_int, [c_void_p, POINTER(c_longlong)]),
    "gem_history_export": (c_int, [c_void_p, c_int, c_void_p, c_longlong, POINTER(c_longlong)]),
    "gem_costmap_mark_history": (c_int, [c_void_p, c_int, c_double, POINTER(c_double)]),
}
# include/gem_hip_footprint.h (footprints on the costmap; gem_hip.h includes it)
FOOTPRINT_SIGNATURES = {
    "gem_costmap_clear_footprint": (c_int, [c_void_p, c_int, POINTER(FootprintPose), POINTER(c_double), c_int, POINTER(c_double), POINTER(c_int)]),
    "gem_costmap_footprint_cost": (c_int, [c_void_p, c_int, c_void_p, c_longlong, POINTER(c_double), c_int, c_int, c_void_p]),
    "gem_costmap_footprint_cost_device": (c_int, [c_void_p, c_int, c_void_p, c_longlong, POINTER(c_double), c_int, c_int, c_void_p]),
    "gem_costmap_score_trajectories": (c_int, [c_void_p, c_int, c_void_p, c_longlong, c_int, POINTER(c_double), c_int, c_int, c_void_p, c_void_p]),
    "gem_costmap_score_trajectories_device": (c_int, [c_void_p, c_int, c_void_p, c_longlong, c_int, POINTER(c_double), c_int, c_int, c_void_p, c_void_p]),
}
# include/gem_hip_inflate.h (inflation on the costmap; gem_hip.h includes it)
INFLATE_SIGNATURES = {
    "gem_inflation_table": (c_int, [POINTER(InflationParams), c_double, c_void_p, POINTER(c_int)]),
    "gem_costmap_inflate": (c_int, [c_void_p, c_int, POINTER(InflationParams), c_int, c_int, c_int, c_int]),
    "gem_costmap_reset_window": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int]),
}
# include/gem_hip_mapgrid.h (path and goal distance grids on the costmap; gem_hip.h includes it)
MAPGRID_PATH, MAPGRID_GOAL = 1, 2
MAPGRID_STOP_ON_FAILURE, MAPGRID_SUM = 1, 2
MAPGRID_MAX_POINTS, MAPGRID_MAX_WORDS = 1 << 20, 4096


class MapGridTiledStatus(C.Structure):
    _fields_ = [("started", c_int), ("goal_cell", c_int * 2), ("rounds", c_int), ("chunks", c_int)]


MAPGRID_SIGNATURES = {
    "gem_mapgrid_adjust_plan": (c_int, [POINTER(c_double), c_longlong, c_double, POINTER(c_double), c_longlong, POINTER(c_longlong)]),
    "gem_costmap_mapgrid_prepare": (c_int, [c_void_p, c_int, POINTER(c_double), c_longlong, c_int]),
    "gem_costmap_mapgrid_read": (c_int, [c_void_p, c_int, c_int, c_void_p, POINTER(c_int), POINTER(c_int)]),
    "gem_costmap_mapgrid_score": (c_int, [c_void_p, c_int, c_int, c_void_p, c_longlong, c_int, c_double, c_int, c_void_p]),
    "gem_costmap_mapgrid_score_device": (c_int, [c_void_p, c_int, c_int, c_void_p, c_longlong, c_int, c_double, c_int, c_void_p]),
}
# include/gem_hip_mapgrid_tiled.h (the same grids on a costmap of any size; gem_hip.h includes it)
MAPGRID_TILED_SIGNATURES = {
    "gem_costmap_mapgrid_prepare_tiled": (c_int, [c_void_p, c_int, POINTER(c_double), c_longlong, c_int, POINTER(MapGridTiledStatus)]),
    "gem_costmap_mapgrid_prepare_front_tiled": (c_int, [c_void_p, c_int, POINTER(c_double), c_longlong, POINTER(MapGridTiledStatus)]),
}
# include/gem_hip_critics.h (the best trajectory: the critic list, the FRONT grid; gem_hip.h includes it)
CRITIC_OBSTACLE, CRITIC_MAPGRID, CRITIC_EXTERNAL, CRITIC_MAX = 1, 2, 3, 8
CRITIC_GRID_PATH, CRITIC_GRID_GOAL, CRITIC_GRID_FRONT = 1, 2, 4
CRITIC_CENTRE_COST = 4


class Critic(C.Structure):
    _fields_ = [("kind", c_int), ("grid", c_int), ("flags", c_int), ("column", c_int), ("scale", c_double), ("xshift", c_double)]


class BestTrajectory(C.Structure):
    _fields_ = [("index", c_longlong), ("n_valid", c_longlong), ("cost", c_double), ("reserved", c_longlong)]


_BEST_ARGS = [c_void_p, c_int, POINTER(Critic), c_int, c_void_p, c_void_p, c_longlong, c_int, POINTER(c_double), c_int, c_void_p, c_int,
              c_void_p, c_void_p]
CRITICS_SIGNATURES = {
    "gem_costmap_mapgrid_prepare_front": (c_int, [c_void_p, c_int, POINTER(c_double), c_longlong]),
    "gem_costmap_mapgrid_read_front": (c_int, [c_void_p, c_int, c_void_p, POINTER(c_int), POINTER(c_int)]),
    "gem_costmap_best_trajectory": (c_int, _BEST_ARGS),
    "gem_costmap_best_trajectory_device": (c_int, _BEST_ARGS),
    "gem_critics_select": (c_int, [POINTER(Critic), c_int, POINTER(c_double), c_longlong, POINTER(c_double), POINTER(BestTrajectory)]),
}
# include/gem_hip_trajgen.h (DWA's sampled trajectories: plan, host twin, generation on the device, dwa_best; gem_hip.h includes it)
TRAJGEN_MAX_LIST = 256
OSC_FORWARD_POS_ONLY, OSC_FORWARD_NEG_ONLY, OSC_STRAFE_POS_ONLY, OSC_STRAFE_NEG_ONLY, OSC_ROT_POS_ONLY, OSC_ROT_NEG_ONLY = 1, 2, 4, 8, 16, 32


class TrajgenLimits(C.Structure):
    _fields_ = [(n, c_double) for n in ("max_vel_x", "min_vel_x", "max_vel_y", "min_vel_y", "max_vel_theta", "min_vel_theta", "max_vel_trans",
                                        "min_vel_trans", "acc_lim_x", "acc_lim_y", "acc_lim_theta")]


class TrajgenConfig(C.Structure):
    _fields_ = [("sim_time", c_double), ("sim_granularity", c_double), ("angular_sim_granularity", c_double), ("sim_period", c_double),
                ("use_dwa", c_int), ("discretize_by_time", c_int), ("continued_acceleration", c_int), ("oscillation_flags", c_int),
                ("vsamples", c_int * 3), ("reserved", c_int)]


class DwaPlan(C.Structure):
    _fields_ = [("limits", TrajgenLimits), ("config", TrajgenConfig), ("n_x", c_int), ("n_y", c_int), ("n_th", c_int), ("max_steps", c_int),
                ("n_traj", c_longlong), ("samples", c_float * TRAJGEN_MAX_LIST)]


_F3 = POINTER(c_float)
_DWA_ARGS = [c_void_p, c_int, POINTER(Critic), c_int, POINTER(DwaPlan), _F3, _F3, c_int, POINTER(c_double), c_int, c_void_p, c_void_p]
TRAJGEN_SIGNATURES = {
    "gem_trajgen_plan": (c_int, [POINTER(TrajgenLimits), POINTER(TrajgenConfig), _F3, _F3, _F3, POINTER(DwaPlan)]),
    "gem_trajgen_generate": (c_int, [POINTER(DwaPlan), _F3, _F3, c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "gem_trajgen_velocity": (c_int, [POINTER(DwaPlan), _F3, c_longlong, _F3]),
    "gem_trajgen_sincos": (c_int, [c_void_p, c_longlong, c_void_p, c_void_p]),
    "gem_trajgen_generate_device": (c_int, [c_void_p, POINTER(DwaPlan), _F3, _F3, c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "gem_costmap_dwa_best": (c_int, _DWA_ARGS),
    "gem_costmap_dwa_best_device": (c_int, _DWA_ARGS),
}
# include/gem_hip_rollout.h (trajectory rollout: TrajectoryPlanner::createTrajectories on the costmap; gem_hip.h includes it)
ROLLOUT_MAX_Y_VELS, ROLLOUT_MAX_LIST, ROLLOUT_MAX_STEPS = 8, 256, 4096
ROLLOUT_ESCAPING, ROLLOUT_STUCK_LEFT, ROLLOUT_STUCK_RIGHT, ROLLOUT_STUCK_LEFT_STRAFE, ROLLOUT_STUCK_RIGHT_STRAFE = 1, 2, 4, 8, 16
ROLLOUT_DOUBLES = ("sim_time", "sim_granularity", "angular_sim_granularity", "sim_period", "pdist_scale", "gdist_scale", "occdist_scale",
                   "heading_lookahead", "max_vel_x", "min_vel_x", "max_vel_th", "min_vel_th", "min_in_place_vel_th", "backup_vel", "acc_lim_x",
                   "acc_lim_y", "acc_lim_theta", "final_goal_x", "final_goal_y")
ROLLOUT_INTS = ("vx_samples", "vtheta_samples", "dwa", "holonomic_robot", "final_goal_valid", "n_y_vels")


class RolloutConfig(C.Structure):
    _fields_ = [(n, c_double) for n in ROLLOUT_DOUBLES] + [(n, c_int) for n in ROLLOUT_INTS] + [("y_vels", c_double * ROLLOUT_MAX_Y_VELS)]


class RolloutPlan(C.Structure):
    """struct gem_rollout_plan"""
    _fields_ = [("config", RolloutConfig)] + [(n, c_double) for n in ("max_x", "min_x", "max_th", "min_th", "dvx", "dvth")] + \
               [(n, c_int) for n in ("n_vx", "n_vth", "state_flags", "max_steps", "off_b", "off_c", "off_d", "n_cand")] + \
               [("lists", c_double * ROLLOUT_MAX_LIST)]


class RolloutBest(C.Structure):
    _fields_ = [("index", c_longlong), ("stage", c_int), ("reserved", c_int), ("cost", c_double), ("raw_cost", c_double), ("xv", c_double),
                ("yv", c_double), ("thetav", c_double), ("reserved1", c_longlong)]


_D3 = POINTER(c_double)
_ROLLOUT_ARGS = [c_void_p, c_int, POINTER(RolloutPlan), _D3, _D3, c_int, POINTER(c_double), c_int, c_int, c_void_p, c_void_p, c_void_p]
ROLLOUT_SIGNATURES = {
    "gem_rollout_plan": (c_int, [POINTER(RolloutConfig), _D3, _D3, c_int, POINTER(RolloutPlan)]),
    "gem_rollout_host": (c_int, [POINTER(RolloutPlan), _D3, _D3, POINTER(CostmapConfig), c_void_p, c_void_p, c_void_p, POINTER(c_double), c_int, c_int,
                                 c_void_p, c_void_p, c_void_p, c_void_p, POINTER(RolloutBest)]),
    "gem_rollout_pick": (c_int, [POINTER(RolloutPlan), c_int, c_void_p, c_void_p, POINTER(RolloutBest)]),
    "gem_costmap_rollout_best": (c_int, _ROLLOUT_ARGS),
    "gem_costmap_rollout_best_device": (c_int, _ROLLOUT_ARGS),
}
# include/gem_hip_navplan.h (the global plan on the costmap: weighted potential and grid path; gem_hip.h includes it)
NAV_OUTLINE, NAV_UNREACHED = 1, 0x7FFFFFFF


class NavplanStatus(C.Structure):
    _fields_ = [("found", c_int), ("n_path", c_int), ("rounds", c_int), ("chunks", c_int), ("goal_potential", c_int),
                ("start_cell", c_int * 2), ("goal_cell", c_int * 2)]


NAVPLAN_SIGNATURES = {
    "gem_navplan_weights": (c_int, [c_int, c_double, c_int, c_int, POINTER(c_int)]),
    "gem_navplan_host": (c_int, [c_void_p, c_int, c_int, POINTER(c_int), c_int, POINTER(c_int), POINTER(c_int), c_void_p, c_void_p, c_longlong,
                                 POINTER(NavplanStatus)]),
    "gem_costmap_navplan": (c_int, [c_void_p, c_int, POINTER(c_double), POINTER(c_double), POINTER(c_int), c_int, c_void_p, c_longlong,
                                    POINTER(NavplanStatus)]),
    "gem_costmap_navplan_status": (c_int, [c_void_p, c_int, POINTER(NavplanStatus)]),
    "gem_costmap_navplan_read": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_longlong]),
}
# include/gem_hip_frontier.h (frontier search on the costmap: components, travel cost, one winner; gem_hip.h includes it)


class FrontierParams(C.Structure):
    _fields_ = [("min_frontier_size", c_double), ("potential_scale", c_double), ("gain_scale", c_double)]


class Frontier(C.Structure):
    _fields_ = [("root", c_int), ("size", c_int), ("sum_x", c_longlong), ("sum_y", c_longlong), ("access_potential", c_int),
                ("access_cell", c_int), ("cost", c_double)]


class FrontierStatus(C.Structure):
    _fields_ = [("n_cells", c_int), ("n_frontiers", c_int), ("n_kept", c_int), ("best", c_int), ("rounds", c_int), ("chunks", c_int),
                ("best_frontier", Frontier)]


FRONTIER_SIGNATURES = {
    "gem_frontiers_host": (c_int, [c_void_p, c_void_p, c_int, c_int, c_double, POINTER(FrontierParams), c_void_p, c_void_p, c_longlong,
                                   POINTER(FrontierStatus)]),
    "gem_costmap_frontiers": (c_int, [c_void_p, c_int, POINTER(FrontierParams), POINTER(FrontierStatus)]),
    "gem_costmap_frontiers_read": (c_int, [c_void_p, c_int, c_void_p, c_longlong, c_void_p]),
    "gem_costmap_navplan_goal": (c_int, [c_void_p, c_int, POINTER(c_double), c_void_p, c_longlong, POINTER(NavplanStatus)]),
}
# include/gem_hip_navpath.h (paths on the last plan's potential, grid or gradient, a batch of goals; gem_hip.h includes it)
NAVPATH_GRID, NAVPATH_GRADIENT = 0, 1
NAVPATH_FOUND, NAVPATH_OFF_MAP, NAVPATH_UNREACHED, NAVPATH_HIGH, NAVPATH_ZERO_GRADIENT, NAVPATH_CAP = 1, 2, 3, 4, 5, 6


class NavpathResult(C.Structure):
    _fields_ = [("status", c_int), ("n_points", c_int), ("goal_cell", c_int * 2), ("goal_potential", c_int), ("reserved", c_int * 3)]


_NAVPATHS_ARGS = [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
NAVPATH_SIGNATURES = {
    "gem_navpath_host": (c_int, [c_void_p, c_int, c_int, POINTER(c_int), POINTER(c_int), c_int, c_int, c_void_p, POINTER(NavpathResult)]),
    "gem_costmap_navplan_paths": (c_int, _NAVPATHS_ARGS),
    "gem_costmap_navplan_paths_device": (c_int, _NAVPATHS_ARGS),
}
# include/gem_hip_navquad.h (the quadratic potential on the costmap, order-free and exact; gem_hip.h includes it)
NAVQUAD_MAX_WEIGHT = 462
NAVQUAD_SIGNATURES = {
    "gem_navquad_host": NAVPLAN_SIGNATURES["gem_navplan_host"],
    "gem_costmap_navplan_quadratic": NAVPLAN_SIGNATURES["gem_costmap_navplan"],
}
# include/gem_hip_obstacle.h (ObstacleLayer on the costmap: ray-traced clearing and marking; gem_hip.h includes it)
OBS_MARKING, OBS_CLEARING, OBS_MAX = 1, 2, 8


class Observation(C.Structure):
    """gem_observation: one observation of an ObservationBuffer -- its cloud, the sensor's origin, the two ranges, the height window."""
    _fields_ = [("points", c_void_p), ("n", c_longlong), ("point_step", C.c_uint), ("flags", C.c_uint), ("origin", c_double * 3),
                ("obstacle_range", c_double), ("raytrace_range", c_double), ("min_obstacle_height", c_double), ("max_obstacle_height", c_double)]


OBSTACLE_SIGNATURES = {
    "gem_costmap_observe": (c_int, [c_void_p, c_int, POINTER(Observation), c_int, c_double, POINTER(c_double)]),
    "gem_costmap_observe_device": (c_int, [c_void_p, c_int, POINTER(Observation), c_int, c_double, POINTER(c_double)]),
    "gem_obstacle_host": (c_int, [c_void_p, POINTER(CostmapConfig), POINTER(Observation), c_int, c_double, POINTER(c_double)]),
}
# include/gem_hip_voxlayer.h (VoxelLayer on the costmap: a voxel column per cell, 3-D ray clearing and marking; gem_hip.h includes it)


class VoxelConfig(C.Structure):
    """gem_voxel_config: the third axis of a costmap with voxels attached and the layer's two thresholds."""
    _fields_ = [("size_z", C.c_uint), ("z_resolution", c_double), ("origin_z", c_double), ("unknown_threshold", C.c_uint), ("mark_threshold", C.c_uint)]


VOXLAYER_SIGNATURES = {
    "gem_costmap_voxels_create": (c_int, [c_void_p, c_int, POINTER(VoxelConfig)]),
    "gem_costmap_voxels_destroy": (c_int, [c_void_p, c_int]),
    "gem_costmap_voxels_read": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, C.c_size_t]),
    "gem_costmap_voxels_write": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, C.c_size_t]),
    "gem_costmap_voxel_observe": (c_int, [c_void_p, c_int, POINTER(Observation), c_int, c_double, POINTER(c_double)]),
    "gem_costmap_voxel_observe_device": (c_int, [c_void_p, c_int, POINTER(Observation), c_int, c_double, POINTER(c_double)]),
    "gem_voxlayer_host": (c_int, [c_void_p, c_void_p, POINTER(CostmapConfig), POINTER(VoxelConfig), POINTER(Observation), c_int, c_double,
                                  POINTER(c_double)]),
}
# include/gem_hip_debug.h (tuning knobs / profiling aids, not part of the drop-in surface)
DEBUG_SIGNATURES = {
    "gem_debug_set": (c_int, [c_void_p, c_char_p, c_longlong]),
    "gem_debug_get": (c_int, [c_void_p, c_char_p, POINTER(c_longlong)]),
    "gem_debug_fuse_stamps": (c_int, [c_void_p, c_int, c_void_p, c_int]),
    "gem_comm_init_loopback": (c_int, [c_void_p, c_longlong, c_int, c_int, c_int]),
}

_lib = None


def load(rebuild_if_stale: bool = True) -> C.CDLL:
    """Load (building first if necessary) libgem_hip.so and declare every prototype."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.build() if rebuild_if_stale else _build.LIB
    # A process that also uses PyTorch must end up with ONE HIP runtime / RCCL: torch ships its own
    # copies (torch/lib), and whichever libamdhip64 is mapped first serves both.  Import torch first
    # so device pointers, streams and events are interchangeable between torch and libgem_hip.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(str(path))
    for name, (res, args) in {**SIGNATURES, **HISTORY_SIGNATURES, **FOOTPRINT_SIGNATURES, **INFLATE_SIGNATURES, **MAPGRID_SIGNATURES, **MAPGRID_TILED_SIGNATURES, **CRITICS_SIGNATURES,
                               **TRAJGEN_SIGNATURES, **ROLLOUT_SIGNATURES, **NAVPLAN_SIGNATURES, **FRONTIER_SIGNATURES, **NAVPATH_SIGNATURES, **NAVQUAD_SIGNATURES, **OBSTACLE_SIGNATURES, **VOXLAYER_SIGNATURES, **DEBUG_SIGNATURES}.items():
        fn = getattr(lib, name)          # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def library_path() -> str:
    return str(_build.LIB)
