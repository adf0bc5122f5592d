"""gem_amd -- MI355X (gfx950) implementation of GEM's point-cloud -> elevation-grid hot path.

The product is libgem_hip.so (hand-written HIP kernels behind the C ABI of include/gem_hip.h);
this package holds its sources (csrc/), the in-tree build (build.py), the ctypes binding (_lib.py)
and a Python mirror of the reference's host interface for that path (api.py).
"""
from .api import (POINT_DTYPE, Costmap, ElevationMap, Frame, GemError, RejectFilter, RobotMotionMapUpdater, SensorModel,  # noqa: F401
                  SensorProcessor, VoxelStage, adjust_plan, contract_sincos, external_critic, inflation_table, map_grid_critic, obstacle_critic,
                  frontiers_host, generate_trajectories, nav_paths_host, nav_plan_host, nav_quad_host, nav_weights, obstacle_host, plan_lists, rollout_answer, rollout_config, rollout_host, rollout_pick, rollout_plan, select_trajectory, trajectory_velocity, trajgen_plan, voxlayer_host)

__all__ = ["POINT_DTYPE", "Costmap", "ElevationMap", "Frame", "GemError", "RejectFilter", "RobotMotionMapUpdater", "SensorModel",
           "SensorProcessor", "VoxelStage", "adjust_plan", "contract_sincos", "external_critic", "inflation_table", "map_grid_critic", "obstacle_critic",
           "frontiers_host", "generate_trajectories", "nav_paths_host", "nav_plan_host", "nav_quad_host", "nav_weights", "obstacle_host", "plan_lists", "rollout_answer", "rollout_config", "rollout_host", "rollout_pick", "rollout_plan", "select_trajectory", "trajectory_velocity", "trajgen_plan", "voxlayer_host"]
