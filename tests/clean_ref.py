"""numpy reference of cleanPointCloud (SensorProcessorBase.cpp:89), the semantics include/gem_hip.h pins:

  REMOVE_NAN     keep i iff x, y, z are all finite (pcl::removeNaNFromPointCloud, is_dense == false), input order kept
  PASSTHROUGH_Z  ... and z_min <= z <= z_max compared in float32 (pcl::PassThrough<PointT> on "z"; PCL keeps its limits as float)
  NONE           keep everything

A plain module the CPU and GPU tests import (not a conftest)."""
import sys

import numpy as np

NONE, REMOVE_NAN, PASSTHROUGH_Z = 0, 1, 2
MODEL_LASER, MODEL_STRUCTURED_LIGHT, MODEL_STEREO, MODEL_PERFECT = range(4)


def to_float32(v: float) -> np.float32:
    """double -> float, round to nearest (what the host does with the cutoffs); beyond the float range -> +-inf."""
    with np.errstate(over="ignore"):
        return np.float32(v)


def params_for_model(kind: int, cutoff_min=None, cutoff_max=None):
    """(mode, z_min, z_max) of gem_clean_params_for_model; None = the reference's numeric_limits<double>::min() / ::max()."""
    if kind == MODEL_STRUCTURED_LIGHT:
        lo = sys.float_info.min if cutoff_min is None else cutoff_min
        hi = sys.float_info.max if cutoff_max is None else cutoff_max
        return PASSTHROUGH_Z, to_float32(lo), to_float32(hi)
    return REMOVE_NAN, np.float32(-np.inf), np.float32(np.inf)


def keep_mask(xyz, mode: int, z_min=-np.inf, z_max=np.inf) -> np.ndarray:
    a = np.asarray(xyz, np.float32)                # [n, 3] or [n, 4]
    if mode == NONE:
        return np.ones(a.shape[0], bool)
    keep = np.isfinite(a[:, 0]) & np.isfinite(a[:, 1]) & np.isfinite(a[:, 2])
    if mode == PASSTHROUGH_Z:
        with np.errstate(invalid="ignore"):
            keep &= (a[:, 2] >= np.float32(z_min)) & (a[:, 2] <= np.float32(z_max))
    return keep


def clean(xyzi, rgb=None, mode: int = REMOVE_NAN, z_min=-np.inf, z_max=np.inf):
    """-> (kept xyzi, kept rgb or None, orig int32): stable compaction."""
    a = np.asarray(xyzi, np.float32).reshape(-1, 4)
    keep = keep_mask(a, mode, z_min, z_max)
    orig = np.flatnonzero(keep).astype(np.int32)
    return a[orig].copy(), (None if rgb is None else np.asarray(rgb)[orig].copy()), orig
