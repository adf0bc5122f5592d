"""Host-side mirror of the reference's interface for the hot path, on top of the C ABI.

The reference's callers are ElevationMapping::processpoints / processmapcells / updateMapLocation
(elevation_mapping/src/ElevationMapping.cpp:254-300, 1001-1044), SensorProcessorBase::process /
GPUPointCloudprocess / readcomputerparam (src/sensor_processors/SensorProcessorBase.cpp:66-94,
126-211, 270-290) and RobotMotionMapUpdater::update (src/RobotMotionMapUpdater.cpp:42-90).
The classes below keep those names and argument meanings so the parity tests read like the
reference's call sites; the C++ twin for the unmodified ROS node is include/gem/gem.hpp.

All compute happens in libgem_hip.so on the GPU; there is no CPU path here.
"""
from __future__ import annotations

import atexit
import ctypes as C
import math
import sys
import weakref
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import _lib

# GridMap layer names of the reference (ElevationMap.cpp:43-44) -> device layers (gpu_process.cu:20-28)
LAYER_BY_NAME = {
    "elevation": _lib.LAYER_ELEVATION, "variance": _lib.LAYER_VARIANCE, "intensity": _lib.LAYER_INTENSITY,
    "traver": _lib.LAYER_TRAVER, "lowest_scan_point": _lib.LAYER_LOWEST, "lowest": _lib.LAYER_LOWEST,
    "color_r": _lib.LAYER_COLOR_R, "color_g": _lib.LAYER_COLOR_G, "color_b": _lib.LAYER_COLOR_B,
    "rough": _lib.LAYER_ROUGH, "slope": _lib.LAYER_SLOPE,
}
_INT_LAYERS = {_lib.LAYER_COLOR_R, _lib.LAYER_COLOR_G, _lib.LAYER_COLOR_B}

# PointXYZRGBICT (include/gem/gem.hpp; the reference's Anypoint): the records of the local map (ElevationMap.local_*)
POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1"),
                        ("covariance", "<f4"), ("intensity", "<f4"), ("travers", "<f4")])


class GemError(RuntimeError):
    pass


# handles still alive at interpreter exit are destroyed before the HIP runtime is torn down
_live_maps: "weakref.WeakSet" = weakref.WeakSet()


@atexit.register
def _close_live_maps() -> None:
    for m in list(_live_maps):
        try:
            m.close()
        except Exception:
            pass


def _is_device_tensor(x) -> bool:
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def _host_ptr(a: Optional[np.ndarray], dtype, n: Optional[int] = None):
    """contiguous numpy array of `dtype` -> (keepalive, void*)"""
    if a is None:
        return None, None
    arr = np.ascontiguousarray(a, dtype=dtype)
    if n is not None and arr.size != n:
        raise ValueError(f"expected {n} elements, got {arr.size}")
    return arr, arr.ctypes.data_as(C.c_void_p)


_XYZI_DEVICE = "xyzi must be a contiguous float32 [N,4] device tensor"


def _cloud(xyzi, rgb=None, orig=None, device_only: bool = False):
    """The cloud of add / add_raw / add_voxel, host arrays or device tensors (device_only: float32 device tensors, clean_device /
    voxel_device) -> (on_device, n, (xyzi, rgb, orig) void*s, the host copies the call must keep alive).  Device rgb / orig: at
    least n contiguous 32-bit words on the cloud's device; host ones: n words."""
    if _is_device_tensor(xyzi):
        n = int(xyzi.shape[0])
        if not xyzi.is_contiguous() or xyzi.element_size() != 4 or xyzi.numel() != 4 * n or (device_only and not xyzi.is_floating_point()):
            raise ValueError(_XYZI_DEVICE)
        ptrs = [C.c_void_p(xyzi.data_ptr())]
        for t, what in ((rgb, "rgb"), (orig, "orig_index")):
            if t is not None and (not _is_device_tensor(t) or t.device != xyzi.device or not t.is_contiguous() or t.element_size() != 4
                                  or t.numel() < n):
                raise ValueError(f"{what} must be a contiguous 32-bit device tensor of at least {n} elements on {xyzi.device}")
            ptrs.append(None if t is None else C.c_void_p(t.data_ptr()))
        return True, n, ptrs, None
    if device_only:
        raise ValueError(_XYZI_DEVICE)
    a = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
    n = a.shape[0]
    kr, pr = _host_ptr(rgb, np.uint32, n)
    ko, po = _host_ptr(orig, np.int32, n)
    return False, n, [a.ctypes.data_as(C.c_void_p), pr, po], (a, kr, ko)


def skew(v) -> np.ndarray:
    """kindr::getSkewMatrixFromVector (same matrix as gpu_process.cu:302-307)."""
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=np.float64)


@dataclass
class SensorModel:
    """sensor_processor/* parameters (config/sensor_processors/*.yaml)."""
    kind: int = _lib.MODEL_LASER
    params: Sequence[float] = (0.018, 0.0006, 0.0015)       # velodyne.yaml: min_radius, beam_angle, beam_constant
    ignore_points_above: float = float("inf")               # SensorProcessorBase.cpp:61
    ignore_points_below: float = float("-inf")              # SensorProcessorBase.cpp:62
    original_width: int = 0
    # structured light: sensor_processor/cutoff_min_depth | cutoff_max_depth (StructuredLightSensorProcessor.cpp:40-41); None = the
    # reference's defaults numeric_limits<double>::min() / ::max().  Used by the raw-cloud entries only (clean_params()).
    cutoff_min_depth: Optional[float] = None
    cutoff_max_depth: Optional[float] = None

    @staticmethod
    def velodyne() -> "SensorModel":                         # velodyne.yaml:4-9
        return SensorModel(_lib.MODEL_LASER, (0.018, 0.0006, 0.0015), 0.8, -5.0)

    @staticmethod
    def realsense_d435() -> "SensorModel":                   # realsense_d435.yaml:4-13
        return SensorModel(_lib.MODEL_STRUCTURED_LIGHT, (0.000611, 0.003587, 0.3515, 0.0, 1.0, 0.01576),
                           cutoff_min_depth=0.2, cutoff_max_depth=3.25)

    def clean_params(self) -> "_lib.CleanParams":
        """The cleanPointCloud step SensorProcessorBase::process runs for this model (gem_clean_params_for_model): REMOVE_NAN for
        laser / stereo / perfect, PASSTHROUGH_Z on the float-rounded cutoffs for structured light."""
        lo = sys.float_info.min if self.cutoff_min_depth is None else float(self.cutoff_min_depth)
        hi = sys.float_info.max if self.cutoff_max_depth is None else float(self.cutoff_max_depth)
        out = _lib.CleanParams()
        rc = _lib.load().gem_clean_params_for_model(int(self.kind), lo, hi, C.byref(out))
        if rc != _lib.GEM_OK:
            raise GemError(f"gem_clean_params_for_model failed ({rc})")
        return out

    @staticmethod
    def perfect() -> "SensorModel":
        return SensorModel(_lib.MODEL_PERFECT, ())


@dataclass
class RejectFilter:
    """The hard-coded sensor-frame filter of gpu_process.cu:393; reference() reproduces it."""
    enabled: bool = False
    box_x: float = 1.5
    box_y: float = 1.5
    band_y: float = 1.0
    plane_y: float = 0.0

    @staticmethod
    def reference() -> "RejectFilter":
        return RejectFilter(True)


@dataclass
class VoxelStage:
    """One pcl::VoxelGrid<pcl::PCLPointCloud2> stage as pcl_ros's nodelet runs it (gem_voxel_params; the contract is in
    include/gem_hip.h).  field: None, "x", "y", "z" or "intensity"; PCL's defaults elsewhere."""
    leaf_size: float = 0.01
    field: Optional[str] = None
    limit_min: float = -3.4028234663852886e38
    limit_max: float = 3.4028234663852886e38
    limit_negative: bool = False

    FIELDS = {None: _lib.VOXEL_FIELD_NONE, "": _lib.VOXEL_FIELD_NONE, "x": _lib.VOXEL_FIELD_X, "y": _lib.VOXEL_FIELD_Y,
              "z": _lib.VOXEL_FIELD_Z, "intensity": _lib.VOXEL_FIELD_INTENSITY}

    def to_struct(self) -> "_lib.VoxelParams":
        if self.field not in self.FIELDS:
            raise ValueError(f"voxel filter field {self.field!r}: none, x, y, z or intensity")
        leaf = self.leaf_size if np.ndim(self.leaf_size) else (self.leaf_size,) * 3
        v = _lib.VoxelParams()
        for k in range(3):
            v.leaf[k] = float(np.float32(leaf[k]))                       # the nodelet's double leaf_size, cast to float
        v.field = self.FIELDS[self.field]
        v.limit_min, v.limit_max = float(self.limit_min), float(self.limit_max)
        v.limit_negative = int(bool(self.limit_negative))
        return v

    @staticmethod
    def filter_launch() -> "list[VoxelStage]":
        """filter.launch: one stage, x in [-10, 10], leaf 0.1."""
        return [VoxelStage(0.1, "x", -10.0, 10.0)]

    @staticmethod
    def filter_kitti_launch() -> "list[VoxelStage]":
        """filter_kitti.launch: x in [-40, 40], then z in [-25, 25], then y in [-40, 40], leaf 0.2 each."""
        return [VoxelStage(0.2, "x", -40.0, 40.0), VoxelStage(0.2, "z", -25.0, 25.0), VoxelStage(0.2, "y", -40.0, 40.0)]


def _voxel_stages(stages) -> "C.Array":
    if isinstance(stages, (VoxelStage, _lib.VoxelParams)):
        stages = [stages]
    stages = list(stages)
    if not 1 <= len(stages) <= 4:
        raise ValueError("1 to 4 voxel stages")
    arr = (_lib.VoxelParams * len(stages))()
    for i, st in enumerate(stages):
        arr[i] = st if isinstance(st, _lib.VoxelParams) else st.to_struct()
    return arr


@dataclass
class Frame:
    """Per-frame constants as plain numpy data (what GPUPointCloudprocess derives, SPB.cpp:171-208)."""
    T: np.ndarray                                            # 4x4 float32, sensor -> map
    lower: float
    upper: float
    model: SensorModel
    sensor_jacobian: np.ndarray
    rotation_variance: np.ndarray = field(default_factory=lambda: np.zeros((3, 3), np.float32))
    C_SB_T: np.ndarray = field(default_factory=lambda: np.eye(3, dtype=np.float32))
    P_mul_C_BM_T: np.ndarray = field(default_factory=lambda: np.array([0, 0, 1], np.float32))
    B_r_BS_skew: np.ndarray = field(default_factory=lambda: np.zeros((3, 3), np.float32))
    filter: RejectFilter = field(default_factory=RejectFilter)

    def __setattr__(self, name, value):
        object.__setattr__(self, name, value)
        if name != "_cache":
            object.__setattr__(self, "_cache", {})

    def to_struct(self, cls=_lib.FrameParams):
        """Fill a ctypes struct with the gem_frame_params field layout (also used, with the oracle's
        own struct class, by the tests).  Cached until a field is reassigned."""
        cache = self.__dict__.setdefault("_cache", {})
        if cls in cache:
            return cache[cls]
        p = cache[cls] = cls()
        p.T[:] = np.asarray(self.T, np.float32).reshape(16).tolist()
        p.lower, p.upper = float(self.lower), float(self.upper)
        p.sensor_model = int(self.model.kind)
        sp = list(self.model.params) + [0.0] * (8 - len(self.model.params))
        if hasattr(p, "sensor_params"):
            p.sensor_params[:] = sp
        else:
            p.sp[:] = sp
        p.sensor_jacobian[:] = np.asarray(self.sensor_jacobian, np.float32).reshape(3).tolist()
        p.rotation_variance[:] = np.asarray(self.rotation_variance, np.float32).reshape(9).tolist()
        p.C_SB_T[:] = np.asarray(self.C_SB_T, np.float32).reshape(9).tolist()
        p.P_mul_C_BM_T[:] = np.asarray(self.P_mul_C_BM_T, np.float32).reshape(3).tolist()
        p.B_r_BS_skew[:] = np.asarray(self.B_r_BS_skew, np.float32).reshape(9).tolist()
        if hasattr(p, "filter"):
            p.filter.enabled = int(self.filter.enabled)
            p.filter.box_x, p.filter.box_y = self.filter.box_x, self.filter.box_y
            p.filter.band_y, p.filter.plane_y = self.filter.band_y, self.filter.plane_y
        else:
            p.filter_on = int(self.filter.enabled)
            p.filter_box_x, p.filter_box_y = self.filter.box_x, self.filter.box_y
            p.filter_band_y, p.filter_plane_y = self.filter.band_y, self.filter.plane_y
        p.original_width = int(self.model.original_width)
        return p


class SensorProcessor:
    """SensorProcessorBase (SensorProcessorBase.hpp:52-180) for the GPU path.

    update_transformations() takes what the three TF lookups of SPB.cpp:97-124 return:
    T_map_sensor (map <- sensor), T_base_sensor (base <- sensor), T_map_base (map <- base), 4x4 doubles.
    """

    def __init__(self, model: SensorModel, reject_filter: Optional[RejectFilter] = None,
                 rotation_variance: Optional[np.ndarray] = None):
        self.model = model
        self.filter = reject_filter or RejectFilter()
        self.rotation_variance = np.zeros((3, 3), np.float32) if rotation_variance is None else np.asarray(rotation_variance, np.float32)
        self.update_transformations(np.eye(4), np.eye(4), np.eye(4))

    def update_transformations(self, T_map_sensor, T_base_sensor, T_map_base) -> None:
        self.T_map_sensor = np.asarray(T_map_sensor, np.float64)
        Tbs = np.asarray(T_base_sensor, np.float64)
        Tmb = np.asarray(T_map_base, np.float64)
        self.rotation_base_to_sensor = Tbs[:3, :3].copy()           # SPB.cpp:110
        self.translation_base_to_sensor = Tbs[:3, 3].copy()         # SPB.cpp:111
        self.rotation_map_to_base = Tmb[:3, :3].copy()              # SPB.cpp:116
        self.translation_map_to_base = Tmb[:3, 3].copy()            # SPB.cpp:117

    def frame(self) -> Frame:
        """readcomputerparam (SPB.cpp:270-290) + the casts of GPUPointCloudprocess (SPB.cpp:171-184)."""
        C_BM_T = self.rotation_map_to_base.T
        C_SB_T = self.rotation_base_to_sensor.T
        sensor_jacobian = (C_BM_T @ C_SB_T).astype(np.float32)[2, :]          # :275 e_z^T (double product, float cast)
        C_BM_T_f = C_BM_T.astype(np.float32)
        P_mul = C_BM_T_f[2, :]                                                 # :281-282
        z_base = float(self.translation_map_to_base[2])
        return Frame(
            T=self.T_map_sensor.astype(np.float32),                           # :175-179
            lower=z_base + self.model.ignore_points_below,                    # :183
            upper=z_base + self.model.ignore_points_above,                    # :184
            model=self.model,
            sensor_jacobian=sensor_jacobian,
            rotation_variance=self.rotation_variance,
            C_SB_T=C_SB_T.astype(np.float32),                                 # :283
            P_mul_C_BM_T=P_mul,
            B_r_BS_skew=skew(self.translation_base_to_sensor.astype(np.float32)).astype(np.float32),   # :284
            filter=self.filter,
        )

    def process(self, elevation_map: "ElevationMap", x, y, z, orig_index=None):
        """SensorProcessorBase::process -> Process_points (SPB.cpp:66-94, 208): returns the
        per-point arrays the reference hands to Fuse."""
        return elevation_map.process_points(self.frame(), x, y, z, orig_index)

    def process_raw(self, elevation_map: "ElevationMap", x, y, z):
        """SensorProcessorBase::process on a RAW cloud: cleanPointCloud (SPB.cpp:89) on the device, then Process_points on the kept
        points; the per-point arrays cover the kept points, "orig" holds their raw positions (ElevationMap.process_points_raw)."""
        return elevation_map.process_points_raw(self.frame(), x, y, z, self.model.clean_params())


class PackedBatch:
    """ctypes arrays of one gem_add_batch_device call (ElevationMap.pack_batch)."""
    __slots__ = ("n", "frames", "offsets", "var_updates")


class ElevationMap:
    """The robot-centric map (device-resident; one libgem_hip handle).

    The reference's ElevationMap::add/fuse were deleted from the tree; the map now lives in
    gpu_process.cu's globals and is driven through Init_GPU_elevationmap / Move / Process_points /
    Fuse / Mapvar_update.  This class exposes exactly those operations plus the fused add().
    """

    # knobs applied to every new map through gem_debug_set (include/gem_hip_debug.h); the tests set this to drive all code paths
    default_debug: dict = {}
    base_debug: dict = {}              # applied before default_debug (the GPU tests run every case on both pipelines through this)

    def __init__(self, length: int, resolution: float, mahalanobis_threshold: float = 5.0,
                 variance_floor: float = 1e-4, strip: tuple = (0, 0), device: int = -1, obstacle_threshold: float = 0.7,
                 debug: Optional[dict] = None):
        self._lib = _lib.load()
        cfg = _lib.MapConfig(int(length), float(resolution), float(mahalanobis_threshold), float(variance_floor),
                             float(obstacle_threshold), int(strip[0]), int(strip[1]), int(device))
        h = C.c_void_p()
        rc = self._lib.gem_create(C.byref(cfg), C.byref(h))
        if rc != _lib.GEM_OK:
            raise GemError(f"gem_create failed ({rc}): {self._lib.gem_last_error(None).decode()}")
        self._h = h
        self.length = int(length)
        self.resolution = float(resolution)
        _live_maps.add(self)
        for k, v in {**type(self).base_debug, **type(self).default_debug, **(debug or {})}.items():
            self.debug_set(k, v)

    # -- plumbing ------------------------------------------------------------------------------
    def _check(self, rc: int, what: str) -> None:
        if rc != _lib.GEM_OK:
            raise GemError(f"{what} failed ({rc}): {self._lib.gem_last_error(self._h).decode()}")

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.gem_destroy(self._h)
            self._h = None

    def __del__(self):
        if sys.is_finalizing():          # too late to talk to the HIP runtime
            return
        try:
            self.close()
        except Exception:
            pass

    def debug_set(self, key: str, value: int) -> None:
        """Tuning / test knob (gem_debug_set, include/gem_hip_debug.h): selects between code paths that produce the same map."""
        self._check(self._lib.gem_debug_set(self._h, key.encode(), int(value)), f"gem_debug_set({key})")

    def debug_get(self, key: str) -> int:
        v = C.c_longlong()
        self._check(self._lib.gem_debug_get(self._h, key.encode(), C.byref(v)), f"gem_debug_get({key})")
        return int(v.value)

    def set_stream(self, hip_stream: Optional[int]) -> None:
        self._check(self._lib.gem_set_stream(self._h, C.c_void_p(hip_stream) if hip_stream else None), "gem_set_stream")

    def _hold(self, *tensors) -> None:
        """gem_add_device / gem_add_batch_device only ENQUEUE: the caller's device buffers must stay untouched until gem_synchronize
        (include/gem_hip.h).  A torch tensor that goes out of scope returns its memory to the caching allocator, which hands it to the
        next `.cuda()` at once -- on torch's stream, which knows nothing of the handle's streams.  So the Python twin keeps a reference
        to every device input until the handle is synchronised (tools/fuzz_parity.py passes temporaries; round 6 found that scenario)."""
        held = getattr(self, "_held", None)
        if not isinstance(held, dict):
            held = self._held = {}
        for t in tensors:
            if t is not None:
                held[id(t)] = t                      # (a stream that cycles through the same few tensors holds each once)
        if len(held) > 256:
            self.synchronize()

    def synchronize(self) -> None:
        self._check(self._lib.gem_synchronize(self._h), "gem_synchronize")
        self._held = {}                              # (the device inputs of the calls so far have been read)

    def wait_event(self, hip_event) -> None:
        """Everything enqueued from now on waits (on the device) for this event -- a hipEvent_t handle, or a torch.cuda.Event that
        has been recorded on the stream producing the next call's device buffers (gem_wait_event)."""
        h = getattr(hip_event, "cuda_event", hip_event)
        self._check(self._lib.gem_wait_event(self._h, C.c_void_p(int(h))), "gem_wait_event")

    # -- Move (ElevationMapping::updateMapLocation -> Move, EMg.cpp:1032) ------------------------
    def move(self, position):
        pos = (C.c_float * 3)(*[float(v) for v in position])
        c = (C.c_float * 2)(); s = (C.c_int * 2)(); a = (C.c_float * 2)()
        self._check(self._lib.gem_move(self._h, pos, c, s, a), "gem_move")
        return np.array(c[:], np.float32), np.array(s[:], np.int32), np.array(a[:], np.float32)

    def pose(self):
        c = (C.c_float * 2)(); s = (C.c_int * 2)()
        self._check(self._lib.gem_get_pose(self._h, c, s), "gem_get_pose")
        return np.array(c[:], np.float32), np.array(s[:], np.int32)

    # -- Process_points (SPB.cpp:208) ---------------------------------------------------------------
    def process_points(self, frame: Frame, x, y, z, orig_index=None, write_back_xyz: bool = False):
        n = int(np.asarray(x).size)
        xa = np.array(x, np.float32, copy=True).reshape(-1); ya = np.array(y, np.float32, copy=True).reshape(-1)
        za = np.array(z, np.float32, copy=True).reshape(-1)
        ok, okp = _host_ptr(orig_index, np.int32, n)
        out = {"index": np.empty(n, np.int32), "var": np.empty(n, np.float32), "x_ts": np.empty(n, np.float32),
               "y_ts": np.empty(n, np.float32), "height": np.empty(n, np.float32)}
        p = frame.to_struct()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self._lib.gem_process_points(self._h, C.byref(p), n, vp(xa), vp(ya), vp(za), okp, int(write_back_xyz),
                                                 vp(out["index"]), vp(out["var"]), vp(out["x_ts"]), vp(out["y_ts"]),
                                                 vp(out["height"])), "gem_process_points")
        if write_back_xyz:
            out["x"], out["y"], out["z"] = xa, ya, za
        return out

    # -- Fuse (EMg.cpp:280) --------------------------------------------------------------------------
    def fuse(self, index, height, var, R=None, G=None, B=None, intensity=None) -> None:
        n = int(np.asarray(index).size)
        ki, pi = _host_ptr(index, np.int32, n); kh, ph = _host_ptr(height, np.float32, n); kv, pv = _host_ptr(var, np.float32, n)
        kr, pr = _host_ptr(R, np.int32, n); kg, pg = _host_ptr(G, np.int32, n); kb, pb = _host_ptr(B, np.int32, n)
        kI, pI = _host_ptr(intensity, np.float32, n)
        self._check(self._lib.gem_fuse(self._h, n, pi, pr, pg, pb, pI, ph, pv), "gem_fuse")

    # -- the fused path: process + Fuse in one call (ElevationMapping::processpoints, EMg.cpp:254-283) --
    def add(self, frame: Frame, xyzi, rgb=None, orig_index=None) -> None:
        p = frame.to_struct()
        dev, n, (px, pr, po), keep = _cloud(xyzi, rgb, orig_index)
        if dev:
            self._check(self._lib.gem_add_device(self._h, C.byref(p), n, px, pr, po), "gem_add_device")
            self._hold(xyzi, rgb, orig_index)
        else:
            self._check(self._lib.gem_add(self._h, C.byref(p), n, px, pr, po), "gem_add")

    def add_aos(self, frame: Frame, points: np.ndarray, off_x: int = 0, off_y: int = 4, off_z: int = 8, off_intensity: int = 24,
                off_rgb: int = 16) -> None:
        """The cloud as an array of point structs (numpy structured array or [n, step] bytes), default offsets =
        PointXYZRGBICT (PointXYZRGBICT.hpp:28-46); unpacked on the device (gem_add_aos)."""
        a = np.ascontiguousarray(points)
        n, step = a.shape[0], a.dtype.itemsize * (int(np.prod(a.shape[1:])) if a.ndim > 1 else 1)
        p = frame.to_struct()
        self._check(self._lib.gem_add_aos(self._h, C.byref(p), n, a.ctypes.data_as(C.c_void_p), step, off_x, off_y, off_z,
                                          off_intensity, off_rgb), "gem_add_aos")

    # -- raw clouds: cleanPointCloud (SensorProcessorBase.cpp:89) on the device -----------------------------------------------------
    @staticmethod
    def _clean(clean, frame: Optional[Frame] = None) -> "_lib.CleanParams":
        if clean is None:
            if frame is None:
                raise ValueError("clean parameters needed")
            return frame.model.clean_params()
        if isinstance(clean, SensorModel):
            return clean.clean_params()
        if isinstance(clean, _lib.CleanParams):
            return clean
        raise TypeError("clean: a SensorModel, a CleanParams or None (the frame's model)")

    def clean_device(self, clean, xyzi, rgb=None, sync: bool = True, out=None):
        """gem_clean_device on a float32 [N, 4] device tensor (+ optional int32 / uint32 rgb [N]): returns (xyzi_out [N, 4],
        rgb_out [N] or None, orig [N] int32, count [1] int32), device tensors whose first count rows hold the kept points in input
        order -- new ones, or the four of `out` (a previous call's result, reused).  Enqueued on the handle's stream; with
        sync=False the caller synchronises the handle before reading them."""
        import torch
        _, n, (px, prgb, _), _ = _cloud(xyzi, rgb, device_only=True)
        cp = self._clean(clean)
        if out is not None:
            out, rgb_out, orig, count = out
            if out.shape != xyzi.shape or orig.numel() < n or count.numel() < 1 or (rgb is not None and (rgb_out is None or rgb_out.numel() < n)):
                raise ValueError("clean_device: `out` does not fit this cloud")
            rgb_out = rgb_out if rgb is not None else None
        else:
            out = torch.empty_like(xyzi)
            orig = torch.empty(n, dtype=torch.int32, device=xyzi.device)
            count = torch.zeros(1, dtype=torch.int32, device=xyzi.device)
            rgb_out = torch.empty(n, dtype=torch.int32, device=xyzi.device) if rgb is not None else None
        dp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._check(self._lib.gem_clean_device(self._h, C.byref(cp), n, px, prgb, dp(out), dp(rgb_out), dp(orig), dp(count)),
                    "gem_clean_device")
        self._hold(xyzi, rgb, out, rgb_out, orig, count)
        if sync:
            self.synchronize()
        return out, rgb_out, orig, count

    def add_raw(self, frame: Frame, xyzi, rgb=None, clean=None) -> None:
        """add() of a RAW cloud (NaN holes, out-of-range depths): the cleanPointCloud step of the frame's model -- or `clean` --
        is done on the device (gem_add_raw / gem_add_raw_device); the raw position is every point's orig index."""
        p = frame.to_struct()
        cp = self._clean(clean, frame)
        dev, n, (px, pr, _), keep = _cloud(xyzi, rgb)
        if dev:
            self._check(self._lib.gem_add_raw_device(self._h, C.byref(p), C.byref(cp), n, px, pr), "gem_add_raw_device")
            self._hold(xyzi, rgb)
        else:
            self._check(self._lib.gem_add_raw(self._h, C.byref(p), C.byref(cp), n, px, pr), "gem_add_raw")

    # -- the VoxelGrid pre-filter of the launch files (pcl/VoxelGrid nodelets) on the device ------------------------------------------
    def voxel_device(self, stages, xyzi, rgb=None, sync: bool = True, out=None):
        """gem_voxel_device on a float32 [N, 4] device tensor (+ optional 32-bit rgb [N]): returns (xyzi_out [N, 4], rgb_out [N] or
        None, count [1] int32), device tensors whose first count rows hold the centroids in voxel order and whose tail has NaN x, y, z
        -- new ones, or the three of `out` (a previous call's result, reused).  Enqueued on the handle's stream; with sync=False the
        caller synchronises the handle before reading them."""
        import torch
        _, n, (px, prgb, _), _ = _cloud(xyzi, rgb, device_only=True)
        arr = _voxel_stages(stages)
        if out is not None:
            out, rgb_out, count = out
            if out.shape != xyzi.shape or count.numel() < 1 or (rgb is not None and (rgb_out is None or rgb_out.numel() < n)):
                raise ValueError("voxel_device: `out` does not fit this cloud")
            rgb_out = rgb_out if rgb is not None else None
        else:
            out = torch.empty_like(xyzi)
            count = torch.zeros(1, dtype=torch.int32, device=xyzi.device)
            rgb_out = torch.empty(n, dtype=torch.int32, device=xyzi.device) if rgb is not None else None
        dp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._check(self._lib.gem_voxel_device(self._h, arr, len(arr), n, px, prgb, dp(out), dp(rgb_out), dp(count)),
                    "gem_voxel_device")
        self._hold(xyzi, rgb, out, rgb_out, count)
        if sync:
            self.synchronize()
        return out, rgb_out, count

    def add_voxel(self, frame: Frame, stages, xyzi, rgb=None) -> None:
        """add() behind the VoxelGrid stages (gem_add_voxel / gem_add_voxel_device): the map of add() on the centroids, orig index =
        position in the filtered cloud."""
        p = frame.to_struct()
        arr = _voxel_stages(stages)
        dev, n, (px, pr, _), keep = _cloud(xyzi, rgb)
        if dev:
            self._check(self._lib.gem_add_voxel_device(self._h, C.byref(p), arr, len(arr), n, px, pr), "gem_add_voxel_device")
            self._hold(xyzi, rgb)
        else:
            self._check(self._lib.gem_add_voxel(self._h, C.byref(p), arr, len(arr), n, px, pr), "gem_add_voxel")

    # -- depth images: the pinhole unprojection (depth_image_proc::convert, restated in include/gem_hip.h) on the device ---------------
    @staticmethod
    def _depth_images(image: "_lib.DepthImage", depth, color, device_only: bool = False):
        """The images of depth_unproject / add_depth, numpy arrays or device tensors laid out as `image` says (rows row_stride bytes
        apart, 0 = tight) -> (on_device, depth void*, colour void*, what the call must keep alive).  Each must reach to the end of
        its last row; None is passed on as NULL (the library rejects it where there are pixels)."""
        w, h = int(image.width), int(image.height)
        esz = 2 if image.format == _lib.DEPTH_U16 else 4
        need = [0, 0]
        if w > 0 and h > 0:
            need = [(h - 1) * (int(image.row_stride) or w * esz) + w * esz, (h - 1) * (int(image.color_row_stride) or w * 3) + w * 3]
        on_device = _is_device_tensor(depth)
        if device_only and depth is not None and not on_device:
            raise ValueError("depth must be a device tensor")
        ptrs, keep = [], []
        for t, what, size, nbytes in ((depth, "depth", esz, need[0]), (color, "color", 1, need[1])):
            if t is None:
                ptrs.append(None)
            elif on_device:
                if not _is_device_tensor(t) or t.device != depth.device or t.element_size() != size:
                    raise ValueError(f"{what} must be a device tensor of {size}-byte elements on {depth.device}")
                if t.untyped_storage().nbytes() - t.storage_offset() * size < nbytes:
                    raise ValueError(f"{what} ends before the image's last row ({nbytes} bytes)")
                ptrs.append(C.c_void_p(t.data_ptr())); keep.append(t)
            else:
                a = np.ascontiguousarray(t)
                if a.dtype.itemsize != size or a.nbytes < nbytes:
                    raise ValueError(f"{what} must be an array of {size}-byte elements of at least {nbytes} bytes")
                ptrs.append(a.ctypes.data_as(C.c_void_p)); keep.append(a)
        return on_device, ptrs[0], ptrs[1], keep

    def depth_unproject(self, image: "_lib.DepthImage", depth, color=None, clean=None, sync: bool = True):
        """gem_depth_unproject_device: the organised cloud of a depth image (a uint16 / float32 device tensor laid out as `image`
        says, + an optional uint8 colour image) -> (xyzi [H * W, 4] float32, rgb [H * W] int32 or None), new device tensors.  `clean`:
        a SensorModel or CleanParams whose PASSTHROUGH_Z mask is applied in the same kernel, None for the plain cloud.  Enqueued on
        the handle's stream; with sync=False the caller synchronises the handle before reading them."""
        import torch
        _, pd, pc, keep = self._depth_images(image, depth, color, device_only=True)
        if depth is None:
            raise ValueError("depth must be a device tensor")
        n = max(int(image.width), 0) * max(int(image.height), 0)
        cp = None if clean is None else self._clean(clean)
        out = torch.empty((n, 4), dtype=torch.float32, device=depth.device)
        rgb_out = torch.empty(n, dtype=torch.int32, device=depth.device) if color is not None and image.color_format != _lib.COLOR_NONE else None
        dp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._check(self._lib.gem_depth_unproject_device(self._h, C.byref(image), pd, pc, None if cp is None else C.byref(cp), dp(out), dp(rgb_out)),
                    "gem_depth_unproject_device")
        self._hold(depth, color, out, rgb_out)
        if sync:
            self.synchronize()
        return out, rgb_out

    def add_depth(self, frame: Frame, image: "_lib.DepthImage", depth, color=None, clean=None, stages=None) -> None:
        """add_raw() -- or, with `stages`, add_voxel() -- of the cloud a depth image unprojects to, without that cloud ever crossing
        the link: numpy images go through gem_add_depth (read before the call returns), device tensors through gem_add_depth_device
        (held until synchronize()).  `clean` as for add_raw (None: the frame's model); it and `stages` exclude each other."""
        p = frame.to_struct()
        arr = None if stages is None else _voxel_stages(stages)
        if arr is not None and clean is not None:
            raise ValueError("add_depth: clean and stages exclude each other")
        cp = None if arr is not None else self._clean(clean, frame)
        dev, pd, pc, keep = self._depth_images(image, depth, color)
        fn, what = (self._lib.gem_add_depth_device, "gem_add_depth_device") if dev else (self._lib.gem_add_depth, "gem_add_depth")
        self._check(fn(self._h, C.byref(p), C.byref(image), pd, pc, None if cp is None else C.byref(cp), arr, 0 if arr is None else len(arr)), what)
        if dev:
            self._hold(depth, color)

    def add_aos_raw(self, frame: Frame, points: np.ndarray, off_x: int = 0, off_y: int = 4, off_z: int = 8, off_intensity: int = 24,
                    off_rgb: int = 16, clean=None) -> None:
        """add_aos() of a RAW cloud of point structs (gem_add_aos_raw)."""
        a = np.ascontiguousarray(points)
        n, step = a.shape[0], a.dtype.itemsize * (int(np.prod(a.shape[1:])) if a.ndim > 1 else 1)
        p = frame.to_struct()
        cp = self._clean(clean, frame)
        self._check(self._lib.gem_add_aos_raw(self._h, C.byref(p), C.byref(cp), n, a.ctypes.data_as(C.c_void_p), step, off_x, off_y, off_z,
                                              off_intensity, off_rgb), "gem_add_aos_raw")

    def process_points_raw(self, frame: Frame, x, y, z, clean=None):
        """process_points() of a RAW cloud (gem_process_points_raw): the arrays cover the kept points only, in order; "orig" holds
        their raw positions and "n_kept" their number."""
        n = int(np.asarray(x).size)
        xa = np.ascontiguousarray(x, np.float32).reshape(-1); ya = np.ascontiguousarray(y, np.float32).reshape(-1)
        za = np.ascontiguousarray(z, np.float32).reshape(-1)
        if ya.size != n or za.size != n:
            raise ValueError("x, y, z differ in length")
        cp = self._clean(clean, frame)
        out = {"orig": np.empty(n, np.int32), "index": np.empty(n, np.int32), "var": np.empty(n, np.float32),
               "x_ts": np.empty(n, np.float32), "y_ts": np.empty(n, np.float32), "height": np.empty(n, np.float32)}
        k = C.c_int()
        p = frame.to_struct()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self._lib.gem_process_points_raw(self._h, C.byref(p), C.byref(cp), n, vp(xa), vp(ya), vp(za), C.byref(k), vp(out["orig"]),
                                                     vp(out["index"]), vp(out["var"]), vp(out["x_ts"]), vp(out["y_ts"]), vp(out["height"])),
                    "gem_process_points_raw")
        kept = int(k.value)
        res = {key: v[:kept].copy() for key, v in out.items()}
        res["n_kept"] = kept
        return res

    @staticmethod
    def pack_batch(frames: Sequence[Frame], offsets, var_updates=None) -> "PackedBatch":
        """The C-ABI arrays of a batched call, built once (32 frames cost ~0.3 ms of ctypes conversion per call otherwise)."""
        ns = len(frames)
        pb = PackedBatch()
        pb.n = ns
        pb.frames = (_lib.FrameParams * ns)(*[f.to_struct() for f in frames])
        pb.offsets = (C.c_longlong * (ns + 1))(*[int(v) for v in offsets])
        pb.var_updates = (C.c_float * ns)(*[float(v) for v in var_updates]) if var_updates is not None else None
        return pb

    def add_batch(self, frames, xyzi_device, offsets=None, var_updates=None) -> None:
        """BASELINE config 4: for each sweep s: Mapvar_update(var_updates[s]); add(frames[s], cloud s).
        `frames` is a sequence of Frame (with `offsets` [, `var_updates`]) or a PackedBatch from pack_batch()."""
        pb = frames if isinstance(frames, PackedBatch) else self.pack_batch(frames, offsets, var_updates)
        if not _is_device_tensor(xyzi_device):
            raise ValueError("add_batch takes a device-resident float32 [N,4] tensor")
        self._check(self._lib.gem_add_batch_device(self._h, pb.n, pb.frames, C.c_void_p(xyzi_device.data_ptr()), pb.offsets,
                                                   pb.var_updates), "gem_add_batch_device")
        self._hold(xyzi_device)

    def add_batch_host(self, frames, clouds, var_updates=None) -> None:
        """The same from HOST memory (gem_add_batch): `clouds` is a sequence of float32 [n_s, 4] numpy arrays, one per
        sweep; `frames` a sequence of Frame or a PackedBatch (whose offsets are not used: the arrays carry their own lengths)."""
        arrs = [np.ascontiguousarray(c, np.float32).reshape(-1, 4) for c in clouds]
        ns = len(arrs)
        if isinstance(frames, PackedBatch):
            if frames.n != ns:
                raise ValueError("one cloud per frame")
            fr, vu = frames.frames, frames.var_updates
        else:
            if len(frames) != ns:
                raise ValueError("one cloud per frame")
            fr = (_lib.FrameParams * ns)(*[f.to_struct() for f in frames])
            vu = (C.c_float * ns)(*[float(v) for v in var_updates]) if var_updates is not None else None
        ptrs = (C.c_void_p * ns)(*[a.ctypes.data for a in arrs])
        counts = (C.c_int * ns)(*[a.shape[0] for a in arrs])
        self._check(self._lib.gem_add_batch(self._h, ns, fr, ptrs, counts, vu), "gem_add_batch")

    # -- Mapvar_update (RMU.cpp:81) ------------------------------------------------------------------
    def reserve(self, max_points: int, max_sweeps: int = 1, with_colours: bool = False) -> None:
        """Pre-size the device arenas for the largest pass to come (gem_reserve): no pass within these bounds allocates afterwards."""
        self._check(self._lib.gem_reserve(self._h, int(max_points), int(max_sweeps), int(with_colours)), "gem_reserve")

    def mapvar_update(self, var_update: float) -> None:
        self._check(self._lib.gem_mapvar_update(self._h, float(var_update)), "gem_mapvar_update")

    # -- loop-closure re-anchoring (Map_optmove, EMg.cpp:1020; Map_closeloop) -------------------------------------
    def map_optmove(self, opt_xy, height_update: float) -> np.ndarray:
        p = (C.c_float * 2)(float(opt_xy[0]), float(opt_xy[1])); out = (C.c_float * 2)()
        self._check(self._lib.gem_map_optmove(self._h, p, float(height_update), out), "gem_map_optmove")
        return np.array([out[0], out[1]], np.float32)

    def map_closeloop(self, xy, height_update: float) -> None:
        p = (C.c_float * 2)(float(xy[0]), float(xy[1]))
        self._check(self._lib.gem_map_closeloop(self._h, p, float(height_update)), "gem_map_closeloop")

    # -- Map_feature (EMg.cpp:410): traversability stage on the fused map --------------------------------------
    # -- visibility clean-up (Raytracing, EMg.cpp:421) --------------------------------------------------------------
    def set_lowest_tracking(self, on: bool) -> None:
        """Maintain the lowest-scan-point layer (gpu_process.cu:430-439) in the fuse kernels; needed by raytracing()."""
        self._check(self._lib.gem_set_lowest_tracking(self._h, int(bool(on))), "gem_set_lowest_tracking")

    def raytracing(self) -> None:
        self._check(self._lib.gem_raytracing(self._h), "gem_raytracing")

    def map_feature(self, fetch: bool = True):
        """Computes the rough / slope / traver layers on the device (gem_map_feature).  With fetch=True returns
        dict(rough, slope, traver) as host arrays; with fetch=False it only enqueues the kernel."""
        L = self.length
        if not fetch:
            self._check(self._lib.gem_map_feature(self._h, *([None] * 9)), "gem_map_feature")
            return None
        out = {k: np.empty((L, L), np.float32) for k in ("rough", "slope", "traver")}
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self._lib.gem_map_feature(self._h, None, None, None, None, None, p(out["rough"]), p(out["slope"]),
                                              p(out["traver"]), None), "gem_map_feature")
        return out

    # -- the feed of ElevationMap::show (ElevationMap.cpp:85-149) ------------------------------------------------------------------
    def show(self, map_length: float = 0.0, resolution: float = 0.0, position=None):
        """visualMap_'s nine layers ([9, L, L], grid_map's column-major layout, NaN for cells without elevation / traversability),
        the coloured point cloud (device-compacted, reference order) and the orthomosaic, from the resident layers (gem_show)."""
        L = self.length
        visual = np.empty((9, L * L), np.float32); xyz = np.empty((L * L, 3), np.float32); rgb = np.empty((L * L, 3), np.uint8)
        img = np.empty((L, L, 3), np.uint8)
        n = C.c_int()
        pos = None if position is None else (C.c_double * 2)(float(position[0]), float(position[1]))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self._lib.gem_show(self._h, float(map_length), float(resolution), pos, vp(visual), vp(xyz), vp(rgb), C.byref(n), vp(img)), "gem_show")
        k = int(n.value)
        return {"visual": visual.reshape(9, L, L), "points_xyz": xyz[:k].copy(), "points_rgb": rgb[:k].copy(), "image_bgr": img, "count": k}

    # -- the rolling-window local map (updateLocalMap, EMg.cpp:609-767; visualPointMap, :520-530) ---------------
    def local_enable(self, capacity: int = 1 << 16) -> None:
        """Switch the device local map on, empty, with room for `capacity` entries (it grows on demand); 0 switches it off and
        frees its memory (gem_local_enable)."""
        self._check(self._lib.gem_local_enable(self._h, int(capacity)), "gem_local_enable")

    def local_capture(self, map_length: float = 0.0, resolution: float = 0.0, position=None) -> None:
        """What show() leaves in visualMap_, with its geometry (gem_show's rules).  Between map_feature() and raytracing()."""
        pos = None if position is None else (C.c_double * 2)(float(position[0]), float(position[1]))
        self._check(self._lib.gem_local_capture(self._h, float(map_length), float(resolution), pos), "gem_local_capture")

    def local_keep_previous(self) -> None:
        """prevMap_ = visualMap_ (EMg.cpp:422): the last capture becomes the previous one."""
        self._check(self._lib.gem_local_keep_previous(self._h), "gem_local_keep_previous")

    def local_grid_cloud(self) -> np.ndarray:
        """gridMaptoPointCloud of the last capture (EMg.cpp:1198-1224): POINT_DTYPE records in iteration order."""
        out = np.empty(self.length * self.length, POINT_DTYPE)
        n = C.c_int()
        self._check(self._lib.gem_local_grid_cloud(self._h, out.ctypes.data_as(C.c_void_p), C.byref(n)), "gem_local_grid_cloud")
        return out[:n.value].copy()

    def local_spill(self, current_position, position_shift, download: bool = True):
        """The "Local mapping" block of updateLocalMap (EMg.cpp:715-764) without its gate, on the previous capture: returns
        (records spilled in iteration order, replaced = the reference's `count`).  Positions and shifts are taken as float.
        download=False leaves the records on the device (the history cloud takes them there while it is enabled) and returns
        (their number, replaced)."""
        cp = (C.c_float * 2)(*[float(np.float32(v)) for v in current_position[:2]])
        ps = (C.c_float * 2)(*[float(np.float32(v)) for v in position_shift[:2]])
        n, rep = C.c_int(), C.c_int()
        if not download:
            self._check(self._lib.gem_local_spill(self._h, cp, ps, None, C.byref(n), C.byref(rep)), "gem_local_spill")
            return int(n.value), int(rep.value)
        out = np.empty(self.length * self.length, POINT_DTYPE)
        self._check(self._lib.gem_local_spill(self._h, cp, ps, out.ctypes.data_as(C.c_void_p), C.byref(n), C.byref(rep)), "gem_local_spill")
        return out[:n.value].copy(), int(rep.value)

    def local_export(self, clear: bool = False) -> np.ndarray:
        """localHashtoPointCloud (EMg.cpp:1124-1140) in last-write order; clear=True empties the local map afterwards."""
        out = np.empty(max(self.local_size(), 1), POINT_DTYPE)
        n = C.c_longlong()
        self._check(self._lib.gem_local_export(self._h, out.ctypes.data_as(C.c_void_p), out.shape[0], C.byref(n), int(bool(clear))),
                    "gem_local_export")
        return out[:n.value].copy()

    def local_size(self) -> int:
        n = C.c_longlong()
        self._check(self._lib.gem_local_size(self._h, C.byref(n)), "gem_local_size")
        return int(n.value)

    # -- composingGlobalMap's filter and split (pointCloudtoOctomap, EMg.cpp:1146-1170) on the previous capture -----------------
    @staticmethod
    def _compose_params(mean_k, stddev_mul, travers_threshold, sqrt_double):
        return _lib.ComposeParams(int(mean_k), float(stddev_mul), float(travers_threshold), _lib.COMPOSE_SQRT_DOUBLE if sqrt_double else 0)

    def local_compose(self, mean_k: int = 20, stddev_mul: float = 1.0, travers_threshold: float = 0.0, sqrt_double: bool = False,
                      want_road: bool = True, want_obstacle: bool = True):
        """StatisticalOutlierRemoval(mean_k, stddev_mul) on the previous capture's grid cloud, then the split by travers
        (gem_local_compose): returns (road, obstacle, removed, threshold); a list that was not asked for comes back as its count."""
        p = self._compose_params(mean_k, stddev_mul, travers_threshold, sqrt_double)
        cells = self.length * self.length
        road = np.empty(cells, POINT_DTYPE) if want_road else None
        obst = np.empty(cells, POINT_DTYPE) if want_obstacle else None
        counts, thr = (C.c_int * 3)(), C.c_double()
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._check(self._lib.gem_local_compose(self._h, C.byref(p), vp(road), vp(obst), counts, C.byref(thr)), "gem_local_compose")
        return (road[:counts[0]].copy() if want_road else int(counts[0]), obst[:counts[1]].copy() if want_obstacle else int(counts[1]),
                int(counts[2]), float(thr.value))

    def local_compose_distances(self, mean_k: int = 20, stddev_mul: float = 1.0, travers_threshold: float = 0.0,
                                sqrt_double: bool = False) -> np.ndarray:
        """The filter's mean neighbour distance of every point of the previous capture, in grid-cloud order."""
        p = self._compose_params(mean_k, stddev_mul, travers_threshold, sqrt_double)
        out = np.empty(self.length * self.length, np.float32)
        n = C.c_int()
        self._check(self._lib.gem_local_compose_distances(self._h, C.byref(p), out.ctypes.data_as(C.c_void_p), C.byref(n)),
                    "gem_local_compose_distances")
        return out[:n.value].copy()

    # -- pointCloudtoOctomap's insertion loop and fullMapToMsg (EMg.cpp:1158-1173) ---------------------------------------------------
    OCTREE_ROAD, OCTREE_OBSTACLE, OCTREE_USER0, OCTREE_USER1 = 0, 1, 2, 3

    @staticmethod
    def _octree_params(resolution, prob_hit=0.0, clamp_min=0.0, clamp_max=0.0):
        return _lib.OctreeParams(float(resolution), float(prob_hit), float(clamp_min), float(clamp_max), 0)

    def octree_build(self, slot: int, cloud, resolution: float, prob_hit: float = 0.0, clamp_min: float = 0.0, clamp_max: float = 0.0) -> dict:
        """A cleared octomap::ColorOcTree(resolution) after updateNode + integrateNodeColor per record of `cloud` in order and
        updateInnerOccupancy, as fullMapToMsg's byte stream, kept on the device in `slot` (gem_octree_build; a CUDA/HIP torch tensor
        of 32-byte records goes through gem_octree_build_device).  Returns the build's statistics; octree_read gives the bytes."""
        p = self._octree_params(resolution, prob_hit, clamp_min, clamp_max)
        st = _lib.OctreeStats()
        if _is_device_tensor(cloud):
            assert cloud.is_contiguous() and cloud.numel() * cloud.element_size() % 32 == 0
            n = cloud.numel() * cloud.element_size() // 32
            self._check(self._lib.gem_octree_build_device(self._h, int(slot), C.byref(p), C.c_void_p(cloud.data_ptr()), n, C.byref(st)),
                        "gem_octree_build_device")
        else:
            a = np.ascontiguousarray(cloud, POINT_DTYPE)
            self._check(self._lib.gem_octree_build(self._h, int(slot), C.byref(p), a.ctypes.data_as(C.c_void_p), a.shape[0], C.byref(st)),
                        "gem_octree_build")
        return st.as_dict()

    def octree_size(self, slot: int) -> int:
        n = C.c_size_t()
        self._check(self._lib.gem_octree_read(self._h, int(slot), None, 0, C.byref(n)), "gem_octree_read")
        return int(n.value)

    def octree_read(self, slot: int) -> bytes:
        """msg.data of the slot's tree (gem_octree_read); id "ColorOcTree", binary = false and the resolution stay with the caller."""
        out = np.empty(max(self.octree_size(slot), 1), np.uint8)
        n = C.c_size_t()
        self._check(self._lib.gem_octree_read(self._h, int(slot), out.ctypes.data_as(C.c_void_p), out.shape[0], C.byref(n)), "gem_octree_read")
        return out[:n.value].tobytes()

    def local_compose_octrees(self, road_resolution: float = 0.2, obstacle_resolution: float = 0.1, mean_k: int = 20, stddev_mul: float = 1.0,
                              travers_threshold: float = 0.0, sqrt_double: bool = False, road_params=None, obstacle_params=None):
        """local_compose with the two lists kept on the device and built into the slots OCTREE_ROAD and OCTREE_OBSTACLE
        (gem_local_compose_octrees): returns (road count, obstacle count, removed, threshold, [road stats, obstacle stats])."""
        p = self._compose_params(mean_k, stddev_mul, travers_threshold, sqrt_double)
        rp = self._octree_params(road_resolution, **(road_params or {}))
        op = self._octree_params(obstacle_resolution, **(obstacle_params or {}))
        counts, thr, st = (C.c_int * 3)(), C.c_double(), (_lib.OctreeStats * 2)()
        self._check(self._lib.gem_local_compose_octrees(self._h, C.byref(p), C.byref(rp), C.byref(op), counts, C.byref(thr), st),
                    "gem_local_compose_octrees")
        return int(counts[0]), int(counts[1]), int(counts[2]), float(thr.value), [st[0].as_dict(), st[1].as_dict()]

    # -- the submap stack (globalMap_: updateLocalMap's new-keyframe branch, EMg.cpp:630-687; updateGlobalMap, :773-905) ----------
    def global_enable(self, capacity: int = 1 << 20) -> None:
        """Switch the device submap stack on, empty, with room for `capacity` records (it grows on demand); 0 switches it off and
        frees its memory (gem_global_enable)."""
        self._check(self._lib.gem_global_enable(self._h, int(capacity)), "gem_global_enable")

    def global_push_local(self, clear_local: bool = True) -> int:
        """globalMap_.push_back(*out_pc + *grid_pc) on the device: the local map's export followed by the last capture's grid cloud.
        clear_local=True empties the local map afterwards.  Returns the new submap's index."""
        i = C.c_int()
        self._check(self._lib.gem_global_push_local(self._h, int(bool(clear_local)), C.byref(i)), "gem_global_push_local")
        return int(i.value)

    def global_push(self, points) -> int:
        """A POINT_DTYPE cloud (host) as a new submap; returns its index."""
        pts = np.ascontiguousarray(points, POINT_DTYPE)
        i = C.c_int()
        self._check(self._lib.gem_global_push(self._h, pts.ctypes.data_as(C.c_void_p) if pts.size else None, pts.shape[0], C.byref(i)),
                    "gem_global_push")
        return int(i.value)

    def global_loop_closure(self, transforms, centres, radius: float = 25.0, resolution: float = 0.0) -> int:
        """updateGlobalMap's body (gem_global_loop_closure): transforms = n_opt 4x4 matrices M[row][col] (laid out column-major for the
        library, as Eigen::Matrix4f::data()), centres = n_opt (x, y) pairs; resolution <= 0 takes the map's.  Returns the fused count."""
        t = np.asarray(transforms, np.float32).reshape(-1, 4, 4)
        c = np.ascontiguousarray(np.asarray(centres, np.float32).reshape(-1, 2))
        n = t.shape[0]
        if c.shape[0] != n:
            raise ValueError("global_loop_closure: one centre per transform")
        tc = np.ascontiguousarray(t.transpose(0, 2, 1))                  # column-major per matrix
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a.size else None
        fused = C.c_longlong()
        self._check(self._lib.gem_global_loop_closure(self._h, n, fp(tc), fp(c), float(np.float32(radius)), float(resolution),
                                                      C.byref(fused)), "gem_global_loop_closure")
        return int(fused.value)

    def global_export(self, index: int = -1) -> np.ndarray:
        """Submap `index` (-1: all, in stack order) as POINT_DTYPE records."""
        n = C.c_longlong()
        self._check(self._lib.gem_global_export(self._h, int(index), None, 0, C.byref(n)), "gem_global_export")
        out = np.empty(max(n.value, 1), POINT_DTYPE)
        self._check(self._lib.gem_global_export(self._h, int(index), out.ctypes.data_as(C.c_void_p), out.shape[0], C.byref(n)),
                    "gem_global_export")
        return out[:n.value].copy()

    def global_count(self) -> int:
        n = C.c_int()
        self._check(self._lib.gem_global_count(self._h, C.byref(n)), "gem_global_count")
        return int(n.value)

    # -- the history cloud (visualCloud_: EMg.cpp:750-760 push_back, :788 / :894-897 rebuild, visualPointMap :520-530) -------------
    def history_enable(self, capacity: int = 1 << 20) -> None:
        """Switch the device history cloud on, empty, with room for `capacity` records (it grows on demand); 0 switches it off and
        frees its memory (gem_history_enable).  While it is on, local_spill appends what it selects."""
        self._check(self._lib.gem_history_enable(self._h, int(capacity)), "gem_history_enable")

    def history_append(self, points) -> None:
        """POINT_DTYPE records behind the history: a host array, or a contiguous device tensor of 32-byte records (uint8 [n, 32] or
        float32 [n, 8]), which is held until the map is synchronised."""
        if _is_device_tensor(points):
            if not points.is_contiguous() or points.numel() * points.element_size() % 32:
                raise ValueError("points must be a contiguous device tensor of 32-byte records")
            n = points.numel() * points.element_size() // 32
            self._hold(points)
            self._check(self._lib.gem_history_append_device(self._h, C.c_void_p(points.data_ptr()) if n else None, n), "gem_history_append_device")
            return
        pts = np.ascontiguousarray(points, POINT_DTYPE)
        self._check(self._lib.gem_history_append(self._h, pts.ctypes.data_as(C.c_void_p) if pts.size else None, pts.shape[0]), "gem_history_append")

    def history_reset_from_global(self) -> None:
        """visualCloud_.clear() and the "Visual step" of updateGlobalMap: the history becomes every submap of the stack, in stack order."""
        self._check(self._lib.gem_history_reset_from_global(self._h), "gem_history_reset_from_global")

    def history_clear(self) -> None:
        self._check(self._lib.gem_history_clear(self._h), "gem_history_clear")

    def history_size(self) -> int:
        n = C.c_longlong()
        self._check(self._lib.gem_history_size(self._h, C.byref(n)), "gem_history_size")
        return int(n.value)

    def history_export(self, with_grid_cloud: bool = False) -> np.ndarray:
        """The history as POINT_DTYPE records (savingMap's cloud); with_grid_cloud=True: followed by the last capture's grid cloud
        (visualPointMap's visualCloud_ + grid_pc)."""
        w = int(bool(with_grid_cloud))
        n = C.c_longlong()
        self._check(self._lib.gem_history_export(self._h, w, None, 0, C.byref(n)), "gem_history_export")
        out = np.empty(max(n.value, 1), POINT_DTYPE)
        self._check(self._lib.gem_history_export(self._h, w, out.ctypes.data_as(C.c_void_p), out.shape[0], C.byref(n)), "gem_history_export")
        return out[:n.value].copy()

    # -- the costmap layers (layers/: PointMapLayer, ElevationMapLayer) ------------------------------------------------------------
    def costmap(self, size_x: int, size_y: int, resolution: float, origin_x: float = 0.0, origin_y: float = 0.0,
                default_value: int = _lib.COST_NO_INFORMATION) -> "Costmap":
        """A device-resident layer costmap bound to this map (gem_costmap_create): size in cells, the world position of cell (0, 0)'s
        lower-left corner, and the value of a cell nothing has written (NO_INFORMATION, or FREE_SPACE without track_unknown_space)."""
        return Costmap(self, size_x, size_y, resolution, origin_x, origin_y, default_value)

    # -- the step in front of the path: input colourisation (EMg.cpp:349-381) -------------------------------
    @staticmethod
    def lidar_to_image(tcamera, tlidar) -> np.ndarray:
        """P_lidar2img = T.camera (3x4) * T.lidar (4x4) in double, sums over k = 0..3 in order (EMg.cpp:343)."""
        a = np.asarray(tcamera, np.float64).reshape(3, 4); b = np.asarray(tlidar, np.float64).reshape(4, 4)
        out = np.empty((3, 4), np.float64)
        for r in range(3):
            for c in range(4):
                acc = a[r, 0] * b[0, c]
                for k in range(1, 4):
                    acc = acc + a[r, k] * b[k, c]
                out[r, c] = acc
        return out

    def colorize(self, lidar_to_image, image_bgr, xyzi):
        """Colours of a cloud from a BGR8 camera image, with the reference's draw-while-sampling order dependence (gem_colorize).
        Host arrays: returns (rgb uint32 [n] 0x00RRGGBB, xyzi copy with intensity zeroed outside the image).  Device tensors
        (image uint8 [H, W, 3], xyzi float32 [n, 4], both on the handle's device): xyzi is updated IN PLACE and the returned rgb is
        an int32 tensor holding the same words; only enqueues."""
        cam = _lib.Camera()
        P = np.asarray(lidar_to_image, np.float64).reshape(12)
        for k in range(12):
            cam.lidar_to_image[k] = float(P[k])
        if hasattr(image_bgr, "is_cuda"):
            import torch
            if not (image_bgr.is_cuda and xyzi.is_cuda and image_bgr.dtype == torch.uint8 and xyzi.dtype == torch.float32):
                raise ValueError("colorize: device tensors must be uint8 [H, W, 3] and float32 [n, 4]")
            if not (xyzi.is_contiguous() and image_bgr.stride(2) == 1 and image_bgr.stride(1) == 3):
                raise ValueError("colorize: xyzi must be contiguous, image rows packed BGR")
            cam.height, cam.width = int(image_bgr.shape[0]), int(image_bgr.shape[1])
            rgb = torch.empty(xyzi.shape[0], dtype=torch.int32, device=xyzi.device)
            self._check(self._lib.gem_colorize_device(self._h, C.byref(cam), int(xyzi.shape[0]), C.c_void_p(xyzi.data_ptr()),
                                                      C.c_void_p(image_bgr.data_ptr()), int(image_bgr.stride(0)), C.c_void_p(rgb.data_ptr())),
                        "gem_colorize_device")
            return rgb, xyzi
        img = np.ascontiguousarray(image_bgr, np.uint8)
        pts = np.ascontiguousarray(xyzi, np.float32).copy()
        cam.height, cam.width = int(img.shape[0]), int(img.shape[1])
        rgb = np.zeros(pts.shape[0], np.uint32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self._lib.gem_colorize(self._h, C.byref(cam), int(pts.shape[0]), vp(pts), vp(img), int(img.strides[0]), vp(rgb)), "gem_colorize")
        return rgb, pts

    # -- layers ----------------------------------------------------------------------------------------
    def layer(self, name_or_id, layout: int = _lib.LAYOUT_STORAGE_ROWMAJOR) -> np.ndarray:
        lid = LAYER_BY_NAME[name_or_id] if isinstance(name_or_id, str) else int(name_or_id)
        is_int = lid in _INT_LAYERS and layout == _lib.LAYOUT_STORAGE_ROWMAJOR
        out = np.empty((self.length, self.length), np.int32 if is_int else np.float32)
        self._check(self._lib.gem_get_layer(self._h, lid, layout, out.ctypes.data_as(C.c_void_p)), "gem_get_layer")
        self._held = {}                              # (a call that returns map data has everything before it behind it)
        if layout == _lib.LAYOUT_GRIDMAP_COLMAJOR_NAN:
            return out.T          # buffer holds column-major data: view it as [row, col]
        return out

    def set_layer(self, name_or_id, values) -> None:
        lid = LAYER_BY_NAME[name_or_id] if isinstance(name_or_id, str) else int(name_or_id)
        a = np.ascontiguousarray(values, np.int32 if lid in _INT_LAYERS else np.float32)
        if a.size != self.length * self.length:
            raise ValueError("layer size mismatch")
        self._check(self._lib.gem_set_layer(self._h, lid, a.ctypes.data_as(C.c_void_p)), "gem_set_layer")

    def layer_device_ptr(self, name_or_id) -> int:
        lid = LAYER_BY_NAME[name_or_id] if isinstance(name_or_id, str) else int(name_or_id)
        out = C.c_void_p()
        self._check(self._lib.gem_layer_device_ptr(self._h, lid, C.byref(out)), "gem_layer_device_ptr")
        return int(out.value)

    # -- stats --------------------------------------------------------------------------------------------
    def set_timing(self, on: bool) -> None:
        self._check(self._lib.gem_set_timing(self._h, int(on)), "gem_set_timing")

    def set_counting(self, on: bool) -> None:
        self._check(self._lib.gem_set_counting(self._h, int(on)), "gem_set_counting")

    def stats(self, reset: bool = False) -> dict:
        s = _lib.Stats()
        self._check(self._lib.gem_get_stats(self._h, C.byref(s), int(reset)), "gem_get_stats")
        return {k: (list(getattr(s, k)) if k == "ms_sort" else getattr(s, k)) for k, _ in _lib.Stats._fields_}

    # -- multi-GPU ------------------------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        rc = _lib.load().gem_comm_unique_id(buf)
        if rc != _lib.GEM_OK:
            raise GemError(f"gem_comm_unique_id failed ({rc})")
        return buf.raw

    def comm_init(self, unique_id: bytes, nranks: int, rank: int) -> None:
        buf = C.create_string_buffer(unique_id, 128)
        self._check(self._lib.gem_comm_init(self._h, buf, int(nranks), int(rank)), "gem_comm_init")

    def allgather_layers(self, with_attributes: bool = False) -> None:
        self._check(self._lib.gem_allgather_layers(self._h, int(with_attributes)), "gem_allgather_layers")

    def comm_init_tiles(self, unique_id: bytes, nranks: int, rank: int) -> None:
        """Like comm_init, with strips made of whole rows of 32 x 32-cell tiles (what the sharded path needs)."""
        buf = C.create_string_buffer(unique_id, 128)
        self._check(self._lib.gem_comm_init_tiles(self._h, buf, int(nranks), int(rank)), "gem_comm_init_tiles")

    def comm_init_loopback(self, world_id: int, nranks: int, rank: int, tile_strips: bool = True) -> None:
        """Join a LOOPBACK communicator (include/gem_hip_debug.h): `nranks` handles of this process on one device, each driven by
        a thread of its own, run the multi-GPU path's code with device-to-device copies in place of the RCCL calls."""
        self._check(self._lib.gem_comm_init_loopback(self._h, int(world_id), int(nranks), int(rank), int(bool(tile_strips))), "gem_comm_init_loopback")

    def strip(self):
        r0, r1 = C.c_int(), C.c_int()
        self._check(self._lib.gem_get_strip(self._h, C.byref(r0), C.byref(r1)), "gem_get_strip")
        return int(r0.value), int(r1.value)

    # -- multi-GPU with the points sharded (SURVEY 8e stage B) --------------------------------------------------------------
    def add_sharded(self, pb: "PackedBatch", xyzi_device, first_global_sweep: int, n_global_sweeps: int, var_updates_global=None,
                    first_point_in_sweep: int = 0) -> None:
        """This rank's contiguous share of a batch (local sweeps of `pb`, numbered first_global_sweep.. globally; its first point is
        point first_point_in_sweep of its sweep): sort, RCCL exchange of the sorted records to the strip owners, walk in rank order
        (gem_add_sharded_device)."""
        vu = None if var_updates_global is None else (C.c_float * n_global_sweeps)(*[float(v) for v in var_updates_global])
        ptr = C.c_void_p(xyzi_device.data_ptr()) if pb.n else None
        self._check(self._lib.gem_add_sharded_device(self._h, pb.n, pb.frames, ptr, pb.offsets, int(first_global_sweep),
                                                     int(n_global_sweeps), int(first_point_in_sweep), vu), "gem_add_sharded_device")

    def shard_sort(self, pb: "PackedBatch", xyzi_device, first_global_sweep: int, n_global_sweeps: int, strip_rows, first_point_in_sweep: int = 0,
                   with_ranges: bool = False):
        """First half: returns (bounds [nstrips + 1], device pointer of the sorted {h, var} records, of their keys[, of the block ranges])."""
        ns = len(strip_rows) - 1
        rows = (C.c_int * (ns + 1))(*[int(v) for v in strip_rows])
        bounds = (C.c_uint32 * (ns + 1))()
        phv, pkey, prng = C.c_void_p(), C.c_void_p(), C.c_void_p()
        ptr = C.c_void_p(xyzi_device.data_ptr()) if pb.n else None
        self._check(self._lib.gem_shard_sort_device(self._h, pb.n, pb.frames, ptr, pb.offsets, int(first_global_sweep), int(n_global_sweeps),
                                                    int(first_point_in_sweep), ns, rows, bounds, C.byref(phv), C.byref(pkey), C.byref(prng)),
                    "gem_shard_sort_device")
        out = (np.array(bounds[:], np.int64), phv.value or 0, pkey.value or 0)
        return out + (prng.value or 0,) if with_ranges else out

    def shard_sort_tensors(self, pb, xyzi_device, first_global_sweep, n_global_sweeps, strip_rows, first_point_in_sweep: int = 0):
        """shard_sort with the sorted records as torch tensors aliasing the handle's arenas ([M, 2] int32 {h, var} bits, [M] int32
        keys); they stay valid until the next pass of this handle."""
        import torch
        from .tiling import _DeviceArray
        bounds, phv, pkey = self.shard_sort(pb, xyzi_device, first_global_sweep, n_global_sweeps, strip_rows, first_point_in_sweep)
        m = int(bounds[-1])
        if m == 0:
            dev = xyzi_device.device
            return bounds, torch.empty((0, 2), dtype=torch.int32, device=dev), torch.empty((0,), dtype=torch.int32, device=dev)
        hv = torch.as_tensor(_DeviceArray(phv, (m, 2), "<i4"), device="cuda")
        key = torch.as_tensor(_DeviceArray(pkey, (m,), "<i4"), device="cuda")
        return bounds, hv, key

    def shard_fuse_tensors(self, hv_list, key_list, n_global_sweeps, var_updates_global=None) -> None:
        import torch
        torch.cuda.synchronize()                     # the exchange ran on torch's stream, the walk runs on the handle's
        self._keep = (hv_list, key_list)             # until the walk has read them
        self.shard_fuse([t.data_ptr() if t.numel() else 0 for t in hv_list], [t.data_ptr() if t.numel() else 0 for t in key_list],
                        [int(t.shape[0]) for t in key_list], n_global_sweeps, var_updates_global)

    def shard_fuse(self, hv_ptrs, key_ptrs, counts, n_global_sweeps: int, var_updates_global=None, range_ptrs=None, bases=None) -> None:
        """Second half: walk this handle's strip through the sources (device pointers + record counts) in the order given; with
        range_ptrs / bases the sources' own block ranges replace the search (gem_hip.h)."""
        n = len(counts)
        a_hv = (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in hv_ptrs])
        a_key = (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in key_ptrs])
        a_cnt = (C.c_uint32 * n)(*[int(c) for c in counts])
        a_rng = None if range_ptrs is None else (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in range_ptrs])
        a_base = None if bases is None else (C.c_uint32 * n)(*[int(b) for b in bases])
        vu = None if var_updates_global is None else (C.c_float * n_global_sweeps)(*[float(v) for v in var_updates_global])
        self._check(self._lib.gem_shard_fuse_device(self._h, n, a_hv, a_key, a_cnt, a_rng, a_base, int(n_global_sweeps), vu), "gem_shard_fuse_device")


class Costmap:
    """One costmap of an ElevationMap's handle (gem_costmap_*): the two layers' updateBounds bodies as marking passes, updateOrigin as
    the rolling step, the two updateCosts rules and a window read-back.  A mark with bounds=None only enqueues; with bounds =
    [min_x, min_y, max_x, max_y] it returns them merged with what it touched (touch() of costmap_2d)."""

    def __init__(self, elevation_map: ElevationMap, size_x, size_y, resolution, origin_x=0.0, origin_y=0.0,
                 default_value=_lib.COST_NO_INFORMATION):
        self.map = elevation_map
        cfg = _lib.CostmapConfig(int(size_x), int(size_y), float(resolution), float(origin_x), float(origin_y), int(default_value))
        i = C.c_int(-1)
        self.map._check(self.map._lib.gem_costmap_create(self.map._h, C.byref(cfg), C.byref(i)), "gem_costmap_create")
        self.id = int(i.value)
        self.size_x, self.size_y = int(size_x), int(size_y)

    def close(self) -> None:
        if self.id >= 0 and getattr(self.map, "_h", None):
            self.map._check(self.map._lib.gem_costmap_destroy(self.map._h, self.id), "gem_costmap_destroy")
        self.id = -1

    def _call(self, name, *args):
        self.map._check(getattr(self.map._lib, name)(self.map._h, self.id, *args), name)

    @staticmethod
    def _bounds(bounds):
        return None if bounds is None else (C.c_double * 4)(*[float(v) for v in bounds])

    def _mark(self, name, bounds, *args):
        b = self._bounds(bounds)
        self._call(name, *args, b)
        return None if b is None else list(b)

    def geometry(self) -> dict:
        """size, resolution, the origin after rolling, default_value"""
        c = _lib.CostmapConfig()
        self._call("gem_costmap_geometry", C.byref(c))
        return {"size_x": c.size_x, "size_y": c.size_y, "resolution": c.resolution, "origin_x": c.origin_x, "origin_y": c.origin_y,
                "default_value": c.default_value}

    def reset(self) -> None:
        self._call("gem_costmap_reset")

    def update_origin(self, new_origin_x: float, new_origin_y: float) -> None:
        self._call("gem_costmap_update_origin", float(new_origin_x), float(new_origin_y))

    def roll_to(self, robot_x: float, robot_y: float) -> None:
        """updateOrigin(robot - sizeInMeters / 2): the rolling_window_ line of both layers"""
        self._call("gem_costmap_roll_to", float(robot_x), float(robot_y))

    def mark_points(self, points, travers_thresh: float = 0.5, bounds=None):
        """PointMapLayer::updateBounds over POINT_DTYPE records: a host array, or a contiguous device tensor of 32-byte records
        (uint8 [n, 32] or float32 [n, 8]), which is held until the map is synchronised."""
        if _is_device_tensor(points):
            if not points.is_contiguous() or points.numel() * points.element_size() % 32:
                raise ValueError("points must be a contiguous device tensor of 32-byte records")
            n = points.numel() * points.element_size() // 32
            self.map._hold(points)
            return self._mark("gem_costmap_mark_points_device", bounds, C.c_void_p(points.data_ptr()) if n else None, n, float(travers_thresh))
        pts = np.ascontiguousarray(points, POINT_DTYPE)
        return self._mark("gem_costmap_mark_points", bounds, pts.ctypes.data_as(C.c_void_p) if pts.size else None, pts.shape[0],
                          float(travers_thresh))

    def mark_grid_cloud(self, travers_thresh: float = 0.5, bounds=None):
        """... over the last capture's records (grid_pc) where they lie"""
        return self._mark("gem_costmap_mark_grid_cloud", bounds, float(travers_thresh))

    def mark_global(self, index: int = -1, travers_thresh: float = 0.5, bounds=None):
        """... over submap `index` of the stack (-1: all of them, in stack order)"""
        return self._mark("gem_costmap_mark_global", bounds, int(index), float(travers_thresh))

    def mark_history(self, travers_thresh: float = 0.5, bounds=None):
        """... over the history cloud where it lies, as one input; mark_grid_cloud after it is PointMapLayer's visualCloud_ + grid_pc"""
        return self._mark("gem_costmap_mark_history", bounds, float(travers_thresh))

    def mark_visual(self, travers_thresh: float = 0.5, bounds=None):
        """ElevationMapLayer::updateBounds over the last capture standing for visualMap_"""
        return self._mark("gem_costmap_mark_visual", bounds, float(travers_thresh))

    def merge(self, master: "Costmap", window=None, mode: int = _lib.COSTMAP_OVERWRITE) -> None:
        """updateCosts onto `master` inside window = (min_i, min_j, max_i, max_j) (None: the whole map): overwrite or max"""
        w = (0, 0, self.size_x, self.size_y) if window is None else tuple(int(v) for v in window)
        self._call("gem_costmap_merge", master.id, *w, int(mode))

    def read(self, window=None, row_stride: int = 0) -> np.ndarray:
        """The window's bytes as [rows, row_stride or width] (None: the whole map); columns beyond the width are left 0."""
        w = (0, 0, self.size_x, self.size_y) if window is None else tuple(int(v) for v in window)
        width, rows = w[2] - w[0], w[3] - w[1]
        stride = max(int(row_stride), width, 0)
        out = np.zeros((max(rows, 0), stride), np.uint8)
        self._call("gem_costmap_read", *w, out.ctypes.data_as(C.c_void_p) if out.size else None, stride)
        return out


    def write(self, values, window=None) -> None:
        """The window's cells from a uint8 [rows, width] array (None: the whole map): costs other layers left in a master."""
        w = (0, 0, self.size_x, self.size_y) if window is None else tuple(int(v) for v in window)
        v = np.ascontiguousarray(values, np.uint8)
        if v.shape != (w[3] - w[1], w[2] - w[0]):
            raise ValueError(f"expected a {(w[3] - w[1], w[2] - w[0])} array, got {v.shape}")
        self._call("gem_costmap_write", *w, v.ctypes.data_as(C.c_void_p) if v.size else None, max(w[2] - w[0], 0))

    # -- footprints (gem_hip_footprint.h) ---------------------------------------------------------------------------------------------
    @staticmethod
    def _spec(spec):
        """[n, 2] footprint vertices -> (keepalive array, double*, n)"""
        v = np.ascontiguousarray(spec, np.float64).reshape(-1, 2)
        return v, (v.ctypes.data_as(C.POINTER(C.c_double)) if v.size else None), int(v.shape[0])

    @staticmethod
    def poses_from_yaw(poses) -> np.ndarray:
        """[n, 3] (x, y, theta) -> [n, 4] (x, y, cos, sin) with math.cos / math.sin element by element: the host's libm, as the C++
        facade's std::cos / std::sin"""
        p = np.asarray(poses, np.float64).reshape(-1, 3)
        out = np.empty((p.shape[0], 4), np.float64)
        out[:, :2] = p[:, :2]
        out[:, 2] = [math.cos(float(t)) for t in p[:, 2]]
        out[:, 3] = [math.sin(float(t)) for t in p[:, 2]]
        return out

    def _poses(self, poses):
        """host [n, 3] (x, y, theta) or [n, 4] (x, y, cos, sin), or a contiguous float64 device tensor [n, 4] -> (keepalive, void*, n,
        on the device)"""
        if _is_device_tensor(poses):
            import torch
            if poses.dtype != torch.float64 or not poses.is_contiguous() or poses.dim() != 2 or poses.shape[1] != 4:
                raise ValueError("device poses must be a contiguous float64 tensor [n, 4]: x, y, cos, sin")
            n = int(poses.shape[0])
            return poses, (C.c_void_p(poses.data_ptr()) if n else None), n, True
        p = np.asarray(poses, np.float64)
        if p.ndim != 2 or p.shape[1] not in (3, 4):
            raise ValueError("poses must be [n, 3] (x, y, theta) or [n, 4] (x, y, cos, sin)")
        p = self.poses_from_yaw(p) if p.shape[1] == 3 else np.ascontiguousarray(p)
        return p, (p.ctypes.data_as(C.c_void_p) if p.size else None), int(p.shape[0]), False

    def clear_footprint(self, pose, spec, bounds=None):
        """updateFootprint + setConvexPolygonCost(FREE_SPACE): pose = (x, y, theta) or (x, y, cos, sin), spec = [n, 2] vertices in
        the robot's frame.  Returns (ok, bounds): every transformed vertex is touched into bounds (None stays None); the call only
        enqueues."""
        p = [float(v) for v in pose]
        if len(p) == 3:
            p = [p[0], p[1], math.cos(p[2]), math.sin(p[2])]
        fp = _lib.FootprintPose(*p)
        keep, ps, n = self._spec(spec)
        b, ok = self._bounds(bounds), C.c_int(-1)
        self._call("gem_costmap_clear_footprint", C.byref(fp), ps, n, b, C.byref(ok))
        return bool(ok.value), (None if b is None else list(b))

    def footprint_cost(self, poses, spec, flags: int = 0):
        """CostmapModel::footprintCost of every pose: -3 off the map, -2 unknown, -1 lethal, else the largest cost on the outline.
        Host poses give an int32 numpy array (the call waits); a device tensor gives an int32 device tensor, only enqueued, held
        with the poses until the map is synchronised."""
        keep, pp, n, dev = self._poses(poses)
        ks, ps, nv = self._spec(spec)
        if dev:
            import torch
            out = torch.empty((n,), dtype=torch.int32, device=poses.device)
            self.map._hold(poses, out)
            self._call("gem_costmap_footprint_cost_device", pp, n, ps, nv, int(flags), C.c_void_p(out.data_ptr()) if n else None)
            return out
        out = np.zeros(n, np.int32)
        self._call("gem_costmap_footprint_cost", pp, n, ps, nv, int(flags), out.ctypes.data_as(C.c_void_p) if n else None)
        return out

    def score_trajectories(self, poses, poses_per_traj: int, spec, flags: int = 0, pose_costs: bool = False):
        """ObstacleCostFunction::scoreTrajectory's loop over trajectories of poses_per_traj consecutive poses each: the first negative
        pose cost, else the maximum (FOOTPRINT_SUM: the sum).  Returns the trajectory costs, or (trajectory costs, pose costs) with
        pose_costs; numpy for host poses, device tensors (only enqueued) for a device tensor."""
        keep, pp, n, dev = self._poses(poses)
        T = int(poses_per_traj)
        if T < 1 or n % T:
            raise ValueError("the poses are not a whole number of trajectories")
        nt = n // T
        ks, ps, nv = self._spec(spec)
        if dev:
            import torch
            traj = torch.empty((nt,), dtype=torch.int32, device=poses.device)
            each = torch.empty((n,), dtype=torch.int32, device=poses.device) if pose_costs else None
            self.map._hold(poses, traj, each)
            self._call("gem_costmap_score_trajectories_device", pp, nt, T, ps, nv, int(flags),
                       C.c_void_p(each.data_ptr()) if pose_costs and n else None, C.c_void_p(traj.data_ptr()) if nt else None)
        else:
            traj = np.zeros(nt, np.int32)
            each = np.zeros(n, np.int32) if pose_costs else None
            self._call("gem_costmap_score_trajectories", pp, nt, T, ps, nv, int(flags),
                       each.ctypes.data_as(C.c_void_p) if pose_costs and n else None, traj.ctypes.data_as(C.c_void_p) if nt else None)
        return (traj, each) if pose_costs else traj

    # -- ObstacleLayer (gem_hip_obstacle.h) ---------------------------------------------------------------------------------------------
    def observe(self, observations, layer_max_obstacle_height: float = 2.0, bounds=None):
        """ObstacleLayer::updateBounds over `observations`: the rays of every clearing observation free the cells they cross, then the
        records of every marking one become lethal.  An observation is a dict: points (a host array, float32 [n, k >= 3] or records
        whose first three floats are x, y, z such as POINT_DTYPE; or a contiguous device tensor, float32 [n, k >= 3] or uint8 [n,
        4 m >= 12]), origin (x, y, z), and optionally obstacle_range (2.5), raytrace_range (3.0), min_obstacle_height (0.0),
        max_obstacle_height (2.0), marking (True), clearing (True): costmap_2d's defaults.  All host or all device; device tensors are
        held until the map is synchronised.  With bounds=None the call only enqueues; else the merged bounds come back."""
        obs, keep, on_device = _observations(observations)
        if on_device:
            self.map._hold(*keep)
        return self._mark("gem_costmap_observe_device" if on_device else "gem_costmap_observe", bounds, obs, len(keep), float(layer_max_obstacle_height))

    # -- VoxelLayer (gem_hip_voxlayer.h) -------------------------------------------------------------------------------------------------
    def attach_voxels(self, size_z: int = 10, z_resolution: float = 0.2, origin_z: float = 0.0, unknown_threshold: int = 15,
                      mark_threshold: int = 0) -> None:
        """A voxel grid on this costmap (gem_costmap_voxels_create), every column unknown: size_z in 1 .. 16 voxels of z_resolution from
        origin_z upwards, and VoxelLayer's two thresholds with costmap_2d's defaults.  reset, update_origin and roll_to then move the
        columns with the bytes."""
        cfg = _lib.VoxelConfig(int(size_z), float(z_resolution), float(origin_z), int(unknown_threshold), int(mark_threshold))
        self._call("gem_costmap_voxels_create", C.byref(cfg))

    def detach_voxels(self) -> None:
        self._call("gem_costmap_voxels_destroy")

    def read_voxels(self, window=None) -> np.ndarray:
        """The window's voxel columns as uint32 [rows, width] (None: the whole map): bit z "not known free", bit 16 + z "marked"."""
        w = (0, 0, self.size_x, self.size_y) if window is None else tuple(int(v) for v in window)
        out = np.zeros((max(w[3] - w[1], 0), max(w[2] - w[0], 0)), np.uint32)
        self._call("gem_costmap_voxels_read", *w, out.ctypes.data_as(C.c_void_p) if out.size else None, out.shape[1])
        return out

    def write_voxels(self, columns, window=None) -> None:
        """The window's voxel columns from a uint32 [rows, width] array (None: the whole map)."""
        w = (0, 0, self.size_x, self.size_y) if window is None else tuple(int(v) for v in window)
        v = np.ascontiguousarray(columns, np.uint32)
        if v.shape != (w[3] - w[1], w[2] - w[0]):
            raise ValueError(f"expected a {(w[3] - w[1], w[2] - w[0])} array, got {v.shape}")
        self._call("gem_costmap_voxels_write", *w, v.ctypes.data_as(C.c_void_p) if v.size else None, max(w[2] - w[0], 0))

    def voxel_observe(self, observations, layer_max_obstacle_height: float = 2.0, bounds=None):
        """VoxelLayer::updateBounds over `observations` (dicts as for observe) on a costmap with voxels attached: the 3-D rays of
        every clearing observation clear the voxels they cross, then the records of every marking one mark theirs; a cell becomes
        free, unknown or lethal by its column's bit counts.  With bounds=None the call only enqueues; else the merged bounds come back."""
        obs, keep, on_device = _observations(observations)
        if on_device:
            self.map._hold(*keep)
        return self._mark("gem_costmap_voxel_observe_device" if on_device else "gem_costmap_voxel_observe", bounds, obs, len(keep),
                          float(layer_max_obstacle_height))

    # -- inflation (gem_hip_inflate.h) --------------------------------------------------------------------------------------------------
    def inflate(self, inflation_radius: float, inscribed_radius: float, cost_scaling_factor: float = 10.0, inflate_unknown: bool = False,
                window=None) -> None:
        """InflationLayer's costs around the 254 cells inside window = (min_i, min_j, max_i, max_j) widened by the cell radius (None:
        the whole map), from the exact nearest lethal cell; the call only enqueues (the first one with new parameters uploads the table)."""
        w = (0, 0, self.size_x, self.size_y) if window is None else tuple(int(v) for v in window)
        p = _lib.InflationParams(float(inflation_radius), float(inscribed_radius), float(cost_scaling_factor), int(bool(inflate_unknown)))
        self._call("gem_costmap_inflate", C.byref(p), *w)

    def reset_window(self, x0: int, y0: int, xn: int, yn: int) -> None:
        """Costmap2D::resetMap(x0, y0, xn, yn): rows y0 <= y < yn become default_value for x0 <= x < xn; only enqueued"""
        self._call("gem_costmap_reset_window", int(x0), int(y0), int(xn), int(yn))

    # -- path and goal distance grids (gem_hip_mapgrid.h) ---------------------------------------------------------------------------------
    def prepare_map_grid(self, plan, which: int = _lib.MAPGRID_PATH | _lib.MAPGRID_GOAL) -> None:
        """MapGrid::setTargetCells / setLocalGoal + computeTargetDistance from plan = [n, 2] world points (adjusted to the resolution
        on the host) through the costmap's non-blocked cells as they are when the call runs on the stream; only enqueued."""
        v = np.ascontiguousarray(plan, np.float64).reshape(-1, 2)
        self._call("gem_costmap_mapgrid_prepare", v.ctypes.data_as(C.POINTER(C.c_double)) if v.size else None, int(v.shape[0]), int(which))

    def prepare_map_grid_tiled(self, plan, which: int = _lib.MAPGRID_PATH | _lib.MAPGRID_GOAL) -> dict:
        """prepare_map_grid on a costmap of any size (gem_costmap_mapgrid_prepare_tiled): the same grids in the same slots, relaxed tile
        by tile in global memory.  The call waits.  dict(started, goal_cell, rounds, chunks): rounds depends on timing, the grids do not."""
        v = np.ascontiguousarray(plan, np.float64).reshape(-1, 2)
        st = _lib.MapGridTiledStatus()
        self._call("gem_costmap_mapgrid_prepare_tiled", v.ctypes.data_as(C.POINTER(C.c_double)) if v.size else None, int(v.shape[0]), int(which),
                   C.byref(st))
        return _map_grid_tiled_status(st)

    def read_map_grid(self, which: int):
        """(distances int32 [size_y, size_x], started, (goal x, goal y)) of MAPGRID_PATH or MAPGRID_GOAL; the call waits."""
        out = np.zeros((self.size_y, self.size_x), np.int32)
        started, goal = C.c_int(-1), (C.c_int * 2)(-1, -1)
        self._call("gem_costmap_mapgrid_read", int(which), out.ctypes.data_as(C.c_void_p), C.byref(started), goal)
        return out, int(started.value), (int(goal[0]), int(goal[1]))

    def score_map_grid(self, which: int, poses, poses_per_traj: int, xshift: float = 0.0, flags: int = 0):
        """MapGridCostFunction::scoreTrajectory over trajectories of poses_per_traj consecutive poses each against the prepared grid:
        -4 off the map, with MAPGRID_STOP_ON_FAILURE -3 / -2 on an obstacle / unreachable cell, else the last pose's distance
        (MAPGRID_SUM: the sum).  int64 numpy for host poses (the call waits), an int64 device tensor, only enqueued, for a device tensor."""
        keep, pp, n, dev = self._poses(poses)
        T = int(poses_per_traj)
        if T < 1 or n % T:
            raise ValueError("the poses are not a whole number of trajectories")
        nt = n // T
        if dev:
            import torch
            out = torch.empty((nt,), dtype=torch.int64, device=poses.device)
            self.map._hold(poses, out)
            self._call("gem_costmap_mapgrid_score_device", int(which), pp, nt, T, float(xshift), int(flags), C.c_void_p(out.data_ptr()) if nt else None)
            return out
        out = np.zeros(nt, np.int64)
        self._call("gem_costmap_mapgrid_score", int(which), pp, nt, T, float(xshift), int(flags), out.ctypes.data_as(C.c_void_p) if nt else None)
        return out

    # -- the global plan (gem_hip_navplan.h) -------------------------------------------------------------------------------------------
    def nav_plan(self, start, goal, weights=None, outline: bool = True):
        """global_planner's makePlan in its order-free configuration (Dijkstra, the non-quadratic potential, the grid path) from the
        world points start to goal over the costmap's bytes as they are when the call runs on the stream; weights = int32 [256] by cost
        byte, 0 = impassable (None: nav_weights()).  The call waits.  Returns (path float64 [n, 2] of cell centres from start to goal,
        status dict: found, n_path, rounds, chunks, goal_potential, start_cell, goal_cell)."""
        w = np.ascontiguousarray(nav_weights() if weights is None else weights, np.int32)
        if w.shape != (256,):
            raise ValueError("weights must be int32 [256]")
        s, g = (C.c_double * 2)(*[float(v) for v in start]), (C.c_double * 2)(*[float(v) for v in goal])
        st = _lib.NavplanStatus()
        self._call("gem_costmap_navplan", s, g, w.ctypes.data_as(C.POINTER(C.c_int)), _lib.NAV_OUTLINE if outline else 0, None, 0, C.byref(st))
        cells = np.zeros(int(st.n_path), np.int32)
        if cells.size:
            self._call("gem_costmap_navplan_read", None, cells.ctypes.data_as(C.c_void_p), int(cells.size))
        geo = self.geometry()                                           # cell centres, in double, as the C entry computes them
        path = np.stack([geo["origin_x"] + ((cells % self.size_x).astype(np.float64) + 0.5) * geo["resolution"],
                         geo["origin_y"] + ((cells // self.size_x).astype(np.float64) + 0.5) * geo["resolution"]], axis=1).reshape(-1, 2)
        return path, _nav_status(st)

    def nav_plan_quadratic(self, start, goal, weights=None, outline: bool = True):
        """nav_plan on the QUADRATIC potential of gem_hip_navquad.h (gem_costmap_navplan_quadratic): the two-axis update stated in exact
        integers, order-free, nowhere above the linear potential; weights at most 462.  The plan takes the linear plan's place: nav_status,
        read_potential, nav_plan_to, nav_paths and frontiers work on it.  Returns what nav_plan returns."""
        w = np.ascontiguousarray(nav_weights() if weights is None else weights, np.int32)
        if w.shape != (256,):
            raise ValueError("weights must be int32 [256]")
        s, g = (C.c_double * 2)(*[float(v) for v in start]), (C.c_double * 2)(*[float(v) for v in goal])
        st = _lib.NavplanStatus()
        self._call("gem_costmap_navplan_quadratic", s, g, w.ctypes.data_as(C.POINTER(C.c_int)), _lib.NAV_OUTLINE if outline else 0, None, 0, C.byref(st))
        cells = np.zeros(int(st.n_path), np.int32)
        if cells.size:
            self._call("gem_costmap_navplan_read", None, cells.ctypes.data_as(C.c_void_p), int(cells.size))
        geo = self.geometry()                                           # cell centres, in double, as the C entry computes them
        path = np.stack([geo["origin_x"] + ((cells % self.size_x).astype(np.float64) + 0.5) * geo["resolution"],
                         geo["origin_y"] + ((cells // self.size_x).astype(np.float64) + 0.5) * geo["resolution"]], axis=1).reshape(-1, 2)
        return path, _nav_status(st)

    def nav_status(self) -> dict:
        """The status of the costmap's last plan (gem_costmap_navplan_status), whoever made it; nothing is enqueued."""
        st = _lib.NavplanStatus()
        self._call("gem_costmap_navplan_status", C.byref(st))
        return _nav_status(st)

    def read_potential(self):
        """(potential int32 [size_y, size_x], path cells int32 [n] as y * size_x + x) of the costmap's last plan; the call waits."""
        n = self.nav_status()["n_path"]
        pot = np.zeros((self.size_y, self.size_x), np.int32)
        cells = np.zeros(n, np.int32)
        self._call("gem_costmap_navplan_read", pot.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p) if n else None, n)
        return pot, cells

    # -- frontier search (gem_hip_frontier.h) --------------------------------------------------------------------------------------------
    def frontiers(self, min_frontier_size: float = 0.0, potential_scale: float = 1.0, gain_scale: float = 1.0) -> dict:
        """The frontiers of the costmap's bytes against the potential of its last plan (gem_costmap_frontiers): 8-connected components
        of the unknown cells that have a known, reached 4-neighbour; cost = potential_scale * access potential - gain_scale * size *
        resolution; the kept frontier of least cost wins.  The call waits.  Returns the status dict: n_cells, n_frontiers, n_kept, best
        (index into the kept list, -1 without one), rounds, chunks, best_frontier (a frontier dict with its centroid, or None)."""
        p = _lib.FrontierParams(float(min_frontier_size), float(potential_scale), float(gain_scale))
        st = _lib.FrontierStatus()
        self._call("gem_costmap_frontiers", C.byref(p), C.byref(st))
        return _frontier_status(st, self.geometry())

    def read_frontiers(self):
        """(kept frontiers: a list of dicts in ascending root order, labels int32 [size_y, size_x]: the root of the cell's frontier, -1
        for a cell that is no frontier cell) of the costmap's last search; the call waits."""
        labels = np.zeros((self.size_y, self.size_x), np.int32)
        self._call("gem_costmap_frontiers_read", None, 0, labels.ctypes.data_as(C.c_void_p))
        n = int((labels.reshape(-1) == np.arange(labels.size, dtype=np.int64)).sum())       # the roots: the kept list has no more records
        rec = (_lib.Frontier * max(n, 1))()
        for r in rec:
            r.root = -1                                                 # (what the read leaves alone: behind the kept list)
        self._call("gem_costmap_frontiers_read", rec, n, None)
        geo = self.geometry()
        return [_frontier(r, geo) for r in rec if r.root >= 0], labels

    def nav_plan_to(self, goal):
        """The grid path from the last plan's start to another goal on the last plan's potential, which stays as it is
        (gem_costmap_navplan_goal): one walk, no second search.  Returns (path, status) as nav_plan does."""
        g = (C.c_double * 2)(*[float(v) for v in goal])
        st = _lib.NavplanStatus()
        self._call("gem_costmap_navplan_goal", g, None, 0, C.byref(st))
        cells = np.zeros(int(st.n_path), np.int32)
        if cells.size:
            self._call("gem_costmap_navplan_read", None, cells.ctypes.data_as(C.c_void_p), int(cells.size))
        geo = self.geometry()                                           # cell centres, in double, as the C entry computes them
        path = np.stack([geo["origin_x"] + ((cells % self.size_x).astype(np.float64) + 0.5) * geo["resolution"],
                         geo["origin_y"] + ((cells // self.size_x).astype(np.float64) + 0.5) * geo["resolution"]], axis=1).reshape(-1, 2)
        return path, _nav_status(st)

    # -- paths on the last plan's potential (gem_hip_navpath.h) ------------------------------------------------------------------------
    def nav_paths(self, goals, form: int = _lib.NAVPATH_GRADIENT, max_points: int = 4096, points: bool = True, raw: bool = False):
        """Paths from the last plan's start to up to 1024 goals (world points [n, 2]) on the last plan's potential, in one launch, one wave
        per goal (gem_costmap_navplan_paths): form NAVPATH_GRADIENT, global_planner's default path of sub-cell points half a cell apart,
        or NAVPATH_GRID, the grid path of nav_plan_to.  The potential, the last path and status and the frontier search stay as they
        are.  The call waits.  Returns (paths, results): paths a list of float64 [n_i, 2] world points from start to goal (cell
        coordinates p become origin + (p + 0.5) * resolution, in double; None with points=False), results a list of dicts (status,
        n_points, goal_cell, goal_potential).  raw=True: (float32 [n, max_points, 2] in walk order, goal first, cell coordinates,
        rows beyond n_points untouched zeros; int32 [n, 8] result words)."""
        g = np.ascontiguousarray(goals, np.float64).reshape(-1, 2)
        n = int(g.shape[0])
        pts = np.zeros((n, int(max_points), 2), np.float32) if points and n and 0 < int(max_points) <= (1 << 24) // max(n, 1) else None
        res = np.zeros((max(n, 1), 8), np.int32)
        self._call("gem_costmap_navplan_paths", g.ctypes.data_as(C.c_void_p) if n else None, n, int(form), int(max_points),
                   pts.ctypes.data_as(C.c_void_p) if pts is not None else None, res.ctypes.data_as(C.c_void_p))
        if raw:
            return pts, res
        return (_nav_world_paths(pts, res, self.geometry()) if pts is not None else None), [_navpath_result(r) for r in res]

    def nav_paths_device(self, goals, form: int = _lib.NAVPATH_GRADIENT, max_points: int = 4096, device=None):
        """nav_paths with its outputs left on the device (gem_costmap_navplan_paths_device): the goal cells are handed over and the walk
        is enqueued on the handle's stream; the call does not wait for it.  Returns (float32 [n, max_points, 2] device tensor in walk
        order, goal first, cell coordinates; int32 [n, 8] device tensor of result words)."""
        import torch
        g = np.ascontiguousarray(goals, np.float64).reshape(-1, 2)
        n = int(g.shape[0])
        if not (1 <= n <= 1024 and 2 <= int(max_points) <= (1 << 24) // n):
            raise ValueError("nav_paths_device: n_goals outside 1 .. 1024, max_points below 2, or n_goals * max_points above 2^24")
        dev = torch.device("cuda") if device is None else device
        pts = torch.empty((n, int(max_points), 2), dtype=torch.float32, device=dev)     # (rows beyond a goal's n_points are not written)
        res = torch.empty((n, 8), dtype=torch.int32, device=dev)
        self.map._hold(pts, res)
        self._call("gem_costmap_navplan_paths_device", g.ctypes.data_as(C.c_void_p), n, int(form), int(max_points), C.c_void_p(pts.data_ptr()),
                   C.c_void_p(res.data_ptr()))
        return pts, res

    # -- the best trajectory (gem_hip_critics.h) ----------------------------------------------------------------------------------------
    def prepare_map_grid_front(self, plan) -> None:
        """The FRONT grid, which DWA's goal_front critic reads: the goal grid of `plan` (the caller's front plan, its last point already
        moved forward) in a slot of its own; PATH and GOAL are not touched.  Only enqueued."""
        v = np.ascontiguousarray(plan, np.float64).reshape(-1, 2)
        self._call("gem_costmap_mapgrid_prepare_front", v.ctypes.data_as(C.POINTER(C.c_double)) if v.size else None, int(v.shape[0]))

    def prepare_map_grid_front_tiled(self, plan) -> dict:
        """prepare_map_grid_front on a costmap of any size (gem_costmap_mapgrid_prepare_front_tiled); the call waits.
        dict(started, goal_cell, rounds, chunks)."""
        v = np.ascontiguousarray(plan, np.float64).reshape(-1, 2)
        st = _lib.MapGridTiledStatus()
        self._call("gem_costmap_mapgrid_prepare_front_tiled", v.ctypes.data_as(C.POINTER(C.c_double)) if v.size else None, int(v.shape[0]), C.byref(st))
        return _map_grid_tiled_status(st)

    def read_map_grid_front(self):
        """(distances int32 [size_y, size_x], started, (goal x, goal y)) of the FRONT grid; the call waits."""
        out = np.zeros((self.size_y, self.size_x), np.int32)
        started, goal = C.c_int(-1), (C.c_int * 2)(-1, -1)
        self._call("gem_costmap_mapgrid_read_front", out.ctypes.data_as(C.c_void_p), C.byref(started), goal)
        return out, int(started.value), (int(goal[0]), int(goal[1]))

    def best_trajectory(self, critics, poses, poses_per_traj: int, spec, ext=None, traj_len=None, totals: bool = False):
        """SimpleScoredSamplingPlanner's scoreTrajectory + findBestTrajectory over trajectories of poses_per_traj pose slots each:
        critics is the ordered list (obstacle_critic / map_grid_critic / external_critic), ext = [columns, n_traj] raw scores of the
        external critics, traj_len = [n_traj] int32 poses each trajectory uses (None: all).  Host poses: (index, cost, n_valid), or
        with totals (index, cost, n_valid, float64 totals); the call waits.  A device tensor of poses (ext and traj_len then device
        tensors too): an int64 device tensor [4] = index, n_valid, the cost's bits (`.view(torch.float64)[2]`), 0 -- or with totals
        (that, a float64 device tensor) -- only enqueued and held until the map is synchronised."""
        keep, pp, n, dev = self._poses(poses)
        T = int(poses_per_traj)
        if T < 1 or n % T:
            raise ValueError("the poses are not a whole number of trajectories")
        nt = n // T
        cs = (_lib.Critic * max(len(critics), 1))(*critics)
        ks, ps, nv = self._spec(spec if spec is not None else [])
        if dev:
            import torch
            for name, t, dt in (("ext", ext, torch.float64), ("traj_len", traj_len, torch.int32)):
                if t is not None and not (_is_device_tensor(t) and t.dtype == dt and t.is_contiguous()):
                    raise ValueError(f"with device poses {name} must be a contiguous device tensor of {dt}")
            if ext is not None and (ext.dim() != 2 or ext.shape[1] != nt):
                raise ValueError("ext must be [columns, n_traj]")
            if traj_len is not None and traj_len.numel() != nt:
                raise ValueError("traj_len must hold one int per trajectory")
            best = torch.empty((4,), dtype=torch.int64, device=poses.device)
            tot = torch.empty((nt,), dtype=torch.float64, device=poses.device) if totals else None
            self.map._hold(poses, ext, traj_len, best, tot)
            self._call("gem_costmap_best_trajectory_device", cs, len(critics), pp, C.c_void_p(traj_len.data_ptr()) if traj_len is not None and nt else None,
                       nt, T, ps, nv, C.c_void_p(ext.data_ptr()) if ext is not None and ext.numel() else None, int(ext.shape[0]) if ext is not None else 0,
                       C.c_void_p(tot.data_ptr()) if totals and nt else None, C.c_void_p(best.data_ptr()))
            return (best, tot) if totals else best
        e = None if ext is None else np.ascontiguousarray(ext, np.float64)
        if e is not None and (e.ndim != 2 or e.shape[1] != nt):
            raise ValueError("ext must be [columns, n_traj]")
        ln = None if traj_len is None else np.ascontiguousarray(traj_len, np.int32).reshape(-1)
        if ln is not None and ln.size != nt:
            raise ValueError("traj_len must hold one int per trajectory")
        best = _lib.BestTrajectory(-9, -9, -9.0, -9)
        tot = np.zeros(nt, np.float64) if totals else None
        self._call("gem_costmap_best_trajectory", cs, len(critics), pp, ln.ctypes.data_as(C.c_void_p) if ln is not None and nt else None, nt, T, ps, nv,
                   e.ctypes.data_as(C.c_void_p) if e is not None and e.size else None, int(e.shape[0]) if e is not None else 0,
                   tot.ctypes.data_as(C.c_void_p) if totals and nt else None, C.byref(best))
        res = (int(best.index), float(best.cost), int(best.n_valid))
        return res + (tot,) if totals else res

    # -- DWA's sampled trajectories (gem_hip_trajgen.h) ------------------------------------------------------------------------------
    def dwa_best(self, critics, plan, pos, vel, poses_per_traj: int, spec, totals: bool = False, device: bool = False):
        """SimpleTrajectoryGenerator's trajectories of `plan` (trajgen_plan) from the state pos = (x, y, theta), vel = (vx, vy, vtheta),
        generated on the device into arenas of the handle, then best_trajectory over them: an external critic's column 0 / 1 is the
        generated oscillation / twirling score.  Host form: (index, cost, n_valid), or with totals (index, cost, n_valid, float64
        totals); the call waits.  device=True: an int64 device tensor [4] as best_trajectory's device form leaves it (with totals:
        that and a float64 device tensor), only enqueued.  trajectory_velocity(plan, vel, index) is the winner's command."""
        T = int(poses_per_traj)
        nt = int(plan.n_traj)
        cs = (_lib.Critic * max(len(critics), 1))(*critics)
        ks, ps, nv = self._spec(spec if spec is not None else [])
        p3, v3 = _float3(pos), _float3(vel)
        if device:
            import torch
            dev = torch.device("cuda")
            best = torch.empty((4,), dtype=torch.int64, device=dev)
            tot = torch.empty((nt,), dtype=torch.float64, device=dev) if totals else None
            self.map._hold(best, tot)
            self._call("gem_costmap_dwa_best_device", cs, len(critics), C.byref(plan), p3, v3, T, ps, nv,
                       C.c_void_p(tot.data_ptr()) if totals and nt else None, C.c_void_p(best.data_ptr()))
            return (best, tot) if totals else best
        best = _lib.BestTrajectory(-9, -9, -9.0, -9)
        tot = np.zeros(nt, np.float64) if totals else None
        self._call("gem_costmap_dwa_best", cs, len(critics), C.byref(plan), p3, v3, T, ps, nv,
                   tot.ctypes.data_as(C.c_void_p) if totals and nt else None, C.byref(best))
        res = (int(best.index), float(best.cost), int(best.n_valid))
        return res + (tot,) if totals else res

    # -- trajectory rollout (gem_hip_rollout.h) ------------------------------------------------------------------------------------------
    def rollout_best(self, plan, pos, vel, state_flags: int, spec, flags: int = 0, costs: bool = False, device: bool = False):
        """TrajectoryPlanner::createTrajectories on this costmap: every candidate of `plan` (rollout_plan, made for this pos = (x, y,
        theta), vel = (vx, vy, vtheta) and state_flags) is rolled out against the bytes and the PATH and GOAL grids (prepare_map_grid
        first), then the pick.  Host form: the answer as a dict (rollout_answer), or with costs (answer, float64 costs [n_cand],
        int32 ahead [n_cand]); the call waits.  device=True: a uint8 device tensor [64] holding gem_rollout_best (rollout_answer reads
        it once it is on the host), with costs (that, a float64 and an int32 device tensor); only enqueued."""
        nc = int(plan.n_cand)
        ks, ps, nv = self._spec(spec if spec is not None else [])
        p3, v3 = _double3(pos), _double3(vel)
        if device:
            import torch
            dev = torch.device("cuda")
            best = torch.empty((64,), dtype=torch.uint8, device=dev)
            cost = torch.empty((nc,), dtype=torch.float64, device=dev) if costs else None
            ahead = torch.empty((nc,), dtype=torch.int32, device=dev) if costs else None
            self.map._hold(best, cost, ahead)
            self._call("gem_costmap_rollout_best_device", C.byref(plan), p3, v3, int(state_flags), ps, nv, int(flags),
                       C.c_void_p(cost.data_ptr()) if costs else None, C.c_void_p(ahead.data_ptr()) if costs else None, C.c_void_p(best.data_ptr()))
            return (best, cost, ahead) if costs else best
        best = _lib.RolloutBest(-9, -9, -9, -9.0, -9.0, -9.0, -9.0, -9.0, -9)
        cost = np.zeros(nc, np.float64) if costs else None
        ahead = np.zeros(nc, np.int32) if costs else None
        self._call("gem_costmap_rollout_best", C.byref(plan), p3, v3, int(state_flags), ps, nv, int(flags),
                   cost.ctypes.data_as(C.c_void_p) if costs else None, ahead.ctypes.data_as(C.c_void_p) if costs else None, C.byref(best))
        return (rollout_answer(best), cost, ahead) if costs else rollout_answer(best)


def inflation_table(resolution: float, inflation_radius: float, inscribed_radius: float, cost_scaling_factor: float = 10.0):
    """(R, table): the cell radius and the R * R + 1 costs by squared cell distance that Costmap.inflate uses (gem_inflation_table;
    host only, no device)."""
    lib = _lib.load()
    p = _lib.InflationParams(float(inflation_radius), float(inscribed_radius), float(cost_scaling_factor), 0)
    r = C.c_int(-1)
    if lib.gem_inflation_table(C.byref(p), float(resolution), None, C.byref(r)) != _lib.GEM_OK:
        raise ValueError("inflation_table: a radius, factor or resolution that is not usable, or more than 127 cells")
    table = np.zeros(r.value * r.value + 1, np.uint8)
    if lib.gem_inflation_table(C.byref(p), float(resolution), table.ctypes.data_as(C.c_void_p), None) != _lib.GEM_OK:
        raise ValueError("inflation_table")
    return int(r.value), table


class RobotMotionMapUpdater:
    """RobotMotionMapUpdater (RobotMotionMapUpdater.cpp:42-145): pose covariance -> scalar variance
    increment -> Mapvar_update.  Host-side doubles, exactly one float reaches the device."""

    def __init__(self, covariance_scale: float = 1.0):
        self.covariance_scale = float(covariance_scale)                 # RMU.cpp:25,38
        self.previous_reduced_covariance = np.zeros((4, 4))            # RMU.cpp:27
        self.previous_position = np.zeros(3)
        self.previous_rotation = np.eye(3)

    @staticmethod
    def _yaw_pitch(R):
        return np.arctan2(R[1, 0], R[0, 0]), np.arctan2(-R[2, 0], np.hypot(R[0, 0], R[1, 0]))

    @staticmethod
    def _rotation_vector_z(R):
        c = min(1.0, max(-1.0, 0.5 * (np.trace(R) - 1.0)))
        angle = np.arccos(c)
        wz = 0.5 * (R[1, 0] - R[0, 1])
        return wz if angle < 1e-12 else wz * angle / np.sin(angle)

    def compute(self, position, R_IB, covariance6x6, map_rotation=None) -> float:
        """Returns var_update (the float handed to Mapvar_update, RMU.cpp:80) and advances the state."""
        R = np.asarray(R_IB, np.float64); p = np.asarray(position, np.float64)
        cov = self.covariance_scale * np.asarray(covariance6x6, np.float64)
        Rm = np.eye(3) if map_rotation is None else np.asarray(map_rotation, np.float64)
        yaw, pitch = self._yaw_pitch(R)
        J = np.zeros((4, 6)); J[:3, :3] = np.eye(3)
        J[3, 3:] = [np.cos(yaw) * np.tan(pitch), np.sin(yaw) * np.tan(pitch), 1.0]
        reduced = J @ cov @ J.T                                         # RMU.cpp:107
        rz = self._rotation_vector_z(R)
        Rt = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1.0]])
        v = self.previous_rotation.T @ (p - self.previous_position)    # RMU.cpp:121-123
        F = np.eye(4); F[:3, 3] = skew([0, 0, 1.0]) @ Rt @ v           # RMU.cpp:126-129
        G = np.zeros((4, 4)); G[3, 3] = 1.0; Gt = G.copy()
        G[:3, :3] = Rt.T; Gt[:3, :3] = Rt                              # RMU.cpp:132-137
        relative = G @ (reduced - F @ self.previous_reduced_covariance @ F.T) @ Gt   # RMU.cpp:140-142
        R_BM = R.T @ Rm                                                # RMU.cpp:62-63
        Jr = -R_BM.T                                                   # RMU.cpp:66
        upd = np.float32((Jr @ relative[:3, :3] @ Jr.T)[2, 2])         # RMU.cpp:69,80
        self.previous_reduced_covariance = reduced
        self.previous_position, self.previous_rotation = p.copy(), R.copy()
        return float(upd)

    def update(self, elevation_map: ElevationMap, position, R_IB, covariance6x6, map_rotation=None) -> float:
        u = self.compute(position, R_IB, covariance6x6, map_rotation)
        elevation_map.mapvar_update(u)                                  # RMU.cpp:81
        return u


def adjust_plan(plan, resolution: float) -> np.ndarray:
    """MapGrid::adjustPlanResolution of plan = [n, 2]: points inserted so that no two neighbours lie more than a resolution apart
    (gem_mapgrid_adjust_plan; host only, no device)."""
    lib = _lib.load()
    v = np.ascontiguousarray(plan, np.float64).reshape(-1, 2)
    pv = v.ctypes.data_as(C.POINTER(C.c_double)) if v.size else None
    n = C.c_longlong(-1)
    if lib.gem_mapgrid_adjust_plan(pv, int(v.shape[0]), float(resolution), None, 0, C.byref(n)) != _lib.GEM_OK:
        raise ValueError("adjust_plan: a coordinate or resolution that is not usable, or more than 2^20 points")
    out = np.zeros((int(n.value), 2), np.float64)
    if lib.gem_mapgrid_adjust_plan(pv, int(v.shape[0]), float(resolution), out.ctypes.data_as(C.POINTER(C.c_double)), int(n.value), None) != _lib.GEM_OK:
        raise ValueError("adjust_plan")
    return out


def nav_weights(neutral_cost: int = 50, cost_factor: float = 3.0, lethal_cost: int = 253, allow_unknown: bool = True) -> np.ndarray:
    """The weight table of Costmap.nav_plan as Expander::getCost gives it: int32 [256] by cost byte, 0 = impassable
    (gem_navplan_weights; host only, no device).  A factor under which a traversable cost is not a whole number is refused."""
    out = np.zeros(256, np.int32)
    if _lib.load().gem_navplan_weights(int(neutral_cost), float(cost_factor), int(lethal_cost), int(bool(allow_unknown)),
                                       out.ctypes.data_as(C.POINTER(C.c_int))) != _lib.GEM_OK:
        raise ValueError("nav_weights: parameters out of range, or a traversable cost that is not a positive whole number")
    return out


def _nav_status(st) -> dict:
    return {"found": int(st.found), "n_path": int(st.n_path), "rounds": int(st.rounds), "chunks": int(st.chunks),
            "goal_potential": int(st.goal_potential), "start_cell": (int(st.start_cell[0]), int(st.start_cell[1])),
            "goal_cell": (int(st.goal_cell[0]), int(st.goal_cell[1]))}


def nav_plan_host(grid, start_cell, goal_cell, weights=None, outline: bool = True):
    """The host twin of Costmap.nav_plan (gem_navplan_host; no device): grid = uint8 [size_y, size_x], start_cell and goal_cell (x, y).
    Returns (potential int32 [size_y, size_x], path cells int32 [n] as y * size_x + x, status dict)."""
    g = np.ascontiguousarray(grid, np.uint8)
    if g.ndim != 2 or not g.size:
        raise ValueError("grid must be uint8 [size_y, size_x]")
    w = np.ascontiguousarray(nav_weights() if weights is None else weights, np.int32)
    if w.shape != (256,):
        raise ValueError("weights must be int32 [256]")
    sy, sx = g.shape
    pot = np.zeros((sy, sx), np.int32)
    cells = np.empty(sx * sy, np.int32)
    st = _lib.NavplanStatus()
    s, e = (C.c_int * 2)(*[int(v) for v in start_cell]), (C.c_int * 2)(*[int(v) for v in goal_cell])
    if _lib.load().gem_navplan_host(g.ctypes.data_as(C.c_void_p), sx, sy, w.ctypes.data_as(C.POINTER(C.c_int)), _lib.NAV_OUTLINE if outline else 0,
                                    s, e, pot.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p), int(cells.size), C.byref(st)) != _lib.GEM_OK:
        raise ValueError("nav_plan_host: a negative weight, or size_x * size_y * max(w) not below 2^31 - 1")
    return pot, cells[:st.n_path].copy(), _nav_status(st)


def nav_quad_host(grid, start_cell, goal_cell, weights=None, outline: bool = True):
    """The host twin of Costmap.nav_plan_quadratic (gem_navquad_host; no device): arguments and results of nav_plan_host, weights at
    most 462."""
    g = np.ascontiguousarray(grid, np.uint8)
    if g.ndim != 2 or not g.size:
        raise ValueError("grid must be uint8 [size_y, size_x]")
    w = np.ascontiguousarray(nav_weights() if weights is None else weights, np.int32)
    if w.shape != (256,):
        raise ValueError("weights must be int32 [256]")
    sy, sx = g.shape
    pot = np.zeros((sy, sx), np.int32)
    cells = np.empty(sx * sy, np.int32)
    st = _lib.NavplanStatus()
    s, e = (C.c_int * 2)(*[int(v) for v in start_cell]), (C.c_int * 2)(*[int(v) for v in goal_cell])
    if _lib.load().gem_navquad_host(g.ctypes.data_as(C.c_void_p), sx, sy, w.ctypes.data_as(C.POINTER(C.c_int)), _lib.NAV_OUTLINE if outline else 0,
                                    s, e, pot.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p), int(cells.size), C.byref(st)) != _lib.GEM_OK:
        raise ValueError("nav_quad_host: a negative weight, one above 462, or size_x * size_y * max(w) not below 2^31 - 1")
    return pot, cells[:st.n_path].copy(), _nav_status(st)


def _navpath_result(r) -> dict:
    return {"status": int(r[0]), "n_points": int(r[1]), "goal_cell": (int(r[2]), int(r[3])), "goal_potential": int(r[4])}


def _nav_world_paths(pts, res, geo) -> list:
    """the walks' points reversed (start first) as world points: origin + ((double)p + 0.5) * resolution"""
    o, r = np.array([geo["origin_x"], geo["origin_y"]], np.float64), float(geo["resolution"])
    return [o + (pts[i, :int(res[i, 1])][::-1].astype(np.float64) + 0.5) * r for i in range(pts.shape[0])]


def nav_paths_host(pot, start_cell, goal_cells, form: int = _lib.NAVPATH_GRADIENT, max_points: int = 4096, points: bool = True):
    """The host twin of Costmap.nav_paths, goal by goal (gem_navpath_host; no device): pot = int32 [size_y, size_x], start_cell (x, y),
    goal_cells [n, 2] of (x, y), on the map or not.  Returns (float32 [n, max_points, 2] in walk order, goal first, cell coordinates,
    or None with points=False; int32 [n, 8] result words: status, n_points, goal_cell, goal_potential, three zeros)."""
    p = np.ascontiguousarray(pot, np.int32)
    if p.ndim != 2 or not p.size:
        raise ValueError("pot must be int32 [size_y, size_x]")
    goals = np.ascontiguousarray(goal_cells, np.int32).reshape(-1, 2)
    n = int(goals.shape[0])
    sy, sx = p.shape
    s = (C.c_int * 2)(*[int(v) for v in start_cell])
    pts = np.zeros((n, int(max_points), 2), np.float32) if points and int(max_points) > 0 else None
    res = np.zeros((n, 8), np.int32)
    fn = _lib.load().gem_navpath_host
    for i in range(n):
        e = (C.c_int * 2)(int(goals[i, 0]), int(goals[i, 1]))
        if fn(p.ctypes.data_as(C.c_void_p), sx, sy, s, e, int(form), int(max_points), pts[i].ctypes.data_as(C.c_void_p) if pts is not None else None,
              C.cast(res[i].ctypes.data_as(C.c_void_p), C.POINTER(_lib.NavpathResult))) != _lib.GEM_OK:
            raise ValueError("nav_paths_host: a size of 2^24 or more, max_points outside 2 .. 2^20, or an unknown form")
    return pts, res


def _frontier(f, geo) -> dict:
    """a gem_frontier as a dict; the centroid is origin + (sum / size + 0.5) * resolution, in double, as the C++ facade computes it"""
    res = float(geo["resolution"])
    return {"root": int(f.root), "size": int(f.size), "sum_x": int(f.sum_x), "sum_y": int(f.sum_y), "access_potential": int(f.access_potential),
            "access_cell": int(f.access_cell), "cost": float(f.cost),
            "centroid": (float(geo["origin_x"]) + (float(f.sum_x) / float(f.size) + 0.5) * res,
                         float(geo["origin_y"]) + (float(f.sum_y) / float(f.size) + 0.5) * res)}


def _frontier_status(st, geo) -> dict:
    return {"n_cells": int(st.n_cells), "n_frontiers": int(st.n_frontiers), "n_kept": int(st.n_kept), "best": int(st.best),
            "rounds": int(st.rounds), "chunks": int(st.chunks), "best_frontier": _frontier(st.best_frontier, geo) if st.best >= 0 else None}


def frontiers_host(grid, pot, resolution: float, min_frontier_size: float = 0.0, potential_scale: float = 1.0, gain_scale: float = 1.0,
                   origin=(0.0, 0.0)):
    """The host twin of Costmap.frontiers (gem_frontiers_host; no device): grid = uint8 [size_y, size_x], pot = int32 of the same shape,
    a plan's potential.  Returns (kept frontiers: a list of dicts in ascending root order, labels int32 [size_y, size_x], status dict)."""
    g = np.ascontiguousarray(grid, np.uint8)
    p = np.ascontiguousarray(pot, np.int32)
    if g.ndim != 2 or not g.size or p.shape != g.shape:
        raise ValueError("grid must be uint8 [size_y, size_x] and pot int32 of the same shape")
    sy, sx = g.shape
    prm = _lib.FrontierParams(float(min_frontier_size), float(potential_scale), float(gain_scale))
    labels = np.zeros((sy, sx), np.int32)
    cap = ((sx + 1) // 2) * ((sy + 1) // 2)                             # components of a map: never two in a 2 x 2 block
    rec = (_lib.Frontier * cap)()
    st = _lib.FrontierStatus()
    if _lib.load().gem_frontiers_host(g.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p), sx, sy, float(resolution), C.byref(prm),
                                      labels.ctypes.data_as(C.c_void_p), rec, cap, C.byref(st)) != _lib.GEM_OK:
        raise ValueError("frontiers_host: a resolution or parameter that is not finite, is negative or is above 1e100")
    geo = {"origin_x": origin[0], "origin_y": origin[1], "resolution": resolution}
    return [_frontier(rec[i], geo) for i in range(st.n_kept)], labels, _frontier_status(st, geo)


def _observations(observations):
    """a list of observation dicts (Costmap.observe) -> (gem_observation array, the arrays it points into, whether they are device tensors)"""
    observations = list(observations)
    obs = (_lib.Observation * max(len(observations), 1))()
    keep, kinds = [], set()
    for k, o in enumerate(observations):
        pts = o["points"]
        if _is_device_tensor(pts):
            import torch
            if not pts.is_contiguous() or pts.dim() != 2 or pts.dtype not in (torch.float32, torch.uint8):
                raise ValueError("device points must be a contiguous float32 [n, k] or uint8 [n, bytes] tensor")
            n, step, ptr = int(pts.shape[0]), int(pts.shape[1]) * pts.element_size(), pts.data_ptr()
            kinds.add(True)
        else:
            pts = np.asarray(pts)
            if pts.dtype.fields is None:
                pts = np.ascontiguousarray(pts, np.float32)
                if pts.ndim != 2:
                    raise ValueError("host points must be float32 [n, k >= 3] or an array of records that begin with float x, y, z")
                n, step = int(pts.shape[0]), int(pts.shape[1]) * 4
            else:
                pts = np.ascontiguousarray(pts).reshape(-1)
                n, step = int(pts.shape[0]), int(pts.dtype.itemsize)
            ptr = pts.ctypes.data
            kinds.add(False)
        if step < 12 or step % 4:
            raise ValueError("a record is at least 12 bytes and a multiple of 4 long")
        keep.append(pts)
        flags = (_lib.OBS_MARKING if o.get("marking", True) else 0) | (_lib.OBS_CLEARING if o.get("clearing", True) else 0)
        obs[k] = _lib.Observation(ptr if n else None, n, step, flags, (C.c_double * 3)(*[float(v) for v in o["origin"]]),
                                  float(o.get("obstacle_range", 2.5)), float(o.get("raytrace_range", 3.0)),
                                  float(o.get("min_obstacle_height", 0.0)), float(o.get("max_obstacle_height", 2.0)))
    if len(kinds) > 1:
        raise ValueError("the observations of one call are all host arrays or all device tensors")
    return obs, keep, kinds == {True}


def obstacle_host(grid, resolution: float, origin, observations, layer_max_obstacle_height: float = 2.0, bounds=None):
    """The host twin of Costmap.observe (gem_obstacle_host; no device) on grid = uint8 [size_y, size_x], which is changed in place.
    Returns the merged bounds (None stays None)."""
    if not (isinstance(grid, np.ndarray) and grid.dtype == np.uint8 and grid.ndim == 2 and grid.flags.c_contiguous and grid.flags.writeable):
        raise ValueError("grid must be a writeable contiguous uint8 [size_y, size_x] array")
    obs, keep, on_device = _observations(observations)
    if on_device:
        raise ValueError("obstacle_host takes host arrays")
    cfg = _lib.CostmapConfig(grid.shape[1], grid.shape[0], float(resolution), float(origin[0]), float(origin[1]), 0)
    b = Costmap._bounds(bounds)
    if _lib.load().gem_obstacle_host(grid.ctypes.data_as(C.c_void_p), C.byref(cfg), obs, len(keep), float(layer_max_obstacle_height), b) != _lib.GEM_OK:
        raise ValueError("obstacle_host: an argument the contract of gem_hip_obstacle.h refuses")
    return None if b is None else list(b)


def voxlayer_host(grid, columns, resolution: float, origin, voxels, observations, layer_max_obstacle_height: float = 2.0, bounds=None):
    """The host twin of Costmap.voxel_observe (gem_voxlayer_host; no device) on grid = uint8 [size_y, size_x] and columns = uint32
    [size_y, size_x], both changed in place.  voxels = (size_z, z_resolution, origin_z, unknown_threshold, mark_threshold).  Returns
    the merged bounds (None stays None)."""
    for a, t in ((grid, np.uint8), (columns, np.uint32)):
        if not (isinstance(a, np.ndarray) and a.dtype == t and a.ndim == 2 and a.flags.c_contiguous and a.flags.writeable):
            raise ValueError("grid must be a writeable contiguous uint8 [size_y, size_x] array, columns a uint32 one")
    if grid.shape != columns.shape:
        raise ValueError("grid and columns differ in shape")
    obs, keep, on_device = _observations(observations)
    if on_device:
        raise ValueError("voxlayer_host takes host arrays")
    cfg = _lib.CostmapConfig(grid.shape[1], grid.shape[0], float(resolution), float(origin[0]), float(origin[1]), 0)
    vox = _lib.VoxelConfig(int(voxels[0]), float(voxels[1]), float(voxels[2]), int(voxels[3]), int(voxels[4]))
    b = Costmap._bounds(bounds)
    if _lib.load().gem_voxlayer_host(grid.ctypes.data_as(C.c_void_p), columns.ctypes.data_as(C.c_void_p), C.byref(cfg), C.byref(vox), obs, len(keep),
                                     float(layer_max_obstacle_height), b) != _lib.GEM_OK:
        raise ValueError("voxlayer_host: an argument the contract of gem_hip_voxlayer.h refuses")
    return None if b is None else list(b)


def obstacle_critic(scale: float, flags: int = 0) -> _lib.Critic:
    """ObstacleCostFunction: flags of FOOTPRINT_INSCRIBED_LETHAL | FOOTPRINT_SUM | CRITIC_CENTRE_COST"""
    return _lib.Critic(_lib.CRITIC_OBSTACLE, 0, int(flags), 0, float(scale), 0.0)


def _map_grid_tiled_status(st: _lib.MapGridTiledStatus) -> dict:
    return {"started": int(st.started), "goal_cell": (int(st.goal_cell[0]), int(st.goal_cell[1])), "rounds": int(st.rounds), "chunks": int(st.chunks)}


def map_grid_critic(scale: float, grid: int, xshift: float = 0.0, flags: int = 0) -> _lib.Critic:
    """MapGridCostFunction on CRITIC_GRID_PATH / _GOAL / _FRONT: flags of MAPGRID_STOP_ON_FAILURE | MAPGRID_SUM"""
    return _lib.Critic(_lib.CRITIC_MAPGRID, int(grid), int(flags), 0, float(scale), float(xshift))


def external_critic(scale: float, column: int) -> _lib.Critic:
    """a critic the caller scored: row `column` of best_trajectory's ext"""
    return _lib.Critic(_lib.CRITIC_EXTERNAL, 0, 0, int(column), float(scale), 0.0)


def select_trajectory(critics, scores):
    """The combination and the winner over scores the caller holds, scores = [n_critics, n_traj] (gem_critics_select; host only, no
    device): (index, cost, n_valid, float64 totals)."""
    lib = _lib.load()
    cs = (_lib.Critic * max(len(critics), 1))(*critics)
    s = np.ascontiguousarray(scores, np.float64)
    if s.ndim != 2 or s.shape[0] != len(critics):
        raise ValueError("scores must be [n_critics, n_traj]")
    nt = int(s.shape[1])
    tot = np.zeros(nt, np.float64)
    best = _lib.BestTrajectory(-9, -9, -9.0, -9)
    if lib.gem_critics_select(cs, len(critics), s.ctypes.data_as(C.POINTER(C.c_double)) if s.size else None, nt,
                              tot.ctypes.data_as(C.POINTER(C.c_double)) if nt else None, C.byref(best)) != _lib.GEM_OK:
        raise ValueError("select_trajectory: 1 .. 8 critics, every scale finite and not negative")
    return int(best.index), float(best.cost), int(best.n_valid), tot


# ---- DWA's sampled trajectories (gem_hip_trajgen.h) ---------------------------------------------------------------------------------
def _float3(v, n: int = 3):
    a = [float(x) for x in np.asarray(v, np.float32).reshape(-1)]
    if len(a) != n:
        raise ValueError(f"expected {n} values")
    return (C.c_float * n)(*a)


TRAJGEN_LIMITS = ("max_vel_x", "min_vel_x", "max_vel_y", "min_vel_y", "max_vel_theta", "min_vel_theta", "max_vel_trans", "min_vel_trans",
                  "acc_lim_x", "acc_lim_y", "acc_lim_theta")


def trajgen_plan(limits: dict, config: dict, pos, vel, goal=(0.0, 0.0)) -> "_lib.DwaPlan":
    """SimpleTrajectoryGenerator::initialise (gem_trajgen_plan; host only, no device): the velocity window and the three sample lists
    for the state pos / vel.  limits: the eleven doubles of TRAJGEN_LIMITS; config: sim_time, sim_granularity, angular_sim_granularity,
    sim_period, use_dwa, discretize_by_time, continued_acceleration, oscillation_flags, vsamples = (nx, ny, nth).  The plan's n_traj,
    n_x / n_y / n_th, samples and max_steps (the poses_per_traj a call needs at least) can be read from it."""
    lib = _lib.load()
    L = _lib.TrajgenLimits(*[float(limits[k]) for k in TRAJGEN_LIMITS])
    c = _lib.TrajgenConfig(float(config["sim_time"]), float(config["sim_granularity"]), float(config.get("angular_sim_granularity", 0.0)),
                           float(config["sim_period"]), int(bool(config.get("use_dwa", True))), int(bool(config.get("discretize_by_time", False))),
                           int(bool(config.get("continued_acceleration", False))), int(config.get("oscillation_flags", 0)),
                           (C.c_int * 3)(*[int(v) for v in config["vsamples"]]), 0)
    plan = _lib.DwaPlan()
    if lib.gem_trajgen_plan(C.byref(L), C.byref(c), _float3(pos), _float3(vel), _float3(goal, 2), C.byref(plan)) != _lib.GEM_OK:
        raise ValueError("trajgen_plan: a parameter that is not finite, a time or granularity <= 0, unknown oscillation bits, or lists "
                         "of more than 256 values in sum")
    return plan


def plan_lists(plan):
    """the plan's three float32 lists (x, y, theta)"""
    a = np.ctypeslib.as_array(plan.samples).copy()
    return a[:plan.n_x], a[plan.n_x:plan.n_x + plan.n_y], a[plan.n_x + plan.n_y:plan.n_x + plan.n_y + plan.n_th]


def generate_trajectories(plan, pos, vel, poses_per_traj: int, elevation_map=None, fill=None):
    """SimpleTrajectoryGenerator's trajectories of every sample of the plan: (poses float64 [n_traj * poses_per_traj, 4], traj_len int32
    [n_traj], ext float64 [2, n_traj] = oscillation | twirling, velocities float32 [n_traj, 3]).  Slot t is the sample; a sample that is
    not generated has length 0 and its pose slots, like the slots past a length, keep `fill` (None: zeros).  Without elevation_map the
    host twin (gem_trajgen_generate) into numpy arrays; with one, the kernel into device tensors, only enqueued
    (gem_trajgen_generate_device)."""
    T, nt = int(poses_per_traj), int(plan.n_traj)
    p3, v3 = _float3(pos), _float3(vel)
    if elevation_map is not None:
        import torch
        m = elevation_map
        dev = torch.device("cuda")
        mk = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev) if fill is None else torch.full(shape, fill, dtype=dt, device=dev)
        poses, lens, ext, vels = mk((max(nt * T, 0), 4), torch.float64), mk((nt,), torch.int32), mk((2, nt), torch.float64), mk((nt, 3), torch.float32)
        m._hold(poses, lens, ext, vels)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
        m._check(m._lib.gem_trajgen_generate_device(m._h, C.byref(plan), p3, v3, ptr(poses), ptr(lens), ptr(ext), ptr(vels), T), "gem_trajgen_generate_device")
        return poses, lens, ext, vels
    lib = _lib.load()
    mk = lambda shape, dt: np.zeros(shape, dt) if fill is None else np.full(shape, fill, dt)
    poses, lens, ext, vels = mk((max(nt * T, 0), 4), np.float64), mk((nt,), np.int32), mk((2, nt), np.float64), mk((nt, 3), np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    if lib.gem_trajgen_generate(C.byref(plan), p3, v3, ptr(poses), ptr(lens), ptr(ext), ptr(vels), T) != _lib.GEM_OK:
        raise ValueError("generate_trajectories: a plan trajgen_plan did not make, a state that is not finite, poses_per_traj below the plan's "
                         "max_steps or outside 1 .. 2^20, more than 2^31 - 2 pose slots, or |theta| beyond 64 pi")
    return poses, lens, ext, vels


def trajectory_velocity(plan, vel, index: int):
    """(xv, yv, thetav) of sample `index` of the plan: the command of dwa_best's winner (gem_trajgen_velocity; host only)"""
    lib = _lib.load()
    out = (C.c_float * 3)()
    if lib.gem_trajgen_velocity(C.byref(plan), _float3(vel), int(index), out) != _lib.GEM_OK:
        raise ValueError("trajectory_velocity: an index outside the plan's samples, or a plan trajgen_plan did not make")
    return float(out[0]), float(out[1]), float(out[2])


# ---- trajectory rollout (gem_hip_rollout.h) -------------------------------------------------------------------------------------------
def _double3(v):
    a = [float(x) for x in np.asarray(v, np.float64).reshape(-1)]
    if len(a) != 3:
        raise ValueError("expected 3 values")
    return (C.c_double * 3)(*a)


def rollout_config(config: dict) -> "_lib.RolloutConfig":
    """gem_rollout_config from a dict: the doubles of _lib.ROLLOUT_DOUBLES, the ints of _lib.ROLLOUT_INTS but n_y_vels, and y_vels (a
    sequence of at most eight).  final_goal = (x, y) sets final_goal_x / _y and final_goal_valid."""
    c = _lib.RolloutConfig()
    d = dict(config)
    if d.get("final_goal") is not None:
        d["final_goal_x"], d["final_goal_y"] = d["final_goal"]
        d["final_goal_valid"] = 1
    for k in _lib.ROLLOUT_DOUBLES:
        setattr(c, k, float(d.get(k, 0.0)))
    for k in _lib.ROLLOUT_INTS[:-1]:
        setattr(c, k, int(d.get(k, 0)))
    ys = [float(v) for v in d.get("y_vels", ())]
    if len(ys) > _lib.ROLLOUT_MAX_Y_VELS:
        raise ValueError("at most eight y_vels")
    c.n_y_vels = int(d.get("n_y_vels", len(ys)))
    for i, v in enumerate(ys):
        c.y_vels[i] = v
    return c


def rollout_plan(config, pos, vel, state_flags: int = 0) -> "_lib.RolloutPlan":
    """TrajectoryPlanner::createTrajectories' window and candidates for the state pos / vel and the caller's state flags
    (gem_rollout_plan; host only, no device).  config: a dict (rollout_config) or a _lib.RolloutConfig.  n_cand, off_b / off_c /
    off_d, max_steps, the window and the lists can be read from the plan."""
    c = config if isinstance(config, _lib.RolloutConfig) else rollout_config(config)
    plan = _lib.RolloutPlan()
    if _lib.load().gem_rollout_plan(C.byref(c), _double3(pos), _double3(vel), int(state_flags), C.byref(plan)) != _lib.GEM_OK:
        raise ValueError("rollout_plan: a parameter that is not finite, a time or granularity <= 0, fewer than two samples, more than 256 "
                         "list values in sum, a negative scale, a zero y_vel, unknown state bits, more than 4096 steps, or |theta| beyond 64 pi")
    return plan


def rollout_answer(best) -> dict:
    """gem_rollout_best as a dict: from the ctypes struct, or from the 64 bytes of the device form (a uint8 array or host tensor)"""
    if not isinstance(best, _lib.RolloutBest):
        best = _lib.RolloutBest.from_buffer_copy(np.ascontiguousarray(np.asarray(best), np.uint8).tobytes())
    return {"index": int(best.index), "stage": int(best.stage), "cost": float(best.cost), "raw_cost": float(best.raw_cost),
            "velocity": (float(best.xv), float(best.yv), float(best.thetav)), "bytes": bytes(best)}


def rollout_host(plan, pos, vel, grid, resolution: float, origin, path, goal, spec, flags: int = 0, poses: bool = False, fill=None):
    """The host twin of Costmap.rollout_best (gem_rollout_host; no device) over grid = uint8 [size_y, size_x] and the PATH and GOAL
    distance grids int32 [size_y, size_x]; the state flags are the plan's.  Returns (answer, costs float64 [n_cand], ahead int32
    [n_cand], steps int32 [n_cand]) and with poses also float64 [n_cand, max_steps, 4] whose slots past a candidate's steps keep
    `fill` (None: zeros)."""
    g = np.ascontiguousarray(grid, np.uint8)
    pa, go = np.ascontiguousarray(path, np.int32), np.ascontiguousarray(goal, np.int32)
    if g.ndim != 2 or pa.shape != g.shape or go.shape != g.shape:
        raise ValueError("grid, path and goal must be [size_y, size_x]")
    cfg = _lib.CostmapConfig(g.shape[1], g.shape[0], float(resolution), float(origin[0]), float(origin[1]), 0)
    ks, ps, nv = Costmap._spec(spec if spec is not None else [])
    nc, T = int(plan.n_cand), max(int(plan.max_steps), 1)
    cost, ahead, steps = np.zeros(nc, np.float64), np.zeros(nc, np.int32), np.zeros(nc, np.int32)
    out_poses = (np.zeros((nc, T, 4), np.float64) if fill is None else np.full((nc, T, 4), fill, np.float64)) if poses else None
    best = _lib.RolloutBest()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    if _lib.load().gem_rollout_host(C.byref(plan), _double3(pos), _double3(vel), C.byref(cfg), ptr(g), ptr(pa), ptr(go), ps, nv, int(flags), ptr(cost),
                                    ptr(ahead), ptr(steps), ptr(out_poses) if poses else None, C.byref(best)) != _lib.GEM_OK:
        raise ValueError("rollout_host: an argument the contract of gem_hip_rollout.h refuses")
    res = (rollout_answer(best), cost, ahead, steps)
    return res + (out_poses,) if poses else res


def rollout_pick(plan, state_flags: int, costs, ahead) -> dict:
    """The pick alone over costs float64 [n_cand] and ahead int32 [n_cand] (gem_rollout_pick; host only)"""
    c, a = np.ascontiguousarray(costs, np.float64).reshape(-1), np.ascontiguousarray(ahead, np.int32).reshape(-1)
    if c.size != int(plan.n_cand) or a.size != c.size:
        raise ValueError("one cost and one ahead per candidate")
    best = _lib.RolloutBest()
    if _lib.load().gem_rollout_pick(C.byref(plan), int(state_flags), c.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), C.byref(best)) != _lib.GEM_OK:
        raise ValueError("rollout_pick: a plan rollout_plan did not make, or state flags whose ESCAPING bit is not the plan's")
    return rollout_answer(best)


def contract_sincos(angles):
    """(sin, cos) of float64 angles by the contract's routine (gem_trajgen_sincos; host only): what the kernel and its twin evaluate"""
    lib = _lib.load()
    a = np.ascontiguousarray(angles, np.float64).reshape(-1)
    s, c = np.zeros_like(a), np.zeros_like(a)
    ptr = lambda v: v.ctypes.data_as(C.c_void_p) if v.size else None
    if lib.gem_trajgen_sincos(ptr(a), int(a.size), ptr(s), ptr(c)) != _lib.GEM_OK:
        raise ValueError("contract_sincos")
    return s, c
