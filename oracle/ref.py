"""ctypes binding of oracle/_ref/libgem_ref.so -- the REFERENCE's own gpu_process.cu compiled for the CPU
(oracle/ref_build/build_ref.py).  TEST INFRASTRUCTURE ONLY: used by tests/ to pin the oracle's restatement against the
reference's code; never imported by gem_amd.

The reference keeps ONE map in file-scope state, so there is one RefMap per process at a time (a new RefMap re-runs
Init_GPU_elevationmap).  Only the laser sensor model and the hard-coded reject filter / thresholds of the reference
exist here (gpu_process.cu:393, 500-504): compare with the oracle configured the same way.

Where the compiled reference cannot be had (no reference sources to build from, no prebuilt library), the tests still run: every
result the reference returned to them is recorded in tests/golden/ref_tape.npz (tests/golden/make_ref_golden.py --tape), keyed
by a digest of the call and of every call before it on the same object, and is played back from there.  A map's answers are
recorded against the oracle's answers to the same calls (SHA-1 of the reference's bits + where they differ from the oracle's,
see _store), the motion / sensor-model answers in full.  A call whose inputs differ from the recorded ones finds no entry, and an
answer that cannot be rebuilt to the recorded digest is refused: both raise.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import sys
from ctypes import POINTER, c_double, c_float, c_int, c_void_p
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE / "ref_build"))
TAPE = HERE.parent / "tests" / "golden" / "ref_tape.npz"
_lib = None


# ---- the recorded results (see the module docstring) ------------------------------------------------------------------------------
_recording = None           # dict of what the live reference returned, while tests/golden/make_ref_golden.py records
_tape = None                # digest -> {field: array}, loaded from TAPE on first use


def _digest(*parts) -> str:
    h = hashlib.sha1()
    for p in parts:
        if isinstance(p, np.ndarray):
            a = np.ascontiguousarray(p)
            h.update(f"{a.dtype.str}{a.shape}".encode()); h.update(a.tobytes())
        else:
            h.update(repr(p).encode())
        h.update(b"|")
    return h.hexdigest()


def start_recording() -> None:
    global _recording
    _recording = {}


def save_recording(path: Path = TAPE) -> int:
    """Writes what was recorded since start_recording(); returns the number of arrays.  The digests and dtypes of every answer go
    into one table (meta_names / meta_sha / meta_dt), the XORs and full arrays one array each."""
    meta = sorted(k.rpartition("@")[0] for k in _recording if k.endswith("@sha"))
    arrays = {k: v for k, v in _recording.items() if not k.endswith(("@sha", "@dt"))}
    arrays["meta_names"] = np.array(meta)
    arrays["meta_sha"] = np.stack([_recording[m + "@sha"] for m in meta]) if meta else np.zeros((0, 20), np.uint8)
    arrays["meta_dt"] = np.array([str(_recording.get(m + "@dt", "")) for m in meta])
    np.savez_compressed(path, **arrays)
    return len(_recording)


def _load_recording(path: Path = TAPE) -> dict:
    """The inverse of save_recording: name@kind -> array."""
    out = {}
    with np.load(path) as z:
        for name in z.files:
            if not name.startswith("meta_"):
                out[name] = z[name]
        for m, sha, dt in zip(z["meta_names"], z["meta_sha"], z["meta_dt"]):
            out[f"{m}@sha"] = sha
            if str(dt):
                out[f"{m}@dt"] = np.array(str(dt))
    return out


def have_tape() -> bool:
    return TAPE.is_file()


# An answer is recorded against the ORACLE's answer to the same call (a twin OracleMap driven in lockstep with the RefMap; where
# there is no twin, in full): per array the SHA-1 of the reference's bits, plus the XOR of its bits with the oracle's where the two
# differ.  Most answers equal the oracle's bit for bit, so the recording holds little more than digests.  Played back, the
# reference's array is rebuilt from the oracle's and must hash to the recorded digest: an oracle that no longer gives what it gave
# when the answer was recorded cannot stand in for the reference, and the call raises.
def _leaves(out) -> dict:
    if isinstance(out, dict):
        return {k: v for k, v in out.items()}
    if isinstance(out, tuple):
        return {f"#{i}": v for i, v in enumerate(out)}
    return {"": out}


def _contig(a) -> np.ndarray:
    a = np.asarray(a)
    return np.ascontiguousarray(a) if a.ndim else a              # (ascontiguousarray makes a 0-d array 1-d)


def _same_size_uint(dt: np.dtype):
    return np.dtype(f"u{dt.itemsize}")


def _store(key: str, out, twin=None) -> None:
    tl = {} if twin is None else _leaves(twin)
    for f, r in _leaves(out).items():
        r = _contig(r)
        name = f"{key}:{f}@"
        _recording[name + "sha"] = np.frombuffer(bytes.fromhex(_digest(r)), np.uint8)
        t = tl.get(f)
        t = None if t is None else _contig(np.asarray(t).astype(r.dtype))
        if t is None or t.shape != r.shape or r.dtype.kind not in "fiub":
            _recording[name + "full"] = r
            continue
        _recording[name + "dt"] = np.array(r.dtype.str)
        u = _same_size_uint(r.dtype)
        x = r.view(u) ^ t.view(u)
        if x.any():
            _recording[name + "xor"] = x


def _played(key: str, twin=None):
    global _tape
    if _tape is None:
        if not have_tape():
            raise RuntimeError(f"the compiled reference is not available and {TAPE.name} is missing")
        _tape = {}
        for name, v in _load_recording().items():
            k, _, rest = name.partition(":")
            f, _, kind = rest.rpartition("@")
            _tape.setdefault(k, {}).setdefault(f, {})[kind] = v
    if key not in _tape:
        raise RuntimeError(f"no recorded result of the reference for this call in {TAPE.name}: its inputs are not the recorded "
                           "ones (re-record with tests/golden/make_ref_golden.py --tape where the reference is available)")
    tl = {} if twin is None else _leaves(twin)
    out = {}
    for f, kinds in _tape[key].items():
        if "full" in kinds:
            r = kinds["full"].copy()
        else:
            dt = np.dtype(str(kinds["dt"]))
            if f not in tl:
                raise RuntimeError(f"{TAPE.name} records this answer against the oracle's, and there is no oracle answer to rebuild it from")
            r = _contig(np.asarray(tl[f]).astype(dt))
            if "xor" in kinds:
                u = _same_size_uint(dt)
                r = (r.view(u) ^ kinds["xor"]).view(dt)
        if _digest(r) != bytes(kinds["sha"]).hex():
            raise RuntimeError(f"the answer of the reference rebuilt from {TAPE.name} does not hash to the recorded digest: the oracle's "
                               "answer to this call has changed since it was recorded")
        out[f] = r
    if "" in out:
        return out[""]
    if all(f.startswith("#") for f in out):
        return tuple(out[f"#{i}"] for i in range(len(out)))
    return out


def _call(key: str, live, twin=None):
    """live() through the compiled reference when it is loaded (recorded when recording), else the recorded result for key; twin:
    the oracle's answer to the same call, what the recording is made against (see _store)."""
    if live is not None:
        out = live()
        if _recording is not None:
            _store(key, out, twin)
        return out
    return _played(key, twin)


def have_map() -> bool:
    return lib() is not None or have_tape()


def have_motion() -> bool:
    return motion_lib() is not None or have_tape()


def have_sensors() -> bool:
    return sensor_lib() is not None or have_tape()


def lib():
    """Load (building when /root/reference is present) the compiled reference; None when neither exists."""
    global _lib
    if _lib is None:
        import build_ref
        path = build_ref.build()
        if path is None:
            return None
        l = C.CDLL(str(path))
        l.gemref_init.argtypes = [c_int, c_float, c_float, c_float]
        l.gemref_process_points.restype = c_int
        l.gemref_process_points.argtypes = [c_void_p] * 9 + [c_int, c_double, c_double, c_float, c_float, c_float] + [c_void_p] * 5
        l.gemref_fuse.argtypes = [c_int, c_int] + [c_void_p] * 7
        l.gemref_mapvar_update.argtypes = [c_int, c_float]
        l.gemref_move.argtypes = [POINTER(c_float), c_float, c_int, POINTER(c_float), POINTER(c_int), POINTER(c_float)]
        l.gemref_map_optmove.argtypes = [POINTER(c_float), c_float, c_float, c_int, POINTER(c_float)]
        l.gemref_map_closeloop.argtypes = [POINTER(c_float), c_float, c_int, c_float]
        l.gemref_map_feature.argtypes = [c_int] + [c_void_p] * 9
        l.gemref_raytracing.argtypes = [c_int]
        l.gemref_get_layer.argtypes = [c_int, c_void_p]; l.gemref_get_layer.restype = c_int
        l.gemref_set_layer.argtypes = [c_int, c_void_p]; l.gemref_set_layer.restype = c_int
        l.gemref_get_pose.argtypes = [POINTER(c_float), POINTER(c_int)]
        _lib = l
    return _lib


def _vp(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


class RefMap:
    """The surface of oracle.OracleMap that the reference implements."""

    FLOAT = {"elevation": 0, "variance": 1, "intensity": 2, "traver": 3, "lowest": 4}
    INT = {"color_r": 5, "color_g": 6, "color_b": 7}

    def __init__(self, length: int, resolution: float, mahalanobis_threshold: float = 5.0, obstacle_threshold: float = 0.7):
        self._l = lib()
        if self._l is None and not have_tape():
            raise RuntimeError("oracle/_ref/libgem_ref.so is missing, the reference is not there to build it from, and there is no recording")
        self.length, self.resolution = int(length), float(resolution)
        self._h = _digest("RefMap", self.length, self.resolution, float(mahalanobis_threshold), float(obstacle_threshold))
        if self._l is not None:
            self._l.gemref_init(self.length, self.resolution, float(mahalanobis_threshold), float(obstacle_threshold))
        self._twin = None                   # the oracle's map, driven in lockstep: what answers are recorded against (see _store)
        if self._l is None or _recording is not None:
            if str(HERE) not in sys.path:
                sys.path.insert(0, str(HERE))
            import oracle
            self._twin = oracle.OracleMap(self.length, self.resolution, float(mahalanobis_threshold))
            self._twin.set_obstacle_threshold(float(obstacle_threshold))

    def _run(self, name, args, live=None, void=False, twin=None):
        """One call on the reference's map: the digest chains every call on this map, so a result is keyed by the whole history.
        twin(oracle_map) makes the same call on the twin."""
        self._h = _digest(self._h, name, *args)
        t = twin(self._twin) if self._twin is not None and twin is not None else None
        if void:
            if self._l is not None:
                live()
            return None
        return _call(self._h, live if self._l is not None else None, t)

    def move(self, position):
        position = [float(v) for v in position]

        def live():
            pos = (c_float * 3)(*position)
            c = (c_float * 2)(); s = (c_int * 2)(); a = (c_float * 2)()
            self._l.gemref_move(pos, self.resolution, self.length, c, s, a)
            return np.array(c[:], np.float32), np.array(s[:], np.int32), np.array(a[:], np.float32)
        return self._run("move", position, live, twin=lambda o: o.move(position))

    def pose(self):
        def live():
            c = (c_float * 2)(); s = (c_int * 2)()
            self._l.gemref_get_pose(c, s)
            return np.array(c[:], np.float32), np.array(s[:], np.int32)
        return self._run("pose", [], live, twin=lambda o: o.pose())

    def process_points(self, frame, x, y, z):
        n = int(np.asarray(x).size)
        xa, ya, za = (np.array(v, np.float32, copy=True).reshape(-1) for v in (x, y, z))
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        T, sj, rv, cs, pm, bs = (f32(frame.T), f32(frame.sensor_jacobian), f32(frame.rotation_variance), f32(frame.C_SB_T),
                                 f32(frame.P_mul_C_BM_T), f32(frame.B_r_BS_skew))
        p = [float(v) for v in frame.model.params]
        lo, hi = float(frame.lower), float(frame.upper)

        def live():
            out = {"index": np.empty(n, np.int32), "var": np.empty(n, np.float32), "x_ts": np.empty(n, np.float32),
                   "y_ts": np.empty(n, np.float32), "height": np.empty(n, np.float32)}
            self._l.gemref_process_points(_vp(out["index"]), _vp(xa), _vp(ya), _vp(za), _vp(out["var"]), _vp(out["x_ts"]), _vp(out["y_ts"]),
                                          _vp(out["height"]), _vp(T), n, lo, hi, p[0], p[1], p[2],
                                          _vp(sj), _vp(rv), _vp(cs), _vp(pm), _vp(bs))
            out["x"], out["y"], out["z"] = xa, ya, za             # the reference overwrites rejected inputs with -1 (GPU:443-446)
            return out
        xyz = (xa.copy(), ya.copy(), za.copy())

        def twin(o):                                              # the oracle configured as the reference is: its hard-coded filter
            import copy
            from gem_amd import RejectFilter
            f = copy.copy(frame); f.filter = RejectFilter.reference()
            out = o.process_points(f, *xyz)
            out["x"], out["y"], out["z"] = xyz                    # (what the reference overwrites of them is in the recording)
            return out
        return self._run("process_points", [*xyz, T, sj, rv, cs, pm, bs, p[:3], lo, hi], live, twin=twin)

    def fuse(self, index, height, var, R=None, G=None, B=None, intensity=None):
        n = int(np.asarray(index).size)
        i, h, v = np.ascontiguousarray(index, np.int32), np.ascontiguousarray(height, np.float32), np.ascontiguousarray(var, np.float32)
        z = lambda a, t: np.zeros(n, t) if a is None else np.ascontiguousarray(a, t)       # the reference always takes the arrays
        r, g, b, I = z(R, np.int32), z(G, np.int32), z(B, np.int32), z(intensity, np.float32)
        self._run("fuse", [i, h, v, r, g, b, I],
                  lambda: self._l.gemref_fuse(self.length, n, _vp(i), _vp(r), _vp(g), _vp(b), _vp(I), _vp(h), _vp(v)), void=True,
                  twin=lambda o: o.fuse(i, h, v, r, g, b, I))

    def mapvar_update(self, u: float):
        self._run("mapvar_update", [float(u)], lambda: self._l.gemref_mapvar_update(self.length, float(u)), void=True,
                  twin=lambda o: o.mapvar_update(float(u)))

    def map_optmove(self, opt_xy, height_update: float):
        xy, hu = [float(opt_xy[0]), float(opt_xy[1])], float(height_update)

        def live():
            p = (c_float * 2)(*xy); out = (c_float * 2)()
            self._l.gemref_map_optmove(p, hu, self.resolution, self.length, out)
            return np.array([out[0], out[1]], np.float32)
        return self._run("map_optmove", [xy, hu], live, twin=lambda o: o.map_optmove(xy, hu))

    def map_closeloop(self, xy, height_update: float):
        xy, hu = [float(xy[0]), float(xy[1])], float(height_update)
        self._run("map_closeloop", [xy, hu],
                  lambda: self._l.gemref_map_closeloop((c_float * 2)(*xy), hu, self.length, self.resolution), void=True,
                  twin=lambda o: o.map_closeloop(xy, hu))

    def raytracing(self):
        self._run("raytracing", [], lambda: self._l.gemref_raytracing(self.length), void=True, twin=lambda o: o.raytracing())

    def map_feature(self):
        def live():
            n = self.length * self.length
            f = {k: np.zeros(n, np.float32) for k in ("elevation", "var", "rough", "slope", "traver", "intensity")}
            c = {k: np.zeros(n, np.int32) for k in "RGB"}
            self._l.gemref_map_feature(self.length, _vp(f["elevation"]), _vp(f["var"]), _vp(c["R"]), _vp(c["G"]), _vp(c["B"]),
                                       _vp(f["rough"]), _vp(f["slope"]), _vp(f["traver"]), _vp(f["intensity"]))
            return {k: f[k].reshape(self.length, self.length) for k in ("rough", "slope", "traver")}
        return self._run("map_feature", [], live, twin=lambda o: o.map_feature())

    def layer(self, name: str) -> np.ndarray:
        def live():
            n = self.length * self.length
            if name in self.INT:
                out = np.empty(n, np.int32); self._l.gemref_get_layer(self.INT[name], _vp(out))
            else:
                out = np.empty(n, np.float32); self._l.gemref_get_layer(self.FLOAT[name], _vp(out))
            return out.reshape(self.length, self.length)
        return self._run("layer", [name], live, twin=lambda o: o.layer(name))

    def set_layer(self, name: str, values):
        if name in self.INT:
            a = np.ascontiguousarray(values, np.int32).reshape(-1)
            self._run("set_layer", [name, a], lambda: self._l.gemref_set_layer(self.INT[name], _vp(a)), void=True,
                      twin=lambda o: o.set_layer(name, a.reshape(self.length, self.length)))
        else:
            a = np.ascontiguousarray(values, np.float32).reshape(-1)
            self._run("set_layer", [name, a], lambda: self._l.gemref_set_layer(self.FLOAT[name], _vp(a)), void=True,
                      twin=lambda o: o.set_layer(name, a.reshape(self.length, self.length)))


# ---- the reference's RobotMotionMapUpdater.cpp compiled against stand-ins for Eigen / kindr / ROS (build_ref.build_motion) ----------
_motion_lib = None


def motion_lib():
    global _motion_lib
    if _motion_lib is None:
        import build_ref
        path = build_ref.build_motion()
        if path is None:
            return None
        l = C.CDLL(str(path))
        l.gemref_motion_create.restype = c_void_p; l.gemref_motion_create.argtypes = [c_double]
        l.gemref_motion_destroy.argtypes = [c_void_p]
        l.gemref_motion_update.restype = c_int
        l.gemref_motion_update.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), c_int, c_double, POINTER(c_float)]
        _motion_lib = l
    return _motion_lib


_sensor_lib = None


def sensor_lib():
    """oracle/_ref/libgem_ref_sensors.so: the reference's Perfect / Stereo / StructuredLight SensorProcessor.cpp (build_ref.build_sensors)."""
    global _sensor_lib
    if _sensor_lib is None:
        import build_ref
        path = build_ref.build_sensors()
        if path is None:
            return None
        l = C.CDLL(str(path))
        l.gemref_sensor_variances.restype = c_int
        l.gemref_sensor_variances.argtypes = [c_int, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double),
                                              c_int, POINTER(c_float), POINTER(c_float), POINTER(c_float), c_int, POINTER(c_int), POINTER(c_float)]
        _sensor_lib = l
    return _sensor_lib


def sensor_variances(model: int, params, rotation_map_to_base, rotation_base_to_sensor, translation_base_to_sensor, pose_covariance,
                     x, y, z, original_width: int = 0, indices=None) -> np.ndarray:
    """What the reference's own computeVariances writes for a cloud (model: 1 structured light, 2 stereo, 3 perfect).  The rotations
    are what SensorProcessorBase::updateTransformations stores (SPB.cpp:110-117); pose_covariance is the 6x6 robot pose covariance."""
    l = sensor_lib()
    if l is None and not have_tape():
        raise RuntimeError("oracle/_ref/libgem_ref_sensors.so is missing, the reference is not there to build it from, and there is no recording")
    dp = lambda a, n: np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1)[:n] if n else np.asarray(a, np.float64).reshape(-1))
    prm = np.zeros(8, np.float64); prm[:len(params)] = params
    cbm, csb, t, cov = dp(rotation_map_to_base, 9), dp(rotation_base_to_sensor, 9), dp(translation_base_to_sensor, 3), dp(pose_covariance, 36)
    xs, ys, zs = (np.ascontiguousarray(v, np.float32) for v in (x, y, z))
    n = xs.size
    idx = np.ascontiguousarray(np.arange(n) if indices is None else indices, np.int32)
    p = lambda a, t_: a.ctypes.data_as(POINTER(t_))

    def live():
        out = np.empty(n, np.float32)
        rc = l.gemref_sensor_variances(int(model), p(prm, c_double), p(cbm, c_double), p(csb, c_double), p(t, c_double), p(cov, c_double), n,
                                       p(xs, c_float), p(ys, c_float), p(zs, c_float), int(original_width), p(idx, c_int), p(out, c_float))
        if rc != n:
            raise RuntimeError(f"gemref_sensor_variances returned {rc}")
        return out
    key = _digest("sensor_variances", int(model), prm, cbm, csb, t, cov, xs, ys, zs, int(original_width), idx)
    return _call(key, live if l is not None else None)


def quaternion_from_matrix(R) -> np.ndarray:
    """Hamilton unit quaternion (w, x, y, z), w >= 0, of a rotation matrix."""
    R = np.asarray(R, np.float64)
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2; q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R))); j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = [0.0] * 4
        q[0] = (R[k, j] - R[j, k]) / s; q[1 + i] = 0.25 * s; q[1 + j] = (R[j, i] + R[i, j]) / s; q[1 + k] = (R[k, i] + R[i, k]) / s
    q = np.array(q); q /= np.linalg.norm(q)
    return q if q[0] >= 0 else -q


class RefMotion:
    """RobotMotionMapUpdater of the reference: update() with a pose (position, rotation matrix R_IB), the 6 x 6 pose covariance and
    the map's rotation; returns the float it hands to Mapvar_update (RMU.cpp:80-81)."""

    def __init__(self, covariance_scale: float = 1.0, length: int = 600):
        self._l = motion_lib()
        if self._l is None and not have_tape():
            raise RuntimeError("oracle/_ref/libgem_ref_motion.so is missing, the reference is not there to build it from, and there is no recording")
        self._u = self._l.gemref_motion_create(covariance_scale) if self._l is not None else None
        self._t, self._len = 0.0, length
        self._h = _digest("RefMotion", float(covariance_scale), int(length))

    def __del__(self):
        if getattr(self, "_u", None):
            self._l.gemref_motion_destroy(self._u); self._u = None

    def compute(self, position, R_IB, cov6x6, map_rotation=None) -> float:
        d = lambda a, n: (c_double * n)(*np.asarray(a, np.float64).reshape(-1).tolist())
        self._t += 1.0
        q, mq = quaternion_from_matrix(R_IB), quaternion_from_matrix(np.eye(3) if map_rotation is None else map_rotation)
        pos, cov = np.asarray(position, np.float64).reshape(-1), np.asarray(cov6x6, np.float64).reshape(-1)
        self._h = _digest(self._h, "compute", pos, q, cov, mq, self._t)

        def live():
            out = c_float()
            ok = self._l.gemref_motion_update(self._u, d(pos, 3), d(q, 4), d(cov, 36), d(mq, 4), self._len, self._t, C.byref(out))
            assert ok == 1, "the reference skipped the update"
            return np.float32(out.value)
        return float(_call(self._h, live if self._l is not None else None))
