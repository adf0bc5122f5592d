#!/usr/bin/env python3
"""Golden vectors produced by the REFERENCE'S OWN CODE: /root/reference/.../gpu_process.cu compiled for the CPU
(oracle/ref_build/build_ref.py -> oracle/_ref/libgem_ref.so; kernels run sequentially over their grids, CUDA runtime and
Eigen are stand-ins).  Run in the build container (needs /root/reference):

    python tests/golden/make_ref_golden.py        # rewrites tests/golden/ref_scene.npz

ref_scene.npz is ONE scripted session of the reference's interface on an 80 x 80 @ 0.1 m map, inputs and outputs:
  Init_GPU_elevationmap -> Move -> [Mapvar_update, Process_points, Fuse] x 3 frames (a Move between them) -> Map_feature
  -> Raytracing.  Stored: the clouds and frame constants; per frame the five Process_points outputs and the elevation /
  variance / lowest layers after the Fuse; the pose after every Move; rough / slope / traver of Map_feature; elevation and
  lowest after Raytracing.
tests/test_golden.py replays the session on the oracle (CPU) and on libgem_hip (GPU) against these arrays, so the pin
travels with the repository (the GPU box has no /root/reference).

    python tests/golden/make_ref_golden.py --tape [--merge] [-- PYTEST ARGS]     # rewrites tests/golden/ref_tape.npz

ref_tape.npz holds every result the compiled reference returns to the tests (oracle/ref.py), recorded while they run against
the live libraries (default: the CPU tests), so that they run where the reference cannot be built: a map's answers as their
SHA-1 and their difference from the oracle's answers to the same calls (mostly none), the rest in full.  --merge keeps the entries
already recorded (e.g. to add those of the GPU tests, recorded on a GPU machine with the prebuilt oracle/_ref libraries).  The
same run rewrites header_pin_ref.bin (the answers tests/cpp/header_pin.cpp gets from the motion / sensor libraries) and
caller_symbols.json (the mangled names the reference's callers link against, tests/test_cabi.py).
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "oracle"))

import ref  # noqa: E402
from gem_amd import RejectFilter, SensorModel, synth  # noqa: E402

F32 = np.float32
L, RES = 80, 0.1
POSES = [(0.3, -0.2, 0.5, 0.0), (0.9, 0.4, 0.55, 0.8), (0.1, 1.3, 0.6, -0.6)]        # x, y, z, yaw of the sensor per frame


def scene_frame(k):
    x, y, z, yaw = POSES[k]
    f = synth._frame_for(synth.pose_matrix(x, y, z, yaw, 0.01, -0.015), SensorModel.velodyne())
    f.filter = RejectFilter.reference()                     # the reference's hard-coded filter (gpu_process.cu:393)
    f.lower, f.upper = -3.0, 3.0
    return f


def scene_cloud(k):
    c = synth.random_cloud(900 + k, 6_000, 4.2, z_sigma=0.25)
    c[:, 3] = 0
    return c


def main():
    if ref.lib() is None:
        raise SystemExit("needs /root/reference (or a prebuilt oracle/_ref/libgem_ref.so)")
    r = ref.RefMap(L, RES)
    out = {"length": np.int32(L), "resolution": F32(RES)}
    for k in range(3):
        pos = np.array(POSES[k][:3], F32)
        c, s, a = r.move(pos)
        out[f"pos_{k}"], out[f"center_{k}"], out[f"start_{k}"], out[f"shift_{k}"] = pos, c, s, a
        f, cloud = scene_frame(k), scene_cloud(k)
        u = F32(1e-5 * (k + 1))
        r.mapvar_update(float(u))
        pp = r.process_points(f, cloud[:, 0], cloud[:, 1], cloud[:, 2])
        r.fuse(pp["index"], pp["height"], pp["var"])
        out[f"cloud_xyz_{k}"], out[f"var_update_{k}"] = np.ascontiguousarray(cloud[:, :3]), u
        for key in ("index", "var", "x_ts", "y_ts", "height"):
            out[f"pp_{key}_{k}"] = pp[key]
        for name in ("elevation", "variance", "lowest"):
            out[f"{name}_{k}"] = r.layer(name)
    feat = r.map_feature()
    live = r.layer("elevation") != -10
    for key in ("rough", "slope", "traver"):
        out[f"feature_{key}"] = np.where(live, feat[key], 0).astype(F32)          # empty cells: uninitialised in the reference
    out["feature_live"] = live
    out["traver_layer"] = r.layer("traver")
    r.raytracing()
    out["elevation_after_raytracing"] = r.layer("elevation")
    out["lowest_after_raytracing"] = r.layer("lowest")
    out["deleted"] = np.int32(int(live.sum()) - int((out["elevation_after_raytracing"] != -10).sum()))
    np.savez_compressed(HERE / "ref_scene.npz", **out)
    print("ref_scene.npz:", {k: (v.shape if hasattr(v, "shape") else v) for k, v in list(out.items())[:6]}, "... deleted by raytracing:", int(out["deleted"]),
          "accepted per frame:", [int((out[f"pp_index_{k}"] >= 0).sum()) for k in range(3)])


def record_tape(merge: bool, pytest_args: list[str]) -> int:
    import pytest
    if ref.lib() is None or ref.motion_lib() is None or ref.sensor_lib() is None:
        raise SystemExit("recording needs the compiled reference (the reference sources, or prebuilt oracle/_ref libraries)")
    ref.start_recording()
    if merge and ref.have_tape():
        ref._recording.update(ref._load_recording())
    before = len(ref._recording)
    class Record:                   # the two C++-side recordings of tests/test_cabi.py
        @staticmethod
        def pytest_collection_finish(session):
            for item in session.items:
                for flag in ("HEADER_PIN_RECORD", "RECORD_CALLER_SYMBOLS"):
                    if hasattr(item.module, flag):
                        setattr(item.module, flag, True)
    rc = pytest.main(["-q", "-p", "no:cacheprovider", str(ROOT / "tests")] + (pytest_args or ["-m", "not gpu"]), plugins=[Record()])
    if rc != 0:
        raise SystemExit(f"pytest failed ({rc}): nothing written")
    n = ref.save_recording()
    print(f"{ref.TAPE.name}: {n} arrays ({n - before} new), {ref.TAPE.stat().st_size} bytes")
    return 0


if __name__ == "__main__":
    if "--tape" in sys.argv:
        args = sys.argv[sys.argv.index("--") + 1:] if "--" in sys.argv else []
        sys.exit(record_tape("--merge" in sys.argv[:sys.argv.index("--")] if "--" in sys.argv else "--merge" in sys.argv, args))
    main()
