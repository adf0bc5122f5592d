#!/usr/bin/env python3
"""A stream of single device-resident LiDAR sweeps (the C2 sensor and pose) into maps of other resolutions: wall time per frame,
the host enqueueing without synchronisation and the device fusing one frame behind (k_frame).  At 0.1 m and 0.2 m the tiles hold
thousands of records and cells tens of them -- the shapes of the reference's own demo maps.

    python tools/res_stream.py [frames]
"""
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from gem_amd import ElevationMap, SensorModel, synth

n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 200
T = synth.pose_matrix(**synth.C2_POSE)
f = synth._frame_for(T, SensorModel.velodyne())
clouds = [torch.from_numpy(synth.lidar_sweep(np.random.default_rng(100 + k), T)).cuda() for k in range(8)]
for L, res in ((600, 0.05), (120, 0.1), (75, 0.2)):
    m = ElevationMap(L, res)
    first = []                                       # the first frames of a fresh map one by one, each fused and synchronised
    for k in range(4):
        t0 = time.perf_counter(); m.add(f, clouds[k % 8]); m.synchronize(); first.append((time.perf_counter() - t0) * 1e6)
    for k in range(16):
        m.add(f, clouds[k % 8])
    m.synchronize()
    t0 = time.perf_counter()
    for k in range(n_frames):
        m.add(f, clouds[k % 8])
    m.synchronize()
    dt = (time.perf_counter() - t0) / n_frames
    out = {"L": L, "res": res, "frames": n_frames, "us_per_frame": dt * 1e6, "first_frames_us_synchronised": [round(x, 1) for x in first]}
    try:                                             # launches of k_frame's lean / generic form ("frame_lean"; a library without the lean form has no such keys)
        out.update({k: m.debug_get(k) for k in ("frame_lean_launches", "frame_generic_launches", "frame_form_seen")})
    except Exception:
        pass
    print(json.dumps(out))
    m.close()
    # the same map WITHOUT a synchronisation behind its first frames: how many launches the host enqueues lean before the slow
    # path's report lands (a handle whose tiles overflow pays the lean slow path on those frames)
    m = ElevationMap(L, res)
    for k in range(64):
        m.add(f, clouds[k % 8])
    m.synchronize()
    try:
        print(json.dumps({"L": L, "res": res, "tight_loop_frames": 64, **{k: m.debug_get(k) for k in ("frame_lean_launches", "frame_generic_launches", "frame_form_seen")}}))
    except Exception:
        pass
    m.close()
