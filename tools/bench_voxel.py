#!/usr/bin/env python3
"""The VoxelGrid pre-filter on the device (gem_voxel.hip), one MI355X: prints ONE JSON line.

    python tools/bench_voxel.py [--reps R]

  voxel_device   gem_voxel_device on the C2 sweep (131 072 points, inputs resident in HBM): filter.launch's one stage and
                 filter_kitti_launch's three, microseconds per call (stream-synchronised loop of R calls, outputs reused)
  add_voxel      add_voxel of the raw C2 sweep from a device tensor (filter + fuse) against add of the same cloud filtered
                 beforehand (device tensor), microseconds per frame; the two maps are checked to be bit-identical
  numpy_ref      tests/voxel_ref.py on the same sweep, milliseconds per call: the CPU restatement, NOT the product
bench.py stays the contract line (C2); kernel times and launches per stage come from rocprofv3 --kernel-trace --stats.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
import torch  # noqa: E402
import voxel_ref  # noqa: E402
from gem_amd import ElevationMap, VoxelStage, synth  # noqa: E402


def per_call(emap, fn, reps, warm=5):
    for _ in range(warm):
        fn()
    emap.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    emap.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_voxel.py needs a HIP device"
    wl = synth.config_c2()
    cloud, f = wl.clouds[0], wl.frames[0]
    d = torch.from_numpy(cloud).cuda()
    res = {"tool": "bench_voxel", "device": torch.cuda.get_device_name(0), "reps": args.reps, "points": int(cloud.shape[0])}
    emap = ElevationMap(64, 0.1)
    emap.reserve(cloud.shape[0])
    for label, stages in (("filter_launch_1_stage", VoxelStage.filter_launch()), ("filter_kitti_launch_3_stages", VoxelStage.filter_kitti_launch())):
        out = emap.voxel_device(stages, d)
        ex, _, k = voxel_ref.voxel(cloud, None, stages)
        assert int(out[2].item()) == k and np.array_equal(out[0].cpu().numpy().view(np.uint32), ex.view(np.uint32))
        s = per_call(emap, lambda: emap.voxel_device(stages, d, sync=False, out=out), args.reps)
        t0 = time.perf_counter()
        for _ in range(3):
            voxel_ref.voxel(cloud, None, stages)
        res[label] = {"centroids": int(k), "us_per_call": round(1e6 * s, 2),
                      "numpy_ref_ms_per_call": round(1e3 * (time.perf_counter() - t0) / 3, 2)}
    emap.close()
    stages = VoxelStage.filter_launch()
    fx, _, k = voxel_ref.voxel(cloud, None, stages)
    d_f = torch.from_numpy(np.ascontiguousarray(fx[:k])).cuda()
    maps = []
    for name, fn in (("add_voxel_device", lambda m: m.add_voxel(f, stages, d)), ("add_device_prefiltered", lambda m: m.add(f, d_f))):
        m = ElevationMap(wl.length, wl.resolution)
        m.reserve(cloud.shape[0])
        res[f"us_{name}"] = round(1e6 * per_call(m, lambda: fn(m), args.reps), 2)
        maps.append(m)
    res["maps_identical"] = all(np.array_equal(maps[0].layer(x).view(np.uint32), maps[1].layer(x).view(np.uint32))
                                for x in ("elevation", "variance", "intensity"))
    for m in maps:
        m.close()
    res["goals_us"] = {"one_stage": 25, "three_stage_chain": 60, "add_voxel_device_per_frame": 40}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
