#!/usr/bin/env python3
"""The rolling-window local map on the device (gem_local.hip), one MI355X: prints ONE JSON line.

    python tools/bench_local.py [--frames F]

C2 geometry (600 x 600 cells at 0.05 m).  The map is filled once with a random valid surface (5 % NaN and 10 % negative
traversability); then every frame moves the robot 0.2 m along a trajectory that turns through all eight shift-sign cases (eight
headings in turn), and runs the node's order capture -> spill (gated as EMg.cpp:715) -> grid_cloud -> keep_previous.  Per frame:

  device_us    hipEvents on the handle's stream around each call: the kernels plus, for spill and grid_cloud, their readbacks
  wall_us      host time of the call, the download to the caller's array included
  cpu_ms       the restatement of tests/local_ref.py on the same frames (numpy + a Python dict), from the device's own show():
               capture (record building) + spill + grid_cloud

bench.py stays the contract line (C2); the kernels' own times come from rocprofv3 --kernel-trace --stats.
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
import local_ref  # noqa: E402
from gem_amd import ElevationMap  # noqa: E402

HEADINGS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--cpu-frames", type=int, default=16, help="frames the CPU restatement is timed on (it is slow)")
    args = ap.parse_args()
    L, res = 600, 0.05
    m = ElevationMap(L, res)
    stream = torch.cuda.Stream()
    m.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(7)
    m.set_layer("elevation", rng.uniform(-0.3, 0.3, (L, L)).astype(np.float32))
    t = rng.uniform(0.0, 1.0, (L, L)).astype(np.float32)
    t[rng.random((L, L)) < 0.10] = -0.2
    t[rng.random((L, L)) < 0.05] = np.nan
    m.set_layer("traver", t)
    m.set_layer("variance", rng.uniform(1e-4, 1e-2, (L, L)).astype(np.float32))
    m.set_layer("intensity", rng.uniform(0, 100, (L, L)).astype(np.float32))
    for c in ("color_r", "color_g", "color_b"):
        m.set_layer(c, rng.integers(0, 256, (L, L)))
    m.local_enable(1 << 20)

    names = ("capture", "spill", "grid_cloud")
    dev = {k: [] for k in names}; wall = {k: [] for k in names}
    spilled = []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(name, fn):
        ev[0].record(stream)
        t0 = time.perf_counter()
        r = fn()
        t1 = time.perf_counter()
        ev[1].record(stream)
        ev[1].synchronize()
        dev[name].append(ev[0].elapsed_time(ev[1]) * 1e3); wall[name].append((t1 - t0) * 1e6)
        return r

    pos, center = np.zeros(2), np.zeros(2, np.float32)
    frames = []
    for k in range(args.frames):
        if k:
            pos = pos + 0.2 * np.array(HEADINGS[(k // 8) % 8], float)
        c = m.move([pos[0], pos[1], 0.0])[0]
        shift = (c - center).astype(np.float32); center = c
        timed("capture", m.local_capture)
        if k == 0:
            m.local_keep_previous()
        if abs(float(shift[0])) >= res or abs(float(shift[1])) >= res:
            out, _ = timed("spill", lambda: m.local_spill(center, shift))
            spilled.append(out.size)
        timed("grid_cloud", m.local_grid_cloud)
        if k < args.cpu_frames:
            frames.append((m.show(), tuple(m.pose()[1]), center.copy(), shift.copy()))
        m.local_keep_previous()

    # the CPU restatement on the first frames: capture from show()'s visual, spill into a dict, grid cloud
    d, prev, cpu = {}, None, []
    for k, (o, start, cen, shift) in enumerate(frames):
        t0 = time.perf_counter()
        cap = local_ref.capture(o, L, L * float(np.float32(res)), float(np.float32(res)), (float(cen[0]), float(cen[1])), start)
        if k == 0:
            prev = cap
        if abs(float(shift[0])) >= res or abs(float(shift[1])) >= res:
            local_ref.spill(prev, cen, shift, d)
        local_ref.grid_cloud(cap)
        cpu.append((time.perf_counter() - t0) * 1e3)
        prev = cap

    med = lambda v: round(float(np.median(v)), 1) if v else None
    line = {"bench": "local_map", "L": L, "resolution": res, "frames": args.frames, "step_m": 0.2,
            "spilled_per_frame_median": int(np.median(spilled)) if spilled else 0, "entries": m.local_size(),
            "grid_cloud_points": int(m.local_grid_cloud().size),
            "device_us": {k: med(dev[k]) for k in names}, "wall_us": {k: med(wall[k]) for k in names},
            "device_us_per_frame": round(sum(med(dev[k]) or 0 for k in names), 1),
            "wall_us_per_frame": round(sum(med(wall[k]) or 0 for k in names), 1),
            "cpu_restatement_ms_per_frame": med(cpu), "cpu_frames": len(cpu),
            "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
