#!/usr/bin/env python3
"""composingGlobalMap's outlier filter and road / obstacle split on the device (gem_compose.hip), one MI355X: prints ONE JSON line.

    python tools/bench_compose.py [--frames F] [--cpu-frames C]

C2 geometry (600 x 600 cells at 0.05 m), the surface of tools/bench_local.py: a random valid surface with 5 % NaN and 10 % negative
traversability.  Every frame moves the robot 0.2 m (eight headings in turn), captures, keeps the capture as the previous one and
runs the composing thread's work on it.  Medians over the frames after the warm-up:

  device_us      hipEvents on the handle's stream around gem_local_compose (mean_k 20, multiplier 1.0, threshold 0.0): its kernels,
                 readbacks and the host part between them
  wall_us        host time of the same call, the two record arrays delivered
  sum_host_us    of that call: the host time of the two ordered double sums themselves (gem_debug_get "compose_sum_ns")
  distances      gem_local_compose_distances (the ring walks, the download of the distances, the sums)
  grid_cloud     wall_us of gem_local_grid_cloud on the same capture: the download any host filter pays before it can start
  cpu_ms         the host filter on that download: tests/compose_ref.py's cKDTree path with 16 workers + the ordered sums + the
                 split, standing in for PCL's single-threaded FLANN search

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
import compose_ref  # noqa: E402
from gem_amd import ElevationMap  # noqa: E402

HEADINGS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--cpu-frames", type=int, default=3, help="frames the host filter is timed on")
    args = ap.parse_args()
    L, res = 600, 0.05
    m = ElevationMap(L, res)
    stream = torch.cuda.Stream()
    m.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(7)
    layers = {"elevation": rng.uniform(-0.3, 0.3, (L, L)).astype(np.float32)}
    t = rng.uniform(0.0, 1.0, (L, L)).astype(np.float32)
    t[rng.random((L, L)) < 0.10] = -0.2
    t[rng.random((L, L)) < 0.05] = np.nan
    layers["traver"] = t
    layers["variance"] = rng.uniform(1e-4, 1e-2, (L, L)).astype(np.float32)
    layers["intensity"] = rng.uniform(0, 100, (L, L)).astype(np.float32)
    for name, v in layers.items():
        m.set_layer(name, v)
    for c in ("color_r", "color_g", "color_b"):
        m.set_layer(c, rng.integers(0, 256, (L, L)))
    m.local_enable(1 << 16)

    keys = ["compose", "distances", "grid_cloud"]
    dev = {k: [] for k in keys}; wall = {k: [] for k in keys}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(name, fn, keep):
        ev[0].record(stream)
        t0 = time.perf_counter()
        r = fn()
        t1 = time.perf_counter()
        ev[1].record(stream)
        ev[1].synchronize()
        if keep:
            dev[name].append(ev[0].elapsed_time(ev[1]) * 1e3); wall[name].append((t1 - t0) * 1e6)
        return r

    pos = np.zeros(2)
    far, counts, clouds, thresholds, sum_host = [], [], [], [], []
    for k in range(args.frames + args.warmup):
        keep = k >= args.warmup
        if k:
            pos = pos + 0.2 * np.array(HEADINGS[(k // 8) % 8], float)
        m.move([pos[0], pos[1], 0.0])
        for name, v in layers.items():                    # (a move empties the cells that enter the window: keep the surface whole)
            m.set_layer(name, v)
        m.local_capture()
        m.local_keep_previous()
        road, obstacle, removed, thr = timed("compose", m.local_compose, keep)
        got = (road.shape[0], obstacle.shape[0], removed, thr)
        if keep:
            sum_host.append(m.debug_get("compose_sum_ns") * 1e-3)
            far.append(m.debug_get("compose_far_points")); counts.append(got[:3]); thresholds.append(thr)
        timed("distances", m.local_compose_distances, keep)
        g = timed("grid_cloud", m.local_grid_cloud, keep)
        if keep and len(clouds) < args.cpu_frames:
            clouds.append((g, got))

    cpu = []
    for g, dev_got in clouds:
        t0 = time.perf_counter()
        road, obstacle, removed, thr, _ = compose_ref.compose(g, 20, 1.0, 0.0, workers=16)
        cpu.append((time.perf_counter() - t0) * 1e3)
        assert (road.shape[0], obstacle.shape[0], removed, thr) == dev_got, ((road.shape[0], obstacle.shape[0], removed, thr), dev_got)

    med = lambda v: round(float(np.median(v)), 1) if v else None
    host_path_us = (med(wall["grid_cloud"]) or 0) + 1e3 * (med(cpu) or 0)
    line = {"bench": "compose", "L": L, "resolution": res, "frames": args.frames, "mean_k": 20, "stddev_mul": 1.0, "travers_threshold": 0.0,
            "points": int(np.median([sum(c) for c in counts])), "road": int(np.median([c[0] for c in counts])),
            "obstacle": int(np.median([c[1] for c in counts])), "removed": int(np.median([c[2] for c in counts])),
            "far_points": int(np.median(far)), "threshold": float(np.median(thresholds)),
            "device_us": {k: med(dev[k]) for k in keys}, "wall_us": {k: med(wall[k]) for k in keys},
            "sum_host_us": med(sum_host), "cpu_ms": med(cpu), "cpu_frames": len(cpu),
            "download_plus_cpu_filter_us": round(host_path_us, 1),
            "host_path_over_compose_wall": round(host_path_us / med(wall["compose"]), 2) if cpu else None,
            "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
