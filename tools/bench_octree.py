#!/usr/bin/env python3
"""composingGlobalMap's two ColorOcTrees on the device (gem_octree.hip), one MI355X: prints ONE JSON line.

    python tools/bench_octree.py [--frames F] [--cpu-frames C]

tools/bench_compose.py's scene (C2 geometry, 600 x 600 cells at 0.05 m, a random valid surface with 5 % NaN and 10 % negative
traversability, seeded) and its frame loop: move 0.2 m, capture, keep the capture as the previous one, run the composing thread's
work on it.  Medians over the frames after the warm-up, both paths measured in the SAME run, in turn, on the same capture:

  octrees        wall_us / device_us of gem_local_compose_octrees (road 0.2 m, obstacle 0.1 m) + both gem_octree_read: what the node
                 publishes
  compose        the path this replaces, as far as the device goes: gem_local_compose with both lists delivered
  build_only     gem_octree_build_device on the road list already on the device (the builder without the filter), for the stage costs
  stream_bytes   the two streams, against list_bytes (32 bytes per record of the two lists)
  insert_cpu_ms  the host insertion the old path still has to do on the lists: tests/octree_ref.py's literal pointer tree in
                 Python.  A STAND-IN for octomap's C++ loop, far slower than it: it says the work exists, not what it costs there.

The kernels' own times come from rocprofv3 --kernel-trace --stats on this script (profiles/octree_c2.txt).
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
import octree_ref  # noqa: E402
from gem_amd import ElevationMap  # noqa: E402

HEADINGS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--cpu-frames", type=int, default=0, help="frames the literal Python insertion is timed (and compared) on")
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

    keys = ["octrees", "compose", "build_only"]
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

    def octrees():
        out = m.local_compose_octrees(0.2, 0.1)
        return out, m.octree_read(0), m.octree_read(1)

    pos = np.zeros(2)
    sizes, lists, stats, kept = [], [], [], []
    for k in range(args.frames + args.warmup):
        keep = k >= args.warmup
        if k:
            pos = pos + 0.2 * np.array(HEADINGS[(k // 8) % 8], float)
        m.move([pos[0], pos[1], 0.0])
        for name, v in layers.items():                    # (a move empties the cells that enter the window: keep the surface whole)
            m.set_layer(name, v)
        m.local_capture()
        m.local_keep_previous()
        order = (0, 1) if k & 1 else (1, 0)               # the two paths in turn, neither always first
        for which in order:
            if which == 0:
                (nr, no, removed, thr, st), road_bytes, obstacle_bytes = timed("octrees", octrees, keep)
            else:
                road, obstacle, removed2, thr2 = timed("compose", m.local_compose, keep)
        assert (nr, no, removed, thr) == (road.shape[0], obstacle.shape[0], removed2, thr2)
        d_road = torch.from_numpy(road.view(np.uint8).reshape(-1, 32)).to("cuda:0")
        torch.cuda.synchronize()
        timed("build_only", lambda: m.octree_build(2, d_road, 0.2), keep)
        assert m.octree_read(2) == road_bytes
        if keep:
            sizes.append((len(road_bytes), len(obstacle_bytes))); lists.append(32 * (nr + no)); stats.append(st)
            if len(kept) < args.cpu_frames:
                kept.append((road, obstacle, road_bytes, obstacle_bytes))

    cpu = []
    for road, obstacle, rb, ob in kept:
        t0 = time.perf_counter()
        a = octree_ref.build_literal(road, octree_ref.Params(0.2))[0]
        b = octree_ref.build_literal(obstacle, octree_ref.Params(0.1))[0]
        cpu.append((time.perf_counter() - t0) * 1e3)
        assert a == rb and b == ob

    med = lambda v: round(float(np.median(v)), 1) if v else None
    spread = lambda v: [round(float(np.min(v)), 1), round(float(np.max(v)), 1)] if v else None
    line = {"bench": "octree", "L": L, "resolution": res, "frames": args.frames, "road_resolution": 0.2, "obstacle_resolution": 0.1,
            "points": int(np.median([s[0]["points_in"] + s[1]["points_in"] for s in stats])),
            "wall_us": {k: med(wall[k]) for k in keys}, "wall_us_min_max": {k: spread(wall[k]) for k in keys},
            "device_us": {k: med(dev[k]) for k in keys},
            "stream_bytes": [int(np.median([s[0] for s in sizes])), int(np.median([s[1] for s in sizes]))], "list_bytes": int(np.median(lists)),
            "nodes": [int(np.median([s[i]["nodes"] for s in stats])) for i in (0, 1)],
            "coupled_blocks": [[int(np.median([s[i]["coupled_blocks"][j] for s in stats])) for j in range(3)] for i in (0, 1)],
            "fallback_points": [int(np.max([s[i]["fallback_points"] for s in stats])) for i in (0, 1)],
            "octrees_over_compose_wall": round(med(wall["octrees"]) / med(wall["compose"]), 3),
            "insert_cpu_ms": med(cpu), "cpu_frames": len(cpu), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
