#!/usr/bin/env python3
"""The submap stack on the device (gem_global.hip), one MI355X: prints ONE JSON line.

    python tools/bench_global.py [--submaps S] [--records N] [--reps R]

  push_local       C2 geometry (600 x 600 cells at 0.05 m), a random valid surface; between two pushes the robot moves 16 frames of
                   0.2 m (capture -> spill -> keep_previous), so the local map holds the band it left behind; then
                   gem_global_push_local(clear) appends the local map's export and the grid cloud as one submap, device to device
  loop_closure     S submaps of N records at 0.05 m (distinct cells drawn from a 40 m square around each centre), centres 10 m
                   apart around a loop, so every neighbour list at radius 25 m has five entries (i, its two neighbours on either
                   side: four pair steps); small random yaw / translation transforms.  Timed in total, and once with the centres
                   moved apart (transforms only, no pair step): per step = (total - transforms only) / steps
  device_ms        hipEvents on the handle's stream around each call; wall_ms the host time of the call
  cpu_restatement  tests/global_ref.py (numpy + Python dicts) on a smaller stack, labelled as what it is: the restatement, not the node

bench.py stays the contract line (C2); the kernels' own times come from rocprofv3 --kernel-trace --stats.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
import torch  # noqa: E402
import global_ref  # noqa: E402
from gem_amd import ElevationMap  # noqa: E402

F32 = np.float32
HEADINGS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]


def submap(rng, n, cx, cy, res=0.05, side=40.0):
    cells = int(side / res)
    pick = rng.choice(cells * cells, n, replace=False)
    ix, iy = pick % cells, pick // cells
    cx, cy = round(cx / res) * res, round(cy / res) * res
    out = np.zeros(n, global_ref.POINT)
    out["x"] = (cx + (ix - cells / 2 + 0.5) * res).astype(F32)
    out["y"] = (cy + (iy - cells / 2 + 0.5) * res).astype(F32)
    out["z"] = rng.uniform(-0.5, 1.5, n).astype(F32)
    out["pad"] = 1.0
    for f in ("r", "g", "b"):
        out[f] = rng.integers(0, 256, n)
    out["covariance"] = rng.uniform(1e-4, 0.05, n).astype(F32)
    out["intensity"] = rng.uniform(0, 100, n).astype(F32)
    out["travers"] = rng.uniform(0, 1, n).astype(F32)
    return out


def loop_centres(S, spacing=10.0):
    r = S * spacing / (2 * math.pi)
    return np.array([[r * math.cos(2 * math.pi * i / S), r * math.sin(2 * math.pi * i / S)] for i in range(S)], F32)


def transforms(rng, S):
    t = np.zeros((S, 4, 4), F32)
    for i in range(S):
        a = rng.uniform(-0.01, 0.01)
        t[i] = [[math.cos(a), -math.sin(a), 0, rng.uniform(-0.1, 0.1)], [math.sin(a), math.cos(a), 0, rng.uniform(-0.1, 0.1)],
                [0, 0, 1, 0], [0, 0, 0, 1]]
    return t


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--submaps", type=int, default=16)
    ap.add_argument("--records", type=int, default=500_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pushes", type=int, default=6)
    ap.add_argument("--cpu-submaps", type=int, default=4)
    ap.add_argument("--cpu-records", type=int, default=50_000)
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record(stream)
        t0 = time.perf_counter()
        r = fn()
        t1 = time.perf_counter()
        ev[1].record(stream)
        ev[1].synchronize()
        return r, ev[0].elapsed_time(ev[1]), (t1 - t0) * 1e3

    # -- push_local at C2 geometry
    L, res = 600, 0.05
    m = ElevationMap(L, res)
    m.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(7)
    m.set_layer("elevation", rng.uniform(-0.3, 0.3, (L, L)).astype(F32))
    tr = rng.uniform(0.0, 1.0, (L, L)).astype(F32)
    tr[rng.random((L, L)) < 0.05] = np.nan
    m.set_layer("traver", tr)
    m.set_layer("variance", rng.uniform(1e-4, 1e-2, (L, L)).astype(F32))
    m.local_enable(1 << 20)
    m.global_enable(1 << 24)
    pos, center = np.zeros(2), np.zeros(2, F32)
    push_dev, push_wall, push_n = [], [], []
    k = 0
    for p in range(args.pushes):
        for _ in range(16):
            if k:
                pos = pos + 0.2 * np.array(HEADINGS[(k // 8) % 8], float)
            c = m.move([pos[0], pos[1], 0.0])[0]
            shift = (c - center).astype(F32); center = c
            m.local_capture()
            if k == 0:
                m.local_keep_previous()
            if abs(float(shift[0])) >= res or abs(float(shift[1])) >= res:
                m.local_spill(center, shift)
            m.local_keep_previous()
            k += 1
        before = m.local_size()
        i, d, w = timed(lambda: m.global_push_local(True))
        if p:                                                     # the first one grows nothing but still allocates its slot
            push_dev.append(d); push_wall.append(w)
        push_n.append(before)
    push_records = int(np.median([s.size for s in (m.global_export(j) for j in range(m.global_count()))]))
    del m

    # -- loop closure on S submaps of N records
    S, N = args.submaps, args.records
    g = ElevationMap(32, res)
    g.set_stream(stream.cuda_stream)
    centres = loop_centres(S)
    far = centres * 100.0
    steps = sum(max(len(global_ref.neighbours(centres, S, i, 25.0)) - 1, 0) for i in range(S)
                if len(global_ref.neighbours(centres, S, i, 25.0)) > 2)
    rng = np.random.default_rng(3)
    clouds = [submap(rng, N, *centres[i]) for i in range(S)]
    t = transforms(rng, S)
    total_dev, total_wall, xf_dev, fused = [], [], [], []
    g.global_enable(S * N)
    for rep in range(args.reps + 1):
        for cen, acc in ((far, xf_dev), (centres, total_dev)):
            g.global_enable(S * N)
            for c in clouds:
                g.global_push(c)
            torch.cuda.synchronize()
            f, d, w = timed(lambda: g.global_loop_closure(t, cen, 25.0, res))
            if rep:                                               # rep 0 allocates the step buffers
                acc.append(d)
                if cen is centres:
                    total_wall.append(w); fused.append(f)
    exported = g.global_export(-1).size

    # -- the CPU restatement on a smaller stack (ring of cpu_submaps, same spacing)
    Sc, Nc = args.cpu_submaps, args.cpu_records
    cc = np.array([[10.0 * i, 0.0] for i in range(Sc)], F32)
    rng = np.random.default_rng(5)
    stack = [submap(rng, Nc, *cc[i]) for i in range(Sc)]
    tc = transforms(rng, Sc)
    cpu_steps = sum(len(global_ref.neighbours(cc, Sc, i, 25.0)) - 1 for i in range(Sc) if len(global_ref.neighbours(cc, Sc, i, 25.0)) > 2)
    t0 = time.perf_counter()
    global_ref.loop_closure(stack, Sc, tc, cc, 25.0, res)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    gc = ElevationMap(32, res)
    gc.set_stream(stream.cuda_stream)
    dev_small = []
    for rep in range(args.reps + 1):
        gc.global_enable(Sc * Nc)
        rng = np.random.default_rng(5)
        for i in range(Sc):
            gc.global_push(submap(rng, Nc, *cc[i]))
        torch.cuda.synchronize()
        _, d, _ = timed(lambda: gc.global_loop_closure(tc, cc, 25.0, res))
        if rep:
            dev_small.append(d)

    med = lambda v: round(float(np.median(v)), 3) if v else None
    tot, xf = med(total_dev), med(xf_dev)
    line = {"bench": "global_map",
            "push_local": {"L": L, "resolution": res, "pushes": len(push_dev), "local_entries_median": int(np.median(push_n)),
                           "submap_records_median": push_records, "device_ms": med(push_dev), "wall_ms": med(push_wall)},
            "loop_closure": {"submaps": S, "records_per_submap": N, "spacing_m": 10.0, "radius_m": 25.0, "pair_steps": steps,
                             "fused": int(fused[0]) if fused else 0, "records_after": int(exported),
                             "device_ms": tot, "wall_ms": med(total_wall), "transforms_only_device_ms": xf,
                             "per_pair_step_device_ms": round((tot - xf) / steps, 3) if steps else None},
            "cpu_restatement": {"what": "tests/global_ref.py (numpy + dicts), not the node", "submaps": Sc, "records_per_submap": Nc,
                                "pair_steps": cpu_steps, "ms": round(cpu_ms, 1), "device_ms_same_stack": med(dev_small)},
            "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
