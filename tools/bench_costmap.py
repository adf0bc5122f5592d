#!/usr/bin/env python3
"""The costmap layers on the device (gem_costmap.hip), one MI355X: prints its rows and ONE JSON line.

    python tools/bench_costmap.py [--reps R] [--submaps S] [--records N]

  (a) grid_cloud   gem_costmap_mark_grid_cloud of a full 600 x 600 capture (C2 geometry, every cell kept) into a 75 x 75 costmap
                   at 0.2 m centred on the map
  (b) visual       gem_costmap_mark_visual of the same capture into the same costmap
  (c) global       gem_costmap_mark_global(-1) of S submaps of N records (0.05 m cells drawn from 40 m squares, centres 10 m apart
                   around a loop) into a 1000 x 1000 costmap at 0.2 m
  device_us        hipEvents on the handle's stream around each call (bounds NULL: the call only enqueues), median of R
  with_bounds_us   wall time of the call with bounds, which waits for them
  baselines        what the path without these entries needs for the same costmap: the download alone (gem_local_grid_cloud for
                   (a), gem_global_export(-1) for (c); wall time, they are synchronous), and a single-thread host loop over the
                   downloaded records -- the restated PointMapLayer::updateBounds body, compiled here with the host compiler

bench.py stays the contract line (C2); the kernels' own times come from rocprofv3 --kernel-trace --stats.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402
from gem_amd import POINT_DTYPE, ElevationMap  # noqa: E402

F32 = np.float32

HOST_LOOP = r"""
#include <math.h>
#include <string.h>
typedef struct { float x, y, z, pad; unsigned bgra; float covariance, intensity, travers; } rec;
/* PointMapLayer::updateBounds' loop with Costmap2D::worldToMap and touch(), as include/gem_hip.h restates them */
void host_mark(const rec* p, long long n, unsigned char* grid, unsigned sx, unsigned sy, double res, double ox, double oy,
               double thresh, double* b)
{
    for (long long i = 0; i < n; ++i) {
        const double px = p[i].x, py = p[i].y;
        if (!(fabs(px) <= 1.7976931348623157e308 && fabs(py) <= 1.7976931348623157e308)) continue;
        if (px < ox || py < oy) continue;
        const double qx = (px - ox) / res, qy = (py - oy) / res;
        if (!(qx < 2147483648.0 && qy < 2147483648.0)) continue;
        const unsigned mx = (unsigned)(int)qx, my = (unsigned)(int)qy;
        if (!(mx < sx && my < sy)) continue;
        grid[(size_t)my * sx + mx] = ((double)p[i].travers > thresh) ? 0 : 254;
        b[0] = b[0] < px ? b[0] : px; b[1] = b[1] < py ? b[1] : py;
        b[2] = px < b[2] ? b[2] : px; b[3] = py < b[3] ? b[3] : py;
    }
}
"""


def host_loop():
    td = tempfile.mkdtemp(prefix="bench_costmap_")
    src, lib = Path(td) / "host_mark.c", Path(td) / "libhost_mark.so"
    src.write_text(HOST_LOOP)
    subprocess.run(["cc", "-O2", "-shared", "-fPIC", str(src), "-o", str(lib), "-lm"], check=True)
    fn = C.CDLL(str(lib)).host_mark
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_uint, C.c_uint, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]

    def run(records, sx, sy, res, ox, oy, thresh):
        grid = np.full((sy, sx), 255, np.uint8)
        b = np.array([1e30, 1e30, -1e30, -1e30])
        t0 = time.perf_counter()
        fn(records.ctypes.data_as(C.c_void_p), records.shape[0], grid.ctypes.data_as(C.c_void_p), sx, sy, res, ox, oy, thresh,
           b.ctypes.data_as(C.c_void_p))
        return (time.perf_counter() - t0) * 1e6, grid
    return run


def submap(rng, n, cx, cy, res=0.05, side=40.0):
    cells = int(side / res)
    pick = rng.choice(cells * cells, n, replace=False)
    ix, iy = pick % cells, pick // cells
    cx, cy = round(cx / res) * res, round(cy / res) * res
    out = np.zeros(n, POINT_DTYPE)
    out["x"] = (cx + (ix - cells / 2 + 0.5) * res).astype(F32)
    out["y"] = (cy + (iy - cells / 2 + 0.5) * res).astype(F32)
    out["pad"] = 1.0
    out["travers"] = rng.uniform(0, 1, n).astype(F32)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--baseline-reps", type=int, default=10)
    ap.add_argument("--submaps", type=int, default=20)
    ap.add_argument("--records", type=int, default=300_000)
    ap.add_argument("--only", default="abc", help="shapes to run (a profile of one shape: --only c --reps 1 --warmup 0)")
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    mark_host = host_loop()
    med = lambda v: round(float(np.median(v)), 2)

    def device_us(fn):
        """median device time of fn (which only enqueues) between two events on the handle's stream"""
        for _ in range(args.warmup):
            fn()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for a, b in evs:
            a.record(stream); fn(); b.record(stream)
        torch.cuda.synchronize()
        return med([a.elapsed_time(b) * 1e3 for a, b in evs])

    def wall_us(fn, reps):
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); fn(); out.append((time.perf_counter() - t0) * 1e6)
        return med(out)

    rows = {}
    if "a" in args.only or "b" in args.only:
        L, res = 600, 0.05
        m = ElevationMap(L, res)
        m.set_stream(stream.cuda_stream)
        rng = np.random.default_rng(7)
        m.set_layer("elevation", rng.uniform(-0.3, 0.3, (L, L)).astype(F32))
        m.set_layer("traver", rng.uniform(0.0, 1.0, (L, L)).astype(F32))
        m.local_enable(1 << 16)
        m.local_capture()
        cm = m.costmap(75, 75, 0.2)
        cm.roll_to(0.0, 0.0)
        g = cm.geometry()
        cloud = m.local_grid_cloud()
        host_us, host_grid = zip(*[mark_host(cloud, 75, 75, 0.2, g["origin_x"], g["origin_y"], 0.5) for _ in range(args.baseline_reps)])
        if "a" in args.only:
            cm.reset(); cm.mark_grid_cloud(0.5, [1e30, 1e30, -1e30, -1e30])
            assert cm.read().tobytes() == host_grid[0].tobytes(), "device and host loop disagree"
            rows["a_grid_cloud"] = {"records": int(cloud.size), "costmap": "75x75@0.2",
                                    "device_us": device_us(lambda: cm.mark_grid_cloud(0.5)),
                                    "with_bounds_us": wall_us(lambda: cm.mark_grid_cloud(0.5, [1e30, 1e30, -1e30, -1e30]), args.baseline_reps),
                                    "baseline_download_us": wall_us(m.local_grid_cloud, args.baseline_reps),
                                    "baseline_host_loop_us": med(host_us)}
        if "b" in args.only:
            rows["b_visual"] = {"cells": L * L, "costmap": "75x75@0.2",
                                "device_us": device_us(lambda: cm.mark_visual(0.5)),
                                "with_bounds_us": wall_us(lambda: cm.mark_visual(0.5, [1e30, 1e30, -1e30, -1e30]), args.baseline_reps)}
        cm.close()
        m.close()
    if "c" in args.only:
        S, N = args.submaps, args.records
        gmap = ElevationMap(32, 0.05)
        gmap.set_stream(stream.cuda_stream)
        gmap.global_enable(S * N)
        r = S * 10.0 / (2 * math.pi)
        rng = np.random.default_rng(3)
        for i in range(S):
            gmap.global_push(submap(rng, N, r * math.cos(2 * math.pi * i / S), r * math.sin(2 * math.pi * i / S)))
        cm = gmap.costmap(1000, 1000, 0.2)
        cm.roll_to(0.0, 0.0)
        g = cm.geometry()
        cloud = gmap.global_export(-1)
        host_us, host_grid = zip(*[mark_host(cloud, 1000, 1000, 0.2, g["origin_x"], g["origin_y"], 0.5) for _ in range(args.baseline_reps)])
        cm.mark_global(-1, 0.5, [1e30, 1e30, -1e30, -1e30])
        assert cm.read().tobytes() == host_grid[0].tobytes(), "device and host loop disagree"
        rows["c_global"] = {"submaps": S, "records": int(cloud.size), "costmap": "1000x1000@0.2",
                            "device_us": device_us(lambda: cm.mark_global(-1, 0.5)),
                            "with_bounds_us": wall_us(lambda: cm.mark_global(-1, 0.5, [1e30, 1e30, -1e30, -1e30]), args.baseline_reps),
                            "baseline_download_us": wall_us(lambda: gmap.global_export(-1), max(args.baseline_reps // 3, 1)),
                            "baseline_host_loop_us": med(host_us)}
        cm.close()
        gmap.close()
    for k, v in rows.items():
        print(k, " ".join(f"{a}={b}" for a, b in v.items()))
    print(json.dumps({"bench": "costmap", "reps": args.reps, "device": torch.cuda.get_device_name(0), **rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
