#!/usr/bin/env python3
"""A C3 frame as a cloud and as a depth image, one MI355X: prints ONE JSON line.

    python tools/bench_depth.py [--frames N] [--warmup W] [--out FILE]

C3 geometry (400 x 400 cells at 0.025 m, 640 x 480 pixels, the structured-light model with the d435 cutoffs: PASSTHROUGH_Z), the same
data in two shapes:
  (a) add_raw     gem_add_raw of the organised host cloud + packed rgb (20 B a pixel over the link) -- the parent's best path
  (b) add_depth   gem_add_depth of the host uint16 image + BGR8 image (5 B a pixel), unprojected and masked on the device
and the two device forms (gem_add_raw_device, gem_add_depth_device).  One process, a map per form, all reserved beforehand.  After
the warm-up the forms ALTERNATE frame by frame -- a, b, a, b, ... -- so that drift of the machine hits both alike; a form's clock is
the host clock around each of its N frames, call to the end of gem_synchronize, summed.  Three repeats; the spread of (a) over
them is the noise (b) is judged against.  "streamed" is the other way to run a form: N calls back to back and one gem_synchronize,
where consecutive frames' staging, link and kernels overlap.  After the timed frames every layer of (a) and (b) (and of the device
forms) must be bit-equal: the maps saw the same frames.  bench.py stays the contract line (C2).
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
import depth_ref  # noqa: E402
from gem_amd import ElevationMap, synth  # noqa: E402

LAYERS = ("elevation", "variance", "intensity", "traver", "lowest", "color_r", "color_g", "color_b", "rough", "slope")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", type=str, default=None, help="also append the line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depth.py needs a HIP device"
    N = max(args.frames, 1)
    wl = synth.config_c3(structured_light=True)
    f = wl.frames[0]
    img, depth, bgr = synth.depth_image_c3()
    n = img.width * img.height
    cloud, rgb = depth_ref.unproject(img, depth, bgr)
    d_cloud, d_rgb = torch.from_numpy(cloud).cuda(), torch.from_numpy(rgb.view(np.int32)).cuda()
    d_depth, d_bgr = torch.from_numpy(depth.view(np.int16)).cuda(), torch.from_numpy(bgr).cuda()
    forms = {
        "add_raw_host": lambda m: m.add_raw(f, cloud, rgb=rgb),
        "add_depth_host": lambda m: m.add_depth(f, img, depth, bgr),
        "add_raw_device": lambda m: m.add_raw(f, d_cloud, rgb=d_rgb),
        "add_depth_device": lambda m: m.add_depth(f, img, d_depth, d_bgr),
    }
    maps = {}
    for name in forms:
        m = maps[name] = ElevationMap(wl.length, wl.resolution)
        m.move(wl.map_position)
        m.reserve(n, 1, True)
    for _ in range(args.warmup):
        for name, fn in forms.items():
            fn(maps[name])
    for m in maps.values():
        m.synchronize()

    def alternate(pair):
        t = {name: 0.0 for name in pair}
        for _ in range(N):
            for name in pair:
                m, fn = maps[name], forms[name]
                t0 = time.perf_counter()
                fn(m)
                m.synchronize()
                t[name] += time.perf_counter() - t0
        return {name: 1e6 * v / N for name, v in t.items()}

    def streamed(name):
        m, fn = maps[name], forms[name]
        t0 = time.perf_counter()
        for _ in range(N):
            fn(m)
        m.synchronize()
        return 1e6 * (time.perf_counter() - t0) / N

    host = [alternate(("add_raw_host", "add_depth_host")) for _ in range(3)]
    dev = [alternate(("add_raw_device", "add_depth_device")) for _ in range(3)]
    stream = {name: [streamed(name) for _ in range(3)] for name in forms}
    med = lambda v: float(np.median(v))
    a = [r["add_raw_host"] for r in host]
    b = [r["add_depth_host"] for r in host]
    res = {"tool": "bench_depth", "device": torch.cuda.get_device_name(0), "frames": N, "pixels": n, "map": [wl.length, wl.resolution],
           "us_per_frame": {"add_raw_host": round(med(a), 2), "add_depth_host": round(med(b), 2),
                            "add_raw_device": round(med([r["add_raw_device"] for r in dev]), 2),
                            "add_depth_device": round(med([r["add_depth_device"] for r in dev]), 2)},
           "repeats_add_raw_host_us": [round(v, 2) for v in a], "repeats_add_depth_host_us": [round(v, 2) for v in b],
           "spread_add_raw_host_us": round(max(a) - min(a), 2),
           "streamed_us_per_frame": {name: round(med(v), 2) for name, v in stream.items()},
           "bytes_uploaded_per_frame": {"add_raw_host": int(cloud.nbytes + rgb.nbytes), "add_depth_host": int(depth.nbytes + bgr.nbytes)}}
    res["depth_not_slower_than_raw_by_more_than_spread"] = bool(med(b) <= med(a) + res["spread_add_raw_host_us"])
    # every map saw warmup + 3 N alternated + 3 N streamed identical frames
    same = lambda x, y: all(np.array_equal(maps[x].layer(k).view(np.uint32), maps[y].layer(k).view(np.uint32)) for k in LAYERS)
    res["maps_identical"] = {"host": same("add_raw_host", "add_depth_host"), "device": same("add_raw_device", "add_depth_device"),
                             "host_device": same("add_depth_host", "add_depth_device")}
    for m in maps.values():
        m.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")
    return 0 if all(res["maps_identical"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
