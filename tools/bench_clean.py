#!/usr/bin/env python3
"""cleanPointCloud on the device (gem_clean.hip), one MI355X: prints ONE JSON line.

    python tools/bench_clean.py [--reps R]

  clean_device   gem_clean_device (count -> scan -> scatter) on a 640 x 480 organised cloud with ~25 % NaN pixels and on 4 194 304
                 points (~25 % NaN), inputs resident in HBM: microseconds per call (stream-synchronised loop of R calls) and algorithmic
                 GB/s, B_alg = 16 N read + 20 K written (kept XYZI + orig index) + 4 B count, against the 8 TB/s HBM peak
  add_raw        a structured-light frame shaped like C3 (the 640 x 480 depth image organised, NaN where no ray hit, d435 cutoffs
                 0.2 / 3.25 m): add_raw of the raw cloud against add of the same cloud cleaned beforehand (with its kept indices), host
                 arrays and device tensors, milliseconds per frame.  The maps of the two are checked to be bit-identical.
bench.py stays the contract line (C2); kernel times of the three compaction kernels (gem_compact.hpp over CleanSrc) come from
rocprofv3 --kernel-trace --stats.
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
import clean_ref  # noqa: E402
from gem_amd import ElevationMap, synth  # noqa: E402

HBM_PEAK_GBPS = 8000.0


def per_call(emap, fn, reps, warm=5):
    for _ in range(warm):
        fn()
    emap.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    emap.synchronize()
    return (time.perf_counter() - t0) / reps


def bench_clean_device(emap, xyzi, reps):
    d = torch.from_numpy(xyzi).cuda()
    p = synth.SensorModel.velodyne().clean_params()
    n = xyzi.shape[0]
    res = emap.clean_device(p, d)
    _, _, orig, count = res
    k = int(count.item())
    assert k == int(clean_ref.keep_mask(xyzi, p.mode).sum())
    assert np.array_equal(orig[:k].cpu().numpy(), np.flatnonzero(clean_ref.keep_mask(xyzi, p.mode)))
    s = per_call(emap, lambda: emap.clean_device(p, d, sync=False, out=res), reps)      # (outputs reused: no allocation in the loop)
    alg = 16 * n + 20 * k + 4
    return {"n": n, "kept": k, "us_per_call": round(1e6 * s, 2), "algorithmic_bytes": alg, "GBps": round(alg / s / 1e9, 1),
            "frac_of_hbm_peak": round(alg / s / 1e9 / HBM_PEAK_GBPS, 3)}


def bench_add_raw(reps):
    wl = synth.config_c3(structured_light=True)
    f = wl.frames[0]
    rng = np.random.default_rng(3)
    raw = np.full((640 * 480, 4), np.nan, np.float32)
    raw[:, 3] = rng.uniform(1, 255, raw.shape[0])
    raw[wl.orig_index] = wl.clouds[0]
    cp = f.model.clean_params()
    kx, _, kept = clean_ref.clean(raw, None, cp.mode, cp.z_min, cp.z_max)
    d_raw, d_kx, d_kept = torch.from_numpy(raw).cuda(), torch.from_numpy(kx).cuda(), torch.from_numpy(kept).cuda()
    out = {"raw_points": int(raw.shape[0]), "kept_points": int(kept.size), "cutoffs_m": [0.2, 3.25]}
    maps = []
    for name, fn in (("add_raw_host", lambda m: m.add_raw(f, raw)), ("add_cleaned_host", lambda m: m.add(f, kx, orig_index=kept)),
                     ("add_raw_device", lambda m: m.add_raw(f, d_raw)), ("add_cleaned_device", lambda m: m.add(f, d_kx, orig_index=d_kept))):
        m = ElevationMap(wl.length, wl.resolution)
        m.move(wl.map_position)
        m.reserve(raw.shape[0])
        out[f"ms_{name}"] = round(1e3 * per_call(m, lambda: fn(m), reps), 4)
        maps.append(m)
    # every map saw warm + reps identical frames: all four must agree bit for bit
    e0, v0 = maps[0].layer("elevation"), maps[0].layer("variance")
    out["maps_identical"] = all(np.array_equal(m.layer("elevation").view(np.uint32), e0.view(np.uint32)) and
                                np.array_equal(m.layer("variance").view(np.uint32), v0.view(np.uint32)) for m in maps[1:])
    for m in maps:
        m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_clean.py needs a HIP device"
    rng = np.random.default_rng(1)
    emap = ElevationMap(64, 0.1)
    res = {"tool": "bench_clean", "device": torch.cuda.get_device_name(0), "reps": args.reps}
    for label, n in (("vga_640x480", 640 * 480), ("n_4194304", 4_194_304)):
        c = rng.normal(0, 3, (n, 4)).astype(np.float32)
        c[rng.random(n) < 0.25, :3] = np.nan
        res[f"clean_device_{label}"] = bench_clean_device(emap, c, args.reps)
    emap.close()
    res["c3_structured_light"] = bench_add_raw(max(20, args.reps // 4))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
