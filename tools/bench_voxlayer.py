"""Timing of gem_costmap_voxel_observe_device (VoxelLayer::updateBounds on the device costmap) against what a caller of the library
without it must do: gem_costmap_read and gem_costmap_voxels_read of the layer, the layer on the CPU -- the host twin gem_voxlayer_host,
plain C++ inside libgem_hip.so, stands for it -- and gem_costmap_write and gem_costmap_voxels_write of the result; and against
gem_costmap_observe_device on the same input, the 2-D layer: the difference is the price of the third axis.  Needs a GPU; prints a table
and, with --out, writes it to a file as well.

The cloud is the C2 sweep (gem_amd.synth.config_c2: 64 x 2048 = 131 072 returns of a spinning LiDAR 1.73 m above flat ground, ranges up
to 80 m) in the map frame, as 16-byte xyzi records; one observation, marking and clearing, the sensor at the sweep's origin, the
buffer's window [-0.5, 2] (the ground's returns count), the layer's maximum 2; ten voxels of 0.2 m from z = 0, thresholds (15, 0).
Workloads, each centred on the sensor:
  local 75x75 @ 0.2      the reference's local costmap (layers/params/local_costmap_params.yaml), ranges 2.5 / 3.0 m
  600x600 @ 0.05         ranges 8 / 10 m
  global 1000x1000 @ 0.2 the reference's global costmap, ranges 2.5 / 3.0 m
Rows, host clock (time.perf_counter) around work that ends in a device synchronise, alternated round by round (--rounds) after
--warmup rounds; each reports its median and the min .. max of its rounds:
  device_voxel     gem_costmap_voxel_observe_device on the state the call before left (the steady state of a stream of sweeps)
  device_fresh     ... on unknown columns: every voxel on a ray still has a bit to clear, no atomic is skipped
  device_2d        gem_costmap_observe_device, the 2-D layer, on the same bytes
  host_baseline    read bytes and columns + gem_voxlayer_host + write both
  reads_only       read and write of bytes and columns: a lower bound of the baseline whatever the CPU layer costs
device_fresh includes the launch that resets the columns; reset_only times that launch alone.
Before timing, the device call is compared with the host twin byte for byte (grid, columns) and value for value (bounds).
--kernels N runs N device calls per workload and nothing else: the run to put under rocprofv3 --kernel-trace --stats."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import gem_amd  # noqa: E402
from gem_amd import ElevationMap  # noqa: E402
from bench_obstacle import EMPTY, WORKLOADS, c2_cloud  # noqa: E402

VOXELS = (10, 0.2, 0.0, 15, 0)
UNKNOWN = 0x0000FFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_voxlayer.py needs a GPU")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    cloud, at = c2_cloud()
    d_cloud = torch.from_numpy(cloud).to("cuda:0")
    m = ElevationMap(32, 0.1)
    rng = np.random.default_rng(7)
    say(f"bench_voxlayer: the C2 sweep, {cloud.shape[0]} records of 16 bytes, sensor at {at}; window [-0.5, 2], layer maximum 2; voxels "
        f"{VOXELS}; rounds {args.rounds} (alternated), warmup {args.warmup}")
    for name, n, res, obstacle_range, raytrace_range in WORKLOADS:
        origin = (at[0] - 0.5 * n * res, at[1] - 0.5 * n * res)
        grid0 = rng.integers(0, 256, (n, n), dtype=np.uint8)
        cols0 = np.full((n, n), UNKNOWN, np.uint32)
        o = {"origin": at, "obstacle_range": obstacle_range, "raytrace_range": raytrace_range, "min_obstacle_height": -0.5, "max_obstacle_height": 2.0}
        o_host, o_dev = {**o, "points": cloud}, {**o, "points": d_cloud}
        cm, flat = m.costmap(n, n, res, *origin), m.costmap(n, n, res, *origin)
        cm.attach_voxels(*VOXELS)

        if args.kernels:
            cm.write(grid0)
            for _ in range(args.kernels):
                cm.voxel_observe([o_dev], 2.0)
            m.synchronize()
            cm.close(); flat.close()
            continue

        # parity before timing: a first call on unknown columns, a second on what it left
        want, want_cols = grid0.copy(), cols0.copy()
        cm.write(grid0)
        for call in range(2):
            want_b = gem_amd.voxlayer_host(want, want_cols, res, origin, VOXELS, [o_host], 2.0, list(EMPTY))
            assert cm.voxel_observe([o_dev], 2.0, list(EMPTY)) == want_b, (name, call)
            assert cm.read().tobytes() == want.tobytes() and cm.read_voxels().tobytes() == want_cols.tobytes(), (name, call)
        freed, unknown, lethal = int(((want == 0) & (grid0 != 0)).sum()), int(((want == 255) & (grid0 != 255)).sum()), int(((want == 254) & (grid0 != 254)).sum())
        changed = int((want_cols != cols0).sum())
        flat.write(grid0)

        rows = ("device_voxel", "device_fresh", "reset_only", "device_2d", "host_baseline", "reads_only")
        times = {r: [] for r in rows}
        host_grid, host_cols = np.zeros((n, n), np.uint8), np.zeros((n, n), np.uint32)

        def run(row):
            m.synchronize()
            t = time.perf_counter()
            if row == "device_voxel":
                cm.voxel_observe([o_dev], 2.0)
            elif row == "device_fresh":
                cm.reset()
                cm.voxel_observe([o_dev], 2.0)
            elif row == "reset_only":
                cm.reset()
            elif row == "device_2d":
                flat.observe([o_dev], 2.0)
            else:
                cm._call("gem_costmap_read", 0, 0, n, n, host_grid.ctypes.data_as(C.c_void_p), n)
                cm._call("gem_costmap_voxels_read", 0, 0, n, n, host_cols.ctypes.data_as(C.c_void_p), n)
                if row == "host_baseline":
                    gem_amd.voxlayer_host(host_grid, host_cols, res, origin, VOXELS, [o_host], 2.0)
                cm._call("gem_costmap_write", 0, 0, n, n, host_grid.ctypes.data_as(C.c_void_p), n)
                cm._call("gem_costmap_voxels_write", 0, 0, n, n, host_cols.ctypes.data_as(C.c_void_p), n)
            m.synchronize()
            return time.perf_counter() - t

        for r in range(args.warmup + args.rounds):
            for row in rows:
                if row == "device_voxel":                                 # the steady state: the call before it was an observe, not a reset
                    cm.voxel_observe([o_dev], 2.0)
                dt = run(row)
                if r >= args.warmup:
                    times[row].append(dt * 1e6)
        say(f"{name}, ranges {obstacle_range} / {raytrace_range} m: {changed} columns changed by the first call, {freed} cells freed, {unknown} "
            f"made unknown and {lethal} made lethal on a random grid; the device call "
            f"equal to the host twin byte for byte, bytes and columns, twice")
        say(f"  {'row':<16} {'median us':>11} {'min us':>11} {'max us':>11}   rounds")
        med = {}
        for row, v in times.items():
            v = np.array(v)
            med[row] = float(np.median(v))
            say(f"  {row:<16} {np.median(v):>11.1f} {v.min():>11.1f} {v.max():>11.1f}   {v.size}")
        fresh = med["device_fresh"] - med["reset_only"]
        say(f"  the device call costs {'less' if med['device_voxel'] < med['host_baseline'] else 'NOT less'} than the baseline "
            f"({med['device_voxel']:.1f} us against {med['host_baseline']:.1f} us) and {'less' if med['device_voxel'] < med['reads_only'] else 'NOT less'} than "
            f"the reads and writes alone ({med['reads_only']:.1f} us); on unknown columns about {fresh:.1f} us; the third axis costs "
            f"{med['device_voxel'] - med['device_2d']:+.1f} us over the 2-D layer ({med['device_2d']:.1f} us)")
        cm.close(); flat.close()
    m.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
