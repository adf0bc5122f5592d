"""Timing of gem_costmap_observe_device (ObstacleLayer::updateBounds on the device costmap) against what a caller of the library
without it must do: gem_costmap_read of the layer, the layer on the CPU -- the host twin gem_obstacle_host, plain C++ inside
libgem_hip.so, stands for it -- and gem_costmap_write of the result.  Needs a GPU; prints a table and, with --out, writes it to a file
as well.

The cloud is the C2 sweep (gem_amd.synth.config_c2: 64 x 2048 = 131 072 returns of a spinning LiDAR 1.73 m above flat ground, ranges up
to 80 m) in the map frame, as 16-byte xyzi records; one observation, marking and clearing, the sensor at the sweep's origin, the
buffer's window [-0.5, 2] (the ground's returns count), the layer's maximum 2.  Workloads, each centred on the sensor:
  local 75x75 @ 0.2      the reference's local costmap (layers/params/local_costmap_params.yaml), ranges 2.5 / 3.0 m
  600x600 @ 0.05         ranges 8 / 10 m
  global 1000x1000 @ 0.2 the reference's global costmap, ranges 2.5 / 3.0 m
Rows, host clock (time.perf_counter) around work that ends in a device synchronise, alternated round by round (--rounds) after
--warmup rounds; each reports its median and the min .. max of its rounds:
  device_cells     gem_costmap_observe_device with "obstacle_direct" 0: one walk per distinct end cell
  device_direct    ... with "obstacle_direct" 1: one walk per accepted record
  host_baseline    gem_costmap_read + gem_obstacle_host + gem_costmap_write
  reads_only       gem_costmap_read + gem_costmap_write: a lower bound of the baseline whatever the CPU layer costs
Before timing, both device forms are compared with the host twin byte for byte (grid) and value for value (bounds), and the number of
accepted rays and of distinct end cells is counted from the host twin's arithmetic (tests/obstacle_ref.py).
--kernels N runs N device calls of either form per workload and nothing else: the run to put under rocprofv3 --kernel-trace --stats."""
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
from gem_amd import ElevationMap, synth  # noqa: E402

EMPTY = [1e30, 1e30, -1e30, -1e30]
WORKLOADS = [("local 75x75 @ 0.2", 75, 0.2, 2.5, 3.0), ("600x600 @ 0.05", 600, 0.05, 8.0, 10.0), ("global 1000x1000 @ 0.2", 1000, 0.2, 2.5, 3.0)]


def c2_cloud():
    """the C2 sweep in the map frame: float32 [131072, 4] xyzi, and the sensor's position"""
    w = synth.config_c2()
    T = synth.pose_matrix(**synth.C2_POSE)
    p = w.clouds[0].astype(np.float64)
    xyz = p[:, :3] @ T[:3, :3].T + T[:3, 3]
    return np.ascontiguousarray(np.concatenate([xyz, p[:, 3:4]], 1).astype(np.float32)), tuple(float(v) for v in T[:3, 3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_obstacle.py needs a GPU")
    import costmap_ref as cref
    import obstacle_ref as ref
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    cloud, at = c2_cloud()
    d_cloud = torch.from_numpy(cloud).to("cuda:0")
    m = ElevationMap(32, 0.1)
    rng = np.random.default_rng(7)
    say(f"bench_obstacle: the C2 sweep, {cloud.shape[0]} records of 16 bytes, sensor at {at}; window [-0.5, 2], layer maximum 2; "
        f"rounds {args.rounds} (alternated), warmup {args.warmup}")
    for name, n, res, obstacle_range, raytrace_range in WORKLOADS:
        origin = (at[0] - 0.5 * n * res, at[1] - 0.5 * n * res)
        grid0 = rng.integers(0, 256, (n, n), dtype=np.uint8)
        o = {"origin": at, "obstacle_range": obstacle_range, "raytrace_range": raytrace_range, "min_obstacle_height": -0.5, "max_obstacle_height": 2.0}
        o_host, o_dev = {**o, "points": cloud}, {**o, "points": d_cloud}
        cm = m.costmap(n, n, res, *origin)

        def device(direct, bounds=None):
            m.debug_set("obstacle_direct", direct)
            return cm.observe([o_dev], 2.0, bounds)

        if args.kernels:
            cm.write(grid0)
            for direct in (0, 1):
                for _ in range(args.kernels):
                    device(direct)
                m.synchronize()
            cm.close()
            continue

        # parity before timing
        want = grid0.copy()
        want_b = gem_amd.obstacle_host(want, res, origin, [o_host], 2.0, list(EMPTY))
        for direct in (0, 1):
            cm.write(grid0)
            assert device(direct, list(EMPTY)) == want_b and cm.read().tobytes() == want.tobytes(), (name, direct)
        shadow = cref.Costmap(n, n, res, *origin)
        c = ref.clear_records(shadow, o_host)
        rays = int(c["ok"].sum())
        ends = int(np.unique((c["y1"] * n + c["x1"])[c["ok"]]).size)
        marks = int(ref.mark_records(shadow, o_host, 2.0)["ok"].sum())
        cleared, lethal = int(((want == 0) & (grid0 != 0)).sum()), int(((want == 254) & (grid0 != 254)).sum())

        rows = ("device_cells", "device_direct", "host_baseline", "reads_only")
        times = {r: [] for r in rows}
        host_grid = np.zeros((n, n), np.uint8)

        def run(row):
            m.synchronize()
            t = time.perf_counter()
            if row == "device_cells":
                device(0)
                m.synchronize()
            elif row == "device_direct":
                device(1)
                m.synchronize()
            else:
                cm._call("gem_costmap_read", 0, 0, n, n, host_grid.ctypes.data_as(C.c_void_p), n)
                if row == "host_baseline":
                    gem_amd.obstacle_host(host_grid, res, origin, [o_host], 2.0)
                cm._call("gem_costmap_write", 0, 0, n, n, host_grid.ctypes.data_as(C.c_void_p), n)
                m.synchronize()
            return time.perf_counter() - t

        for r in range(args.warmup + args.rounds):
            for row in rows:
                dt = run(row)
                if r >= args.warmup:
                    times[row].append(dt * 1e6)
        m.debug_set("obstacle_direct", 1)
        say(f"{name}, ranges {obstacle_range} / {raytrace_range} m: {rays} accepted rays onto {ends} distinct end cells "
            f"({rays / max(ends, 1):.0f} records per end cell), {marks} marking records; {cleared} cells cleared and {lethal} made lethal on a "
            f"random grid; both device forms equal to the host twin byte for byte")
        say(f"  {'row':<16} {'median us':>11} {'min us':>11} {'max us':>11}   rounds")
        med = {}
        for row, v in times.items():
            v = np.array(v)
            med[row] = float(np.median(v))
            say(f"  {row:<16} {np.median(v):>11.1f} {v.min():>11.1f} {v.max():>11.1f}   {v.size}")
        best = min(med["device_cells"], med["device_direct"])
        say(f"  the end-cell form costs {'less' if med['device_cells'] < med['device_direct'] else 'NOT less'} than the direct form; the device "
            f"call costs {'less' if best < med['host_baseline'] else 'NOT less'} than the baseline ({best:.1f} us against {med['host_baseline']:.1f} us) and "
            f"{'less' if best < med['reads_only'] else 'NOT less'} than the read and the write alone ({med['reads_only']:.1f} us)")
        cm.close()
    m.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
