#!/usr/bin/env python3
"""Randomised node-cycle soak on the GPU box: the device local map (gem_local_*) and submap stack (gem_global_*) driven in the node's
order every frame -- move -> add -> map_feature -> capture -> spill -> raytracing (with lowest tracking) -> keep_previous, a
push_local every few frames, sometimes a loop closure -- with random map sizes (1025 and above included), resolutions, starting
capacities, trajectories (all eight shift signs, sub-resolution shifts the gate skips, half-map jumps, returns, offsets far from the
origin), front ends (host / device add, add_raw, add_voxel, add_batch) and pipeline knobs (tools/fuzz_parity.py's KNOBS,
defer_walk, walk_always_wait).  Every
map layer against the CPU oracle, everything gem_local_* / gem_global_* return against tests/local_ref.py / tests/global_ref.py
(their array forms), bit for bit (test infrastructure: this tool is a test, not the product).

    python tools/fuzz_node.py [--seconds 120] [--seed 1]
Prints one line per scenario and a final summary; exit code 1 on the first mismatch (the scenario's seed is printed).
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "oracle", ROOT / "tests", ROOT / "tools"):
    sys.path.insert(0, str(p))
import torch  # noqa: E402
import oracle  # noqa: E402
from gem_amd import ElevationMap, SensorModel, VoxelStage, synth  # noqa: E402
import clean_ref  # noqa: E402
import global_ref  # noqa: E402
import local_ref  # noqa: E402
import voxel_ref  # noqa: E402
from fuzz_parity import KNOBS  # noqa: E402

F32 = np.float32
HEADINGS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
FRONT_ENDS = ["add host", "add device", "add_raw host", "add_raw device", "add_voxel host", "add_voxel device", "add_batch device",
              "add_batch host"]


def check(ok, what):
    if not ok:
        raise AssertionError(what)


class Node:
    """the device map and the oracle in lockstep, with the local map and the submap stack restated"""

    def __init__(self, rng, L, res, knobs, local_cap, global_cap, explicit, lowest):
        self.rng, self.L, self.res, self.explicit, self.lowest = rng, L, res, explicit, lowest
        self.gpu, self.ora = ElevationMap(L, res, debug=knobs), oracle.OracleMap(L, res)
        if lowest:
            self.gpu.set_lowest_tracking(True)
            self.gpu.set_layer("lowest", self.ora.layer("lowest"))
        self.gpu.local_enable(local_cap)
        self.gpu.global_enable(global_cap)
        self.local, self.stack, self.centres = local_ref.LocalMap(), [], []
        self.cap = self.prev = None
        self.center = np.zeros(2, F32)
        self.spilled = self.fused = 0

    def move(self, xy, what):
        g = self.gpu.move([xy[0], xy[1], 0.5]); o = self.ora.move([xy[0], xy[1], 0.5])
        check(np.array_equal(g[0], np.asarray(o[0], F32)) and tuple(g[1]) == tuple(o[1]), f"{what}: move {g} != {o}")
        shift = (np.asarray(g[0], F32) - self.center).astype(F32)
        self.center = np.asarray(g[0], F32)
        return shift

    def add(self, k, xy):
        rng, L, res = self.rng, self.L, self.res
        how = FRONT_ENDS[int(rng.integers(len(FRONT_ENDS)))]
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        n = int(rng.choice([200, 5000, 30000, 131072, 200000]))
        sweeps = int(rng.integers(1, 4)) if how.startswith("add_batch") else 1
        frames, clouds = [], []
        for s in range(sweeps):
            c = synth.random_cloud(int(rng.integers(1 << 30)), n, 0.4 * L * res, z_sigma=float(rng.uniform(0.02, 0.3)),
                                   dup_fraction=float(rng.uniform(0, 0.5)))
            T = synth.pose_matrix(xy[0] + float(rng.normal(0, 0.1)), xy[1] + float(rng.normal(0, 0.1)), 0.5, float(rng.uniform(-3, 3)))
            frames.append(synth._frame_for(T, SensorModel.velodyne())); clouds.append(c)
        f, c = frames[0], clouds[0]
        rgb = None
        if how.startswith(("add ", "add_raw", "add_voxel")) and rng.random() < 0.4:
            rgb = ((rng.integers(0, 3, c.shape[0]).astype(np.uint32) * 100) << 16) | (rng.integers(0, 256, c.shape[0]).astype(np.uint32) << 8)
        dv_rgb = None if rgb is None else dev(rgb.view(np.int32))
        if how.startswith("add_batch"):
            incs = [float(rng.uniform(0, 1e-4)) for _ in range(sweeps)] if rng.random() < 0.6 else None
            if how == "add_batch host":
                self.gpu.add_batch_host(frames, clouds, incs)
            else:
                off = np.concatenate([[0], np.cumsum([a.shape[0] for a in clouds])])
                self.gpu.add_batch(frames, dev(np.concatenate(clouds)), off, incs)
            for s in range(sweeps):
                if incs:
                    self.ora.mapvar_update(incs[s])
                self.ora.add(frames[s], clouds[s])
        elif how.startswith("add_raw"):
            raw = c.copy()
            holes = rng.random(raw.shape[0]) < 0.1
            raw[holes, int(rng.integers(3))] = np.nan
            self.gpu.add_raw(f, dev(raw) if how.endswith("device") else raw, rgb=dv_rgb if how.endswith("device") else rgb)
            cp = f.model.clean_params()
            kx, kc, kept = clean_ref.clean(raw, rgb, cp.mode, cp.z_min, cp.z_max)
            self.ora.add(f, kx, rgb=kc, orig_index=kept)
        elif how.startswith("add_voxel"):
            stages = VoxelStage.filter_launch()
            self.gpu.add_voxel(f, stages, dev(c) if how.endswith("device") else c, rgb=dv_rgb if how.endswith("device") else rgb)
            fx, fc, m = voxel_ref.voxel(c, rgb, stages)
            self.ora.add(f, fx[:m], rgb=None if fc is None else fc[:m])
        else:
            if how.endswith("device"):
                self.gpu.add(f, dev(c), dv_rgb)
            else:
                self.gpu.add(f, c, rgb)
            self.ora.add(f, c, rgb)
        return how, sum(a.shape[0] for a in clouds)

    def feature(self):
        o = self.ora.map_feature()
        self.gpu.map_feature(fetch=False)
        self.gpu.set_layer("traver", o["traver"])          # (rough / slope agree to a tolerance only; they are not in the records)
        return o

    def capture(self, feat, k, what):
        if self.explicit and k % 2:                          # visualMap_'s own geometry: doubles, an off-centre position
            length, res = self.L * self.res + 0.125 * (k % 3), self.res
            pos = (float(self.center[0]) + 0.013, float(self.center[1]) - 0.021)
            o = self.ora.show(feat["rough"], feat["slope"], map_length=length, resolution=res, position=pos)
            self.gpu.local_capture(length, res, pos)
        else:
            res = float(F32(self.res))
            length, pos = self.L * res, (float(self.center[0]), float(self.center[1]))
            o = self.ora.show(feat["rough"], feat["slope"])
            self.gpu.local_capture()
        self.cap = local_ref.capture(o, self.L, length, res, pos, self.ora.pose()[1])
        g = self.gpu.local_grid_cloud()
        check(g.tobytes() == self.cap.rec.tobytes(), f"{what}: grid cloud ({g.size} records, restatement {self.cap.rec.size})")

    def spill(self, shift, what):
        g, rg = self.gpu.local_spill(self.center, shift)
        o, ro = local_ref.spill_fast(self.prev, self.center, shift, self.local)
        check(g.tobytes() == o.tobytes(), f"{what}: spill of {g.size} records, restatement {o.size}")
        check(rg == ro, f"{what}: replaced {rg} != {ro}")
        check(self.gpu.local_size() == len(self.local), f"{what}: local_size {self.gpu.local_size()} != {len(self.local)}")
        self.spilled += g.size

    def gate(self, shift):
        return abs(float(shift[0])) >= self.res or abs(float(shift[1])) >= self.res

    def compare_layers(self, what):
        for name in ("elevation", "variance") + (("lowest",) if self.lowest else ()):
            g, o = self.gpu.layer(name), self.ora.layer(name)
            if not np.array_equal(g, o, equal_nan=True):
                bad = np.flatnonzero(g.ravel() != o.ravel())
                raise AssertionError(f"{what}: {name}: {bad.size} cells differ, first {bad[:5]}")

    def push_local(self, clear, what):
        i = self.gpu.global_push_local(clear)
        self.stack.append(np.concatenate([local_ref.export_fast(self.local), local_ref.grid_cloud(self.cap)]))
        check(i == len(self.stack) - 1, f"{what}: push_local index {i}")
        check(self.gpu.global_export(i).tobytes() == self.stack[i].tobytes(), f"{what}: pushed submap {i}")
        if clear:
            self.local.clear()
        self.centres.append([float(self.center[0]), float(self.center[1])])

    def loop_closure(self, what):
        rng, S = self.rng, len(self.stack)
        n_opt = max(0, S + int(rng.integers(-1, 3)))
        t = np.zeros((n_opt, 4, 4), F32)
        for s in range(n_opt):
            a = rng.uniform(-0.03, 0.03)
            t[s] = [[np.cos(a), -np.sin(a), 0, rng.uniform(-0.3, 0.3)], [np.sin(a), np.cos(a), 0, rng.uniform(-0.3, 0.3)],
                    [0, 0, 1, rng.uniform(-0.05, 0.05)], [0, 0, 0, 1]]
        c = np.array((self.centres + [self.centres[-1]] * n_opt)[:n_opt], F32).reshape(-1, 2) + rng.normal(0, 0.5, (n_opt, 2)).astype(F32)
        if n_opt > 2 and rng.random() < 0.3:
            c[1] = c[0]                                      # a coincident centre: the k == i step
        radius = float(rng.choice([3.0, 10.0, 25.0, 1e4]))
        resolution = float(rng.choice([0.0, self.res, 0.05]))
        fused = self.gpu.global_loop_closure(t, c, radius, resolution)
        want = global_ref.loop_closure(self.stack, n_opt, t, c, radius, resolution, map_resolution=self.res, fast=True)
        check(fused == want, f"{what}: loop closure fused {fused} != {want}")
        self.fused += fused
        self.check_stack(what)

    def check_stack(self, what):
        check(self.gpu.global_count() == len(self.stack), f"{what}: {self.gpu.global_count()} submaps != {len(self.stack)}")
        for i, s in enumerate(self.stack):
            check(global_ref.same(self.gpu.global_export(i), s), f"{what}: submap {i}")


def trajectory(rng, L, res, frames):
    """positions: steps of whole cells in all eight sign cases, sub-resolution shifts, half-map jumps and returns, around an origin
    that may lie far from (0, 0)"""
    origin = np.array([(0.0, 0.0), (137.3, -52.1), (-1.2e3, 8.4e2), (2.0e5, -1.5e5)][int(rng.integers(4))])
    p, out = origin.copy(), [origin.copy()]
    for _ in range(frames - 1):
        kind = rng.random()
        d = np.array(HEADINGS[int(rng.integers(8))], float)
        if kind < 0.15:
            p = p + rng.uniform(-0.45, 0.45, 2) * res
        elif kind < 0.75:
            p = p + d * res * (int(rng.integers(1, max(2, L // 6))) + float(rng.uniform(0, 0.9)))
        elif kind < 0.88:
            p = p + d * 0.5 * L * res
        else:
            p = out[int(rng.integers(len(out)))].copy()
        out.append(p.copy())
    return out


def scenario(seed, frames=None):
    rng = np.random.default_rng(seed)
    big = rng.random() < 0.12
    L = int(rng.choice([1025, 1100])) if big else int(rng.choice([24, 33, 48, 64, 101, 128, 200, 333]))
    res = float(rng.choice([0.05, 0.1, 0.2]))
    knobs = dict(KNOBS[int(rng.integers(len(KNOBS)))])
    if rng.random() < 0.5:
        knobs["overlap_min_points"] = 1
    knobs["defer_walk"] = int(rng.random() < 0.8)
    knobs.setdefault("walk_always_wait", int(rng.random() < 0.5))
    # ray tracing reads map_lowest, and a pass that maintains it launches its own walk: without lowest tracking the frame has no ray
    # tracing, and a sorted pass of device input leaves its walk to the next call (map_feature, or push_local before it)
    lowest = bool(rng.random() < 0.5)
    node = Node(rng, L, res, knobs, int(rng.choice([16, 256, 4096, 1 << 16])), int(rng.choice([16, 1 << 12, 1 << 20])),
                bool(rng.random() < 0.3), lowest)
    frames = frames or int(rng.integers(6, 10 if big else 24))
    push_every = int(rng.integers(2, 6))
    early_push = bool(rng.random() < 0.3)                      # push_local as the call right after the add, as well
    pts, fronts = 0, set()
    for k, xy in enumerate(trajectory(rng, L, res, frames)):
        what = f"seed {seed} frame {k} (L {L}, res {res}, knobs {knobs})"
        shift = node.move(xy, what)
        how, n = node.add(k, xy)
        pts += n; fronts.add(how)
        what += f" after {how}"
        if early_push and k and k % push_every == 0:
            node.push_local(bool(rng.random() < 0.5), what)
        feat = node.feature()
        node.capture(feat, k, what)
        if k == 0:
            node.gpu.local_keep_previous(); node.prev = node.cap        # the init frame: prevMap_ = map_.visualMap_
        if k and node.gate(shift):                                       # (the gate of EMg.cpp:715; not on the init frame)
            node.spill(shift, what)
        if lowest:
            node.gpu.raytracing(); node.ora.raytracing()
        node.compare_layers(what)
        node.gpu.local_keep_previous(); node.prev = node.cap
        if k % push_every == push_every - 1:
            node.push_local(bool(rng.random() < 0.8), what)
            if len(node.stack) >= 2 and rng.random() < 0.4:
                node.loop_closure(what)
    what = f"seed {seed} end (L {L}, knobs {knobs})"
    g = node.gpu.local_export()
    check(g.tobytes() == local_ref.export_fast(node.local).tobytes(), f"{what}: local export")
    if node.stack:
        node.loop_closure(what)
        check(global_ref.same(node.gpu.global_export(-1), global_ref.export_all(node.stack)), f"{what}: stack export")
    if knobs.get("walk_always_wait"):
        check(node.gpu.debug_get("walks_unwaited") == 0, f"{what}: a walk launched without its wait")
    summary = dict(L=L, res=res, lowest=int(lowest), frames=frames, points=pts, spilled=node.spilled, submaps=len(node.stack), fused=node.fused,
                   walks_left=node.gpu.debug_get("walks_left"), fronts=len(fronts), knobs=knobs)
    node.gpu.close()
    return summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    t0 = time.time(); n = 0; tot = dict(points=0, spilled=0, submaps=0, fused=0, walks_left=0); big = 0
    seed = a.seed * 100000
    while time.time() - t0 < a.seconds:
        try:
            s = scenario(seed)
        except AssertionError as e:
            print(f"MISMATCH in scenario seed {seed}: {e}", flush=True)
            return 1
        n += 1; big += s["L"] > 1024
        for key in tot:
            tot[key] += s[key]
        print(f"ok seed {seed} " + " ".join(f"{k} {v}" for k, v in s.items()), flush=True)
        seed += 1
    print(f"SUMMARY: {n} scenarios ({big} with L > 1024), {tot['points']} points, {tot['spilled']} records spilled, {tot['submaps']} submaps, "
          f"{tot['fused']} keys fused, {tot['walks_left']} walks left to the next call, {time.time() - t0:.0f} s, no mismatch", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
