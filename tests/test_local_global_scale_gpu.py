"""The device local map (gem_local_*) and submap stack (gem_global_*) at the sizes a node runs them at, and on the edges the CPU tests
pin only on the restatement, bit for bit against tests/local_ref.py / tests/global_ref.py (their array forms at node sizes):

  1. L = 1025 with every cell set: the capture, spill and export compactions over more than 2^20 items (two trips of compact_scan),
     from local_enable(16) (one spill grows the log past twice its capacity), a diagonal move and an axis move with dx == 0 exactly,
     the second spill compacting and growing a log of ~460 000 live entries and rebuilding the table;
  2. a back-and-forth trajectory: the log is compacted without growing, spills and export stay exact through it (export order after
     rewritten keys), and a second identical loop allocates nothing;
  3. the CPU-pinned edges on the device: two cells sharing one float key far from the origin within one spill, negative and NaN
     traversability, export order after a reinsert;
  4. submaps of 1.1-1.3 M records (k_global_keys past 2^20 records, compact_scan for two trips), one of a million records in 8 keys
     (atomicMin contention across every workgroup), one of 2^20 records each its own key (the table at its designed half load);
  5. neighbour lists with exact distance ties, a centre exactly at the radius, lists of 2 and 3 entries, coincident centres (the
     k == i step) and n_opt above the stack size;
  6. a sorted pass of device input leaving its walk to the next call, that call being gem_local_capture / gem_global_push_local,
     with walk_always_wait 0 and 1 (then no walk is launched without its stream wait)."""
import sys
from pathlib import Path

import numpy as np
import pytest

from gem_amd import ElevationMap, SensorModel, synth

sys.path.insert(0, str(Path(__file__).resolve().parent))
import global_ref  # noqa: E402
import local_ref  # noqa: E402
from test_global_map_gpu import check_stack, synthetic, transforms  # noqa: E402
from test_local_map_gpu import Pair  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
F32 = np.float32


class FastPair(Pair):
    """Pair with the local map restated on arrays (local_ref.LocalMap), and the spill's log arithmetic of gem_local_spill mirrored so
    that a test can state which host path a spill took"""

    def __init__(self, oracle_mod, L, res, capacity):
        super().__init__(oracle_mod, L, res, capacity)
        self.local = local_ref.LocalMap()
        self.log_len, self.log_cap = 0, capacity
        self.paths = []

    def spill(self, shift, frame):
        live = len(self.local)
        g, rg = self.gpu.local_spill(self.center, shift)
        o, ro = local_ref.spill_fast(self.prev, self.center, shift, self.local)
        assert g.size == o.size and g.tobytes() == o.tobytes(), f"frame {frame}: {g.size} spilled, restatement {o.size}"
        assert rg == ro, f"frame {frame}: replaced {rg} != {ro}"
        assert self.gpu.local_size() == len(self.local)
        n = g.size
        if self.log_len + n > self.log_cap:                             # the log is compacted first (gem_local_spill)
            need = live + n
            grow = need > self.log_cap // 2
            self.paths.append(("grow" if grow else "compact", need, self.log_cap, live))
            self.log_cap = max(2 * self.log_cap, 2 * need) if grow else self.log_cap
            self.log_len = live
        self.log_len += n
        return n

    def check_export(self, clear=False):
        g = self.gpu.local_export(clear)
        assert g.tobytes() == local_ref.export_fast(self.local).tobytes()
        if clear:
            self.local.clear()
            self.log_len = 0


def fill(p: Pair, rng, frac_special=0.01):
    """every cell set on both maps; a few with elevation -10 / traversability -10 (not captured), negative or NaN traversability
    (captured, never spilled)"""
    L = p.L
    t = rng.uniform(0, 1, (L, L)).astype(F32)
    e = rng.uniform(-1, 1, (L, L)).astype(F32)
    pick = rng.random((L, L))
    t[pick < frac_special] = F32(-0.5)
    t[(pick >= frac_special) & (pick < 2 * frac_special)] = np.nan
    t[(pick >= 2 * frac_special) & (pick < 2.2 * frac_special)] = F32(-10)
    e[(pick >= 2.2 * frac_special) & (pick < 2.4 * frac_special)] = F32(-10)
    layers = {"elevation": e, "traver": t, "variance": rng.uniform(1e-4, 1e-2, (L, L)).astype(F32),
              "intensity": rng.uniform(0, 100, (L, L)).astype(F32),
              "color_r": rng.integers(0, 256, (L, L)), "color_g": rng.integers(0, 256, (L, L)), "color_b": rng.integers(0, 256, (L, L))}
    for name, v in layers.items():
        p.gpu.set_layer(name, v); p.ref.set_layer(name, v)


def zero_feat(L):
    return {"rough": np.zeros((L, L), F32), "slope": np.zeros((L, L), F32)}


def test_local_map_past_2_20_items(oracle_mod):
    L, res = 1025, 0.1
    assert L * L > 1 << 20
    p = FastPair(oracle_mod, L, res, capacity=16)
    rng = np.random.default_rng(1025)
    W = L * res
    p.move((0.0, 0.0))
    fill(p, rng)
    p.capture(zero_feat(L))
    assert p.cap.rec.size > 0.95 * L * L
    p.keep_previous()
    # a diagonal move: ~44 % of the window spills into a log of capacity 16
    shift = p.move((0.3 * W, 0.2 * W))
    assert shift[0] > 0 and shift[1] > 0
    fill(p, rng)
    p.capture(zero_feat(L), 1)
    n1 = p.spill(shift, 1)
    assert n1 > 400_000 and p.paths[-1][0] == "grow" and p.paths[-1][1] > 2 * 16
    p.keep_previous()
    # an axis move with dx == 0 exactly: 70 % spills, more than the first spill, so the log of ~460 000 live entries is compacted,
    # grown by more than 2x (need > capacity) and the table rebuilt around it
    shift = p.move((float(p.center[0]), float(p.center[1]) + 0.7 * W))     # (the map's own x: a target x would snap to the grid)
    assert shift[0] == 0.0 and shift[1] > 0
    fill(p, rng)
    p.capture(zero_feat(L), 2)
    n2 = p.spill(shift, 2)
    assert n2 > n1 and p.paths[-1][0] == "grow" and p.paths[-1][1] > p.paths[-1][2] and p.paths[-1][3] > 400_000
    assert p.log_len > 1 << 20                                           # the export compacts more than 2^20 log entries
    p.check_export()
    p.keep_previous()
    # and back: a half-map jump onto the first spills' ground
    shift = p.move((-0.2 * W, 0.0))
    fill(p, rng)
    p.capture(zero_feat(L), 3)
    p.spill(shift, 3)
    p.check_export(clear=True)
    assert p.gpu.local_size() == 0


def test_back_and_forth_compacts_without_growing(oracle_mod):
    """returns to the same positions rewrite the same keys: the log fills with dead entries and is compacted in place (what is live
    plus the spill fits in half of it); the export after every spill is in last-write order"""
    L, res, cap = 64, 0.1, 4096
    p = FastPair(oracle_mod, L, res, capacity=cap)
    stops = [(0.0, 0.0), (0.3, 0.0), (0.0, 0.0), (0.3, 0.3), (0.0, 0.0), (0.0, -0.3), (0.0, 0.0), (-0.3, 0.3)]

    def loop(frames=60):
        p.gpu.local_enable(cap)
        p.local.clear()
        p.log_len, p.log_cap, p.paths = 0, cap, []
        p.move(stops[0])
        fill(p, np.random.default_rng(7), 0.02)
        p.capture(zero_feat(L))
        p.keep_previous()
        total = 0
        for k in range(1, frames):
            shift = p.move(stops[k % len(stops)])
            fill(p, np.random.default_rng(7 + k), 0.02)
            p.capture(zero_feat(L), k)
            if p.gate(shift):
                total += p.spill(shift, k)
                p.check_export()
            p.keep_previous()
        return total

    first = loop()
    a1 = p.gpu.debug_get("arena_allocations")
    assert [q[0] for q in p.paths].count("compact") >= 3 and "grow" not in [q[0] for q in p.paths], p.paths
    second = loop()
    a2 = p.gpu.debug_get("arena_allocations")
    assert first == second
    assert a2 == a1, (a1, a2)


def edge_pair(oracle_mod, traver=None, L=8, res=0.5):
    """tests/test_local_map_cpu.py's map (every cell valid, elevation = linear index / 8) on both sides"""
    gpu, ref = ElevationMap(L, res), oracle_mod.OracleMap(L, res)
    layers = {"elevation": np.arange(L * L, dtype=F32).reshape(L, L) / 8,
              "traver": np.full((L, L), 0.5, F32) if traver is None else traver,
              "color_r": np.full((L, L), 300), "color_g": np.full((L, L), 7), "color_b": np.full((L, L), 255)}
    for name, v in layers.items():
        gpu.set_layer(name, v); ref.set_layer(name, v)
    gpu.local_enable(16)
    return gpu, ref


def capture_at(gpu, ref, L, res, position):
    o = ref.show(position=position)
    gpu.local_capture(0.0, 0.0, position)                                 # the map's own length and resolution, as show() takes them
    cap = local_ref.capture(o, L, L * float(F32(res)), float(F32(res)), position, ref.pose()[1])
    assert gpu.local_grid_cloud().tobytes() == cap.rec.tobytes()
    gpu.local_keep_previous()
    return cap


def spill_both(gpu, cap, cur, shift, lm):
    g, rg = gpu.local_spill(cur, shift)
    o, ro = local_ref.spill_fast(cap, cur, shift, lm)
    assert g.tobytes() == o.tobytes() and rg == ro and gpu.local_size() == len(lm)
    assert gpu.local_export().tobytes() == local_ref.export_fast(lm).tobytes()
    return o, ro


def test_two_cells_one_float_key_far_from_origin(oracle_mod):
    """at x ~ 3e6 the float spacing is 0.25: cells 0.05 m apart round to one key within one spill; the later cell wins (atomicMax on
    the log position) and counts as replaced"""
    L, res, far = 8, 0.05, (3.0e6, 0.0)
    gpu, ref = edge_pair(oracle_mod, L=L, res=res)
    cap = capture_at(gpu, ref, L, res, far)
    lm = local_ref.LocalMap()
    out, replaced = spill_both(gpu, cap, (far[0] + 0.25, 0.0), (0.25, 0.0), lm)
    assert out.size == 40 and len(lm) == 16 and replaced == 24


def test_negative_and_nan_traversability_not_spilled(oracle_mod):
    L = 8
    t = np.full((L, L), 0.5, F32)
    t[7, 0], t[7, 1], t[7, 2], t[7, 3] = F32(-0.25), np.nan, F32(0.0), F32(-0.0)
    gpu, ref = edge_pair(oracle_mod, t)
    cap = capture_at(gpu, ref, L, 0.5, (0.0, 0.0))
    assert cap.rec.size == 63
    out, _ = spill_both(gpu, cap, (0.6, 0.0), (0.6, 0.0), local_ref.LocalMap())
    assert out.size == 6 and not np.any(out["travers"] < 0) and not np.any(np.isnan(out["travers"]))


def test_export_order_after_reinsert(oracle_mod):
    gpu, ref = edge_pair(oracle_mod)
    cap = capture_at(gpu, ref, 8, 0.5, (0.0, 0.0))
    lm = local_ref.LocalMap()
    spill_both(gpu, cap, (0.0, 0.6), (0.0, 0.6), lm)                       # row iy = 7
    _, replaced = spill_both(gpu, cap, (0.6, 0.0), (0.6, 0.0), lm)         # column ix = 7: (7, 7) rewritten, goes last
    assert replaced == 1 and len(lm) == 15


def dup_cloud(rng, n, cells=600, res=0.05):
    """n records over a cells x cells square of [0, cells * res)^2, ~n / cells^2 per cell, jittered inside the cell"""
    out = np.zeros(n, global_ref.POINT)
    out["x"] = ((rng.integers(0, cells, n) + rng.uniform(0.05, 0.95, n)) * res).astype(F32)
    out["y"] = ((rng.integers(0, cells, n) + rng.uniform(0.05, 0.95, n)) * res).astype(F32)
    out["z"], out["pad"] = rng.uniform(-1, 2, n).astype(F32), 1.0
    for f in ("r", "g", "b", "a"):
        out[f] = rng.integers(0, 256, n)
    out["covariance"] = rng.uniform(-0.1, 1.1, n).astype(F32)
    out["intensity"], out["travers"] = rng.uniform(0, 100, n).astype(F32), rng.uniform(0, 1, n).astype(F32)
    return out


def test_submap_steps_past_2_20_records():
    rng = np.random.default_rng(2020)
    res = 0.05
    own = dup_cloud(rng, 1 << 20)
    i = np.arange(1 << 20)
    own["x"], own["y"] = ((i % 1024 + 0.5) * res).astype(F32), ((i // 1024 + 0.5) * res).astype(F32)
    few = dup_cloud(rng, 1_100_000)
    spots = rng.integers(0, 600, (8, 2))
    pick = rng.integers(0, 8, few.size)
    few["x"] = ((spots[pick, 0] + rng.uniform(0.05, 0.95, few.size)) * res).astype(F32)
    few["y"] = ((spots[pick, 1] + rng.uniform(0.05, 0.95, few.size)) * res).astype(F32)
    clouds = [dup_cloud(rng, 1_200_000), own, few, dup_cloud(rng, 1_300_000)]
    assert len(global_ref.hash_fast(own, res)[0]) == 1 << 20 and len(global_ref.hash_fast(few, res)[0]) <= 8
    m = ElevationMap(32, res)
    m.global_enable(1 << 16)                                             # grows on the pushes
    stack = []
    for k, c in enumerate(clouds):
        assert m.global_push(c) == k
        global_ref.push(stack, c)
    check_stack(m, stack)
    t = transforms(rng, 4)
    t[1] = np.eye(4, dtype=F32)                                          # exact: the own-key submap keeps 2^20 keys through every step
    centres = np.array([[0, 0], [1, 0], [0, 2], [3, 0]], F32)             # every list holds all four: 12 pair steps
    fused = m.global_loop_closure(t, centres, 25.0, res)
    want = global_ref.loop_closure(stack, 4, t, centres, 25.0, res, fast=True)
    assert fused == want and fused > 1_000_000
    assert stack[1].size == 1 << 20 and stack[2].size < 64               # (its transform moves a few of the 8 clusters across cell borders)
    check_stack(m, stack)


def test_neighbour_list_edges():
    """radius 10: centre 1 is exactly at the radius from centre 0 (not a neighbour); 2 and 3 tie at d2 = 25 from 0; 4 coincides with
    0 (its list is [0, 4, 2, 3]: the step (4, 4)); 1's list has 3 entries (two steps), 5 and 6 form a list of 2 (no step); n_opt 9
    on a stack of 7"""
    m = ElevationMap(32, 0.05)
    m.global_enable(1 << 12)
    rng = np.random.default_rng(77)
    stack = []
    for k in range(7):
        c = synthetic(rng, 4000, 0.3 * k)
        assert m.global_push(c) == k
        global_ref.push(stack, c)
    centres = np.array([[0, 0], [6, 8], [3, 4], [4, 3], [0, 0], [100, 0], [101, 0], [0, 0], [1, 1]], F32)
    assert global_ref.neighbours(centres, 7, 0, 10.0) == [0, 4, 2, 3]
    assert global_ref.neighbours(centres, 7, 4, 10.0) == [0, 4, 2, 3]
    assert global_ref.neighbours(centres, 7, 1, 10.0) == [1, 2, 3]
    assert global_ref.neighbours(centres, 7, 5, 10.0) == [5, 6]
    t = transforms(rng, 9)
    fused = m.global_loop_closure(t, centres, 10.0, 0.05)
    assert fused == global_ref.loop_closure(stack, 9, t, centres, 10.0, 0.05) and fused > 0
    check_stack(m, stack)


@pytest.mark.parametrize("always_wait", [0, 1])
def test_capture_and_push_local_after_a_deferred_walk(oracle_mod, always_wait):
    """device clouds through the overlapped sorted pipeline leave their walks to the next call; that call is gem_local_capture
    (flush_pending -> settle -> flush_walk) or gem_global_push_local, as in the node"""
    import torch
    L, res = 160, 0.1
    p = Pair(oracle_mod, L, res)
    p.gpu.set_lowest_tracking(False)                                     # (a pass that maintains map_lowest launches its own walk)
    for k, v in {"sort_min_points": 1, "overlap_min_points": 1, "defer_walk": 1, "walk_always_wait": always_wait}.items():
        p.gpu.debug_set(k, v)
    p.gpu.global_enable(1 << 14)
    rng = np.random.default_rng(160)
    stack, adds = [], 0
    for k in range(12):
        xy = (0.35 * k, -0.2 * k)
        shift = p.move(xy)
        t = rng.uniform(0, 1, (L, L)).astype(F32)
        p.gpu.set_layer("traver", t); p.ref.set_layer("traver", t)
        c = synth.random_cloud(1600 + k, int(rng.integers(20_000, 90_000)), 0.4 * L * res, z_sigma=0.15)
        f = synth._frame_for(synth.pose_matrix(xy[0], xy[1], 0.5, 0.1 * k), SensorModel.velodyne())
        p.gpu.add(f, torch.from_numpy(c).cuda()); p.ref.add(f, c)
        adds += 1
        if k % 4 == 3:                                                  # the push is the call after the add
            i = p.gpu.global_push_local(True)
            assert i == global_ref.push_local(stack, p.local, p.cap)
            p.local.clear()
            assert p.gpu.global_export(i).tobytes() == stack[i].tobytes()
        p.capture(zero_feat(L), k)
        if k == 0:
            p.keep_previous()
        if p.gate(shift):
            p.spill(shift, k)
        p.keep_previous()
    assert np.array_equal(p.gpu.layer("elevation"), p.ref.layer("elevation"))
    assert p.gpu.debug_get("walks_left") >= adds - 1
    if always_wait:
        assert p.gpu.debug_get("walks_unwaited") == 0
    check_stack(p.gpu, stack)
