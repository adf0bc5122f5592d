"""k_frame's lean form with its head words preloaded into scalar registers (gem_frame_lean.hpp FrameLeanHead, gem_frame_lean.hip)
against the CPU oracle, bit for bit: elevation and variance, plus lowest when it is tracked.  Every stream runs with "frame_lean" =
0 (always generic), 1 (always lean) and 2 (the host's choice), with and without lowest tracking; the oracle runs each stream once.

A wrong head word cannot hide in these streams:
- maps of 32, 40 and 272 cells at 0.1 m: tiles_per_row 2, 3 and 17 (tile_div, and 60 / 55 / 31 padding blocks beyond T), every
  one fed clouds of 1, 63, 64, 65, 255, 256, 257 and 1025 points (n, B, the last partial unit and binning block), before and behind
  a move by whole cells;
- the 272-cell map moved so that the centre tile lies in the first / last tile row and column (center_tr, center_tc, the wrap);
- two handles with different maps taking turns in one process (the words belong to the launch, not to the kernel);
- the stamp buffer on (the stamped kernel shares the signature; its start stamps are stored behind the first loads now);
- a cell of eight records: the slow path, the hand-over to the generic form and what follows it;
- the 16-sweep C2 stream against tests/golden/digests.json c2_stream16."""
import ctypes as C
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from gem_amd import ElevationMap, SensorModel, synth

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
F32 = np.float32
RES = 0.1
MODES = [0, 1, 2]
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
LAYERS = ("elevation", "variance", "lowest")
_REF = {}                                              # stream name -> the oracle's snapshots (computed once, never modified)
_OPS = {}                                              # stream name -> its ops (built once)


def frame_at():
    return synth._frame_for(synth.pose_matrix(0.0, 0.0, 0.0, yaw=0.0), SensorModel.velodyne())


def cloud(L, n, rng, centre=(0.0, 0.0)):
    """n points drawn over a map of L cells centred at `centre` (sensor pose = identity)"""
    c = np.zeros((n, 4), F32)
    half = 0.49 * L * RES
    c[:, 0] = centre[0] + rng.uniform(-half, half, n)
    c[:, 1] = centre[1] + rng.uniform(-half, half, n)
    c[:, 2] = rng.normal(0.0, 0.15, n)
    c[:, 3] = 1.0
    return c


def adds(clouds, every=2):
    """the clouds as frames, a check behind every `every`-th: a frame is fused by the next frame's k_frame or by the check's flush"""
    ops = []
    for i, c in enumerate(clouds):
        ops.append(("add", frame_at(), c))
        if i % every == every - 1 or i == len(clouds) - 1:
            ops.append(("check",))
    return ops


def assert_fast(oracle_mod, L, ops):
    """every sweep of the stream stays on the fast path (no tile above 768 records, no cell above 7) and, all but the single
    points, keeps records: the comparison below compares something"""
    o = oracle_mod.OracleMap(L, RES)
    for op in ops:
        if op[0] == "move":
            o.move(op[1])
        elif op[0] == "add":
            idx = np.asarray(o.process_points(op[1], op[2][:, 0], op[2][:, 1], op[2][:, 2])["index"])
            idx = idx[idx >= 0]
            assert idx.size >= op[2].shape[0] // 2, (idx.size, op[2].shape[0])
            if idx.size:
                tpr = (L + 15) // 16
                tiles = np.bincount((idx // L >> 4) * tpr + (idx % L >> 4))
                assert tiles.max() <= 768 and np.bincount(idx).max() <= 7, (tiles.max(), np.bincount(idx).max())


def reference(oracle_mod, name, L, ops):
    if name not in _REF:
        ref = oracle_mod.OracleMap(L, RES)
        snaps = [{n: ref.layer(n).copy() for n in LAYERS}]
        for op in ops:
            if op[0] == "add":
                ref.add(op[1], op[2])
            elif op[0] == "move":
                ref.move(op[1])
            elif op[0] == "check":
                snaps.append({n: ref.layer(n).copy() for n in LAYERS})
        _REF[name] = snaps
    return _REF[name]


class Stream:
    """one handle running one stream's ops, one at a time (two of them can take turns)"""

    def __init__(self, oracle_mod, name, L, ops, mode, track, stamps=False):
        import torch
        from gem_amd import _lib
        self.name, self.mode, self.track, self.ops = name, mode, track, ops
        self.snaps = reference(oracle_mod, name, L, ops)
        self.gpu = ElevationMap(L, RES, debug={"frame_lean": mode})
        if track:
            self.gpu.set_lowest_tracking(True)
            self.gpu.set_layer("lowest", self.snaps[0]["lowest"])    # the oracle always tracks: start both from the same layer
        self.lib = _lib.load()
        if stamps:
            self.gpu.debug_set("dbg_frame", 1)
            self.lib.gem_debug_fuse_stamps(self.gpu._h, 1, None, 0)
        self.dev = {id(op[2]): torch.from_numpy(op[2]).cuda() for op in ops if op[0] == "add"}
        torch.cuda.synchronize()
        self.at, self.k, self.rows = 0, 0, None

    def step(self):
        """the next op; False when the stream is done"""
        if self.at == len(self.ops):
            return False
        op = self.ops[self.at]
        self.at += 1
        if op[0] == "add":
            self.gpu.add(op[1], self.dev[id(op[2])])
        elif op[0] == "move":
            self.gpu.move(op[1])
        elif op[0] == "stamps":                        # the rows of the last k_frame launch (the read switches the stamps off)
            buf = np.zeros((512, 16), np.uint64)
            n = self.lib.gem_debug_fuse_stamps(self.gpu._h, 0, buf.ctypes.data_as(C.c_void_p), 512)
            self.rows = buf[:n].copy()
        elif op[0] == "check":
            self.gpu.synchronize()
            self.k += 1
            for n in LAYERS[:3 if self.track else 2]:
                g, o = self.gpu.layer(n), self.snaps[self.k][n]
                assert np.array_equal(g, o), f"{self.name}, mode {self.mode}, check {self.k}: {n} differs in {np.count_nonzero(g != o)} cells"
        return True

    def run(self):
        while self.step():
            pass
        return self

    def counts(self):
        return self.gpu.debug_get("frame_lean_launches"), self.gpu.debug_get("frame_generic_launches"), self.gpu.debug_get("frame_form_seen")

    def check_stays(self):
        """a stream that never needs the slow path launches one form only: mode 0 the generic, modes 1 and 2 the lean one"""
        lean, generic, seen = self.counts()
        assert seen == 0, seen
        assert (lean == 0 and generic > 0) if self.mode == 0 else (generic == 0 and lean > 0), (self.mode, lean, generic)

    def close(self):
        self.gpu.close()


def start_of(oracle_mod, L, pos):
    o = oracle_mod.OracleMap(L, RES)
    _, start, _ = o.move(pos)
    return [int(s) for s in start]


# ---- 1. map sizes x cloud sizes, before and behind a move ---------------------------------------------------------------------------
def sizes_ops(L):
    name = f"preload_sizes{L}"
    if name not in _OPS:
        rng = np.random.default_rng(2100 + L)
        pos = (3 * RES, -5 * RES, 0.0)                 # whole cells: start0 / start1 leave zero
        ops = adds([cloud(L, n, rng) for n in SIZES]) + [("move", pos)] + adds([cloud(L, n, rng, pos) for n in (1025, 1, 257, 64)])
        _OPS[name] = (ops, pos)
    return (name,) + _OPS[name]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [32, 40, 272])
def test_map_sizes_and_cloud_sizes(oracle_mod, L, mode, track):
    name, ops, pos = sizes_ops(L)
    assert [op[2].shape[0] for op in ops if op[0] == "add"][:len(SIZES)] == list(SIZES)
    assert (L + 15) // 16 == {32: 2, 40: 3, 272: 17}[L]
    assert all(s != 0 for s in start_of(oracle_mod, L, pos))
    assert_fast(oracle_mod, L, ops)
    s = Stream(oracle_mod, name, L, ops, mode, track).run()
    s.check_stays()
    s.close()


# ---- 2. the centre tile in the first / last tile row and column ---------------------------------------------------------------------
CORNERS = {"first-first": (128, 128), "last-last": (144, 144), "first-last": (128, 144), "last-first": (144, 128)}   # cells the 272-cell map moves by


def corner_ops(where):
    name = f"preload_corner_{where}"
    if name not in _OPS:
        rng = np.random.default_rng(2200 + sum(map(ord, where)))
        s0, s1 = CORNERS[where]
        pos = (s0 * RES, s1 * RES, 0.0)
        ops = [("move", pos)] + adds([cloud(272, n, rng, pos) for n in (600, 1025, 600)], every=3)
        _OPS[name] = (ops, pos)
    return (name,) + _OPS[name]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("where", list(CORNERS))
def test_centre_tile_in_first_and_last_row_and_column(oracle_mod, where, mode, track):
    L = 272
    name, ops, pos = corner_ops(where)
    centre_tile = [((L // 2 + s) % L) >> 4 for s in start_of(oracle_mod, L, pos)]
    assert centre_tile == [0 if w == "first" else 16 for w in where.split("-")], centre_tile
    assert_fast(oracle_mod, L, ops)
    s = Stream(oracle_mod, name, L, ops, mode, track).run()
    s.check_stays()
    s.close()


# ---- 3. two handles, different maps, taking turns -----------------------------------------------------------------------------------
def turns_ops(L):
    name = f"preload_turns{L}"
    if name not in _OPS:
        rng = np.random.default_rng(2300 + L)
        pos = (7 * RES, 2 * RES, 0.0)
        _OPS[name] = [("move", pos)] + adds([cloud(L, n, rng, pos) for n in (300, 65, 1025, 257, 300, 64)], every=3)
    return name, _OPS[name]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_two_handles_take_turns(oracle_mod, mode, track):
    (name_a, ops_a), (name_b, ops_b) = turns_ops(40), turns_ops(272)
    a = Stream(oracle_mod, name_a, 40, ops_a, mode, track)
    b = Stream(oracle_mod, name_b, 272, ops_b, mode, track)
    assert_fast(oracle_mod, 40, a.ops); assert_fast(oracle_mod, 272, b.ops)
    more = True
    while more:                                        # one op each, in turn: every k_frame launch follows one of the other handle
        more = a.step()
        more = b.step() or more
    a.check_stays(); b.check_stays()
    a.close(); b.close()


# ---- 4. the stamp buffer on ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("track", [False, True])
def test_stamped_kernel_takes_the_head_too(oracle_mod, track):
    L = 40
    name = "preload_stamped"
    if name not in _OPS:
        rng = np.random.default_rng(2400)
        c = [cloud(L, n, rng) for n in (1025, 257)]
        _OPS[name] = [("add", frame_at(), c[0]), ("add", frame_at(), c[1]), ("stamps",), ("check",)]
    ops = _OPS[name]
    assert_fast(oracle_mod, L, ops)
    s = Stream(oracle_mod, name, L, ops, 1, track, stamps=True).run()
    T, nbin = 9, (257 + 255) // 256
    rows = s.rows
    # rows [0, T): the tiles of the last k_frame (the fuse of the first frame: every tile of the map holds records), then its binning
    # blocks (the pass plan's unit count: at least the cloud's)
    assert rows is not None and rows.shape[0] >= T + nbin, None if rows is None else rows.shape
    tiles, bins = rows[:T].astype(np.int64), rows[T:].astype(np.int64)
    assert np.all(tiles[:, 15] > 0) and np.all(tiles[:, 0] > 0) and np.all(tiles[:, 1] >= tiles[:, 0]), tiles
    assert np.all(tiles[:, 12] > 0) and np.all(tiles[:, 13] >= tiles[:, 12]), tiles
    assert np.all(bins[:, 15] > 0) and np.all(bins[:, 0] > 0) and np.all(bins[:, 1] >= bins[:, 0]), bins
    assert np.all(bins[:, 12] > 0) and np.all(bins[:, 13] >= bins[:, 12]), bins
    s.check_stays()
    s.close()


# ---- 5. a cell of eight records: over to the generic form and on -----------------------------------------------------------------
def cell8_ops(L):
    name = f"preload_cell8_{L}"
    if name not in _OPS:
        rng = np.random.default_rng(2500 + L)
        wall = np.zeros((8, 4), F32)
        wall[:, 0] = 0.45; wall[:, 1] = -0.65; wall[:, 2] = rng.normal(0.3, 0.05, 8); wall[:, 3] = 1.0     # one cell, well inside it
        light = lambda: cloud(L, 40, rng)
        heavy = np.concatenate([light()[:10], wall[:4], light(), wall[4:], light()[:7]]).astype(F32)
        ops = [("add", frame_at(), light()), ("add", frame_at(), heavy), ("check",),
               ("add", frame_at(), light()), ("add", frame_at(), light()), ("check",)]
        _OPS[name] = (ops, heavy)
    return (name,) + _OPS[name]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_cell_of_eight_hands_over_to_the_generic_form(oracle_mod, mode, track):
    L = 40
    name, ops, heavy = cell8_ops(L)
    o = oracle_mod.OracleMap(L, RES)
    idx = np.asarray(o.process_points(frame_at(), heavy[:, 0], heavy[:, 1], heavy[:, 2])["index"])
    assert np.bincount(idx[idx >= 0]).max() == 8, np.bincount(idx[idx >= 0]).max()
    s = Stream(oracle_mod, name, L, ops, mode, track).run()
    lean, generic, seen = s.counts()
    assert seen == 1, seen                                                              # the slow path reports in every mode
    if mode == 0:
        assert lean == 0
    elif mode == 1:
        assert generic == 0 and lean > 0
    else:
        assert lean > 0 and generic >= 3, (lean, generic)   # behind the first check: a binning, a k_frame and the fuse-only launch, generic
    s.close()


# ---- 6. the C2 stream of bench.py -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_c2_stream_digest(mode):
    import torch
    d = json.loads((Path(__file__).resolve().parent / "golden" / "digests.json").read_text())["c2_stream16"]
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    wl = synth.config_c4(n_sweeps=8, seed0=100)
    assert sha(np.concatenate(wl.clouds)) == d["cloud"], "generator drift"
    dc = [torch.from_numpy(c).cuda() for c in wl.clouds]
    m = ElevationMap(wl.length, wl.resolution, debug={"frame_lean": mode})
    for k in range(16):
        m.add(wl.frames[k % 8], dc[k % 8])
    assert sha(m.layer("elevation")) == d["elevation"] and sha(m.layer("variance")) == d["variance"]
    m.close()
