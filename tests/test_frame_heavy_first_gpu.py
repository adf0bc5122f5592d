"""k_frame with its binning waves at a raised issue priority (s_setprio behind the issue of the load of their points), next to tiles
of every weight the tile's code branches on (kFrameSpec = 256 records, the bucket's 768) -- against the CPU oracle, bit for bit: elevation and variance, plus lowest
when it is tracked.  A priority changes when a wave issues, never what it computes: no record, bucket or chain step may move, so
every stream here is one whose tiles sit on the boundaries the tile's code branches on, next to the centre tile (where a
robot-centric sweep puts its heavy tiles) and far from it.  Every stream runs with "frame_lean" = 0, 1 and 2, with and without
lowest tracking; the oracle runs each stream once.

The clouds are BUILT as tests/test_frame_sized_sort_gpu.py builds them (a point at the centre of a chosen cell, sensor pose =
identity, record k of every cell in block k of the sweep, blocks padded to whole binning blocks with points outside the map), on maps
at 0.05 m of L = 32, 256 and 272 cells (2, 16 and 17 tiles per row: the last tile row and column of 272 are whole, of 600 -- run
once -- they are half tiles).  What a stream says about itself is asserted from the oracle's own projection.
- counts: 255 / 256 / 257, 511 / 512 / 513 and 767 / 768 records in one tile, at most 7 per cell: each count once in a tile next to
  the centre tile and once in a tile far from it (on L = 32 there are four tiles in all); the fast path throughout;
- the slow path: 769 records in one tile (one more than the bucket holds: the spill), and a cell of eight in a tile of 300;
- stale slots: 600 records, a filler frame, 3 records, a filler frame into the same tile -- the pass buffers are double-buffered, so
  the 3 records land in the bucket the 600 were in, whose slots 3..599 are stale -- compared after every frame;
- a moved map: the centre tile in the first and in the last tile row and column of the circular buffer, tiles of more than 256
  records on either side of the wrap;
- the stamp buffer on, once: the stamped kernel gives the same maps and a full row of stamps per tile;
- the 16-sweep C2 stream against tests/golden/digests.json c2_stream16."""
import ctypes as C
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import oracle
from gem_amd import ElevationMap, SensorModel, synth

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
F32 = np.float32
RES = 0.05
MODES = [0, 1, 2]
LAYERS = ("elevation", "variance", "lowest")
_REF = {}                                              # stream name -> the oracle's snapshots (computed once, never modified)
_OPS = {}                                              # stream name -> its ops (built once)


def frame_at():
    return synth._frame_for(synth.pose_matrix(0.0, 0.0, 0.0, yaw=0.0), SensorModel.velodyne())


def tpr_of(L):
    return (L + 15) // 16


def cell_points(L, rows, cols, z, centre=(0.0, 0.0)):
    """one point at the centre of each GEOGRAPHIC cell (rows[i], cols[i]) of a map of L cells centred at `centre`"""
    rows, cols = np.asarray(rows, np.float64), np.asarray(cols, np.float64)
    c = np.zeros((rows.size, 4), F32)
    c[:, 0] = centre[0] + (L // 2 - rows - 0.5) * RES
    c[:, 1] = centre[1] + (L // 2 - cols - 0.5) * RES
    c[:, 2] = z
    c[:, 3] = 1.0
    return c


def outside(n):
    c = np.zeros((n, 4), F32)
    c[:, 0] = 500.0; c[:, 1] = 500.0; c[:, 3] = 1.0
    return c


def spread(rng, n, top=7):
    """n records over a tile's 256 cells, at most `top` per cell"""
    per = np.zeros(256, np.int64)
    np.add.at(per, rng.permutation(256 * top)[:n] % 256, 1)
    return per


def sweep(L, tiles, rng, centre=(0.0, 0.0)):
    """tiles: {(geographic tile row, tile column): records per cell [256]}.  Block k of the sweep holds record k of every cell that
    has one, the cells shuffled, padded to whole binning blocks (256 points) with points outside the map."""
    keys = list(tiles)
    per = np.stack([np.asarray(tiles[k]) for k in keys])
    base = np.array(keys, np.int64) * 16
    parts = []
    for k in range(int(per.max())):
        t, cell = np.nonzero(per > k)
        p = rng.permutation(t.size)
        t, cell = t[p], cell[p]
        parts.append(cell_points(L, base[t, 0] + cell // 16, base[t, 1] + cell % 16, rng.normal(0.02 * k, 0.1, t.size).astype(F32), centre))
        parts.append(outside(-t.size % 256 + 256))
    return np.concatenate(parts).astype(F32)


def tile_counts(oracle_mod, L, cloud, position=None):
    """records per circular-buffer tile and the largest count of a cell, from the oracle's projection (on a map moved to `position`)"""
    o = oracle_mod.OracleMap(L, RES)
    if position is not None:
        o.move(position)
    idx = np.asarray(o.process_points(frame_at(), cloud[:, 0], cloud[:, 1], cloud[:, 2])["index"])
    idx = idx[idx >= 0]
    n = tpr_of(L)
    per = np.zeros((n, n), np.int64)
    np.add.at(per, ((idx // L) >> 4, (idx % L) >> 4), 1)
    return per, (int(np.bincount(idx).max()) if idx.size else 0)


def snapshot(ref):
    return {n: ref.layer(n).copy() for n in LAYERS}


def reference(oracle_mod, name, L, ops):
    if name not in _REF:
        ref = oracle_mod.OracleMap(L, RES)
        snaps = [snapshot(ref)]
        for op in ops:
            if op[0] == "add":
                ref.add(op[1], op[2])
            elif op[0] == "move":
                ref.move(op[1])
            elif op[0] == "check":
                snaps.append(snapshot(ref))
        _REF[name] = snaps
    return _REF[name]


def run(oracle_mod, name, L, ops, mode, track, stamps=False):
    """The stream on the device with "frame_lean" = mode; ("check",) synchronises and compares with the oracle's snapshot.
    Returns (map, stamp rows or None)."""
    import torch
    from gem_amd import _lib
    snaps = reference(oracle_mod, name, L, ops)
    gpu = ElevationMap(L, RES, debug={"frame_lean": mode})
    if track:
        gpu.set_lowest_tracking(True)
        gpu.set_layer("lowest", snaps[0]["lowest"])    # the oracle always tracks: start both from the same layer
    lib = _lib.load()
    if stamps:
        gpu.debug_set("dbg_frame", 1)
        lib.gem_debug_fuse_stamps(gpu._h, 1, None, 0)
    dev = {id(op[2]): torch.from_numpy(op[2]).cuda() for op in ops if op[0] == "add"}
    torch.cuda.synchronize()
    k, rows = 0, None
    for op in ops:
        if op[0] == "add":
            gpu.add(op[1], dev[id(op[2])])
        elif op[0] == "move":
            gpu.move(op[1])
        elif op[0] == "stamps":                        # the rows of the last k_frame launch (the read switches the stamps off)
            buf = np.zeros((512, 16), np.uint64)
            n = lib.gem_debug_fuse_stamps(gpu._h, 0, buf.ctypes.data_as(C.c_void_p), 512)
            rows = buf[:n].copy()
        elif op[0] == "check":
            gpu.synchronize()
            k += 1
            for n in LAYERS[:3 if track else 2]:
                g, o = gpu.layer(n), snaps[k][n]
                assert np.array_equal(g, o), f"{name}, mode {mode}, check {k}: {n} differs in {np.count_nonzero(g != o)} cells"
    return gpu, rows


def check_form(gpu, mode, slow):
    """a stream that never needs the slow path launches one form only (mode 0 the generic, modes 1 and 2 the lean one); the slow
    path reports itself in every mode"""
    lean, generic, seen = gpu.debug_get("frame_lean_launches"), gpu.debug_get("frame_generic_launches"), gpu.debug_get("frame_form_seen")
    assert seen == (1 if slow else 0), seen
    if not slow:
        assert (lean == 0 and generic > 0) if mode == 0 else (generic == 0 and lean > 0), (mode, lean, generic)


# ---- 1. the counts the kernel branches on, next to the centre tile and far from it ----------------------------------------------
COUNTS = (255, 256, 257, 511, 512, 513, 767, 768)


def places(L):
    """(tiles next to the centre tile, tiles far from it): four each, all whole tiles; L = 32 has four tiles in all"""
    n = tpr_of(L)
    if n == 2:
        t = [(0, 0), (0, 1), (1, 0), (1, 1)]
        return t, t
    c = (L // 2) >> 4
    whole = L // 16 - 1                                # the last whole tile row / column
    return [(c, c), (c - 1, c + 1), (c + 1, c - 1), (c, c - 2)], [(0, 0), (whole, whole), (0, whole), (whole, 3)]


def counts_ops(L):
    name = f"counts{L}"
    if name not in _OPS:
        rng = np.random.default_rng(900 + L)
        near, far = places(L)
        if tpr_of(L) == 2:
            want = [dict(zip(near, COUNTS[:4])), dict(zip(near, COUNTS[4:]))]
        else:                                          # every count once next to the centre and once far from it
            want = [{**dict(zip(near, COUNTS[:4])), **dict(zip(far, COUNTS[4:]))}, {**dict(zip(near, COUNTS[4:])), **dict(zip(far, COUNTS[:4]))}]
        clouds = [sweep(L, {t: spread(rng, n) for t, n in w.items()}, rng) for w in want]
        ops = [("add", frame_at(), clouds[0]), ("add", frame_at(), clouds[1]), ("check",), ("add", frame_at(), clouds[0][::-1].copy()), ("check",)]
        _OPS[name] = (ops, want, clouds)
    return (name,) + _OPS[name]


def assert_counts(oracle_mod, L, want, clouds):
    for w, cloud in zip(want, clouds):
        per, top = tile_counts(oracle_mod, L, cloud)
        assert top <= 7 and per.sum() == sum(w.values())
        for t, n in w.items():
            assert per[t] == n, (t, n, per[t])


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [32, 256, 272])
def test_counts_near_and_far(oracle_mod, L, mode, track):
    name, ops, want, clouds = counts_ops(L)
    assert_counts(oracle_mod, L, want, clouds)
    gpu, _ = run(oracle_mod, name, L, ops, mode, track)
    check_form(gpu, mode, slow=False)
    gpu.close()


def test_counts_on_a_map_with_half_tiles(oracle_mod):
    name, ops, want, clouds = counts_ops(600)          # 38 tiles per row, the last of 8 cells
    assert_counts(oracle_mod, 600, want, clouds)
    gpu, _ = run(oracle_mod, name, 600, ops, 2, False)
    check_form(gpu, 2, slow=False)
    gpu.close()


# ---- 2. the slow path: one record more than the bucket holds, and a cell of eight ----------------------------------------------
def slow_ops(kind, L=256):
    name = f"slow_{kind}"
    if name not in _OPS:
        rng = np.random.default_rng(940 + len(kind))
        c = (L // 2) >> 4
        if kind == "spill":
            tiles = {(c, c + 1): spread(rng, 769), (2, 2): spread(rng, 300)}
        else:
            per = spread(rng, 292, top=4); per[77] = 8
            while per.sum() < 300:                     # 300 records in all, the cell of eight the only one above four
                k = int(rng.integers(0, 256))
                if k != 77 and per[k] < 4:
                    per[k] += 1
            tiles = {(c + 1, c): per, (13, 1): spread(rng, 257)}
        a, b = sweep(L, tiles, rng), sweep(L, {(c, c): spread(rng, 100)}, rng)
        ops = [("add", frame_at(), a), ("add", frame_at(), b), ("check",), ("add", frame_at(), a[::-1].copy()), ("add", frame_at(), b), ("check",)]
        _OPS[name] = (ops, tiles, a)
    return (name,) + _OPS[name]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["spill", "eight"])
def test_slow_path_is_still_right(oracle_mod, kind, mode, track):
    name, ops, tiles, a = slow_ops(kind)
    per, top = tile_counts(oracle_mod, 256, a)
    assert (per.max() == 769 and top <= 7) if kind == "spill" else (per.max() == 300 and top == 8), (per.max(), top)
    gpu, _ = run(oracle_mod, name, 256, ops, mode, track)
    check_form(gpu, mode, slow=True)
    gpu.close()


# ---- 3. stale slots: 600 records, then 3, in the same bucket -------------------------------------------------------------------
def stale_ops(L=272):
    if "stale" not in _OPS:
        rng = np.random.default_rng(950)
        c = (L // 2) >> 4
        target, other = (c, c + 1), (3, 12)
        heavy = sweep(L, {target: spread(rng, 600)}, rng)
        light = np.zeros(256, np.int64); light[[5, 130, 255]] = 1
        few = sweep(L, {target: light}, rng)
        fill = sweep(L, {other: spread(rng, 40, top=1)}, rng)
        ops = []
        for cloud in (heavy, fill, few, fill, heavy[::-1].copy(), few):
            ops += [("add", frame_at(), cloud), ("check",)]
        _OPS["stale"] = (ops, target, heavy, few)
    return _OPS["stale"]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_stale_slots_behind_a_small_count(oracle_mod, mode, track):
    ops, target, heavy, few = stale_ops()
    assert tile_counts(oracle_mod, 272, heavy)[0][target] == 600 and tile_counts(oracle_mod, 272, few)[0][target] == 3
    gpu, _ = run(oracle_mod, "stale", 272, ops, mode, track)
    check_form(gpu, mode, slow=False)
    gpu.close()


# ---- 4. a moved map: the centre tile in the first / last tile row and column of the circular buffer ----------------------------
MOVES = {"first": (6.4, 6.4, 0.0), "last": (7.2, 7.2, 0.0)}          # start index 128 / 112: whole tiles, the buffer's wrap between two of them


def moved_ops(where, L=256):
    name = f"moved_{where}"
    if name not in _OPS:
        rng = np.random.default_rng(960 + len(where))
        pos = MOVES[where]
        o = oracle.OracleMap(L, RES)
        start = int(o.move(pos)[1][0])
        g = ((L - 16 - start) % L) // 16 + 1           # geographic tiles g - 1 and g land in the buffer's last and first tile row / column
        tiles = {(g - 1, g - 1): spread(rng, 300), (g, g): spread(rng, 513), (g - 1, g): spread(rng, 257), (g + 3, g - 4): spread(rng, 90)}
        a = sweep(L, tiles, rng, centre=pos)
        ops = [("move", pos), ("add", frame_at(), a), ("add", frame_at(), a[::-1].copy()), ("check",), ("add", frame_at(), a), ("check",)]
        _OPS[name] = (ops, pos, a)
    return (name,) + _OPS[name]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("where", ["first", "last"])
def test_moved_map_heavy_tiles_across_the_wrap(oracle_mod, where, mode, track):
    L = 256
    name, ops, pos, a = moved_ops(where)
    o = oracle_mod.OracleMap(L, RES)
    _, start, _ = o.move(pos)
    centre_tile = [((L // 2 + int(s)) % L) >> 4 for s in start]
    assert centre_tile == ([0, 0] if where == "first" else [15, 15]), (start, centre_tile)
    per, top = tile_counts(oracle_mod, L, a, pos)
    assert per.sum() == 300 + 513 + 257 + 90 and top <= 7
    rows, cols = np.nonzero(per > 256)
    # the tiles of more than 256 records sit on either side of the buffer's wrap, in rows and in columns
    assert rows.size == 3 and {int(rows.min()), int(rows.max())} == {0, 15} == {int(cols.min()), int(cols.max())}, (rows, cols)
    gpu, _ = run(oracle_mod, name, L, ops, mode, track)
    check_form(gpu, mode, slow=False)
    gpu.close()


# ---- 5. the stamp buffer on, once: the same maps, and the tile's record count in its stamp row ---------------------------------
def test_stamped_kernel_gives_the_same_maps(oracle_mod):
    L = 32
    name, ops, want, clouds = counts_ops(L)
    stamped = ops[:2] + [("stamps",), ("check",)]      # (the second k_frame-less flush follows the read: the check synchronises)
    gpu, rows = run(oracle_mod, name, L, stamped, 2, True, stamps=True)
    # rows [0, 4): the tiles of the last k_frame (the fuse of the first frame), then its binning blocks
    assert rows is not None and rows.shape[0] >= 4, None if rows is None else rows.shape
    tiles = rows[:4]
    assert np.all(tiles[:, 15] > 0) and np.all((tiles[:, :6] > 0).sum(1) == 6), tiles
    assert np.all(tiles[:, 12] > 0) and np.all(tiles[:, 13] >= tiles[:, 12]), tiles
    gpu.close()


# ---- 6. the C2 stream of bench.py ----------------------------------------------------------------------------------------------
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
