"""k_frame's light path (frame_tile, lean form: a tile of at most 64 records is fused by wave 0 alone, one lane per record; an empty
tile leaves before any cell load) against the CPU oracle, bit for bit: elevation and variance, plus lowest when it is tracked.
Every stream runs with "frame_lean" = 0 (always generic: the cell-centric path), 1 (always lean) and 2 (the host's choice), with and
without lowest tracking; the oracle runs each stream once.

The clouds are BUILT as tests/test_frame_heavy_first_gpu.py builds them (a point at the centre of a chosen cell, sensor pose =
identity, record k of every cell in block k of the sweep, blocks padded to whole binning blocks with points outside the map), on maps
at 0.05 m of L = 32 (four whole tiles), L = 40 (nine tiles, the last tile row and column overhang the map by half) and once L = 272.
What a stream says about itself is asserted from the oracle's own projection.  A frame is fused by the k_frame launch of the frame
behind it, or by the fuse-only launch of a synchronise: the streams check behind both.
- boundary counts: a tile of exactly 1, 2, 63, 64 and 65 records next to an empty tile and next to a tile of 300;
- seven per cell: 64 records in 64 cells, and 63 records as nine cells of 7;
- out-of-order arrival: one cell whose 7 records lie more than 256 point indices apart (different binning waves), heights such that
  the oracle's own result changes when any two of them are swapped (behind a frame that fills the cell: see ORDER_Z);
- a cell of 8 in a tile of exactly 64: the verdict sends all four waves into the general path, which takes the slow path;
- a queued Mapvar_update in front of a frame of light tiles (dense: every cell takes the increment), then a plain frame;
- light, heavy (600), light (3) through the same pass-buffer set: stale slots behind the count;
- a moved map: light tiles on either side of the circular buffer's wrap, the centre tile in the first / last tile row and column;
- the stamp buffer on: the same maps, and six stamps plus words 12, 13, 15 per live tile;
- the 16-sweep C2 stream against tests/golden/digests.json c2_stream16."""
import ctypes as C
import hashlib
import itertools
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


def inside(L, tile):
    """the cells of a tile that lie inside a map of L cells (an overhanging tile has fewer than 256)"""
    cell = np.arange(256)
    return cell[(tile[0] * 16 + cell // 16 < L) & (tile[1] * 16 + cell % 16 < L)]


def spread(rng, n, top=7, cells=None):
    """n records over a tile's cells (all 256, or `cells`), at most `top` per cell"""
    cells = np.arange(256) if cells is None else np.asarray(cells)
    assert n <= cells.size * top
    per = np.zeros(256, np.int64)
    np.add.at(per, cells[rng.permutation(cells.size * top)[:n] % cells.size], 1)
    return per


def sweep(L, tiles, rng, centre=(0.0, 0.0), z=None):
    """tiles: {(geographic tile row, tile column): records per cell [256]}.  Block k of the sweep holds record k of every cell that
    has one, the cells shuffled, padded to whole binning blocks (256 points) with points outside the map.  z: {(tile, cell): heights
    of the cell's records, in sweep order} for the cells whose heights the test chooses."""
    keys = list(tiles)
    per = np.stack([np.asarray(tiles[k]) for k in keys])
    base = np.array(keys, np.int64) * 16
    parts = []
    for k in range(int(per.max())):
        t, cell = np.nonzero(per > k)
        p = rng.permutation(t.size)
        t, cell = t[p], cell[p]
        h = rng.normal(0.02 * k, 0.1, t.size).astype(F32)
        for i in range(t.size):
            if z and (keys[t[i]], int(cell[i])) in z:
                h[i] = z[(keys[t[i]], int(cell[i]))][k]
        parts.append(cell_points(L, base[t, 0] + cell // 16, base[t, 1] + cell % 16, h, centre))
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
            elif op[0] == "var":
                ref.mapvar_update(op[1])
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
        elif op[0] == "var":
            gpu.mapvar_update(op[1])
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


def check_stays(gpu, mode):
    """a stream that never needs the slow path launches one form only: mode 0 the generic, modes 1 and 2 the lean one"""
    lean, generic, seen = gpu.debug_get("frame_lean_launches"), gpu.debug_get("frame_generic_launches"), gpu.debug_get("frame_form_seen")
    assert seen == 0, seen
    assert (lean == 0 and generic > 0) if mode == 0 else (generic == 0 and lean > 0), (mode, lean, generic)


def adds(clouds, every=2):
    """the clouds as frames, a check behind every `every`-th: a frame is fused by the next frame's k_frame or by the check's flush"""
    ops = []
    for i, c in enumerate(clouds):
        ops.append(("add", frame_at(), c))
        if i % every == every - 1 or i == len(clouds) - 1:
            ops.append(("check",))
    return ops


# ---- 1. boundary counts: 1, 2, 63, 64, 65 records next to an empty tile and next to a tile of 300 -------------------------------
COUNTS = (1, 2, 63, 64, 65)
PLACES = {32: dict(n=(0, 0), empty=(0, 1), heavy=(1, 0), few=(1, 1)),          # four whole tiles
          40: dict(n=(1, 2), empty=(0, 2), heavy=(1, 1), few=(2, 2)),          # (1, 2): 128 cells inside the map, (2, 2): 64
          272: dict(n=(8, 9), empty=(7, 9), heavy=(8, 8), few=(16, 16))}


def counts_ops(L):
    name = f"light_counts{L}"
    if name not in _OPS:
        rng = np.random.default_rng(1300 + L)
        pl = PLACES[L]
        clouds = [sweep(L, {pl["n"]: spread(rng, n, cells=inside(L, pl["n"])), pl["heavy"]: spread(rng, 300),
                            pl["few"]: spread(rng, 5, cells=inside(L, pl["few"]))}, rng) for n in COUNTS]
        clouds.append(clouds[0][::-1].copy())
        _OPS[name] = (adds(clouds), clouds)
    return (name,) + _OPS[name]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [32, 40])
def test_boundary_counts(oracle_mod, L, mode, track):
    name, ops, clouds = counts_ops(L)
    pl = PLACES[L]
    for n, cloud in zip(COUNTS, clouds):
        per, top = tile_counts(oracle_mod, L, cloud)
        assert per[pl["n"]] == n and per[pl["empty"]] == 0 and per[pl["heavy"]] == 300 and per[pl["few"]] == 5 and top <= 7, (n, per, top)
    gpu, _ = run(oracle_mod, name, L, ops, mode, track)
    check_stays(gpu, mode)
    gpu.close()


def test_boundary_counts_on_a_large_map(oracle_mod):
    name, ops, clouds = counts_ops(272)
    pl = PLACES[272]
    for n, cloud in zip(COUNTS, clouds):
        per, top = tile_counts(oracle_mod, 272, cloud)
        assert per[pl["n"]] == n and per[pl["empty"]] == 0 and per[pl["heavy"]] == 300 and top <= 7, (n, per[pl["n"]], top)
    gpu, _ = run(oracle_mod, name, 272, ops, 2, True)
    check_stays(gpu, 2)
    gpu.close()


# ---- 2. seven per cell: 64 records in 64 cells, 63 records as nine cells of 7 ---------------------------------------------------
def seven_ops(L):
    name = f"light_seven{L}"
    if name not in _OPS:
        rng = np.random.default_rng(1340 + L)
        far = (tpr_of(L) - 1, tpr_of(L) - 1)
        clouds = []
        for _ in range(3):
            one = np.zeros(256, np.int64); one[rng.permutation(inside(L, (0, 0)))[:64]] = 1
            nine = np.zeros(256, np.int64); nine[rng.permutation(inside(L, far))[:9]] = 7
            clouds.append(sweep(L, {(0, 0): one, far: nine}, rng))
        _OPS[name] = (adds(clouds, every=3), clouds, far)
    return (name,) + _OPS[name]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [32, 40])
def test_seven_records_per_cell(oracle_mod, L, mode, track):
    name, ops, clouds, far = seven_ops(L)
    for cloud in clouds:
        per, top = tile_counts(oracle_mod, L, cloud)
        assert per[0, 0] == 64 and per[far] == 63 and per.sum() == 127 and top == 7, (per, top)
    gpu, _ = run(oracle_mod, name, L, ops, mode, track)
    check_stays(gpu, mode)
    gpu.close()


# ---- 3. out-of-order arrival: a cell of 7 whose records come from seven binning blocks -------------------------------------------
ORDER_TILE, ORDER_CELL = (0, 1), 5 * 16 + 9
# Every record of a sweep has the same variance here (3.24e-4: the range term is far below the constant one), and the first steps
# into an EMPTY cell commute exactly: two records average, replace or ignore symmetrically.  So the cell is filled by a frame in front
# (seven records at height 0: elevation 0, variance at the floor of 1e-4), behind which every step is e += g (h - e) with the same
# g = 1e-4 / 4.24e-4: heights a centimetre apart all pass the gate, and any two of them swapped give another elevation.
ORDER_Z = np.array([0.0052, -0.0060, 0.0112, 0.0049, -0.0111, 0.0104, 0.0133], F32)


def order_cloud(L, z, seed=1370):
    rng = np.random.default_rng(seed)
    per = spread(rng, 20, top=1, cells=np.setdiff1d(np.arange(256), [ORDER_CELL])); per[ORDER_CELL] = 7
    return sweep(L, {ORDER_TILE: per, (1, 0): spread(rng, 12, top=2)}, rng, z={(ORDER_TILE, ORDER_CELL): z})


def order_ops(L=32):
    name = "light_order"
    if name not in _OPS:
        pre, a = order_cloud(L, np.zeros(7, F32), seed=1369), order_cloud(L, ORDER_Z)
        _OPS[name] = (adds([pre, a, a[::-1].copy(), a], every=2), pre, a)
    return (name,) + _OPS[name]


def cell_after(oracle_mod, L, pre, cloud, cell):
    o = oracle_mod.OracleMap(L, RES)
    o.add(frame_at(), pre)
    o.add(frame_at(), cloud)
    return o.layer("elevation").ravel()[cell].tobytes() + o.layer("variance").ravel()[cell].tobytes()


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_records_of_a_cell_arrive_out_of_order(oracle_mod, mode, track):
    L = 32
    name, ops, pre, a = order_ops(L)
    o = oracle_mod.OracleMap(L, RES)
    idx = np.asarray(o.process_points(frame_at(), a[:, 0], a[:, 1], a[:, 2])["index"])
    cell = (ORDER_TILE[0] * 16 + ORDER_CELL // 16) * L + ORDER_TILE[1] * 16 + ORDER_CELL % 16
    at = np.flatnonzero(idx == cell)
    assert at.size == 7 and np.all(np.diff(at) > 256), at                               # seven binning blocks: no two in one wave
    assert np.array_equal(a[at, 2], ORDER_Z)
    per, top = tile_counts(oracle_mod, L, a)
    assert per[ORDER_TILE] == 27 and top == 7
    # the order decides: the oracle's own result for the cell changes when any two of its records are swapped
    base = cell_after(oracle_mod, L, pre, a, cell)
    seen = {base}
    for i, j in itertools.combinations(range(7), 2):
        z = ORDER_Z.copy(); z[[i, j]] = z[[j, i]]
        swapped = cell_after(oracle_mod, L, pre, order_cloud(L, z), cell)
        assert swapped != base, (i, j)
        seen.add(swapped)
    assert len(seen) == 22, len(seen)                                                   # 21 swaps, 21 other results
    gpu, _ = run(oracle_mod, name, L, ops, mode, track)
    check_stays(gpu, mode)
    gpu.close()


# ---- 4. a cell of 8 in a tile of exactly 64: the general path's slow path ---------------------------------------------------------
def eight_ops(L):
    name = f"light_eight{L}"
    if name not in _OPS:
        rng = np.random.default_rng(1400 + L)
        tile = (1, 1)
        def light():
            return sweep(L, {(0, 0): spread(rng, 30, top=2), tile: spread(rng, 17, top=1, cells=inside(L, tile)), (1, 0): spread(rng, 9, top=3)}, rng)
        cells = inside(L, tile)
        per = np.zeros(256, np.int64); per[cells[3]] = 8; per[rng.permutation(cells[4:])[:56]] = 1
        heavy = sweep(L, {tile: per, (0, 0): spread(rng, 40, top=2)}, rng)
        ops = [("add", frame_at(), light()), ("add", frame_at(), heavy), ("check",), ("add", frame_at(), light()), ("add", frame_at(), light()), ("check",)]
        _OPS[name] = (ops, heavy, tile)
    return (name,) + _OPS[name]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [32, 40])
def test_cell_of_eight_in_a_tile_of_64(oracle_mod, L, mode, track):
    name, ops, heavy, tile = eight_ops(L)
    per, top = tile_counts(oracle_mod, L, heavy)
    assert per[tile] == 64 and per.max() == 64 and top == 8, (per, top)
    gpu, _ = run(oracle_mod, name, L, ops, mode, track)
    lean, generic, seen = gpu.debug_get("frame_lean_launches"), gpu.debug_get("frame_generic_launches"), gpu.debug_get("frame_form_seen")
    assert seen == 1, seen                                                              # the slow path reports in every mode
    if mode == 0:
        assert lean == 0
    elif mode == 1:
        assert generic == 0 and lean > 0
    else:
        assert lean > 0 and generic >= 3, (lean, generic)   # behind the first synchronise: a binning, a k_frame and the fuse-only launch, generic
    gpu.close()


# ---- 5. a queued Mapvar_update in front of a frame of light tiles, then a plain frame --------------------------------------------
def pending_ops(L):
    name = f"light_pending{L}"
    if name not in _OPS:
        rng = np.random.default_rng(1430 + L)
        n = tpr_of(L)
        def light(k):
            return sweep(L, {(tr, tc): spread(rng, k + 3 * tr + tc, top=2, cells=inside(L, (tr, tc))) for tr in range(n) for tc in range(n)}, rng)
        clouds = [light(20), light(9), light(31), light(14), light(5)]
        ops = [("add", frame_at(), clouds[0]), ("add", frame_at(), clouds[1]), ("var", 3e-4), ("add", frame_at(), clouds[2]), ("check",),
               ("add", frame_at(), clouds[3]), ("var", 1e-4), ("var", 2e-4), ("add", frame_at(), clouds[4]), ("add", frame_at(), clouds[0]), ("check",)]
        _OPS[name] = (ops, clouds)
    return (name,) + _OPS[name]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [32, 40])
def test_pending_increment_in_front_of_light_tiles(oracle_mod, L, mode, track):
    name, ops, clouds = pending_ops(L)
    for cloud in clouds:
        per, top = tile_counts(oracle_mod, L, cloud)
        assert 0 < per.min() and per.max() <= 64 and top <= 7, (per, top)              # every tile of every frame is light
    gpu, _ = run(oracle_mod, name, L, ops, mode, track)
    check_stays(gpu, mode)
    gpu.close()


# ---- 6. light, heavy, light through the same pass-buffer set ---------------------------------------------------------------------
def stale_ops(L=40):
    name = "light_stale"
    if name not in _OPS:
        rng = np.random.default_rng(1460)
        target, other = (1, 1), (0, 2)
        first = sweep(L, {target: spread(rng, 40, top=2)}, rng)
        heavy = sweep(L, {target: spread(rng, 600)}, rng)
        three = np.zeros(256, np.int64); three[[5, 130, 255]] = 1
        few = sweep(L, {target: three}, rng)
        fill = sweep(L, {other: spread(rng, 30, top=1, cells=inside(L, other))}, rng)
        # the pass buffers are double-buffered: frames two apart share a bucket, whose slots behind the count keep the older records
        _OPS[name] = (adds([first, fill, heavy, fill, few, fill, first[::-1].copy(), few], every=1), target, first, heavy, few)
    return (name,) + _OPS[name]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_light_heavy_light_in_one_bucket(oracle_mod, mode, track):
    name, ops, target, first, heavy, few = stale_ops()
    assert [int(tile_counts(oracle_mod, 40, c)[0][target]) for c in (first, heavy, few)] == [40, 600, 3]
    gpu, _ = run(oracle_mod, name, 40, ops, mode, track)
    check_stays(gpu, mode)
    gpu.close()
    # ... and with the k_frame launches fusing (a check behind every second frame only)
    ops2 = [op for i, op in enumerate(ops) if not (op[0] == "check" and i % 4 == 1)]
    gpu, _ = run(oracle_mod, name + "_pairs", 40, ops2, mode, track)
    check_stays(gpu, mode)
    gpu.close()


# ---- 7. a moved map: light tiles on either side of the wrap -----------------------------------------------------------------------
MOVES = {"first": (6.4, 6.4, 0.0), "last": (7.2, 7.2, 0.0)}          # start index 128 / 112: whole tiles, the buffer's wrap between two of them


def moved_ops(where, L=256):
    name = f"light_moved_{where}"
    if name not in _OPS:
        rng = np.random.default_rng(1490 + len(where))
        pos = MOVES[where]
        o = oracle.OracleMap(L, RES)
        start = int(o.move(pos)[1][0])
        g = ((L - 16 - start) % L) // 16 + 1           # geographic tiles g - 1 and g land in the buffer's last and first tile row / column
        tiles = {(g - 1, g - 1): spread(rng, 20, top=3), (g, g): spread(rng, 64, top=7), (g - 1, g): spread(rng, 7, top=7), (g, g - 1): spread(rng, 33, top=2),
                 (g + 3, g - 4): spread(rng, 40, top=1)}
        a = sweep(L, tiles, rng, centre=pos)
        ops = [("move", pos), ("add", frame_at(), a), ("add", frame_at(), a[::-1].copy()), ("check",), ("add", frame_at(), a), ("check",)]
        _OPS[name] = (ops, pos, a)
    return (name,) + _OPS[name]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("where", ["first", "last"])
def test_moved_map_light_tiles_across_the_wrap(oracle_mod, where, mode, track):
    L = 256
    name, ops, pos, a = moved_ops(where)
    o = oracle_mod.OracleMap(L, RES)
    _, start, _ = o.move(pos)
    centre_tile = [((L // 2 + int(s)) % L) >> 4 for s in start]
    assert centre_tile == ([0, 0] if where == "first" else [15, 15]), (start, centre_tile)
    per, top = tile_counts(oracle_mod, L, a, pos)
    assert per.sum() == 20 + 64 + 7 + 33 + 40 and per.max() == 64 and top <= 7
    rows, cols = np.nonzero((per > 0) & (per != 40))
    # the four light tiles sit on either side of the buffer's wrap, in rows and in columns
    assert rows.size == 4 and {int(rows.min()), int(rows.max())} == {0, 15} == {int(cols.min()), int(cols.max())}, (rows, cols)
    gpu, _ = run(oracle_mod, name, L, ops, mode, track)
    check_stays(gpu, mode)
    gpu.close()


# ---- 8. the stamp buffer on, on a frame of light tiles only ------------------------------------------------------------------------
def test_stamped_kernel_on_light_tiles(oracle_mod):
    L = 32
    rng = np.random.default_rng(1520)
    want = {(0, 0): 1, (0, 1): 20, (1, 0): 64, (1, 1): 33}
    clouds = [sweep(L, {t: spread(rng, n) for t, n in want.items()}, rng) for _ in range(2)]
    per, top = tile_counts(oracle_mod, L, clouds[0])
    assert all(per[t] == n for t, n in want.items()) and top <= 7
    ops = [("add", frame_at(), clouds[0]), ("add", frame_at(), clouds[1]), ("stamps",), ("check",)]
    gpu, rows = run(oracle_mod, "light_stamped", L, ops, 2, True, stamps=True)
    # rows [0, 4): the tiles of the last k_frame (the fuse of the first frame), then its binning blocks
    assert rows is not None and rows.shape[0] >= 4, None if rows is None else rows.shape
    tiles = rows[:4]
    assert np.all(tiles[:, 15] > 0) and np.all((tiles[:, :6] > 0).sum(1) == 6) and np.all((tiles[:, :12] > 0).sum(1) == 6), tiles
    assert np.all(np.diff(tiles[:, :6].astype(np.int64), axis=1) >= 0), tiles
    assert np.all(tiles[:, 12] > 0) and np.all(tiles[:, 13] >= tiles[:, 12]), tiles
    check_stays(gpu, 2)
    gpu.close()


# ---- 9. the C2 stream of bench.py ----------------------------------------------------------------------------------------------
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
