"""k_frame's lean form from its own argument block (gem_frame_lean.hpp) against the CPU oracle, bit for bit: elevation and variance,
plus lowest when it is tracked.  Every stream runs with "frame_lean" = 0 (always generic), 1 (always lean) and 2 (the host's
choice), with and without lowest tracking; the oracle runs each stream once.

The clouds are BUILT, not drawn: a point is put into a chosen cell (its centre, sensor pose = identity), and what the test says
about a stream -- records per tile, records per cell, which tiles are touched -- is asserted from the oracle's own projection.
- every tile touched once, again after a move that makes the circular-buffer start and the centre tile non-zero: the multiply-high
  division of the block -> tile map, the fields of the tile half;
- for every m in 1..7 a wave (64 consecutive cells of a tile) whose cells hold 1..m records, the points of a cell in 64-point
  units far apart in the sweep and in descending order of arrival: the owner's key gather and its sort decide the result;
- tiles of exactly 255, 256, 257, 511, 512, 513, 767 and 768 records: the three rank rows, the second DMA round;
- a cell of 8 records in a light tile: the slow path gives the oracle's map and the handle leaves the lean form;
- the scalars that moved into the block: queued Mapvar_update increments (1 and 4), the reject filter, a row strip, a height window
  that rejects part of the sweep, kept h == -1 sentinels with lowest tracking.
Maps: L = 75 @ 0.2 m (25 tiles, padded tile blocks, edge tiles) and L = 160 @ 0.1 m (100 tiles, the run permutation)."""
import numpy as np
import pytest

from gem_amd import ElevationMap, RejectFilter, SensorModel, synth

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
F32 = np.float32
MODES = [0, 1, 2]
MAPS = [(75, 0.2), (160, 0.1)]
_REF = {}                                              # stream name -> the oracle's snapshots (computed once, never modified)


def frame_at(x=0.0, y=0.0, yaw=0.0, flt=None):
    return synth._frame_for(synth.pose_matrix(x, y, 0.0, yaw=yaw), SensorModel.velodyne(), flt)


def cell_points(L, res, rows, cols, rng, z=None):
    """one point at the centre of each (geographic) cell (rows[i], cols[i]) of an unmoved map, sensor pose = identity"""
    rows, cols = np.asarray(rows, np.float64), np.asarray(cols, np.float64)
    off = 0.5 if L % 2 == 0 else 0.0                   # GPU:340-348: even L truncates L/2 - shift/res, odd L rounds shift/res
    c = np.zeros((rows.size, 4), F32)
    c[:, 0] = (L // 2 - rows - off) * res
    c[:, 1] = (L // 2 - cols - off) * res
    c[:, 2] = rng.normal(0.0, 0.15, rows.size) if z is None else z
    c[:, 3] = 1.0
    return c


def projection(oracle_mod, L, res, frame, cloud, moves=()):
    o = oracle_mod.OracleMap(L, res)
    for p in moves:
        o.move(p)
    return np.asarray(o.process_points(frame, cloud[:, 0], cloud[:, 1], cloud[:, 2])["index"])


def tile_and_cell_counts(L, idx):
    idx = idx[idx >= 0]
    tpr = (L + 15) // 16
    tiles = (idx // L >> 4) * tpr + (idx % L >> 4)
    return np.bincount(tiles, minlength=tpr * tpr), np.bincount(idx, minlength=L * L)


def assert_fast(oracle_mod, L, res, ops):
    """every sweep of the stream stays on the fast path: no tile above 768 records, no cell above 7"""
    moves = []
    for op in ops:
        if op[0] == "move":
            moves.append(op[1])
        elif op[0] == "add":
            t, c = tile_and_cell_counts(L, projection(oracle_mod, L, res, op[1], op[2], moves))
            assert t.max() <= 768 and c.max() <= 7, (t.max(), c.max())


def reference(oracle_mod, name, L, res, ops):
    if name not in _REF:
        ref = oracle_mod.OracleMap(L, res)
        snaps = [{"lowest": ref.layer("lowest").copy()}]
        for op in ops:
            if op[0] == "add":
                ref.add(op[1], op[2])
            elif op[0] == "var":
                ref.mapvar_update(op[1])
            elif op[0] == "move":
                ref.move(op[1])
            elif op[0] == "check":
                snaps.append({n: ref.layer(n).copy() for n in ("elevation", "variance", "lowest")})
        _REF[name] = snaps
    return _REF[name]


def run(oracle_mod, name, L, res, ops, mode, track, strip=None):
    """The stream on the device with "frame_lean" = mode; ("check",) compares with the oracle's snapshot (inside the strip, when
    the handle owns one: nothing outside it may be written)."""
    import torch
    snaps = reference(oracle_mod, name, L, res, ops)
    gpu = ElevationMap(L, res, debug={"frame_lean": mode}, **({"strip": (strip[0], strip[1] - strip[0])} if strip else {}))
    if track:
        gpu.set_lowest_tracking(True)
        gpu.set_layer("lowest", snaps[0]["lowest"])    # the oracle always tracks: start both from the same layer
    dev = {id(op[2]): torch.from_numpy(op[2]).cuda() for op in ops if op[0] == "add"}
    torch.cuda.synchronize()
    k = 0
    for op in ops:
        if op[0] == "add":
            gpu.add(op[1], dev[id(op[2])])
        elif op[0] == "var":
            gpu.mapvar_update(op[1])
        elif op[0] == "move":
            gpu.move(op[1])
        elif op[0] == "sync":
            gpu.synchronize()
        elif op[0] == "check":
            k += 1
            for n in ("elevation", "variance") + (("lowest",) if track else ()):
                g, o = gpu.layer(n), snaps[k][n]
                if strip:
                    # outside the strip every layer is what it started as (lowest is indexed by the geographic cell: the strip
                    # streams do not move the map, so its rows are the storage rows)
                    init = snaps[0]["lowest"] if n == "lowest" else np.full_like(g, -10)
                    out = np.s_[strip[0]:strip[1]]
                    assert np.array_equal(np.delete(g, out, axis=0), np.delete(init, out, axis=0)), f"{name}, mode {mode}: {n} written outside the strip"
                    g, o = g[strip[0]:strip[1]], o[strip[0]:strip[1]]
                assert np.array_equal(g, o), f"{name}, mode {mode}, check {k}: {n} differs in {np.count_nonzero(g != o)} cells"
    return gpu


def counts(gpu):
    return gpu.debug_get("frame_lean_launches"), gpu.debug_get("frame_generic_launches"), gpu.debug_get("frame_form_seen")


def check_stays(gpu, mode):
    """a stream that never needs the slow path: mode 0 launches the generic form only, modes 1 and 2 the lean form only"""
    lean, generic, seen = counts(gpu)
    assert seen == 0, seen
    if mode == 0:
        assert lean == 0 and generic > 0, (lean, generic)
    else:
        assert generic == 0 and lean > 0, (lean, generic)


# ---- 1. every tile touched once, before and after a move ----------------------------------------------------------------------------
_EVERY = {}


def every_tile_ops(oracle_mod, L, res):
    if L in _EVERY:
        return _EVERY[L]
    rng = np.random.default_rng(31 + L)
    tpr = (L + 15) // 16
    move = np.array([(L // 7) * res, -(L // 5) * res, 0.0], F32)   # a whole number of cells: start0 / start1 leave zero, the centre tile moves
    # every cell centre of the map, before and behind the move, and the storage cell the oracle puts it into
    gr, gc = np.divmod(np.arange(L * L), L)
    grid = cell_points(L, res, gr, gc, rng)
    moved = grid.copy(); moved[:, 0] += move[0]; moved[:, 1] += move[1]
    def sweep(cloud, moves):                           # one point per STORAGE tile, shuffled
        idx = projection(oracle_mod, L, res, frame_at(), cloud, moves)
        assert np.array_equal(np.sort(idx), np.arange(L * L))                 # (the centres cover the map, cell by cell)
        tile = (idx // L >> 4) * tpr + (idx % L >> 4)
        pick = np.array([rng.choice(np.flatnonzero(tile == t)) for t in range(tpr * tpr)])
        c = cloud[rng.permutation(pick)].copy()
        c[:, 2] = rng.normal(0.0, 0.15, c.shape[0])
        return c
    ops = [("add", frame_at(), sweep(grid, [])), ("add", frame_at(), sweep(grid, [])), ("sync",), ("check",),
           ("move", move), ("add", frame_at(), sweep(moved, [move])), ("add", frame_at(), sweep(moved, [move])), ("var", 2e-5),
           ("add", frame_at(), sweep(moved, [move])), ("sync",), ("check",)]
    _EVERY[L] = (ops, move)
    return _EVERY[L]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L,res", MAPS)
def test_every_tile_touched_once(oracle_mod, L, res, mode, track):
    ops, move = every_tile_ops(oracle_mod, L, res)
    moves = []
    for op in ops:                                     # every sweep, before and behind the move, puts one record into every tile
        if op[0] == "move":
            moves.append(op[1])
        elif op[0] == "add":
            t, _ = tile_and_cell_counts(L, projection(oracle_mod, L, res, op[1], op[2], moves))
            assert np.all(t == 1), t
    gpu = run(oracle_mod, f"every-tile-{L}", L, res, ops, mode, track)
    check_stays(gpu, mode)
    gpu.close()


# ---- 2. mixed record counts in one wave ---------------------------------------------------------------------------------------------
def mixed_ops(L, res, m):
    """Tile (1, 1): the wave of cells 64..127 (rows 4..7 of the tile) holds 1 + (lane mod m) records per cell.  The k-th record of
    a cell sits in unit block m - 1 - k of the sweep (blocks of 64 cells x 64 points apart, filler points between them), so the
    binning waves reserve the cell's records in an order that is not the order of the point indices."""
    rng = np.random.default_rng(40 + m + L)
    lanes = np.arange(64)
    per = 1 + lanes % m
    rows, cols = 16 + 4 + lanes // 16, 16 + lanes % 16
    tpr = (L + 15) // 16
    ftr, ftc = np.divmod(rng.integers(0, tpr * tpr, 64 * 40), tpr)                    # filler: a point here and there, far below any limit
    ok = ~((ftr == 1) & (ftc == 1))
    filler = cell_points(L, res, (ftr * 16 + rng.integers(0, 11, ftr.size))[ok], (ftc * 16 + rng.integers(0, 11, ftc.size))[ok], rng)
    parts, used = [], 0
    for k in range(m - 1, -1, -1):                                                    # block for record k of every cell that has one
        sel = per > k
        parts.append(cell_points(L, res, rows[sel], cols[sel], rng, z=rng.normal(0.02 * k, 0.1, int(sel.sum())).astype(F32)))
        parts.append(filler[used:used + 200]); used += 200
    cloud = np.concatenate(parts).astype(F32)
    ops = [("add", frame_at(), cloud), ("add", frame_at(), cloud[::-1].copy()), ("add", frame_at(), cloud), ("sync",), ("check",)]
    return ops, rows, cols, per


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6, 7])
def test_mixed_record_counts_in_one_wave(oracle_mod, m, mode, track):
    L, res = 160, 0.1
    ops, rows, cols, per = mixed_ops(L, res, m)
    idx = projection(oracle_mod, L, res, ops[0][1], ops[0][2])
    _, c = tile_and_cell_counts(L, idx)
    assert np.array_equal(c[rows * L + cols], per) and per.max() == m, (c[rows * L + cols], per)     # the wave holds 1..m per cell
    first = [np.flatnonzero(idx == r * L + cc)[0] // 64 for r, cc in zip(rows, cols)]
    last = [np.flatnonzero(idx == r * L + cc)[-1] // 64 for r, cc in zip(rows, cols)]
    if m > 1:
        assert max(np.subtract(last, first)) >= m - 1                                  # a cell's records come from different units
    assert_fast(oracle_mod, L, res, ops)
    gpu = run(oracle_mod, f"mixed-{m}", L, res, ops, mode, track)
    check_stays(gpu, mode)
    gpu.close()


# ---- 3. rank-row boundaries -----------------------------------------------------------------------------------------------------------
BOUNDARY = [255, 256, 257, 511, 512, 513, 767, 768]


def boundary_ops(L, res):
    """eight tiles of exactly 255 ... 768 records (at most three per cell), the rest of the map a point here and there"""
    rng = np.random.default_rng(50 + L)
    tpr = (L + 15) // 16
    tiles = [(1, 1), (1, 2), (2, 1), (2, 2), (0, 1), (1, 0), (2, 0), (0, 2)] if tpr < 8 else [(2, 2), (2, 5), (5, 2), (5, 5), (3, 3), (4, 6), (6, 4), (7, 7)]
    rows, cols = [], []
    for (tr, tc), n in zip(tiles, BOUNDARY):
        cell = np.arange(n) % 256                       # n records over the tile's 256 cells: 1..3 per cell
        rows.append(tr * 16 + cell // 16); cols.append(tc * 16 + cell % 16)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    def sweep():
        p = rng.permutation(rows.size)
        return cell_points(L, res, rows[p], cols[p], rng)
    ops = [("add", frame_at(), sweep()), ("add", frame_at(), sweep()), ("var", 1e-5), ("add", frame_at(), sweep()), ("sync",), ("check",)]
    return ops, tiles


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L,res", MAPS)
def test_rank_row_boundaries(oracle_mod, L, res, mode, track):
    ops, tiles = boundary_ops(L, res)
    tpr = (L + 15) // 16
    t, c = tile_and_cell_counts(L, projection(oracle_mod, L, res, ops[0][1], ops[0][2]))
    assert [int(t[tr * tpr + tc]) for tr, tc in tiles] == BOUNDARY and c.max() <= 3
    assert_fast(oracle_mod, L, res, ops)
    gpu = run(oracle_mod, f"boundary-{L}", L, res, ops, mode, track)
    check_stays(gpu, mode)
    gpu.close()


# ---- 4. a cell of 8 records: the slow path ----------------------------------------------------------------------------------------------
def cell8_ops(L, res):
    rng = np.random.default_rng(60 + L)
    tpr = (L + 15) // 16
    tr, tc = np.divmod(np.arange(tpr * tpr), tpr)
    def light():
        return cell_points(L, res, tr * 16 + rng.integers(0, 11, tr.size), tc * 16 + rng.integers(0, 11, tc.size), rng)
    wall = cell_points(L, res, np.full(8, 16 + 13), np.full(8, 32 + 13), rng, z=rng.normal(0.3, 0.05, 8).astype(F32))
    heavy = np.concatenate([light()[:10], wall[:4], light(), wall[4:], light()[:7]]).astype(F32)
    ops = [("add", frame_at(), light()), ("add", frame_at(), heavy), ("sync",), ("check",),
           ("add", frame_at(), light()), ("add", frame_at(), light()), ("sync",), ("check",)]
    return ops, heavy


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L,res", MAPS)
def test_cell_of_eight_takes_the_slow_path(oracle_mod, L, res, mode, track):
    ops, heavy = cell8_ops(L, res)
    t, c = tile_and_cell_counts(L, projection(oracle_mod, L, res, frame_at(), heavy))
    assert c.max() == 8 and t.max() <= 16, (c.max(), t.max())                           # one cell of 8 in a light tile
    gpu = run(oracle_mod, f"cell8-{L}", L, res, ops, mode, track)
    lean, generic, seen = counts(gpu)
    assert seen == 1, seen                                                              # the slow path reports in every mode
    if mode == 0:
        assert lean == 0
    elif mode == 1:
        assert generic == 0 and lean > 0
    else:
        assert lean > 0 and generic >= 3, (lean, generic)   # behind the first synchronise: a binning, a k_frame and the fuse-only launch, generic
    gpu.close()


# ---- 5. the scalars that moved into the block ---------------------------------------------------------------------------------------------
def scalar_sweeps(L, res, rng, n=3, z_sigma=0.15, per_tile=20):
    tpr = (L + 15) // 16
    tr, tc = np.divmod(np.repeat(np.arange(tpr * tpr), per_tile), tpr)
    out = []
    for _ in range(n):
        p = rng.permutation(tr.size)
        r, c = (tr * 16 + rng.integers(0, 11, tr.size))[p], (tc * 16 + rng.integers(0, 11, tc.size))[p]
        out.append(cell_points(L, res, r, c, rng, z=rng.normal(0.0, z_sigma, tr.size).astype(F32)))
    return out


def scalar_ops(kind, L, res):
    rng = np.random.default_rng(70 + L + sum(map(ord, kind)))
    if kind == "pending":                              # 1 and 4 queued increments in front of a frame
        s = scalar_sweeps(L, res, rng, 4)
        return [("add", frame_at(), s[0]), ("var", 3e-4), ("add", frame_at(), s[1]),
                ("var", 1e-4), ("var", 2e-4), ("var", 5e-5), ("var", 7e-4), ("add", frame_at(), s[2]), ("add", frame_at(), s[3]), ("sync",), ("check",)]
    if kind == "filter":                               # the reject filter: box +-1.5 m, band |y| < 1 m, plane y > 0
        f = frame_at(flt=RejectFilter.reference())
        return [("add", f, c) for c in scalar_sweeps(L, res, rng, 3)] + [("sync",), ("check",)]
    if kind == "window":                               # z in [-5, 0.8] (velodyne.yaml): a spread of 1 m rejects a fifth of the sweep
        return [("add", frame_at(), c) for c in scalar_sweeps(L, res, rng, 3, z_sigma=1.0)] + [("sync",), ("check",)]
    if kind == "sentinel":                             # h == -1 exactly: fused nowhere (GPU:482), seen by the lowest layer when it is tracked
        s = scalar_sweeps(L, res, rng, 3)
        for c in s:
            c[::5, 2] = -1.0
        return [("add", frame_at(), c) for c in s] + [("sync",), ("check",)]
    assert kind == "strip"
    return [("add", frame_at(), c) for c in scalar_sweeps(L, res, rng, 3)] + [("sync",), ("check",)]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L,res", MAPS)
@pytest.mark.parametrize("kind", ["pending", "filter", "window", "sentinel", "strip"])
def test_scalars_of_the_block(oracle_mod, kind, L, res, mode, track):
    ops = scalar_ops(kind, L, res)
    first = next(op for op in ops if op[0] == "add")
    idx = projection(oracle_mod, L, res, first[1], first[2])
    kept = np.count_nonzero(idx >= 0) / idx.size
    if kind in ("filter", "window"):
        assert 0.2 < kept < 0.9, kept                  # part of the sweep is rejected, part is not
    else:
        assert kept == 1.0, kept
    if kind == "sentinel":
        assert np.count_nonzero(first[2][:, 2] == -1.0) >= idx.size // 5
    assert_fast(oracle_mod, L, res, ops)
    strip = (L // 3 + 2, 2 * L // 3 + 5) if kind == "strip" else None                   # rows inside the map, not tile-aligned
    gpu = run(oracle_mod, f"scalar-{kind}-{L}", L, res, ops, mode, track, strip=strip)
    check_stays(gpu, mode)
    gpu.close()
