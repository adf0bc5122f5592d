"""frame_tile's owner phase sized by the wave's largest record count (no record: skipped; 1: no key; 2: one exchange; 3-4: the
4-key network; 5-7: the 8-key network), the lean production kernel without stamps and the stamped diagnostic kernel -- against the
CPU oracle, bit for bit: elevation and variance, plus lowest when it is tracked.  Every stream runs with "frame_lean" = 0, 1 and 2,
with and without lowest tracking; the oracle runs each stream once.

The clouds are BUILT on a 32 x 32 map at 0.05 m (2 x 2 tiles; a wave owns 64 consecutive cells of a tile): a point is put at the
centre of a chosen cell (sensor pose = identity), record k of every cell lies in block k of the sweep, the blocks are padded to whole
binning blocks (256 points) with points outside the map -- so the records of a cell come from different 64-point units of different
binning blocks, and the order a bucket is filled in is not the order of the point indices.  A second sweep lists the same cloud
backwards.  What a stream says about itself (records per cell, per wave, per tile) is asserted from the oracle's own projection.
- classes: one tile whose waves have largest counts (0, 1, 2, 7), one with (3, 4, 5, 6), one with a single record in all 256
  cells, one whose waves sit on the class boundaries: a single cell of 2 among cells of 1, of 3 among <= 2, of 5 among <= 4, and a
  single cell of 4 among cells of <= 1 (lanes far below the wave's class);
- rank rounds: tiles of 255, 256, 257 and 300 records;
- a two-record cell whose second record the Mahalanobis test rejects;
- queued variance increments in front of sweeps that leave waves of a live tile without a record (the skipped owner phase): on a
  fresh map the initial cells do not take the increment, later every cell of such a wave does;
- three frames with the stamp buffer on ("dbg_frame"): the maps of the same stream with it off, and non-zero stamp rows -- the
  production lean kernel carries no stamp code, so the stamped kernel is what ran."""
import ctypes as C

import numpy as np
import pytest

from gem_amd import ElevationMap, SensorModel, synth

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
F32 = np.float32
L, RES = 32, 0.05
MODES = [0, 1, 2]
_REF = {}                                              # stream name -> the oracle's snapshots (computed once, never modified)
_OPS = {}                                              # stream name -> its ops (built once)


def frame_at():
    return synth._frame_for(synth.pose_matrix(0.0, 0.0, 0.0, yaw=0.0), SensorModel.velodyne())


def cell_points(rows, cols, z):
    """one point at the centre of each cell (rows[i], cols[i]) of the unmoved map (GPU:340-348: an even L truncates L/2 - shift/res)"""
    rows, cols = np.asarray(rows, np.float64), np.asarray(cols, np.float64)
    c = np.zeros((rows.size, 4), F32)
    c[:, 0] = (L // 2 - rows - 0.5) * RES
    c[:, 1] = (L // 2 - cols - 0.5) * RES
    c[:, 2] = z
    c[:, 3] = 1.0
    return c


def outside(n):
    c = np.zeros((n, 4), F32)
    c[:, 0] = 500.0; c[:, 1] = 500.0; c[:, 3] = 1.0
    return c


def sweep(per, rng, z=None):
    """per[4][256]: records per cell of tile t = 2 tr + tc.  Block k of the sweep holds record k of every cell that has one, the
    cells shuffled, padded to whole binning blocks with points outside the map.  z(t, cell, k) -> height, default N(0.02 k, 0.1)."""
    per = np.asarray(per)
    parts = []
    for k in range(int(per.max())):
        t, cell = np.nonzero(per > k)
        p = rng.permutation(t.size)
        t, cell = t[p], cell[p]
        zz = rng.normal(0.02 * k, 0.1, t.size).astype(F32) if z is None else np.array([z(a, b, k) for a, b in zip(t, cell)], F32)
        parts.append(cell_points((t // 2) * 16 + cell // 16, (t % 2) * 16 + cell % 16, zz))
        parts.append(outside(-t.size % 256 + 256))
    return np.concatenate(parts).astype(F32)


def projection(oracle_mod, cloud):
    o = oracle_mod.OracleMap(L, RES)
    return o.process_points(frame_at(), cloud[:, 0], cloud[:, 1], cloud[:, 2])


def per_of(oracle_mod, cloud):
    """records per (tile, cell) of a sweep, from the oracle's projection"""
    idx = np.asarray(projection(oracle_mod, cloud)["index"])
    idx = idx[idx >= 0]
    r, c = idx // L, idx % L
    per = np.zeros((4, 256), np.int64)
    np.add.at(per, ((r >> 4) * 2 + (c >> 4), (r & 15) * 16 + (c & 15)), 1)
    return per


def wave_max(per):
    return per.reshape(4, 4, 64).max(2)


def assert_units_apart(oracle_mod, cloud):
    """the records of every cell with more than one lie in different binning blocks (256 points)"""
    idx = np.asarray(projection(oracle_mod, cloud)["index"])
    for cell in np.unique(idx[idx >= 0]):
        at = np.flatnonzero(idx == cell)
        assert np.unique(at // 256).size == at.size, (cell, at)


def reference(oracle_mod, name, ops):
    if name not in _REF:
        ref = oracle_mod.OracleMap(L, RES)
        snaps = [{n: ref.layer(n).copy() for n in ("elevation", "variance", "lowest")}]
        for op in ops:
            if op[0] == "add":
                ref.add(op[1], op[2])
            elif op[0] == "var":
                ref.mapvar_update(op[1])
            elif op[0] == "check":
                snaps.append({n: ref.layer(n).copy() for n in ("elevation", "variance", "lowest")})
        _REF[name] = snaps
    return _REF[name]


def run(oracle_mod, name, ops, mode, track, stamps=False):
    """The stream on the device with "frame_lean" = mode; ("check",) compares with the oracle's snapshot.  Returns (map, layers at
    the last check, stamp rows or None)."""
    import torch
    from gem_amd import _lib
    snaps = reference(oracle_mod, name, ops)
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
    k, last, rows = 0, None, None
    for op in ops:
        if op[0] == "add":
            gpu.add(op[1], dev[id(op[2])])
        elif op[0] == "var":
            gpu.mapvar_update(op[1])
        elif op[0] == "sync":
            gpu.synchronize()
        elif op[0] == "stamps":                        # the rows of the last k_frame launch (the read switches the stamps off)
            buf = np.zeros((256, 16), np.uint64)
            n = lib.gem_debug_fuse_stamps(gpu._h, 0, buf.ctypes.data_as(C.c_void_p), 256)
            rows = buf[:n].copy()
        elif op[0] == "check":
            k += 1
            last = {}
            for n in ("elevation", "variance") + (("lowest",) if track else ()):
                g, o = gpu.layer(n), snaps[k][n]
                assert np.array_equal(g, o), f"{name}, mode {mode}, check {k}: {n} differs in {np.count_nonzero(g != o)} cells"
                last[n] = g
    return gpu, last, rows


def check_stays(gpu, mode):
    """a stream that never needs the slow path: mode 0 launches the generic form only, modes 1 and 2 the lean form only"""
    lean, generic, seen = gpu.debug_get("frame_lean_launches"), gpu.debug_get("frame_generic_launches"), gpu.debug_get("frame_form_seen")
    assert seen == 0, seen
    if mode == 0:
        assert lean == 0 and generic > 0, (lean, generic)
    else:
        assert generic == 0 and lean > 0, (lean, generic)


def mix(rng, top, least=0):
    """64 counts in [least, top], every value present, shuffled over the lanes"""
    v = least + np.arange(64) % (top - least + 1)
    return rng.permutation(v)


def one_above(rng, high, top, least=0):
    """64 counts in [least, top] and a single lane of `high`"""
    v = mix(rng, top, least)
    v[rng.integers(0, 64)] = high
    return v


# ---- 1. the classes and their boundaries ----------------------------------------------------------------------------------------
def classes_per():
    rng = np.random.default_rng(81)
    per = np.zeros((4, 4, 64), np.int64)
    per[0] = [np.zeros(64, np.int64), mix(rng, 1), mix(rng, 2), mix(rng, 7)]
    per[1] = [mix(rng, 3), mix(rng, 4), mix(rng, 5), mix(rng, 6)]
    per[2] = 1                                                     # every wave: count 1 in every lane, no key at all
    per[3] = [one_above(rng, 2, 1, least=1), one_above(rng, 3, 2), one_above(rng, 5, 4), one_above(rng, 4, 1)]
    return per.reshape(4, 256)


def classes_ops():
    if "classes" not in _OPS:
        rng = np.random.default_rng(82)
        per = classes_per()
        a, b = sweep(per, rng), sweep(per, rng)
        _OPS["classes"] = ([("add", frame_at(), a), ("add", frame_at(), a[::-1].copy()), ("var", 2e-4), ("add", frame_at(), b),
                            ("sync",), ("check",)], per)
    return _OPS["classes"]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_every_class_and_boundary(oracle_mod, mode, track):
    ops, per = classes_ops()
    for op in ops:
        if op[0] == "add":
            got = per_of(oracle_mod, op[2])
            assert np.array_equal(got, per)
            assert_units_apart(oracle_mod, op[2])
    wm = wave_max(per)
    assert wm[0].tolist() == [0, 1, 2, 7] and wm[1].tolist() == [3, 4, 5, 6] and wm[2].tolist() == [1, 1, 1, 1] and wm[3].tolist() == [2, 3, 5, 4]
    w = per.reshape(4, 4, 64)
    assert (w[3, 0] == 2).sum() == 1 and (w[3, 1] == 3).sum() == 1 and (w[3, 2] == 5).sum() == 1 and (w[3, 3] == 4).sum() == 1   # one cell decides the class
    assert np.sort(w[3, 3])[-2] <= 1 and (w[0, 2] < 2).any() and (w[1, 1] < 3).any()       # lanes below the wave's class
    gpu, _, _ = run(oracle_mod, "classes", ops, mode, track)
    check_stays(gpu, mode)
    gpu.close()


# ---- 2. all records of a tile in one cell of one wave; the other waves hold none ------------------------------------------------
def single_ops():
    if "single" not in _OPS:
        rng = np.random.default_rng(83)
        pers = []
        for n in (1, 2, 3, 4, 5, 7):                               # every class, a lone cell: all other lanes hold nothing
            per = np.zeros((4, 256), np.int64)
            per[0, 64 * 2 + 17] = n; per[3, 5] = 1
            pers.append(per)
        ops = [("add", frame_at(), sweep(p, rng)) for p in pers] + [("sync",), ("check",)]
        _OPS["single"] = (ops, pers)
    return _OPS["single"]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_all_zero_but_one_cell(oracle_mod, mode, track):
    ops, pers = single_ops()
    for op, per in zip(ops, pers):
        assert np.array_equal(per_of(oracle_mod, op[2]), per)
    gpu, _, _ = run(oracle_mod, "single", ops, mode, track)
    check_stays(gpu, mode)
    gpu.close()


# ---- 3. rank rounds: tiles around 256 records -----------------------------------------------------------------------------------
def ranks_ops():
    if "ranks" not in _OPS:
        rng = np.random.default_rng(84)
        per = np.zeros((4, 256), np.int64)
        for t, n in enumerate((255, 256, 257, 300)):
            np.add.at(per[t], rng.permutation(256 * 2)[:n] % 256, 1)       # n records over the tile's cells, at most 2 per cell
        a, b = sweep(per, rng), sweep(per[::-1], rng)
        _OPS["ranks"] = ([("add", frame_at(), a), ("add", frame_at(), b), ("add", frame_at(), a[::-1].copy()), ("sync",), ("check",)], per)
    return _OPS["ranks"]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_tiles_around_256_records(oracle_mod, mode, track):
    ops, per = ranks_ops()
    assert per.sum(1).tolist() == [255, 256, 257, 300] and per.max() <= 2
    assert np.array_equal(per_of(oracle_mod, ops[0][2]), per) and np.array_equal(per_of(oracle_mod, ops[1][2]), per[::-1])
    gpu, _, _ = run(oracle_mod, "ranks", ops, mode, track)
    check_stays(gpu, mode)
    gpu.close()


# ---- 4. a Mahalanobis-rejected record in a two-record cell ----------------------------------------------------------------------
MAHAL_CELL = (1, 64 + 9)                                           # tile 1, wave 1


def mahal_ops():
    if "mahal" not in _OPS:
        rng = np.random.default_rng(85)
        per1 = np.zeros((4, 256), np.int64); per1[MAHAL_CELL] = 1; per1[2, :40] = 1
        per2 = per1.copy(); per2[MAHAL_CELL] = 2
        z = lambda t, cell, k: (-0.7 if k == 1 else 0.01) if (t, cell) == MAHAL_CELL else 0.05 * ((cell % 7) - 3)
        _OPS["mahal"] = ([("add", frame_at(), sweep(per1, rng, z)), ("sync",), ("check",),
                          ("add", frame_at(), sweep(per2, rng, z)), ("add", frame_at(), sweep(per1, rng, z)), ("sync",), ("check",)], per2)
    return _OPS["mahal"]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_rejected_record_in_a_two_record_cell(oracle_mod, mode, track):
    ops, per2 = mahal_ops()
    assert np.array_equal(per_of(oracle_mod, ops[3][2]), per2) and wave_max(per2)[1, 1] == 2
    snaps = reference(oracle_mod, "mahal", ops)
    t, cell = MAHAL_CELL
    r, c = (t // 2) * 16 + cell // 16, (t % 2) * 16 + cell % 16
    # in front of the second sweep the cell holds e ~ 0.01 with variance s1; the sweep's first record (0.01) can only shrink s, so the
    # second (-0.7) is at least 0.6 / sqrt(s1) deviations out: beyond the threshold of 5.  An outlier BELOW the cell is dropped
    # (GPU:505-507; one above would replace it): the oracle kept the elevation where it was.
    e1, s1 = float(snaps[1]["elevation"][r, c]), float(snaps[1]["variance"][r, c])
    assert abs(e1 - 0.01) < 1e-3 and 0.6 / np.sqrt(s1) > 5.0, (e1, s1)
    assert abs(float(snaps[2]["elevation"][r, c]) - 0.01) < 0.05, snaps[2]["elevation"][r, c]
    gpu, _, _ = run(oracle_mod, "mahal", ops, mode, track)
    check_stays(gpu, mode)
    gpu.close()


# ---- 5. a queued increment on waves without a record: the skipped owner phase ---------------------------------------------------
def pending_ops():
    if "pending" not in _OPS:
        rng = np.random.default_rng(86)
        per1 = np.zeros((4, 256), np.int64)
        per1[0, 64:128] = mix(rng, 1); per1[0, 128:192] = mix(rng, 2); per1[0, 192:] = 1; per1[3, :64] = 1
        per2 = np.zeros((4, 256), np.int64)
        per2[0, 192:] = mix(rng, 3)                                # tile 0 is live, its waves 0, 1, 2 hold no record
        per3 = np.zeros((4, 256), np.int64)
        per3[3, 200:230] = 1
        _OPS["pending"] = ([("var", 5e-4), ("add", frame_at(), sweep(per1, rng)), ("sync",), ("check",), ("var", 3e-4),
                            ("add", frame_at(), sweep(per2, rng)), ("add", frame_at(), sweep(per3, rng)), ("sync",), ("check",)], (per1, per2, per3))
    return _OPS["pending"]


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_pending_increment_on_waves_without_a_record(oracle_mod, mode, track):
    ops, (per1, per2, per3) = pending_ops()
    for i, per in ((1, per1), (5, per2), (6, per3)):
        assert np.array_equal(per_of(oracle_mod, ops[i][2]), per)
    assert wave_max(per1)[0].tolist() == [0, 1, 2, 1] and wave_max(per2)[0].tolist() == [0, 0, 0, 3]
    snaps = reference(oracle_mod, "pending", ops)
    v1, v2 = snaps[1]["variance"][:16, :16].reshape(256), snaps[2]["variance"][:16, :16].reshape(256)
    floor = F32(1e-4)
    # the first increment meets a map of initial cells: it is applied nowhere -- the cells of tile 0 without a record (all of wave 0,
    # part of waves 1 and 2) leave the first fuse at the variance floor, not at floor + 5e-4
    blank = per1[0] == 0
    assert blank[:64].all() and blank.sum() > 80 and np.all(v1[blank] == floor), np.unique(v1[blank])
    assert np.all(v1[~blank] > floor)
    # the second one meets tile 0 with records in wave 3 only: every cell of waves 0, 1, 2 -- fused before or at the floor -- gets it
    quiet = np.arange(256) < 192
    assert (quiet & ~blank).sum() > 60 and np.array_equal(v2[quiet], (v1[quiet] + F32(3e-4)).astype(F32))
    gpu, _, _ = run(oracle_mod, "pending", ops, mode, track)
    check_stays(gpu, mode)
    gpu.close()


# ---- 6. the stamp buffer on: the stamped kernel runs, the maps are the same -----------------------------------------------------
@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_stamp_buffer_on_gives_the_same_maps_and_stamps(oracle_mod, mode, track):
    base, per = classes_ops()
    plain = base[:4] + [("sync",), ("check",)]                     # three frames (and the queued increment)
    stamped = base[:4] + [("stamps",), ("sync",), ("check",)]
    off, layers_off, _ = run(oracle_mod, "classes", plain, mode, track)
    on, layers_on, rows = run(oracle_mod, "classes", stamped, mode, track, stamps=True)
    for n in layers_off:
        assert np.array_equal(layers_off[n], layers_on[n]), n
    # rows [0, 4): the tiles of the last k_frame (fuse of the second frame: every tile holds records), then its binning blocks
    nbin = (base[3][2].shape[0] // 64 + 3) // 4                   # (at least: the unit count of a pass is padded)
    assert rows is not None and rows.shape[0] >= 4 + nbin, (None if rows is None else rows.shape, nbin)
    tiles, bins = rows[:4], rows[4:]
    assert np.all(tiles[:, 15] > 0) and np.all(tiles[:, 0] > 0) and np.all(tiles[:, 12] > 0) and np.all(tiles[:, 13] >= tiles[:, 12]), tiles
    assert np.all((tiles[:, :6] > 0).sum(1) == 6), tiles           # start, loads, arrival, ranked, chains, stores
    assert np.all(bins[:, 15] > 0) and np.all(bins[:, 0] > 0) and np.all(bins[:, 1] > 0), bins
    check_stays(on, mode); check_stays(off, mode)
    on.close(); off.close()
