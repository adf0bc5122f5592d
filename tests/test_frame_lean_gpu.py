"""k_frame's two forms -- the generic one and the lean, bucket-only one the host picks while no tile has needed the slow path --
against the CPU oracle, bit for bit: elevation and variance, plus lowest when it is tracked.

Every stream runs with "frame_lean" = 0 (always generic: the kernel as it was), 1 (always lean) and 2 (the host's choice, the
default), with and without lowest tracking (k_frame<0, .> / <4, .>).  The oracle runs each stream once; the six variants compare
against the same snapshots.
- an ordinary stream of clean frames (no tile above 768 records, no cell above 7) stays lean from the first binning to the
  fuse-only launch at the synchronisation;
- geometry: edge tiles partly outside the map and padded tile blocks (L = 75), the XCD run permutation (100 tiles), a last binning
  block with idle waves (5 003 points), a sweep that leaves no record at all;
- the switch: a tile above 768 records (or a cell of 9) reports to the host, which launches the generic form from then on --
  exact wherever the switch falls, with and without a synchronisation behind the heavy frame;
- forced lean: overflowing frames on both buffer sets through the lean form's slow path, then clean frames (the counts and spill
  slots it leaves behind are clean).
"""
import numpy as np
import pytest

from gem_amd import ElevationMap, SensorModel, synth

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
F32 = np.float32
MODES = [0, 1, 2]
_REF = {}                                              # stream name -> the oracle's snapshots (computed once, never modified)


def blob(rng, n, cx, cy, half):
    c = np.zeros((n, 4), F32)
    c[:, 0] = rng.uniform(cx - half, cx + half, n)
    c[:, 1] = rng.uniform(cy - half, cy + half, n)
    c[:, 2] = rng.normal(0.0, 0.2, n)
    c[:, 3] = 1.0
    return c


def spread(rng, n, L, res):
    return blob(rng, n, 0.0, 0.0, 0.45 * L * res)


def frame_at(x=0.0, y=0.0, yaw=0.0):
    return synth._frame_for(synth.pose_matrix(x, y, 0.0, yaw=yaw), SensorModel.velodyne())


def loads(oracle_mod, L, res, frame, cloud, moves=()):
    """(most records in one 16x16 tile, most records in one cell, records) of a sweep, from the oracle's own projection into a
    fresh map moved as the stream's map was"""
    o = oracle_mod.OracleMap(L, res)
    for p in moves:
        o.move(p)
    idx = np.asarray(o.process_points(frame, cloud[:, 0], cloud[:, 1], cloud[:, 2])["index"])
    idx = idx[idx >= 0]
    if idx.size == 0:
        return 0, 0, 0
    tpr = (L + 15) // 16
    tiles = (idx // L >> 4) * tpr + (idx % L >> 4)
    return int(np.bincount(tiles).max()), int(np.bincount(idx).max()), int(idx.size)


def assert_clean(oracle_mod, L, res, ops):
    """every sweep of the stream stays on the fast path: no tile above 768 records, no cell above 7"""
    moves = []
    for op in ops:
        if op[0] == "move":
            moves.append(op[1])
        elif op[0] == "add":
            t, c, _ = loads(oracle_mod, L, res, op[1], op[2], moves)
            assert t <= 768 and c <= 7, (t, c)


def reference(oracle_mod, name, L, res, ops):
    """the oracle's layers at every ("check",) of the stream, and the lowest layer both maps start from"""
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


def run(oracle_mod, name, L, res, ops, mode, track):
    """The stream on the device with "frame_lean" = mode; ("check",) compares with the oracle's snapshot (a read: it flushes the
    deferred fuse), ("sync",) synchronises, ("probe", fn) calls fn(gpu).  Returns the map (open) for the caller's own probes."""
    import torch
    snaps = reference(oracle_mod, name, L, res, ops)
    gpu = ElevationMap(L, res, debug={"frame_lean": mode})
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
        elif op[0] == "probe":
            op[1](gpu)
        elif op[0] == "check":
            k += 1
            for n in ("elevation", "variance") + (("lowest",) if track else ()):
                g, o = gpu.layer(n), snaps[k][n]
                assert np.array_equal(g, o), f"{name}, mode {mode}, check {k}: {n} differs in {np.count_nonzero(g != o)} cells"
    return gpu


def counts(gpu):
    return gpu.debug_get("frame_lean_launches"), gpu.debug_get("frame_generic_launches"), gpu.debug_get("frame_form_seen")


def check_mode_counts(gpu, mode, clean):
    """what each mode may launch; `clean`: no sweep of the stream needed the slow path"""
    lean, generic, seen = counts(gpu)
    if mode == 0:
        assert lean == 0 and generic > 0, (lean, generic)
    elif mode == 1:
        assert generic == 0 and lean > 0, (lean, generic)
    elif clean:
        assert generic == 0 and lean > 0 and seen == 0, (lean, generic, seen)
    if clean:
        assert seen == 0, seen


# ---- 1. an ordinary stream --------------------------------------------------------------------------------------------------------
def ordinary_ops():
    L, res = 96, 0.1
    rng = np.random.default_rng(21)
    ops = []
    for k, n in enumerate((5000, 3000, 4000, 5003, 3500, 4500)):
        if k % 2 == 1:
            ops.append(("var", 1e-4 * k))
        if k == 2:
            ops.append(("var", 3e-5))
        if k in (3, 5):
            ops.append(("move", np.array([0.35 * k, -0.2 * k, 0.0], F32)))
        ops.append(("add", frame_at(0.05 * k, -0.03 * k, 0.1 * k), spread(rng, n, L, res)))
    ops += [("sync",), ("check",)]
    return L, res, ops


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_ordinary_stream(oracle_mod, mode, track):
    L, res, ops = ordinary_ops()
    assert_clean(oracle_mod, L, res, ops)
    gpu = run(oracle_mod, "ordinary", L, res, ops, mode, track)
    lean, generic, seen = counts(gpu)
    print("mode", mode, "lean launches", lean, "generic launches", generic, "form seen", seen)
    check_mode_counts(gpu, mode, clean=True)
    if mode == 2:
        assert generic == 0 and seen == 0 and lean >= 6, (lean, generic, seen)
    gpu.close()


# ---- 2. geometry edges ------------------------------------------------------------------------------------------------------------
def geometry_ops(L, res):
    rng = np.random.default_rng(22 + L)
    outside = blob(rng, 3000, 500.0, 500.0, 2.0)       # no point inside the map: every tile leaves with its speculative load in flight
    ops = [("add", frame_at(0.1, 0.0, 0.2), spread(rng, 5003, L, res)),     # 5 003 points: 79 units, a last binning block with an idle wave
           ("add", frame_at(0.1, 0.0, 0.2), spread(rng, 3000, L, res)),
           ("add", frame_at(), outside),
           ("add", frame_at(), outside),
           ("add", frame_at(-0.2, 0.1, -0.4), spread(rng, 5003, L, res)),
           ("var", 2e-5),
           ("add", frame_at(-0.2, 0.1, -0.4), spread(rng, 4000, L, res)),
           ("sync",), ("check",)]
    return ops, outside


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L,res", [(75, 0.2), (160, 0.1)])     # 25 tiles: edge tiles partly outside, padded tile blocks | 100 tiles: the XCD run permutation
def test_geometry_edges(oracle_mod, L, res, mode, track):
    ops, outside = geometry_ops(L, res)
    assert_clean(oracle_mod, L, res, ops)
    assert loads(oracle_mod, L, res, frame_at(), outside)[2] == 0
    assert loads(oracle_mod, L, res, ops[0][1], ops[0][2])[2] > 4000          # (the spread clouds do land in the map)
    gpu = run(oracle_mod, f"geometry{L}", L, res, ops, mode, track)
    check_mode_counts(gpu, mode, clean=True)
    gpu.close()


# ---- 3. the switch ----------------------------------------------------------------------------------------------------------------
SW_L, SW_RES = 96, 0.1


def heavy_cloud(rng, kind):
    if kind == "tile":                                  # a blob of 1.6 m: a tile above 768 records
        return blob(rng, 4000, 1.0, -0.7, 0.8), frame_at()
    c = spread(rng, 3000, SW_L, SW_RES)                 # a wall: nine records in one cell of a tile that stays far below 768
    w = blob(rng, 9, 0.73, 1.12, 0.002)
    w[:, 2] = rng.normal(0.5, 0.05, 9)
    return np.concatenate([c[:1000], w, c[1000:]]), frame_at(0.1, -0.2, 0.3)


def switch_ops(kind, mid_sync, probe=None):
    rng = np.random.default_rng(23)
    clean = [spread(rng, n, SW_L, SW_RES) for n in (4000, 3000, 5000, 3500, 4500, 3000)]
    hc, hf = heavy_cloud(rng, kind)
    ops = [("add", frame_at(), c) for c in clean[:3]]
    ops.append(("add", hf, hc))
    if mid_sync:
        ops += [("sync",), ("check",)]
        if probe:
            ops.append(("probe", probe))
    ops += [("add", frame_at(0.05, 0.0, 0.1), c) for c in clean[3:]]
    ops += [("sync",), ("check",)]
    return ops, clean, (hc, hf)


def assert_heavy(oracle_mod, kind, hc, hf, clean):
    t, c, _ = loads(oracle_mod, SW_L, SW_RES, hf, hc)
    if kind == "tile":
        assert t > 768, t
    else:
        assert t <= 768 and c >= 9, (t, c)
    for cl in clean:
        for f in (frame_at(), frame_at(0.05, 0.0, 0.1)):
            tt, cc, _ = loads(oracle_mod, SW_L, SW_RES, f, cl)
            assert tt <= 768 and cc <= 7, (tt, cc)


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["tile", "cell"])
def test_switch_with_a_synchronise(oracle_mod, kind, mode, track):
    at_sync = {}
    ops, clean, (hc, hf) = switch_ops(kind, True, probe=lambda g: at_sync.update(zip(("lean", "generic", "seen"), counts(g))))
    assert_heavy(oracle_mod, kind, hc, hf, clean)
    gpu = run(oracle_mod, f"switch-{kind}-sync", SW_L, SW_RES, ops, mode, track)
    lean, generic, seen = counts(gpu)
    print("mode", mode, "at the synchronise", at_sync, "at the end", (lean, generic, seen))
    check_mode_counts(gpu, mode, clean=False)
    assert at_sync["seen"] == 1 and seen == 1           # the slow path reports in every mode (the generic form's frame_tile too)
    if mode == 2:
        assert lean == at_sync["lean"], (lean, at_sync)                  # every launch behind the synchronise is generic:
        assert generic >= at_sync["generic"] + 4, (generic, at_sync)     # the first binning, two k_frame, the fuse-only launch
    gpu.close()


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["tile", "cell"])
def test_switch_wherever_it_falls(oracle_mod, kind, mode, track):
    """no synchronisation behind the heavy frame: the host sees the word whenever the store lands"""
    ops, clean, (hc, hf) = switch_ops(kind, False)
    assert_heavy(oracle_mod, kind, hc, hf, clean)
    gpu = run(oracle_mod, f"switch-{kind}", SW_L, SW_RES, ops, mode, track)
    check_mode_counts(gpu, mode, clean=False)
    assert counts(gpu)[2] == 1
    gpu.close()


# ---- 4. forced lean: the slow path of the lean form on both buffer sets -------------------------------------------------------------
def forced_ops():
    rng = np.random.default_rng(24)
    ht = [blob(rng, 4000, 1.0, -0.7, 0.8), blob(rng, 20000, -1.3, 0.4, 0.8), blob(rng, 4000, 1.0, -0.7, 0.8), blob(rng, 6000, 0.3, 0.3, 0.8)]
    ops = [("add", frame_at(), spread(rng, 4000, SW_L, SW_RES))]
    ops += [("add", frame_at(), c) for c in ht]                         # four overflowing frames in a row: both buffer sets, twice
    wall = [heavy_cloud(rng, "cell") for _ in range(2)]
    ops += [("add", f, c) for c, f in wall]                             # ... and two frames with a cell of nine
    ops += [("var", 1e-4)]
    ops += [("add", frame_at(), spread(rng, n, SW_L, SW_RES)) for n in (5000, 3000, 4000)]
    ops += [("sync",), ("check",)]
    return ops, ht, wall


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_forced_lean(oracle_mod, mode, track):
    ops, ht, wall = forced_ops()
    for c in ht:
        assert loads(oracle_mod, SW_L, SW_RES, frame_at(), c)[0] > 768
    for c, f in wall:
        t, cm, _ = loads(oracle_mod, SW_L, SW_RES, f, c)
        assert t <= 768 and cm >= 9, (t, cm)
    gpu = run(oracle_mod, "forced", SW_L, SW_RES, ops, mode, track)
    lean, generic, seen = counts(gpu)
    print("mode", mode, "lean launches", lean, "generic launches", generic, "form seen", seen)
    check_mode_counts(gpu, mode, clean=False)
    assert seen == 1
    if mode == 1:
        assert generic == 0 and lean >= 11, (lean, generic)             # ten frames: one binning, nine k_frame, the fuse-only launch
    gpu.close()
