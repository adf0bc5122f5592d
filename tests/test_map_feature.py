"""Traversability stage: Map_feature / G_Mapfeature + the Jacobi eigen-solver
(gpu_process.cu:549-670, 66-187, 1256-1302).  CPU tests pin the oracle with hand-derived cases; the GPU
tests compare gem_map_feature with the oracle.

Tolerances.  Every float operation of the stage is replayed in the same order on both sides (FMA
contraction off); the only library calls are sin / cos / atan2 / acos, evaluated in double and rounded to
float on both sides, so results normally agree bit for bit.  A double result within ~1e-16 of a float rounding
boundary may round differently between glibc and the device library; slope = acos(|n_z|) amplifies such a
last-bit difference near n_z = 1 (slope ~ sqrt(2 (1 - n_z))), hence the absolute bounds below.
"""
import numpy as np
import pytest

import feature_scenes as fs

F32 = np.float32
SLOPE_ABS, ROUGH_ABS, TRAVER_ABS = fs.SLOPE_ABS, 1e-6, 2e-3


terrain = fs.terrain          # slope + waves + noise, 15 % holes, a gap wider than the window's reach on one side, a step


# ---- oracle known answers (CPU) -----------------------------------------------------------------------------------------
def test_flat_plane_is_fully_traversable(oracle_mod):
    m = oracle_mod.OracleMap(16, 0.1)
    m.set_layer("elevation", np.full((16, 16), 0.25, F32))
    f = m.map_feature()
    assert np.all(f["slope"] == 0) and np.all(f["rough"] == 0) and np.all(f["traver"] == 1.0)
    assert np.array_equal(m.layer("traver"), f["traver"])          # map_traver is updated (GPU:658)


def test_isolated_cells_and_empty_cells(oracle_mod):
    m = oracle_mod.OracleMap(16, 0.1)
    e = np.full((16, 16), -10, F32); e[5, 5] = 1.0; e[5, 6] = 1.1
    m.set_layer("elevation", e)
    f = m.map_feature()
    assert f["traver"][5, 5] == -10 and f["slope"][5, 5] == 0 and f["rough"][5, 5] == 0      # p_n <= 7 (GPU:660-666)
    assert f["traver"][0, 0] == -10 and f["rough"][0, 0] == 0                                  # empty cell: untouched map_traver


def test_tilted_plane_slope_is_the_plane_angle(oracle_mod):
    # z = a*x on a 5x5 patch: cov_xz = a * cov_xx > 0.01 -> the Jacobi loop runs; normal = (-a, 0, 1)/sqrt(1+a^2)
    L, res, a = 32, 0.2, 0.5
    x = (np.arange(L) * res)[:, None] * np.ones((1, L))
    m = oracle_mod.OracleMap(L, res)
    m.set_layer("elevation", (a * x).astype(F32))
    f = m.map_feature()
    inner = f["slope"][4:-4, 4:-4]
    assert np.allclose(inner, np.arctan(a), atol=2e-3)             # Jacobi stops at |off-diagonal| < 0.01
    assert np.allclose(f["rough"][4:-4, 4:-4], 0.0, atol=1e-5)
    assert np.allclose(f["traver"][4:-4, 4:-4], 0.5 * (1 - inner / 0.6) + 0.5, atol=1e-6)


def test_neighbourhood_bounds_follow_the_unrolled_index(oracle_mod):
    # after Move the window is clipped at the map edge in UNROLLED coordinates while storage reads wrap
    L = 24
    m = oracle_mod.OracleMap(L, 0.1)
    m.move(np.array([0.5, -0.3, 0.0], F32))
    e = np.full((L, L), 0.1, F32)
    m.set_layer("elevation", e)
    f = m.map_feature()
    sx, sy = m.pose()[1]
    # unrolled corner cell (0, 0) sits at storage (sx, sy): it sees a 3x3 window = 9 cells > 7 -> valid
    assert f["traver"][sx % L, sy % L] != -10
    # the plane is flat in z but the storage x/y coordinates jump across the wrap: the reference uses storage
    # coordinates for the fit, which only changes the in-plane eigenvectors; slope stays 0
    assert np.all(f["slope"] == 0)


# ---- the oracle's test switches: trig nudge and rotation counter (CPU) ------------------------------------------------------------
def test_nudge_moves_only_the_slopes_of_rotating_cells(oracle_mod):
    L, res = 64, 0.1
    m = oracle_mod.OracleMap(L, res)
    z = fs.terrain(L, res, 1); z[40:60, 5:25] = 0.75                  # a flat patch: cells that do not rotate
    m.set_layer("elevation", z)
    plain = m.map_feature(); rot = m.feature_rotations()
    again = m.map_feature()                                            # the switch is off again after every call
    nudged = m.map_feature(nudge=(7, 3))
    after = m.map_feature()
    for k in ("rough", "slope", "traver"):
        assert np.array_equal(again[k], plain[k]) and np.array_equal(after[k], plain[k]), k
    assert np.array_equal(nudged["rough"], plain["rough"])
    still = rot == 0
    assert still.sum() > 200 and np.array_equal(nudged["slope"][still], plain["slope"][still])
    assert np.array_equal(nudged["traver"][still], plain["traver"][still])
    moved = nudged["slope"] != plain["slope"]
    assert moved.any() and not moved[rot == 255].any()
    assert np.array_equal(m.feature_rotations() == 255, plain["traver"] == -10)
    assert np.array_equal(m.map_feature(nudge=(7, 3))["slope"], nudged["slope"])            # seeded: repeatable
    assert not np.array_equal(m.map_feature(nudge=(8, 3))["slope"], nudged["slope"])


def test_rotation_counter_follows_the_pivot_scan(oracle_mod):
    def sym(a00, a11, a22, a01, a02, a12):
        return np.array([[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]], F32)
    cases = {
        "diagonal": (sym(2, 1, 0.5, 0, 0, 0), 0, None),
        "below dbEps": (sym(2, 1, 0.5, 0, 0.0099, 0), 0, None),
        "at dbEps": (sym(2, 1, 0.5, 0, 0.01, 0), None, (0, 2)),       # 0.01f < 0.01f is false: it rotates
        "negative a01 wins": (sym(2, 1, 0.5, -0.4, 0.3, 0.2), None, (0, 1)),     # the signed start value loses to its own magnitude
        "positive a01 ties a02": (sym(2, 1, 0.5, 0.25, 0.25, 0.1), None, (0, 1)),  # strict >: the first of two equals stays
        "negative a01 ties a02": (sym(2, 1, 0.5, -0.25, 0.25, 0.1), None, (0, 1)),
        "a02 ties a12": (sym(2, 1, 0.5, 0, 0.25, -0.25), None, (0, 2)),
    }
    for name, (m, count, first) in cases.items():
        assert fs.pivot_replay(m) == first, name
        c, normal = oracle_mod.jacobi_rotations(m)
        rc, pivots, rnormal = fs.jacobi_replay(m)
        assert c == rc and np.array_equal(normal, rnormal), name
        assert (pivots[0] if pivots else None) == first, name
        if count is not None:
            assert c == count, name
        else:
            assert 1 <= c <= 31, name
    # the replay notices a restated scan: with >= the tie goes to the later entry and the result changes
    for name in ("positive a01 ties a02", "a02 ties a12"):
        m = cases[name][0]
        assert fs.jacobi_replay(m, strict=False)[1][0] != fs.jacobi_replay(m)[1][0], name
    # ... and the layer of gemo_map_feature holds the same counts: a cell's covariance, replayed
    L, res = 16, 0.125
    z = fs._tie_holes(fs._plane(L, res, 1, -1).astype(F32))
    om = oracle_mod.OracleMap(L, res); om.set_layer("elevation", z); om.map_feature()
    rot = om.feature_rotations()
    n, a = fs.covariance_replay(z, res)
    for r in range(L):
        for c in range(L):
            if n[r, c] > 7 and z[r, c] != -10:
                assert rot[r, c] == fs.jacobi_replay(sym(*a[r, c]))[0], (r, c)
            else:
                assert rot[r, c] == 255


_SCENES = fs.all_scenes()


@pytest.mark.parametrize("scene", _SCENES, ids=[s.name for s in _SCENES])
def test_scene_reaches_what_it_was_written_for(oracle_mod, scene):
    """The preconditions of the device tests' scenes (tests/test_map_feature_edges_gpu.py) need only the oracle: a scene that
    stops covering its case fails here, without a GPU.  Every scene's oracle-derived bound stays within SLOPE_ABS."""
    ev = fs.check_precondition(oracle_mod, scene)
    assert ev.bound <= SLOPE_ABS, f"{scene.name}: bound {ev.bound:.3e}"
    if ev.rotating.any() and scene.L > 2:
        assert ev.bound > 0 or not np.isfinite(ev.out["slope"][ev.rotating]).any()      # the switch does something


# ---- GPU parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L,res,seed", [(64, 0.1, 1), (75, 0.2, 2), (200, 0.05, 3)])
def test_map_feature_parity(oracle_mod, L, res, seed):
    from gem_amd import ElevationMap
    gpu, ref = ElevationMap(L, res), oracle_mod.OracleMap(L, res)
    if seed == 2:
        gpu.move(np.array([1.3, -0.7, 0], F32)); ref.move(np.array([1.3, -0.7, 0], F32))
    z = terrain(L, res, seed)
    gpu.set_layer("elevation", z); ref.set_layer("elevation", z)
    g, o = gpu.map_feature(), ref.map_feature()
    assert np.array_equal(g["traver"] == -10, o["traver"] == -10)
    exact = np.mean(g["slope"] == o["slope"])
    assert exact > 0.999, f"only {exact:.4f} of the slopes agree bit for bit"
    assert np.max(np.abs(g["slope"] - o["slope"])) <= SLOPE_ABS
    assert np.max(np.abs(g["rough"] - o["rough"])) <= ROUGH_ABS
    assert np.max(np.abs(g["traver"] - o["traver"])) <= TRAVER_ABS
    # roughness is |h - mean z|, no library call: bit-identical; and the device's traver follows, bit for bit, from the device's
    # own slope and roughness, so a traver error can only come from a slope error
    assert np.array_equal(g["rough"], o["rough"])
    fitted = o["traver"] != -10
    assert np.array_equal(g["traver"][fitted], fs.traver_from(g["slope"], g["rough"])[fitted])
    assert (o["slope"] > 0.05).mean() > 0.3                          # the Jacobi path is what is being compared
    # the layers are resident: traver / rough / slope can be fetched like any other layer
    assert np.array_equal(gpu.layer("traver"), g["traver"]) and np.array_equal(gpu.layer("slope"), g["slope"])
    assert np.array_equal(gpu.layer("rough"), g["rough"])


@pytest.mark.gpu
def test_map_feature_after_fusion(oracle_mod):
    from gem_amd import ElevationMap, synth
    wl = synth.config_c2()
    gpu, ref = ElevationMap(wl.length, wl.resolution), oracle_mod.OracleMap(wl.length, wl.resolution)
    gpu.add(wl.frames[0], wl.clouds[0]); ref.add(wl.frames[0], wl.clouds[0])
    g, o = gpu.map_feature(), ref.map_feature()
    for k in ("rough", "slope", "traver"):
        assert np.array_equal(g[k], o[k]), k
    assert (o["traver"] != -10).sum() > 10000


# ---- loop-closure re-anchoring: Map_optmove / Map_closeloop (gpu_process.cu:1215-1254) ---------------------------------------
def test_optmove_relabels_the_centre_and_shifts_heights(oracle_mod):
    m = oracle_mod.OracleMap(16, 0.1)
    e = np.full((16, 16), -10, F32); e[3, 4] = 0.5; e[9, 9] = -0.25
    m.set_layer("elevation", e)
    m.move(np.array([0.3, -0.2, 0.0], F32))
    c0, s0 = m.pose()
    aligned = m.map_optmove([c0[0] + 0.234, c0[1] - 0.561], 0.125)
    c1, s1 = m.pose()
    assert tuple(s1) == tuple(s0)                                           # the circular buffer is not shifted
    assert np.allclose(aligned, [c0[0] + 0.2, c0[1] - 0.6], atol=1e-6) and np.allclose(c1, aligned)
    out = m.layer("elevation")
    assert out[3, 4] == F32(0.5) + F32(0.125) and out[9, 9] == F32(-0.25) + F32(0.125) and out[0, 0] == -10


@pytest.mark.gpu
def test_optmove_and_closeloop_parity(oracle_mod):
    from gem_amd import ElevationMap
    L, res = 64, 0.1
    gpu, ref = ElevationMap(L, res), oracle_mod.OracleMap(L, res)
    z = terrain(L, res, 5)
    for m in (gpu, ref):
        m.move(np.array([1.03, -0.46, 0], F32)); m.set_layer("elevation", z)
    a_g, a_o = gpu.map_optmove([1.31, -0.77], 0.071), ref.map_optmove([1.31, -0.77], 0.071)
    assert np.array_equal(a_g, a_o)
    gpu.map_closeloop([0.52, 0.18], -0.033); ref.map_closeloop([0.52, 0.18], -0.033)
    cg, sg = gpu.pose(); co, so = ref.pose()
    assert np.array_equal(np.asarray(cg, F32), np.asarray(co, F32)) and tuple(sg) == tuple(so)
    assert np.array_equal(gpu.layer("elevation"), ref.layer("elevation"))
