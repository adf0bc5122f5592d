"""k_map_feature (5x5 plane fit + Jacobi eigen-solver behind gem_map_feature) against the oracle, at the edges the parity tests of
tests/test_map_feature.py do not reach: workgroups in which every cell / no cell rotates, exact ties in the pivot scan, near-flat
cells that still rotate (acos near 1), 8 and more rotations, cancellation in the covariance, non-finite heights, a genuine -10,
windows of exactly 7 and 8 cells, the storage seam on / before / after a tile edge, maps smaller than the staging tile
(L = 1 .. 6), a ragged last tile at L = 1025, and row-strip handles.

The comparison (feature_scenes.compare) carries no hand-chosen number: masks, roughness and the slopes of cells that do not
rotate are bit-identical; traver follows bit for bit from the device's own slope and roughness; the slopes of rotating cells
agree within a bound measured at test time on the oracle alone (what one-ulp differences between two libms' double
sin / cos / atan2 / acos are worth in that scene, times 2), which is itself asserted to be within SLOPE_ABS; and at least 0.999
of the rotating cells are bit-equal.  The scenes' preconditions are asserted here and, without a GPU, in tests/test_map_feature.py.

What the MI355X run showed per scene (cells not bit-equal, largest difference, bound) is in profiles/map_feature_edges.txt.

GEM_FEATURE_EDGES_REPORT=<file> appends one line per scene: scene, fitted, rotating, not bit-equal, max |slope diff|, bound.
"""
import os

import numpy as np
import pytest

import feature_scenes as fs

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
F32 = np.float32

_SCENES = fs.all_scenes()


def _report(row):
    path = os.environ.get("GEM_FEATURE_EDGES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(f"{row['scene']:40s} {row['fitted']:8d} {row['rotating']:8d} {row['not_bit_equal']:6d} "
                    f"{row['max_abs_slope_diff']:.3e} {row['bound']:.3e}\n")


@pytest.mark.parametrize("scene", _SCENES, ids=[s.name for s in _SCENES])
def test_scene(oracle_mod, scene):
    from gem_amd import ElevationMap
    ev = fs.check_precondition(oracle_mod, scene)
    gpu = ElevationMap(scene.L, scene.res)
    assert fs.prepare(gpu, scene) == ev.start
    g = gpu.map_feature()
    row = fs.compare(g, ev, scene, fs.SLOPE_ABS)
    _report(row)
    for k in fs.LAYERS:                                               # what was returned is what is resident
        assert fs._same_bits(gpu.layer(k), g[k]), k
    g2 = gpu.map_feature()                                            # a second call on the same layers: the same bits
    for k in fs.LAYERS:
        assert fs._same_bits(g2[k], g[k]), k
    gpu.close()


def _strip_rows(L, world, kind):
    from gem_amd import tiling
    if kind == "tiles":
        return tiling.tile_strip_rows(L, world)
    return [tiling.strip_bounds(L, world, r)[0] for r in range(world)] + [L]


@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("kind", ["rows", "tiles"])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("L", [75, 96])
def test_row_strip_handles_write_their_rows_only(L, world, kind, moved):
    """A handle created with strip=(row0, rows) computes its rows from the whole elevation layer (the 2-row halo lies outside
    the strip) and leaves the other rows of traver / rough / slope alone."""
    from gem_amd import ElevationMap
    res, sentinel = 0.1, F32(123.25)
    rows = _strip_rows(L, world, kind)
    assert rows[0] == 0 and rows[-1] == L and all(b > a for a, b in zip(rows, rows[1:]))
    z = fs.terrain(L, res, 20 + world)
    handles = [ElevationMap(L, res)] + [ElevationMap(L, res, strip=(rows[r], rows[r + 1] - rows[r])) for r in range(world)]
    for h in handles:
        if moved:                                                     # the storage seam (row L - 40, column 9) inside a strip
            h.move(np.array([40 * res, -9 * res, 0], F32))
            assert tuple(h.pose()[1]) == (L - 40, 9)
        h.set_layer("elevation", z)
        for k in fs.LAYERS:
            h.set_layer(k, np.full((L, L), sentinel, F32))
    whole = handles[0].map_feature()
    assert (whole["slope"] > 0).sum() > 0.4 * L * L and not (whole["slope"] == sentinel).any()
    if moved:
        assert any(a < L - 40 < b - 1 for a, b in zip(rows, rows[1:])), "the seam is not inside a strip"
    for r, h in enumerate(handles[1:]):
        assert tuple(h.strip()) == (rows[r], rows[r + 1])
        out = h.map_feature()
        own = np.zeros((L, L), bool); own[rows[r]:rows[r + 1]] = True
        for k in fs.LAYERS:
            assert fs._same_bits(out[k][own], whole[k][own]), f"rank {r}: {k} differs inside the strip"
            assert np.all(out[k][~own] == sentinel), f"rank {r}: {k} was written outside the strip"
    for h in handles:
        h.close()
