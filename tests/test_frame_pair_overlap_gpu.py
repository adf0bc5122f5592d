"""The overlapping pair kernel (pairov_k_frame, gem_amd/csrc/gem_frame_pair.hip) against the CPU oracle, bit for bit, with the debug
knob "frame_pair_overlap" at 1 (the overlapping kernel) and at 0 (pair_k_frame).  Maps of 32, 40 and 272 cells; the helpers are
tests/test_frame_pair_gpu.py's.

The overlapping kernel loads both sweeps' counts of a tile in front of the first round and runs both rounds of frame_tile from
them, the second round's DMA right behind the barrier between the rounds.  Every case builds two sweeps A and B under different
poses with a chosen number of records in ONE 16x16 tile (and, where it says so, in one cell of it), lets one launch bin both and the
next launch fuse both, and reads the map.  "frame_pairs" is asserted against the policy model, so a case that stopped pairing
fails.  The rest of each sweep goes to the other tiles, a few records each (tiles live in A only, in B only and in both, by the
sweeps' sizes).
- general pairs: 65 + 65, 256 + 256, 257 + 300 (the second round trip), 300 + 468, 320 + 449, 653 + 626, 768 + 768;
- a cell of 7 + 7; a cell of eight in A only and in B only with more than 64 records in the tile (the slow path: the handle stops
  pairing); 769 records in one tile of B, of A (bucket overflow); a gem_mapvar_update in front of the stream;
- light rounds: 1 + 1 in one cell, 32 + 32, 64 + 0, 0 + 64 (a count of zero handed to a round), 40 + 24 with a cell of 3 + 4 and of
  4 + 4, 64 + 64, light / general and general / light;
- the variance floor between the sweeps (see test_floor_between_sweeps)."""
import numpy as np
import pytest

from gem_amd import ElevationMap
from test_frame_pair_gpu import POSES, RES, Stream, built_sweep, clean_clouds, frame_at, records, tile_of

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
F32 = np.float32

_FILL = {}


def fill_clouds(oracle_mod, L):
    if L not in _FILL:
        _FILL[L] = clean_clouds(oracle_mod, L, 7, (300, 200) if L <= 40 else (3000, 2000))
    return _FILL[L]


def run_pair(oracle_mod, overlap, L, A, B, name, lean=True, stream=None, before=None):
    """fill, fill, A (held), B (one launch bins both), fill (held), fill (one launch fuses A, then B), read"""
    fill = fill_clouds(oracle_mod, L)
    s = stream or Stream(oracle_mod, L, debug={"frame_pair": 1, "frame_pair_overlap": overlap}, name=name)
    assert s.gpu.debug_get("frame_pair_overlap") == overlap
    if before:
        before(s)
    s.add(POSES[0], fill[0]); s.add(POSES[1], fill[1])
    s.add(POSES[2], A); s.add(POSES[3], B)
    s.add(POSES[0], fill[0]); s.add(POSES[1], fill[1])
    if not lean:
        s.torch.cuda.synchronize()
        assert s.gpu.debug_get("frame_form_seen") == 1
    assert s.model.pairs == 2                                # the launch that binned A and B, the launch that fused them
    s.read(lean=lean)
    if lean:
        assert s.model.pairs == 3 and s.gpu.debug_get("frame_form_seen") == 0
    s.close()


def pair_of(oracle_mod, L, tile, ta, tb, na, nb, ca=0, cb=0):
    rng = np.random.default_rng(ta * 1009 + tb * 7 + ca + L)
    A = built_sweep(oracle_mod, rng, L, POSES[2], tile, ta, na, ca)
    B = built_sweep(oracle_mod, rng, L, POSES[3], tile, tb, nb, cb)
    tpr = (L + 15) // 16
    for sw, p, want in ((A, POSES[2], ta), (B, POSES[3], tb)):
        idx = records(oracle_mod, L, frame_at(*p), sw)
        assert int(np.count_nonzero(tile_of(idx, L) == tile[0] * tpr + tile[1])) == want
    return A, B


#          records of the tile in A, in B | points of sweep A, of B | of those in ONE cell of the tile in A, in B
GENERAL = [(65, 65, 130, 65, 0, 0), (256, 256, 256, 300, 0, 0), (257, 300, 300, 340, 0, 0), (300, 468, 360, 468, 0, 0), (320, 449, 320, 500, 0, 0),
           (653, 626, 700, 650, 0, 0), (768, 768, 800, 790, 0, 0), (100, 90, 160, 120, 7, 7)]
LIGHT = [(1, 1, 30, 40, 1, 1), (32, 32, 32, 70, 0, 0), (64, 0, 100, 30, 0, 0), (0, 64, 30, 64, 0, 0), (40, 24, 80, 60, 3, 4), (40, 24, 80, 60, 4, 4),
         (64, 64, 90, 64, 0, 0), (30, 100, 60, 130, 0, 0), (100, 30, 130, 60, 0, 0)]


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("ta,tb,na,nb,ca,cb", GENERAL + LIGHT)
def test_pair_contents(oracle_mod, overlap, ta, tb, na, nb, ca, cb):
    L, tile = 40, (1, 1)
    A, B = pair_of(oracle_mod, L, tile, ta, tb, na, nb, ca, cb)
    if ca > 1 and cb > 1:                                            # the cell both sweeps load is the tile's first
        ia, ib = records(oracle_mod, L, frame_at(*POSES[2]), A), records(oracle_mod, L, frame_at(*POSES[3]), B)
        assert np.bincount(ia).argmax() == np.bincount(ib).argmax() and np.bincount(ia).max() == ca and np.bincount(ib).max() == cb
    run_pair(oracle_mod, overlap, L, A, B, f"contents{ta}+{tb}/{overlap}")


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("L,tile", [(32, (0, 1)), (272, (8, 8)), (272, (3, 12))])
def test_pair_other_maps(oracle_mod, overlap, L, tile):
    """two by two tiles, and 17 by 17 (the centre tile, which the block order starts with, and one far from it): a light pair and a general pair each
    (the 40-cell map of the other tests has a partial last tile row and column)"""
    for ta, tb, na, nb in ((20, 30, 600, 500), (300, 200, 900, 700)):
        A, B = pair_of(oracle_mod, L, tile, ta, tb, na, nb)
        run_pair(oracle_mod, overlap, L, A, B, f"maps{L}-{ta}+{tb}/{overlap}")


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("where", ["A", "B"])
def test_cell_of_eight_behind_the_prefetch(oracle_mod, overlap, where):
    """more than 64 records in the tile, eight of them in one cell, in A only or in B only: the slow path of that round; the other
    round's cells are right (A's have been stored before B's round reads them)"""
    L, tile = 40, (1, 1)
    A, B = pair_of(oracle_mod, L, tile, 70, 66, 140, 130, 8, 0) if where == "A" else pair_of(oracle_mod, L, tile, 66, 70, 130, 140, 0, 8)
    run_pair(oracle_mod, overlap, L, A, B, f"eight-{where}/{overlap}", lean=False)


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("ta,tb", [(100, 769), (769, 100)])
def test_bucket_overflow(oracle_mod, overlap, ta, tb):
    L, tile = 40, (1, 1)
    A, B = pair_of(oracle_mod, L, tile, ta, tb, ta + 50, tb + 50)
    run_pair(oracle_mod, overlap, L, A, B, f"overflow{ta}+{tb}/{overlap}", lean=False)


@pytest.mark.parametrize("overlap", [1, 0])
def test_mapvar_update_in_front(oracle_mod, overlap):
    """queued increments in front of the stream: the sweep that carries them is dense (every tile takes the general path)"""
    L, tile = 40, (1, 1)
    A, B = pair_of(oracle_mod, L, tile, 40, 20, 90, 60)

    def before(s):
        fill = fill_clouds(oracle_mod, L)
        s.add(POSES[0], fill[0]); s.read()
        s.ref.mapvar_update(1e-4); s.gpu.mapvar_update(1e-4)
        s.model.flush()
    run_pair(oracle_mod, overlap, L, A, B, f"mapvar/{overlap}", before=before)


def _floor_case(oracle_mod, L, floor):
    tile = (1, 1)
    A, B = pair_of(oracle_mod, L, tile, 40, 24, 40, 24, 3, 4)
    return A, B


@pytest.mark.parametrize("overlap", [1, 0])
def test_floor_between_sweeps(oracle_mod, overlap):
    """A variance floor far above every fused variance (0.5): the floor acts at the end of A's Fuse on every cell A touched, in front
    of B's records of the same cells (a cell of 3 + 4 among them).

    Checked on the CPU with the oracle alone, below: with this floor A's Fuse leaves variances that the floor raises (the case
    does exercise the clamp between the sweeps), but the oracle's map after B is the SAME whether or not that clamp is applied --
    fusing A's and B's records of the pair in one Fuse call gives the bits of two calls.  The recurrence raises a cell's variance to
    the floor at the start of every record's step (gpu_process.cu:500-501, written back), and a cell that has a record of B takes
    such a step right behind the clamp, so no choice of variances can make the clamp between the sweeps visible in the map: the
    assertion here is that the device's map is the oracle's, and the CPU check states what it found."""
    L, floor = 40, 0.5
    A, B = _floor_case(oracle_mod, L, floor)
    # ---- the oracle alone: two Fuse calls against one Fuse call over both sweeps' records
    two, one, probe = (oracle_mod.OracleMap(L, RES, variance_floor=floor) for _ in range(3))
    pa = probe.process_points(frame_at(*POSES[2]), A[:, 0], A[:, 1], A[:, 2])
    pb = probe.process_points(frame_at(*POSES[3]), B[:, 0], B[:, 1], B[:, 2])
    assert (pa["index"] >= 0).all() and (pb["index"] >= 0).all()
    # warm cells first, so that A's records are fused (Kalman) and not just stored
    for m in (two, one):
        m.fuse(pa["index"], pa["height"] + F32(0.01), pa["var"])
    unclamped = oracle_mod.OracleMap(L, RES, variance_floor=0.0)
    unclamped.fuse(pa["index"], pa["height"] + F32(0.01), pa["var"]); unclamped.fuse(pa["index"], pa["height"], pa["var"])
    touched = np.unique(pa["index"])
    assert (unclamped.layer("variance").ravel()[touched] < floor).all(), "A's Fuse leaves nothing for the floor to raise"
    two.fuse(pa["index"], pa["height"], pa["var"]); two.fuse(pb["index"], pb["height"], pb["var"])
    one.fuse(np.concatenate([pa["index"], pb["index"]]), np.concatenate([pa["height"], pb["height"]]), np.concatenate([pa["var"], pb["var"]]))
    both = np.intersect1d(pa["index"], pb["index"])
    assert both.size >= 1
    same = all(np.array_equal(two.layer(n), one.layer(n)) for n in ("elevation", "variance"))
    print(f"oracle alone: clamp between the sweeps changes the map: {not same} ({both.size} cells hold records of both sweeps)")
    assert same, "the oracle's map depends on the clamp between the sweeps after all: this case then discriminates"
    # ---- the device against the oracle
    s = Stream(oracle_mod, L, debug={"frame_pair": 1, "frame_pair_overlap": overlap}, name=f"floor/{overlap}")
    s.ref.close(); s.gpu.close()
    s.ref = oracle_mod.OracleMap(L, RES, variance_floor=floor)
    s.gpu = ElevationMap(L, RES, variance_floor=floor, debug={"frame_pair": 1, "frame_pair_overlap": overlap})
    run_pair(oracle_mod, overlap, L, A, B, f"floor/{overlap}", stream=s)


def test_knob_default_and_range(oracle_mod):
    m = ElevationMap(32, RES)
    assert m.debug_get("frame_pair_overlap") == 1
    m.debug_set("frame_pair_overlap", 0)
    assert m.debug_get("frame_pair_overlap") == 0
    with pytest.raises(Exception):
        m.debug_set("frame_pair_overlap", 2)
    m.close()
