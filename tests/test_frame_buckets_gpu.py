"""k_frame's per-tile record buckets against the CPU oracle, bit for bit, with and without lowest tracking (k_frame<0> / <4>).

A stream of single device-resident sweeps runs as one k_frame launch per frame: the binning half reserves ranges of per-tile
buckets, the fuse half takes a tile's records from its bucket.  These streams drive every path of the fuse half:
- a tile of more than kFrameBucket (768) records, whose bucket overflows into the spill arena;
- a cell with 8 or more records of one sweep (more than the register network of the fast path holds);
- row strips (stage A of the tiled map: every rank fuses its own rows);
- moves and queued variance increments between frames, and the deferred fuse at synchronisation.
Overflowing frames follow each other (both halves of the double buffer), then ordinary frames: the counts and spill slots a
frame leaves behind must be clean, and a buffer set that met the slow path bins its later frames in the descriptor form.
"""
import numpy as np
import pytest

from gem_amd import ElevationMap, SensorModel, synth

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
F32 = np.float32
L, RES = 96, 0.1                                       # 6 x 6 tiles of 16 x 16 cells (1.6 m)


def blob(rng, n, cx, cy, half):
    """n points in a square of side 2 * half around (cx, cy), heights near the sensor's."""
    c = np.zeros((n, 4), F32)
    c[:, 0] = rng.uniform(cx - half, cx + half, n)
    c[:, 1] = rng.uniform(cy - half, cy + half, n)
    c[:, 2] = rng.normal(0.0, 0.2, n)
    c[:, 3] = 1.0
    return c


def spread(rng, n):
    return blob(rng, n, 0.0, 0.0, 0.45 * L * RES)


def frame_at(x=0.0, y=0.0, yaw=0.0):
    return synth._frame_for(synth.pose_matrix(x, y, 0.0, yaw=yaw), SensorModel.velodyne())


def make_pair(oracle_mod, track):
    gpu, ref = ElevationMap(L, RES), oracle_mod.OracleMap(L, RES)
    if track:
        gpu.set_lowest_tracking(True)
        gpu.set_layer("lowest", ref.layer("lowest"))   # the oracle always tracks: start both from the same layer
    return gpu, ref


def check(gpu, ref, track, what):
    for name in ("elevation", "variance") + (("lowest",) if track else ()):
        g, o = gpu.layer(name), ref.layer(name)
        assert np.array_equal(g, o), f"{what}: {name} differs in {np.count_nonzero(g != o)} cells"


def loads(oracle_mod, frame, cloud):
    """(most records in one 16x16 tile, most records in one cell) of a sweep into a fresh map, from the oracle's projection"""
    o = oracle_mod.OracleMap(L, RES).process_points(frame, cloud[:, 0], cloud[:, 1], cloud[:, 2])
    idx = np.asarray(o["index"]); idx = idx[idx >= 0]
    tpr = (L + 15) // 16
    tiles = (idx // L >> 4) * tpr + (idx % L >> 4)
    return int(np.bincount(tiles).max()), int(np.bincount(idx).max())


def run_stream(gpu, ref, frames, clouds, between=None):
    import torch
    d = [torch.from_numpy(c).cuda() for c in clouds]
    torch.cuda.synchronize()
    for k, (f, c) in enumerate(zip(frames, clouds)):
        if between:
            between(k)
        gpu.add(f, d[k]); ref.add(f, c)


@pytest.mark.parametrize("track", [False, True])
def test_tiles_above_the_bucket(oracle_mod, track):
    """Blobs of 1.6 m: at least one tile gets more than 768 records (about 4 per cell at 4000 points, about 20 at 20000)."""
    rng = np.random.default_rng(11)
    gpu, ref = make_pair(oracle_mod, track)
    clouds = [spread(rng, 20000), blob(rng, 4000, 1.0, -0.7, 0.8), blob(rng, 20000, -1.3, 0.4, 0.8),
              blob(rng, 4000, 1.0, -0.7, 0.8), spread(rng, 20000), spread(rng, 5000)]
    tile_max = [loads(oracle_mod, frame_at(), c)[0] for c in clouds]
    assert max(tile_max) > 768 and sum(t > 768 for t in tile_max) >= 3, tile_max       # buckets do overflow, in both buffer sets
    run_stream(gpu, ref, [frame_at()] * len(clouds), clouds)
    check(gpu, ref, track, "after the stream")


@pytest.mark.parametrize("track", [False, True])
def test_cells_of_eight_records_and_more(oracle_mod, track):
    """A wall in front of the sensor: 8, 9, 30 and 200 records in single cells of tiles that stay far below 768 records."""
    rng = np.random.default_rng(12)
    gpu, ref = make_pair(oracle_mod, track)
    clouds = []
    for m in (8, 9, 30, 200):
        c = spread(rng, 3000)
        w = blob(rng, m, 0.73, 1.12, 0.02)              # one cell (0.1 m) and its neighbours at most
        w[:, 2] = rng.normal(0.5, 0.05, m)
        mix = np.concatenate([c[:1000], w, c[1000:]])   # input order matters: the wall sits in the middle of the sweep
        clouds.append(mix)
    clouds.append(spread(rng, 3000))
    lt = [loads(oracle_mod, frame_at(0.1, -0.2, 0.3), c) for c in clouds[:4]]
    assert all(t <= 768 and c >= 8 for t, c in lt), lt                                   # cells past the register network, tiles that fit
    run_stream(gpu, ref, [frame_at(0.1, -0.2, 0.3)] * len(clouds), clouds)
    check(gpu, ref, track, "after the stream")


@pytest.mark.parametrize("track", [False, True])
def test_moves_and_increments_between_frames(oracle_mod, track):
    """Queued Mapvar_update increments, moves of the map and whole-map reads between the frames of the stream (the deferred fuse
    is flushed by each read), with an overflowing tile in some of the frames."""
    rng = np.random.default_rng(13)
    gpu, ref = make_pair(oracle_mod, track)
    clouds = [spread(rng, 15000) if k % 3 else np.concatenate([spread(rng, 8000), blob(rng, 3000, 0.2, 0.2, 0.7)]) for k in range(9)]
    poses = [frame_at(0.05 * k, -0.03 * k, 0.1 * k) for k in range(9)]

    def between(k):
        if k % 2 == 1:
            gpu.mapvar_update(1e-4 * k); ref.mapvar_update(1e-4 * k)
        if k % 3 == 2:
            gpu.mapvar_update(3e-5); ref.mapvar_update(3e-5)
        if k % 4 == 3:
            p = np.array([0.35 * k, -0.2 * k, 0.0], F32)
            gpu.move(p); ref.move(p)
        if k == 6:
            check(gpu, ref, track, f"before frame {k}")
    run_stream(gpu, ref, poses, clouds, between)
    gpu.synchronize()
    check(gpu, ref, track, "after the stream")


def test_row_strips(oracle_mod):
    """Stage A of the tiled map: every rank bins the whole sweep and fuses its own rows (uneven strips: L = 75 over three ranks)."""
    import torch
    from gem_amd.tiling import TiledElevationMap
    from test_loopback_gpu import run_ranks
    Ls, res, world = 75, 0.2, 3
    rng = np.random.default_rng(14)
    clouds = [blob(rng, 12000, 0.0, 0.0, 0.45 * Ls * res), blob(rng, 6000, -2.0, 1.0, 1.6), blob(rng, 9000, 0.0, 0.0, 0.45 * Ls * res)]
    frames = [frame_at(0.1, 0.0, 0.2)] * len(clouds)
    upd = [1e-5, 0.0, 2e-5]
    ref = oracle_mod.OracleMap(Ls, res)
    for f, c, u in zip(frames, clouds, upd):
        ref.mapvar_update(u); ref.add(f, c)
    maps = [TiledElevationMap(Ls, res, r, world, exchange="loopback", tile_strips=False, world_id=4242) for r in range(world)]
    dc = [torch.from_numpy(c).cuda() for c in clouds]

    def rank(r):
        tm = maps[r]
        for f, c, u in zip(frames, dc, upd):
            tm.mapvar_update(u)
            tm.add(f, c)
        tm.allgather(with_attributes=False)
        tm.map.synchronize()
    run_ranks(world, rank)
    for r, tm in enumerate(maps):
        for name in ("elevation", "variance"):
            assert np.array_equal(tm.layer(name), ref.layer(name)), (r, name)
        tm.map.close()
