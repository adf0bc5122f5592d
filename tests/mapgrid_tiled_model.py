"""A numpy model of the PROTOCOL under gem_costmap_mapgrid_prepare_tiled (gem_amd/csrc/gem_mapgrid_tiled.hip on gem_tile_round.hpp), not
of the kernel: what the tile rounds compute when the tiles of a round run in any order and read halo cells that are old or new.

    fill UN -> 0 into the sources -> mark the sources' tiles and their four neighbours -> rounds -> the rim pass

A round takes the tiles marked for it in a random order.  A tile reads its own cells as they are and, PER EDGE, either the neighbour's
cells as they are now or as they were when the round started (drawn at random: inside a launch nothing orders a tile's halo loads
against its neighbour's stores).  It relaxes to its local fixed point under the blocked rule -- at a blocked cell v = old, at any other
v = min(old, v + 1) along the four directions until nothing changes --, stores what changed and marks, for the NEXT round, the
neighbours whose facing edge changed.  The computation has converged when a round marks nothing.  Then a blocked cell that is not 0 and
has a 4-neighbour below OB becomes OB.

The tile size is a parameter: the protocol does not depend on it, and small tiles put many seams into a small grid."""
import numpy as np

import mapgrid_ref as ref

TILE = 64
_BIG = 1 << 40


def _scan(v, blk):
    """one directional scan along axis 1, left to right: column 0 of v is the halo cell in front of each line (blk there is False,
    it only feeds).  At a blocked cell the running value becomes the cell's own, elsewhere min(own, running + 1).  Vectorised: inside
    a stretch between blocked cells the running value at k is min over j <= k of (own_j - j) + k; every blocked cell starts a new
    stretch, and a stretch's keys lie a whole _BIG below the one before, so one cumulative minimum serves all stretches."""
    k = np.arange(v.shape[1], dtype=np.int64)[None, :]
    seg = np.cumsum(blk, axis=1, dtype=np.int64)
    key = v - k - seg * _BIG
    return np.minimum.accumulate(key, axis=1) + k + seg * _BIG


def local_fixed_point(v, blk):
    """v: int64 [h + 2, w + 2] with the halo, blk: bool of the same shape (its halo entries are ignored).  Own cells change in place;
    returns whether one did."""
    own = (slice(1, -1), slice(1, -1))
    b = blk.copy()
    b[0, :] = b[-1, :] = b[:, 0] = b[:, -1] = False
    changed = False
    for _ in range(v[own].size + 1):                                     # (every pass but the last lowers a cell)
        before = v[own].copy()
        for flip, transpose in ((False, False), (True, False), (False, True), (True, True)):
            a, bb = (v.T, b.T) if transpose else (v, b)
            if flip:
                a, bb = a[:, ::-1], bb[:, ::-1]
            # only the lines' own cells: the scan reads the halo cell in front, never writes a halo cell
            new = _scan(a[1:-1, :-1], bb[1:-1, :-1])
            a[1:-1, 1:-1] = new[:, 1:]
        if (v[own] == before).all():
            break
        changed = True
    return changed


def tiled_distance(grid, sources, rng, tile=TILE, stale=0.5):
    """(dist int32 [sy, sx], rounds): the protocol from the fill to the rim pass"""
    sy, sx = grid.shape
    ob, un = ref.constants(grid)
    blocked = ref.blocked(grid)
    dist = np.full((sy, sx), un, np.int64)
    ntx, nty = -(-sx // tile), -(-sy // tile)
    active = set()
    for x, y in sources:
        dist[y, x] = 0
        tx, ty = x // tile, y // tile
        for dx, dy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
            if 0 <= tx + dx < ntx and 0 <= ty + dy < nty:
                active.add((tx + dx, ty + dy))
    rounds = 0
    for _ in range(sx * sy + 2):                                         # run_tile_rounds' bound
        if not active:
            break
        rounds += 1
        start = dist.copy()
        marked = set()
        order = sorted(active)
        rng.shuffle(order)
        for tx, ty in order:
            x0, y0 = tx * tile, ty * tile
            x1, y1 = min(x0 + tile, sx), min(y0 + tile, sy)
            h, w = y1 - y0, x1 - x0
            v = np.full((h + 2, w + 2), un, np.int64)
            b = np.ones((h + 2, w + 2), bool)
            v[1:-1, 1:-1] = dist[y0:y1, x0:x1]
            b[1:-1, 1:-1] = blocked[y0:y1, x0:x1]
            pick = lambda: start if rng.random() < stale else dist       # noqa: E731
            if y0 > 0:
                v[0, 1:-1] = pick()[y0 - 1, x0:x1]
            if y1 < sy:
                v[-1, 1:-1] = pick()[y1, x0:x1]
            if x0 > 0:
                v[1:-1, 0] = pick()[y0:y1, x0 - 1]
            if x1 < sx:
                v[1:-1, -1] = pick()[y0:y1, x1]
            if not local_fixed_point(v, b):
                continue
            new, old = v[1:-1, 1:-1], dist[y0:y1, x0:x1].copy()
            assert (new <= old).all() and (new[b[1:-1, 1:-1]] == old[b[1:-1, 1:-1]]).all()     # values only fall; a blocked cell is never written
            dist[y0:y1, x0:x1] = new
            ch = new != old
            if ch[0, :].any() and ty > 0:
                marked.add((tx, ty - 1))
            if ch[-1, :].any() and y1 == y0 + tile and ty + 1 < nty:
                marked.add((tx, ty + 1))
            if ch[:, 0].any() and tx > 0:
                marked.add((tx - 1, ty))
            if ch[:, -1].any() and x1 == x0 + tile and tx + 1 < ntx:
                marked.add((tx + 1, ty))
        active = marked
    assert not active, "not converged within the bound"
    # the rim pass
    reached = dist < ob
    near = np.zeros_like(reached)
    near[:, 1:] |= reached[:, :-1]
    near[:, :-1] |= reached[:, 1:]
    near[1:, :] |= reached[:-1, :]
    near[:-1, :] |= reached[1:, :]
    dist[blocked & (dist != 0) & near] = ob
    return dist.astype(np.int32), rounds
