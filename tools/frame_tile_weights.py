#!/usr/bin/env python3
"""Records per 16 x 16 tile of the C2 sweeps, from the CPU oracle alone (no GPU): what k_frame's tile workgroups carry.

    python tools/frame_tile_weights.py [sweeps] [seed0]

Every sweep of synth.config_c4 goes through the oracle's process_points on the unmoved map; the records kept are counted per tile.
Printed per sweep: the count classes frame_tile sets its waves' issue priority by (more than kFrameSpec = 256 records, 65..256,
1..64), records per tile by Chebyshev ring around the centre tile, and where the heavy tiles sit in dispatch order -- the block
indices frame_tile_of (gem_amd/csrc/gem_frame_lean.hpp) gives them, mirrored below."""
import sys
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "oracle"))
import oracle
from gem_amd import synth

RUN_BITS, SPEC, MID = 3, 256, 64                     # kFrameRunBits, kFrameSpec, the middle priority class's lower bound


def tile_of_block(block, tpr, ctr, ctc):
    """frame_tile_of: (tile row, tile column, ring) of a block, or None"""
    x, i = block & 7, block >> 3
    rnk = ((((i >> RUN_BITS) << 3) + x) << RUN_BITS) + (i & ((1 << RUN_BITS) - 1))
    if rnk >= tpr * tpr:
        return None
    bi, bj = divmod(rnk, tpr)
    oi = -((bi + 1) >> 1) if bi & 1 else bi >> 1
    cj, t = bj >> RUN_BITS, bj & ((1 << RUN_BITS) - 1)
    oj = -(((cj - 1) >> 1) << RUN_BITS) - 1 - t if cj & 1 else ((cj >> 1) << RUN_BITS) + t
    return (ctr + oi) % tpr, (ctc + oj) % tpr, max(abs(oi), abs(oj))


def main():
    n_sw = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    oracle.build()
    wl = synth.config_c4(n_sweeps=n_sw, seed0=seed0)
    L = wl.length
    tpr = (L + 15) // 16
    ctr = ctc = (L // 2) >> 4                        # the unmoved map: gem_capi_pipeline.cpp, fa.center_tr / center_tc
    nf = (tpr * tpr + (8 << RUN_BITS) - 1) & ~((8 << RUN_BITS) - 1)
    block_of, ring_of = {}, np.zeros((tpr, tpr), np.int64)
    for b in range(nf):
        t = tile_of_block(b, tpr, ctr, ctc)
        if t is not None:
            block_of[(t[0], t[1])] = b; ring_of[t[0], t[1]] = t[2]
    assert len(block_of) == tpr * tpr
    for k in range(n_sw):
        c = wl.clouds[k]
        o = oracle.OracleMap(L, wl.resolution)
        idx = np.asarray(o.process_points(wl.frames[k], c[:, 0], c[:, 1], c[:, 2])["index"])
        idx = idx[idx >= 0]
        per = np.zeros((tpr, tpr), np.int64)
        np.add.at(per, ((idx // L) >> 4, (idx % L) >> 4), 1)
        live = per[per > 0]
        print(f"sweep {k}: {idx.size} records kept, {live.size} live tiles of {tpr * tpr}; per live tile median {int(np.median(live))}, mean {live.mean():.0f}, largest {int(per.max())}")
        print(f"  tiles with 1..{MID} records {int(((per > 0) & (per <= MID)).sum())}, {MID + 1}..{SPEC} {int(((per > MID) & (per <= SPEC)).sum())}, "
              f"more than 128 {int((per > 128).sum())}, more than {SPEC} {int((per > SPEC).sum())}")
        heavy = per > SPEC
        if heavy.any():
            print(f"  tiles above {SPEC} records lie in rings {int(ring_of[heavy].min())}..{int(ring_of[heavy].max())}")
        for name, sel in ((f"above {SPEC}", heavy), ("above 128", per > 128)):
            blocks = np.array(sorted(block_of[(int(r), int(cc))] for r, cc in zip(*np.nonzero(sel))))
            if blocks.size:
                print(f"  blocks of the tiles {name}: {blocks.size} in [{blocks.min()}, {blocks.max()}], median {int(np.median(blocks))}; "
                      f"light tiles (at most 128 records) in front of the last one {int(sum(1 for (r, cc), b in block_of.items() if b < blocks.max() and per[r, cc] <= 128))}")
        if k == 0:
            print("  ring: tiles, mean records per tile, tiles above 256")
            for r in range(int(ring_of.max()) + 1):
                m = ring_of == r
                print(f"  {r:4d}: {int(m.sum()):5d} {per[m].mean():8.1f} {int((per[m] > SPEC).sum()):5d}")


if __name__ == "__main__":
    main()
