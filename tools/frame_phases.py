#!/usr/bin/env python3
"""Profiling aid: the time line of ONE k_frame launch of the C2 stream -- cycle stamps of thread 0 of every tile workgroup (fuse of the
previous sweep) and of every binning block (this sweep), put on a common clock per XCD (HW_REG_XCC_ID; the XCDs'
counters are not synchronised, so every XCD's earliest stamp is its zero).
The lean form's start stamps (tiles and binning blocks) are taken into registers where the wave starts and stored once the stamp
buffer's pointer has arrived (it is not among the preloaded head words), so a block's first phase and its life include the scalar
fetch of its arguments; the generic form's start stamp is stored through that pointer, behind the fetch.

    python tools/frame_phases.py [sweeps] [light=0]
"""
import ctypes as C
import sys
from pathlib import Path
import numpy as np
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from gem_amd import ElevationMap, synth, _lib

n_sw = next((int(a) for a in sys.argv[1:] if a.isdigit()), 8)
wl = synth.config_c4(n_sweeps=n_sw)
m = ElevationMap(wl.length, wl.resolution)
lib = _lib.load()
d = [torch.from_numpy(c).cuda() for c in wl.clouds]
for k in range(n_sw - 2):
    if k == max(0, n_sw - 5):                    # the last frames of the lead-in run stamped as well: the lean form's stamped kernel is a
        m.synchronize()                          # kernel of its own (k_frame_stamped), and its first launch would be timed with cold code
        assert lib.gem_debug_set(m._h, b"dbg_frame", 1) == 0
        lib.gem_debug_fuse_stamps(m._h, 1, None, 0)
    m.add(wl.frames[k], d[k])
m.synchronize()
assert lib.gem_debug_set(m._h, b"dbg_frame", 1) == 0
lib.gem_debug_fuse_stamps(m._h, 1, None, 0)
m.add(wl.frames[n_sw - 2], d[n_sw - 2])          # binning alone (the synchronisation above flushed the deferred fuse)
m.add(wl.frames[n_sw - 1], d[n_sw - 1])          # k_frame: fuse of sweep n-2 + binning of sweep n-1  <- the launch whose stamps are read
ROWS = 8192
buf = np.zeros((ROWS, 16), np.uint64)
n = lib.gem_debug_fuse_stamps(m._h, 0, buf.ctypes.data_as(C.c_void_p), ROWS)
st = buf[:n].astype(np.int64)
T = ((wl.length + 15) // 16) ** 2
tiles, bins = st[:T], st[T:]
# records per tile of the sweep the stamped launch fuses, from the CPU oracle's projection (the C2 map does not move: a tile's row of
# stamps is its circular-buffer tile, which is its geographic one)
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
import oracle
oracle.build()
_c = wl.clouds[n_sw - 2]
_idx = np.asarray(oracle.OracleMap(wl.length, wl.resolution).process_points(wl.frames[n_sw - 2], _c[:, 0], _c[:, 1], _c[:, 2])["index"])
_idx = _idx[_idx >= 0]
_tpr = (wl.length + 15) // 16
nrec = np.bincount(((_idx // wl.length) >> 4) * _tpr + ((_idx % wl.length) >> 4), minlength=T)[:T]
nrec = nrec[tiles[:, 15] > 0]
tiles = tiles[tiles[:, 15] > 0]; bins = bins[bins[:, 15] > 0]
blk_t = tiles[:, 15] - 1; blk_b = bins[:, 15] - 1
nst = (tiles[:, :12] > 0).sum(1)
# time line on s_memrealtime (100 MHz, one clock for the whole chip): 10 ns ticks
rt0 = min(tiles[:, 12].min(), bins[:, 12].min() if len(bins) else tiles[:, 12].min())
ts, te = (tiles[:, 12] - rt0) / 100.0, (tiles[:, 13] - rt0) / 100.0             # us
bs, be = (bins[:, 12] - rt0) / 100.0, (bins[:, 13] - rt0) / 100.0
xt = tiles[:, 14] - 1
print(f"k_frame: {len(tiles)} tile workgroups with stamps, {len(bins)} binning blocks; stamps per tile hist {np.bincount(nst).tolist()}")
print("workgroups per XCD (HW_REG_XCC_ID):", np.bincount(np.concatenate([xt, bins[:, 14] - 1]), minlength=8).tolist())
print(f"first start -> last tile end {te.max():.2f} us; last binning block end {be.max() if len(be) else 0:.2f} us")
step = 0.5
edges = np.arange(0, max(te.max(), be.max() if len(be) else 0) + step, step)
print("window (us)     tiles starting  tiles ending  bin blocks starting  bin blocks ending")
for a_, b_ in zip(edges[:-1], edges[1:]):
    print(f"  [{a_:4.1f},{b_:4.1f})   {((ts >= a_) & (ts < b_)).sum():8d}      {((te >= a_) & (te < b_)).sum():8d}      {((bs >= a_) & (bs < b_)).sum():8d}           {((be >= a_) & (be < b_)).sum():8d}")
dur = tiles[np.arange(len(tiles)), nst - 1] - tiles[:, 0]                        # cycles (the workgroup's own counter)
NS = int(nst.max())                                                              # stamps of a tile that took the fast path
full = nst == NS

if NS == 7:     # libraries before the per-tile buckets: the unit-indexed descriptor table
    names = ["flags (round trip 1)", "descriptor words (round trip 2)", "scan + list", "records in LDS + ranks (round trip 3)", "chains", "stores"]
else:           # per-tile buckets (frame_tile)
    names = ["loads issued", "count + records + tile (round trip)", "ranks", "sort + chains", "stores"]
if full.any():
    dd = np.diff(tiles[full, :NS], axis=1)
    print("tiles with records:", int(full.sum()), "| mean cycles per phase:", dict(zip(names, dd.mean(0).astype(int).tolist())))
    order = np.argsort(-dur)
    for i in order[:5]:
        print(f"  slow tile: block {blk_t[i]:5d} start {ts[i]:6.2f} us end {te[i]:6.2f} us total {dur[i]:6d} cycles, phases {np.diff(tiles[i, :nst[i]]).tolist()}")
    late = np.argsort(-te)[:5]
    for i in late:
        print(f"  last to end: block {blk_t[i]:5d} start {ts[i]:6.2f} us end {te[i]:6.2f} us total {dur[i]:6d} cycles ({dur[i] / max(1e-9, (te[i] - ts[i])) / 1000:.2f} GHz)")
if full.any():
    # the tiles the launch waits for: more than kFrameSpec = 256 records (a second, dependent DMA round trip)
    SPEC, MID = 256, 64
    print(f"weight classes (oracle): {int((nrec > SPEC).sum())} tiles above {SPEC} records, {int(((nrec > MID) & (nrec <= SPEC)).sum())} with {MID + 1}..{SPEC}, "
          f"{int(((nrec > 0) & (nrec <= MID)).sum())} with 1..{MID}; largest {int(nrec.max())}")
    # a tile of at most MID records takes the light path (GEM_FRAME_LIGHT, the default; `light=0` as the last argument names the phases
    # of a build without it): wave 0 alone, six stamps with their own meaning
    light_names = ["count + own records, cell loads issued", "lanes grouped by cell, verdict, barrier", "ranks, rank rows", "cells arrived, chains", "stores"]
    has_light = NS == 6 and "light=0" not in sys.argv[1:]
    for label, sel in ((f"tiles above {SPEC} records", full & (nrec > SPEC)), (f"tiles of at most {MID} records", full & (nrec > 0) & (nrec <= MID))):
        if sel.any():
            dh = np.diff(tiles[sel, :NS], axis=1)
            names_ = light_names if has_light and label.startswith("tiles of at most") else names
            print(f"{label}{' (light path)' if names_ is light_names else ''}: {int(sel.sum())} | mean cycles per phase: {dict(zip(names_, dh.mean(0).astype(int).tolist()))} | mean total {int(dur[sel].mean())} "
                  f"| mean life {(te[sel] - ts[sel]).mean():.2f} us | last end {te[sel].max():.2f} us")
print("tiles that left early (no record) or took another path:", int((nst < NS).sum()), "mean life", int(dur[nst < NS].mean()) if (nst < NS).any() else 0)
if len(bins):
    print(f"binning blocks: mean life {(be - bs).mean():.2f} us, max {(be - bs).max():.2f} | first start {bs.min():.2f} us, last start {bs.max():.2f} us")
