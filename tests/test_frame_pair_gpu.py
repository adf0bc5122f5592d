"""Two sweeps per k_frame launch (gem_amd/csrc/gem_frame_pair.hpp, gem_frame_pair.hip) against the CPU oracle, bit for bit: elevation
and variance, plus lowest where tracking is switched on between runs.  Maps of 32, 40 and 272 cells.

A handle that has seen two pairable gem_add_device calls in a row holds every other call and launches one grid for two sweeps;
whatever observes or modifies the map settles a held sweep first.  PairModel below is the policy written down once more, in
Python: every test asserts the counters "frame_pairs" and "frame_held_flushed" against what it gives for the test's own sequence
of calls, so a test that never pairs fails.
- runs of 1..7 adds between two reads, cycling: eager first call, single k_frame, held, pair, flush with and without a held sweep;
- sweep contents: sweeps of 1 / 63 / 64 / 65 / 255 / 256 / 257 / 1025 points built cell by cell so that one tile holds 0 or 64
  records in A with 1 in B, 64 + 64, 256 + 257, 513 + 257 (the second round trip), and one cell 7 + 7;
- the two sweeps of a pair carry different poses; the same device tensor for both sweeps of a pair;
- a cell of eight in A, or in B, of a pair: the slow path runs, the host is told, the handle stops pairing, the map is right;
- interruptions between the calls of a would-be pair, each of which must flush; set_timing, which must not;
- two handles taking turns; the node patterns (add, read) and (add, add, read), which never pair; a caller-provided stream, where
  nothing is ever held; the knob; the 16-sweep C2 stream's digest with pairing on."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from gem_amd import ElevationMap, SensorModel, synth

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
F32 = np.float32
RES = 0.1
LAYERS = ("elevation", "variance")


# ---- the policy, once more (gem_frame_pair.hpp: frame_pair_step) ---------------------------------------------------------------------
class PairModel:
    def __init__(self):
        self.streak, self.deferred, self.held = 0, 0, False
        self.pairs, self.held_flushed, self.launches = 0, 0, 0

    def _launch(self, fuse, binned):
        self.launches += max(fuse, binned)              # ("frame_lean_launches" counts a launch of two sweeps as the two it stands for)
        self.pairs += 1 if (fuse == 2 or binned == 2) else 0
        self.deferred, self.held = binned, False

    def flush(self, lean=True):
        """lean=False: a tile has reported the slow path, so the launches are the single generic ones a launch of two stands for"""
        pairs = self.pairs
        if self.held:
            self._launch(self.deferred, 1)
            self.held_flushed += 1
        if self.deferred:
            self._launch(self.deferred, 0)
        self.streak = 0
        if not lean:
            self.pairs = pairs

    def add(self, pairable=True):
        if not pairable:                                # an add of k_frame's single form
            if self.held or self.deferred == 2:
                self.flush()
            self.streak = 0
            self._launch(self.deferred, 1)
        elif self.held:
            self._launch(self.deferred, 2)
            self.streak += 1
        elif self.streak >= 2:
            self.held = True
            self.streak += 1
        else:
            self._launch(self.deferred, 1)
            self.streak += 1


def counters(gpu):
    return gpu.debug_get("frame_pairs"), gpu.debug_get("frame_held_flushed")


def assert_counters(gpu, model):
    assert counters(gpu) == (model.pairs, model.held_flushed), (counters(gpu), (model.pairs, model.held_flushed))


# ---- clouds ----------------------------------------------------------------------------------------------------------------------------
def frame_at(x=0.0, y=0.0, yaw=0.0):
    return synth._frame_for(synth.pose_matrix(x, y, 0.0, yaw=yaw), SensorModel.velodyne())


POSES = [(0.0, 0.0, 0.0), (0.04, -0.03, 0.02), (-0.05, 0.02, -0.03), (0.02, 0.05, 0.04)]      # (a pair's two sweeps never share one)


def blob(rng, n, half):
    c = np.zeros((n, 4), F32)
    c[:, 0] = rng.uniform(-half, half, n)
    c[:, 1] = rng.uniform(-half, half, n)
    c[:, 2] = rng.normal(0.0, 0.2, n)
    c[:, 3] = 1.0
    return c


def records(oracle_mod, L, frame, cloud):
    """the storage cell of every point of a sweep (-1: none), from the oracle's own projection into a fresh map"""
    o = oracle_mod.OracleMap(L, RES)
    return np.asarray(o.process_points(frame, cloud[:, 0], cloud[:, 1], cloud[:, 2])["index"])


def tile_of(idx, L):
    return (idx // L >> 4) * ((L + 15) // 16) + (idx % L >> 4)


def loads(oracle_mod, L, frame, cloud):
    idx = records(oracle_mod, L, frame, cloud)
    idx = idx[idx >= 0]
    if idx.size == 0:
        return 0, 0
    return int(np.bincount(tile_of(idx, L)).max()), int(np.bincount(idx).max())


_CENTRES = {}


def centres(oracle_mod, L, pose):
    """[L * L, 2]: a sensor-frame position that lands in each storage cell under this pose (NaN: none found), by probing"""
    key = (L, pose)
    if key not in _CENTRES:
        half = 0.5 * L * RES + 0.3
        g = np.arange(-half, half, RES / 4, dtype=np.float64)
        xs, ys = np.meshgrid(g, g, indexing="ij")
        probe = np.zeros((xs.size, 4), F32)
        probe[:, 0], probe[:, 1], probe[:, 3] = xs.ravel(), ys.ravel(), 1.0
        idx = records(oracle_mod, L, frame_at(*pose), probe)
        ok = idx >= 0
        cnt = np.bincount(idx[ok], minlength=L * L).astype(np.float64)
        c = np.full((L * L, 2), np.nan)
        with np.errstate(invalid="ignore", divide="ignore"):
            c[:, 0] = np.bincount(idx[ok], weights=probe[ok, 0].astype(np.float64), minlength=L * L) / cnt
            c[:, 1] = np.bincount(idx[ok], weights=probe[ok, 1].astype(np.float64), minlength=L * L) / cnt
        c[cnt < 4] = np.nan                                   # (a cell only grazed: its mean may sit on the border)
        _CENTRES[key] = c
    return _CENTRES[key]


def built_sweep(oracle_mod, rng, L, pose, tile_rc, in_tile, total, one_cell=0):
    """A sweep of `total` points: `in_tile` of them in the 16x16 tile (tr, tc), dealt round-robin over its cells (`one_cell` of them
    in its first cell instead), the rest round-robin over the cells of the other tiles -- in random order.  Checked against the
    oracle's projection before it is returned."""
    c = centres(oracle_mod, L, pose)
    rows, cols = np.divmod(np.arange(L * L), L)
    inside = ((rows >> 4) == tile_rc[0]) & ((cols >> 4) == tile_rc[1])
    have = ~np.isnan(c[:, 0])
    tcells = np.flatnonzero(inside & have)
    ocells = np.flatnonzero(~inside & have)
    assert tcells.size == 256 and ocells.size >= 256, (tcells.size, ocells.size)
    cells = [np.full(one_cell, tcells[0]), tcells[1 + np.arange(in_tile - one_cell) % 255] if one_cell else tcells[np.arange(in_tile) % 256],
             ocells[(np.arange(total - in_tile) * 7) % ocells.size]]
    cells = rng.permutation(np.concatenate(cells).astype(np.int64))
    assert cells.size == total
    cloud = np.zeros((total, 4), F32)
    cloud[:, 0], cloud[:, 1] = c[cells, 0], c[cells, 1]
    cloud[:, 2] = rng.normal(0.0, 0.2, total)
    cloud[:, 3] = 1.0
    idx = records(oracle_mod, L, frame_at(*pose), cloud)
    assert np.array_equal(idx, cells), "a built point landed in another cell"
    return cloud


# ---- streams: the same calls to the oracle and to the device -----------------------------------------------------------------------------
class Stream:
    """Calls go to the oracle, the device map and the policy model alike; read() compares the layers bit for bit."""

    def __init__(self, oracle_mod, L, debug=None, name=""):
        import torch
        self.torch, self.L, self.name = torch, L, name
        self.ref = oracle_mod.OracleMap(L, RES)
        self.gpu = ElevationMap(L, RES, debug=debug or {"frame_pair": 1})
        self.model = PairModel()
        self.pairing = True                              # what the model takes a plain device add for
        self.track = False
        self.dev = {}

    def tensor(self, cloud):
        if id(cloud) not in self.dev:
            self.dev[id(cloud)] = (cloud, self.torch.from_numpy(cloud).cuda())
            self.torch.cuda.synchronize()
        return self.dev[id(cloud)][1]

    def add(self, pose, cloud, pairable=None):
        self.ref.add(frame_at(*pose), cloud)
        self.gpu.add(frame_at(*pose), self.tensor(cloud))
        self.model.add(self.pairing if pairable is None else pairable)

    def read(self, lean=True):
        self.model.flush(lean)
        for n in LAYERS + (("lowest",) if self.track else ()):
            g, o = self.gpu.layer(n), self.ref.layer(n)
            assert np.array_equal(g, o), f"{self.name}: {n} differs in {np.count_nonzero(g != o)} cells"
        assert_counters(self.gpu, self.model)

    def close(self):
        self.gpu.close()


def clean_clouds(oracle_mod, L, seed, sizes):
    rng = np.random.default_rng(seed)
    out = [blob(rng, n, 0.45 * L * RES) for n in sizes]
    for k, c in enumerate(out):
        for p in POSES:
            t, cm = loads(oracle_mod, L, frame_at(*p), c)
            assert t <= 768 and cm <= 7, (k, t, cm)
    return out


SIZES = {32: (300, 257, 200, 333), 40: (400, 513, 300, 257), 272: (5003, 3000, 4000, 2049)}


# ---- 1. runs of 1..7 adds between two reads ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [32, 40, 272])
def test_runs_between_reads(oracle_mod, L):
    clouds = clean_clouds(oracle_mod, L, 40 + L, SIZES[L])
    s = Stream(oracle_mod, L, name=f"runs{L}")
    k = 0
    for run in (1, 2, 3, 4, 5, 6, 7, 3, 1, 4):
        for _ in range(run):
            s.add(POSES[k % 4], clouds[k % 4 if k % 3 else (k + 1) % 4])
            k += 1
        s.read()
    assert s.model.pairs >= 8 and s.model.held_flushed >= 3, (s.model.pairs, s.model.held_flushed)     # (the sequence visits every state)
    s.close()


# ---- 2. sweep contents ------------------------------------------------------------------------------------------------------------------
#       records of the tile in A, in B | points of sweep A, of B | of those in ONE cell of the tile in A, in B
CONTENTS = [(0, 1, 63, 1, 0, 0), (64, 1, 64, 65, 0, 0), (64, 64, 255, 256, 0, 0), (256, 257, 256, 257, 0, 0), (513, 257, 1025, 257, 0, 0),
            (40, 30, 65, 255, 7, 7)]


@pytest.mark.parametrize("ta,tb,na,nb,ca,cb", CONTENTS)
def test_sweep_contents(oracle_mod, ta, tb, na, nb, ca, cb):
    L, tile = 40, (1, 1)
    rng = np.random.default_rng(ta * 1000 + tb)
    fill = clean_clouds(oracle_mod, L, 7, (300, 200))
    A = built_sweep(oracle_mod, rng, L, POSES[2], tile, ta, na, ca)
    B = built_sweep(oracle_mod, rng, L, POSES[3], tile, tb, nb, cb)
    for sw, p, t_want, c_want in ((A, POSES[2], ta, ca), (B, POSES[3], tb, cb)):
        idx = records(oracle_mod, L, frame_at(*p), sw)
        in_tile = int(np.count_nonzero(tile_of(idx, L) == tile[0] * 3 + tile[1]))
        assert in_tile == t_want and int(np.bincount(idx).max()) <= 7, (in_tile, t_want)
        if c_want:
            assert int(np.bincount(idx).max()) == c_want
    s = Stream(oracle_mod, L, name=f"contents{ta}+{tb}")
    s.add(POSES[0], fill[0]); s.add(POSES[1], fill[1])
    s.add(POSES[2], A)                                   # held
    s.add(POSES[3], B)                                   # one launch bins A and B (and fuses the sweep before)
    s.add(POSES[0], fill[0])                             # held
    s.add(POSES[1], fill[1])                             # one launch fuses A, then B
    s.read()
    assert s.model.pairs == 3 and s.gpu.debug_get("frame_form_seen") == 0
    # ... and once more with A held by the flush: fuse(previous) || bin(A), the fuse-only launch of A; B as an eager first call
    s.add(POSES[0], fill[0]); s.add(POSES[1], fill[1]); s.add(POSES[2], A)
    s.read()
    s.add(POSES[3], B)
    s.read()
    assert s.model.held_flushed == 1
    s.close()


# ---- 3. the same device tensor for both sweeps of a pair, under two poses ---------------------------------------------------------------
@pytest.mark.parametrize("L", [40, 272])
def test_shared_buffer(oracle_mod, L):
    clouds = clean_clouds(oracle_mod, L, 50 + L, SIZES[L][:2])
    s = Stream(oracle_mod, L, name=f"shared{L}")
    for k in range(8):
        s.add(POSES[k % 4], clouds[0])                   # every pair: one tensor, two poses
    s.read()
    assert s.model.pairs == 4                            # three launches of two, and the fuse-only launch of a pair
    s.close()


# ---- 4. a cell of eight: the slow path, the descriptor form, no more pairs --------------------------------------------------------------
@pytest.mark.parametrize("where", ["A", "B"])
def test_cell_of_eight(oracle_mod, where):
    L, tile = 40, (1, 1)
    rng = np.random.default_rng(80)
    fill = clean_clouds(oracle_mod, L, 8, (300, 200))
    heavy = built_sweep(oracle_mod, rng, L, POSES[2 if where == "A" else 3], tile, 60, 257, 8)
    light = built_sweep(oracle_mod, rng, L, POSES[3 if where == "A" else 2], tile, 64, 129)
    A, B = (heavy, light) if where == "A" else (light, heavy)
    s = Stream(oracle_mod, L, name=f"eight-{where}")
    s.add(POSES[0], fill[0]); s.add(POSES[1], fill[1])
    s.add(POSES[2], A); s.add(POSES[3], B)               # binned by one launch
    s.add(POSES[0], fill[0]); s.add(POSES[1], fill[1])   # fused by one launch: the pair kernel's slow path
    s.torch.cuda.synchronize()                           # (the device alone: the handle is not touched, nothing is flushed)
    assert s.gpu.debug_get("frame_form_seen") == 1 and s.model.pairs == 2
    s.read(lean=False)                                   # the pair still deferred is fused by two generic launches
    # the host has seen the word: every launch is the generic single one from here on, nothing is held
    s.pairing = False
    before = s.gpu.debug_get("frame_lean_launches")
    for k in range(6):
        s.add(POSES[k % 4], fill[k % 2])
    s.read()
    assert s.gpu.debug_get("frame_lean_launches") == before
    s.close()


# ---- 5. interruptions -------------------------------------------------------------------------------------------------------------------
def _move(s, fill):
    s.ref.move(np.array([0.35, -0.2, 0.0], F32)); s.gpu.move(np.array([0.35, -0.2, 0.0], F32))
    s.model.flush()


def _mapvar(s, fill):
    s.ref.mapvar_update(1e-4); s.gpu.mapvar_update(1e-4)
    s.model.flush()


def _lowest(s, fill):
    s.gpu.set_lowest_tracking(True)
    s.gpu.set_layer("lowest", s.ref.layer("lowest"))     # (the oracle always tracks: both go on from the same layer)
    s.track, s.pairing = True, False                     # sweeps with lowest tracking take the single form
    s.model.flush()


def _counting(s, fill):
    s.gpu.set_counting(True)
    s.pairing = None                                     # counting: no k_frame at all (every add fuses at once)
    s.model.flush()


def _host_add(s, fill):
    s.ref.add(frame_at(*POSES[1]), fill[1]); s.gpu.add(frame_at(*POSES[1]), fill[1])
    s.model.add(False)                                   # (staged into the handle's own memory: k_frame's single form, never held)


def _coloured(s, fill):
    rgb = np.arange(fill[1].shape[0], dtype=np.uint32) * 2654435761 % (1 << 24)
    s.ref.add(frame_at(*POSES[1]), fill[1], rgb=rgb)
    s.gpu.add(frame_at(*POSES[1]), s.tensor(fill[1]), rgb=s.torch.from_numpy(rgb.astype(np.int32)).cuda())
    s.model.flush()


def _zero(s, fill):
    s.gpu.add(frame_at(*POSES[1]), s.torch.zeros((0, 4), dtype=s.torch.float32, device="cuda"))
    s.model.flush()


def _batch(s, fill):
    both = s.torch.from_numpy(np.concatenate([fill[0], fill[1]])).cuda()
    s.torch.cuda.synchronize()
    s.ref.add(frame_at(*POSES[2]), fill[0]); s.ref.add(frame_at(*POSES[3]), fill[1])
    s.gpu.add_batch([frame_at(*POSES[2]), frame_at(*POSES[3])], both, offsets=[0, fill[0].shape[0], fill[0].shape[0] + fill[1].shape[0]])
    s.model.flush()


INTERRUPTIONS = {"move": _move, "mapvar_update": _mapvar, "set_lowest_tracking": _lowest, "set_counting": _counting, "host_add": _host_add,
                 "coloured_add": _coloured, "zero_point_add": _zero, "add_batch": _batch}


@pytest.mark.parametrize("what", list(INTERRUPTIONS))
def test_interruption_flushes(oracle_mod, what):
    L = 40
    fill = clean_clouds(oracle_mod, L, 9, (300, 200))
    s = Stream(oracle_mod, L, name=what)
    for k in range(3):
        s.add(POSES[k], fill[k % 2])                     # the third is held
    assert s.model.held
    INTERRUPTIONS[what](s, fill)
    assert not s.model.held
    assert_counters(s.gpu, s.model)                      # the held sweep has been settled: by the flush, not by a pair
    assert s.model.held_flushed == 1 and s.model.pairs == 0
    if s.pairing is None:                                # (counting: the model's launches do not describe the adds that follow)
        for k in range(3):
            s.ref.add(frame_at(*POSES[k]), fill[k % 2]); s.gpu.add(frame_at(*POSES[k]), s.tensor(fill[k % 2]))
    else:
        for k in range(4):
            s.add(POSES[k], fill[k % 2])                 # ... and the stream goes on: singles, held, a pair (while it may)
    s.read()
    if s.pairing:
        assert s.model.pairs == 2, s.model.pairs         # the launch of two and the fuse-only launch behind it
    s.close()


def test_set_timing_neither_flushes_nor_unpairs(oracle_mod):
    L = 40
    fill = clean_clouds(oracle_mod, L, 9, (300, 200))
    s = Stream(oracle_mod, L, name="timing")
    for k in range(3):
        s.add(POSES[k], fill[k % 2])
    s.gpu.set_timing(True)
    assert_counters(s.gpu, s.model)
    assert s.model.held and s.model.held_flushed == 0
    for k in range(3):
        s.add(POSES[k], fill[k % 2])                     # a launch of two (timed), a held sweep, a launch of two (timed)
    st = s.gpu.stats()                                   # (settles: the fuse-only launch of the pair)
    s.model.flush()
    assert_counters(s.gpu, s.model)
    assert s.model.pairs == 3 and s.model.held_flushed == 0
    assert st["launches_frame"] == 4 and st["launches_fuse"] == 1, st      # launches_frame counts SWEEPS: two launches of two
    s.read()
    s.close()


# ---- 6. two handles, call by call ---------------------------------------------------------------------------------------------------------
def test_two_handles(oracle_mod):
    a = Stream(oracle_mod, 40, name="two-40")
    b = Stream(oracle_mod, 272, name="two-272")
    ca, cb = clean_clouds(oracle_mod, 40, 90, SIZES[40]), clean_clouds(oracle_mod, 272, 312, SIZES[272])
    for k in range(9):
        a.add(POSES[k % 4], ca[k % 4])
        b.add(POSES[(k + 1) % 4], cb[k % 4])
        if k == 4:
            b.read()
    a.read(); b.read()
    assert a.model.pairs == 4 and a.model.held_flushed == 1 and b.model.pairs == 4      # (nine adds: three launches of two, and the flush bins the held ninth beside the fuse of a pair)
    a.close(); b.close()


# ---- 7. the node patterns never pair and launch what they always did --------------------------------------------------------------------
@pytest.mark.parametrize("adds", [1, 2])
def test_node_patterns(oracle_mod, adds):
    L = 40
    fill = clean_clouds(oracle_mod, L, 9, (300, 200))
    s = Stream(oracle_mod, L, name=f"node{adds}")
    for r in range(8):
        for k in range(adds):
            s.add(POSES[(r + k) % 4], fill[k])
        s.read()
    assert counters(s.gpu) == (0, 0)
    # add, read: the binning and the fuse-only launch; add, add, read: the binning, one k_frame, the fuse-only launch
    assert s.gpu.debug_get("frame_lean_launches") == 8 * (adds + 1) and s.gpu.debug_get("frame_generic_launches") == 0
    s.close()


# ---- 8. a caller-provided stream: the work is on that stream when the call returns --------------------------------------------------------
def test_caller_stream_never_holds(oracle_mod):
    import torch
    L = 40
    fill = clean_clouds(oracle_mod, L, 9, (300, 200))
    s = Stream(oracle_mod, L, name="caller-stream")
    st = torch.cuda.Stream()
    s.gpu.set_stream(st.cuda_stream)
    s.pairing = False
    for k in range(7):
        s.add(POSES[k % 4], fill[k % 2])
        assert counters(s.gpu) == (0, 0)
    s.read()
    assert s.gpu.debug_get("frame_lean_launches") == 8   # the binning, six k_frame, the fuse-only launch: as ever
    s.gpu.set_stream(None)
    s.close()


# ---- 9. the knob ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [32, 272])
def test_knob_off(oracle_mod, L):
    clouds = clean_clouds(oracle_mod, L, 40 + L, SIZES[L])
    s = Stream(oracle_mod, L, debug={"frame_pair": 0}, name=f"knob{L}")
    s.pairing = False
    for k in range(9):
        s.add(POSES[k % 4], clouds[k % 4])
    s.read()
    assert counters(s.gpu) == (0, 0) and s.gpu.debug_get("frame_lean_launches") == 10
    s.close()


# ---- 10. the C2 stream of bench.py, pairing on ------------------------------------------------------------------------------------------
def test_c2_stream_digest():
    import torch
    d = json.loads((Path(__file__).resolve().parent / "golden" / "digests.json").read_text())["c2_stream16"]
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    wl = synth.config_c4(n_sweeps=8, seed0=100)
    assert sha(np.concatenate(wl.clouds)) == d["cloud"], "generator drift"
    dc = [torch.from_numpy(c).cuda() for c in wl.clouds]
    torch.cuda.synchronize()
    m = ElevationMap(wl.length, wl.resolution, debug={"frame_pair": 1})
    model = PairModel()
    for k in range(16):
        m.add(wl.frames[k % 8], dc[k % 8])
        model.add()
    assert sha(m.layer("elevation")) == d["elevation"] and sha(m.layer("variance")) == d["variance"]
    model.flush()
    assert_counters(m, model)
    assert model.pairs == 8 and m.debug_get("frame_form_seen") == 0
    m.close()
