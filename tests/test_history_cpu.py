"""The history cloud (gem_history_*, gem_costmap_mark_history) without a GPU: hand-computed known answers for the restatement the GPU
tests compare the device with (tests/history_ref.py) -- the box of a block, the culling rule at each of the four edges -- the property
that makes culling exact (no record worldToMap accepts lies in a culled block) over random windows, resolutions and clouds, the
symbols, and that the C++ gem::History builds."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))

import costmap_ref as cref  # noqa: E402
import history_ref as ref  # noqa: E402
from local_ref import POINT  # noqa: E402

F32 = np.float32
NAN, INF = np.nan, np.inf


def records(x, y, travers=0.9):
    r = np.zeros(len(x), POINT)
    r["x"], r["y"], r["travers"] = x, y, travers
    return r


# ---- the box of a block -------------------------------------------------------------------------------------------------------------
def test_box_known_answers():
    assert ref.box_of([1.0, -2.0, 3.0], [0.5, 0.25, -0.75]) == (-2.0, -0.75, 3.0, 0.5)
    assert ref.box_of([NAN, 1.0, NAN], [2.0, NAN, NAN]) == (1.0, 2.0, 1.0, 2.0)                  # NaN is ignored, per coordinate
    assert ref.box_of([1.0, INF], [-INF, 2.0]) == (1.0, -INF, INF, 2.0)                          # an inf only widens the box
    assert ref.box_of([NAN, NAN], [NAN, NAN]) == ref.EMPTY_BOX == (INF, INF, -INF, -INF)         # no coordinate at all
    assert ref.box_of([NAN, 4.0], [NAN, NAN]) == (4.0, INF, 4.0, -INF)                           # ... in one of them
    assert ref.box_of([0.1], [0.2]) == (float(F32(0.1)), float(F32(0.2)), float(F32(0.1)), float(F32(0.2)))   # floats, not doubles


def test_box_table_blocks_and_a_partial_last_block():
    n = 2 * ref.BLOCK + 3
    x, y = np.arange(n, dtype=F32), -np.arange(n, dtype=F32)
    x[5], y[ref.BLOCK] = NAN, NAN
    x[ref.BLOCK + 1] = -INF
    rec = records(x, y)
    t = ref.boxes(rec)
    B = ref.BLOCK
    assert t.shape == (3, 4) and t.dtype == F32 and ref.n_blocks(n) == 3
    assert t[0].tolist() == [0.0, -(B - 1), B - 1, 0.0]
    assert t[1].tolist() == [-INF, -(2 * B - 1), 2 * B - 1, -(B + 1)]
    assert t[2].tolist() == [2 * B, -(2 * B + 2), 2 * B + 2, -(2 * B)]                           # three records
    for b in range(3):                                                                            # the vectorised table is the literal fold
        assert tuple(t[b].tolist()) == ref.box_of(x[b * B:(b + 1) * B], y[b * B:(b + 1) * B])
    rec["x"][2 * B:], rec["y"][2 * B:] = NAN, NAN
    assert tuple(ref.boxes(rec)[2].tolist()) == ref.EMPTY_BOX
    assert ref.n_blocks(0) == 0 and ref.n_blocks(1) == 1 and ref.n_blocks(B) == 1 and ref.n_blocks(B + 1) == 2
    assert ref.boxes(records([], [])).shape == (0, 4)


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
def test_cull_rule_known_answers_at_the_four_edges():
    cm = cref.Costmap(10, 6, 0.5, origin_x=-3.0, origin_y=2.0)          # [-3, 2) x [2, 5); everything here is exact in binary
    ox, oy, ex, ey = -3.0, 2.0, 2.0, 5.0
    below = lambda v: float(np.nextafter(F32(v), F32(-INF)))
    point = lambda x, y: (x, y, x, y)                                   # the box of a single record
    mid_x, mid_y = -1.0, 3.0
    assert ref.cull_exact(cm)
    # near edges: a record exactly on the origin is in the map and must be kept; the next float below it is refused and culled
    assert cref.world_to_map(cm, ox, mid_y) == (0, 2) and not ref.culled(cm, point(ox, mid_y))
    assert cref.world_to_map(cm, mid_x, oy) == (4, 0) and not ref.culled(cm, point(mid_x, oy))
    assert cref.world_to_map(cm, below(ox), mid_y) is None and ref.culled(cm, point(below(ox), mid_y))
    assert cref.world_to_map(cm, mid_x, below(oy)) is None and ref.culled(cm, point(mid_x, below(oy)))
    # far edges: a record on origin + size * res is refused, but inside the margin cell: kept (conservative, not tight) ...
    assert cref.world_to_map(cm, ex, mid_y) is None and not ref.culled(cm, point(ex, mid_y))
    assert cref.world_to_map(cm, mid_x, ey) is None and not ref.culled(cm, point(mid_x, ey))
    assert cref.world_to_map(cm, below(ex), mid_y) == (9, 2) and not ref.culled(cm, point(below(ex), mid_y))
    # ... and culled from origin + (size + 1) * res on
    assert not ref.culled(cm, point(below(ex + 0.5), mid_y)) and ref.culled(cm, point(ex + 0.5, mid_y))
    assert not ref.culled(cm, point(mid_x, below(ey + 0.5))) and ref.culled(cm, point(mid_x, ey + 0.5))
    # boxes: one that straddles an edge is kept, one that spans the whole map is kept, the empty one and infinite ones off the map go
    assert not ref.culled(cm, (-10.0, 3.0, ox, 3.0)) and ref.culled(cm, (-10.0, 3.0, below(ox), 3.0))
    assert not ref.culled(cm, (-100.0, -100.0, 100.0, 100.0)) and not ref.culled(cm, (-INF, -INF, INF, INF))
    assert ref.culled(cm, ref.EMPTY_BOX)
    assert ref.culled(cm, (INF, 3.0, INF, 3.0)) and ref.culled(cm, (-INF, 3.0, -INF, 3.0))
    assert ref.culled(cm, (INF, INF, -INF, 3.0)) and ref.culled(cm, (0.0, INF, 0.0, -INF))        # one coordinate without a value
    # a geometry whose far limit double cannot resolve: the rule is not applied at all
    far = cref.Costmap(10, 6, 0.5, origin_x=2.0 ** 57, origin_y=0.0)
    assert not ref.cull_exact(far) and not ref.culled_blocks(far, records([0.0], [0.0])).any()


def test_culled_blocks_of_a_small_history():
    cm = cref.Costmap(10, 6, 0.5, origin_x=-3.0, origin_y=2.0)
    B = ref.BLOCK
    x = np.concatenate([np.full(B, -1.0), np.full(B, 50.0), np.full(B, NAN), [-1.0, 50.0]]).astype(F32)
    rec = records(x, np.full(x.size, 3.0, F32))
    assert ref.culled_blocks(cm, rec).tolist() == [False, True, True, False]                      # inside, outside, all NaN, straddling
    assert ref.culled_blocks(cm, rec, cull=False).tolist() == [False] * 4
    rec["y"][:] = NAN
    assert ref.culled_blocks(cm, rec).all()


@pytest.mark.parametrize("seed", range(8))
def test_no_accepted_record_lies_in_a_culled_block(seed):
    """over random windows, resolutions and clouds with float coordinates on and around the edges"""
    rng = np.random.default_rng(seed)
    accepted_total = culled_total = 0
    for _ in range(60):
        sx, sy = int(rng.integers(1, 1200)), int(rng.integers(1, 1200))
        res = float(rng.choice([0.05, 0.1, 0.2, 0.25, 1.0 / 3.0, 1.0, float(rng.uniform(0.01, 5.0))]))
        scale = float(rng.choice([1.0, 100.0, 1e4, 1e6]))
        cm = cref.Costmap(sx, sy, res, rng.uniform(-scale, scale), rng.uniform(-scale, scale))
        if rng.random() < 0.5:                                           # an origin that is a float: records can sit exactly on it
            cm.ox, cm.oy = float(F32(cm.ox)), float(F32(cm.oy))
        assert ref.cull_exact(cm)
        n = 512
        edges_x = np.array([cm.ox, cm.ox + sx * res, cm.ox + (sx + 1) * res, cm.ox + (sx - 1) * res])
        edges_y = np.array([cm.oy, cm.oy + sy * res, cm.oy + (sy + 1) * res, cm.oy + (sy - 1) * res])
        x = np.where(rng.random(n) < 0.5, rng.choice(edges_x, n), cm.ox + rng.uniform(-0.5, 1.5, n) * sx * res).astype(F32)
        y = np.where(rng.random(n) < 0.5, rng.choice(edges_y, n), cm.oy + rng.uniform(-0.5, 1.5, n) * sy * res).astype(F32)
        for v in (x, y):                                                 # the floats next to those, both ways
            step = rng.integers(-2, 3, n)
            for _k in range(2):
                v[step > 0] = np.nextafter(v[step > 0], F32(INF)); v[step < 0] = np.nextafter(v[step < 0], F32(-INF))
                step = step - np.sign(step)
        x[rng.random(n) < 0.02] = NAN
        y[rng.random(n) < 0.02] = INF
        ok, _ = cref.world_to_map_v(cm, x, y)
        # every record as a block of its own (the tightest boxes there are), and blocks of a few neighbours
        single = np.array([ref.culled(cm, (x[i], y[i], x[i], y[i])) for i in range(n)])
        assert not (ok & single).any()
        for g in (4, 64):
            for lo in range(0, n, g):
                if ref.culled(cm, ref.box_of(x[lo:lo + g], y[lo:lo + g])):
                    assert not ok[lo:lo + g].any()
        accepted_total += int(ok.sum()); culled_total += int(single.sum())
    assert accepted_total > 3000 and culled_total > 3000                 # both sides of the rule were exercised


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def declared(header):
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(gem_[a-z_0-9]+)\s*\(", text)))


def test_history_symbols_are_declared_exported_and_bound():
    from gem_amd import _lib
    lib = _lib.load()
    names = declared(ROOT / "include" / "gem_hip_history.h")
    assert names == sorted(_lib.HISTORY_SIGNATURES) and len(names) == 8
    assert "gem_costmap_mark_history" in names and "gem_history_append_device" in names
    for n in names:
        fn = getattr(lib, n)
        assert fn.argtypes == _lib.HISTORY_SIGNATURES[n][1]
    assert '#include "gem_hip_history.h"' in (ROOT / "include" / "gem_hip.h").read_text()
    assert lib.gem_abi_version() == 9
    dbg = (ROOT / "include" / "gem_hip_debug.h").read_text()
    assert all(f'"{k}"' in dbg for k in ("history_cull", "history_blocks", "history_blocks_culled"))


def test_python_facade_has_the_history():
    from gem_amd import Costmap, ElevationMap
    import inspect
    for name in ("history_enable", "history_append", "history_reset_from_global", "history_clear", "history_size", "history_export"):
        assert callable(getattr(ElevationMap, name))
    assert callable(Costmap.mark_history)
    assert inspect.signature(ElevationMap.local_spill).parameters["download"].default is True


def build_history_check(out: Path) -> Path:
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc", "-std=c++17", "-O1", "-Wall", "-Werror",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "history_check.cpp"), "-o", str(out),
           f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_history_facade_builds():
    """gem::History and gem::Costmap::markHistory compile with hipcc against the installed header and the library; without a GPU the
    check exits early."""
    import tempfile
    from gem_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as td:
        exe = build_history_check(Path(td) / "history_check")
        res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: built)"), res.stdout + res.stderr
