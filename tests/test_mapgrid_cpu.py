"""CPU tests of the MapGrid contract of include/gem_hip_mapgrid.h: the restatement itself (tests/mapgrid_ref.py: the literal queue
against the set form, known answers derived by hand), the host-only gem_mapgrid_adjust_plan against the restatement, and the ABI
(symbols, the include line, the Python and C++ facades).  Every comparison is exact."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import costmap_ref as cr  # noqa: E402
import mapgrid_ref as ref  # noqa: E402


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def random_case(rng, k):
    sy, sx = int(rng.integers(1, 41)), int(rng.integers(1, 41))
    share = (0.0, 0.1, 0.3, 0.5)[k % 4]
    g = rng.integers(0, 253, (sy, sx)).astype(np.uint8)
    blk = rng.random((sy, sx)) < share
    g[blk] = rng.integers(253, 256, int(blk.sum())).astype(np.uint8)
    n = int(rng.integers(1, 6))
    src = [(int(rng.integers(0, sx)), int(rng.integers(0, sy))) for _ in range(n)]
    if k % 3 == 0:
        src.append(src[0])                                               # a duplicate
    if k % 5 == 0 and blk.any():
        ys, xs = np.nonzero(blk)
        j = int(rng.integers(0, ys.size))
        src.append((int(xs[j]), int(ys[j])))                             # a source on a blocked cell
    return g, src


def test_literal_queue_equals_set_form_on_random_grids():
    rng = np.random.default_rng(20261019)
    on_blocked = 0
    for k in range(400):
        g, src = random_case(rng, k)
        on_blocked += any(g[y, x] >= 253 for x, y in src)
        a, b = ref.distance_queue(g, src), ref.distance_levels(g, src)
        assert a.dtype == np.int32 and a.tobytes() == b.tobytes(), (k, g.shape, src)
    assert on_blocked >= 40


def test_known_answer_empty_grid_centre_source():
    g = np.zeros((5, 5), np.uint8)
    want = np.array([[abs(x - 2) + abs(y - 2) for x in range(5)] for y in range(5)], np.int32)
    for f in (ref.distance_queue, ref.distance_levels):
        assert (f(g, [(2, 2)]) == want).all()


def test_known_answer_wall_with_one_gap():
    g = np.zeros((5, 5), np.uint8)
    g[0:4, 2] = 254
    OB = 25
    want = np.array([[0, 1, OB, 11, 12], [1, 2, OB, 10, 11], [2, 3, OB, 9, 10], [3, 4, OB, 8, 9], [4, 5, 6, 7, 8]], np.int32)
    for f in (ref.distance_queue, ref.distance_levels):
        assert (f(g, [(0, 0)]) == want).all()


def test_known_answer_enclosed_pocket():
    """a 7 x 7 grid, a two-cell-thick ring of 254 around the free centre cell (3, 3), the source outside at (0, 0): the pocket stays
    UN, the ring's outer face gets OB, the ring's inner cells touch no reached cell and stay UN"""
    g = np.zeros((7, 7), np.uint8)
    g[1:6, 1:6] = 254
    g[3, 3] = 0
    OB, UN = 49, 50
    d = [[0, 1, 2, 3, 4, 5, 6],
         [1, OB, OB, OB, OB, OB, 7],
         [2, OB, UN, UN, UN, OB, 8],
         [3, OB, UN, UN, UN, OB, 9],
         [4, OB, UN, UN, UN, OB, 10],
         [5, OB, OB, OB, OB, OB, 11],
         [6, 7, 8, 9, 10, 11, 12]]
    want = np.array(d, np.int32)
    for f in (ref.distance_queue, ref.distance_levels):
        assert (f(g, [(0, 0)]) == want).all()
    assert ref.constants(g) == (OB, UN)


def test_a_blocked_source_expands_and_keeps_zero():
    g = np.zeros((3, 4), np.uint8)
    g[1, 1] = 253
    g[1, 2] = 255
    for f in (ref.distance_queue, ref.distance_levels):
        d = f(g, [(1, 1)])
        assert d[1, 1] == 0 and d[1, 0] == 1 and d[0, 1] == 1 and d[1, 2] == 12 and d[1, 3] == 4


def test_the_run_takes_the_first_stretch_only():
    cm = cr.Costmap(6, 4, 1.0, 0.0, 0.0, 0)
    cm.grid[1, 3] = 255
    cells = ref.plan_cells(cm, [(-1.0, 0.5), (0.5, 0.5), (1.5, 0.5), (9.0, 0.5), (2.5, 0.5)])
    assert cells == [None, (0, 0), (1, 0), None, (2, 0)] and ref.run(cm.grid, cells) == (1, 3)
    cells = ref.plan_cells(cm, [(0.5, 1.5), (3.5, 1.5), (4.5, 1.5)])        # the second point lies on 255
    assert ref.run(cm.grid, cells) == (0, 1)
    assert ref.run(cm.grid, ref.plan_cells(cm, [(-1.0, -1.0), (3.5, 1.5)])) is None
    assert ref.run(cm.grid, []) is None
    r = ref.grids(cm, [(-5.0, -5.0)])
    assert r["started"] == 0 and r["goal_cell"] == (-1, -1) and (r["path"] == 25).all() and (r["goal"] == 25).all()


def test_score_is_the_sequential_loop():
    cm = cr.Costmap(5, 5, 1.0, 0.0, 0.0, 0)
    cm.grid[0:4, 2] = 254
    d = ref.distance_queue(cm.grid, [(0, 0)])
    poses = [(0.5, 0.5, 1, 0), (4.5, 4.5, 1, 0), (2.5, 1.5, 1, 0), (1.5, 1.5, 1, 0), (1.5, 1.5, 1, 0), (5.5, 1.5, 1, 0)]
    assert ref.score(cm, d, poses, 2).tolist() == [8, 2, -4]
    assert ref.score(cm, d, poses, 2, flags=ref.SUM).tolist() == [8, 27, -4]
    assert ref.score(cm, d, poses, 2, flags=ref.STOP_ON_FAILURE).tolist() == [8, -3, -4]
    assert ref.score(cm, d, poses, 2, xshift=1.0).tolist() == [-4, 25, -4]
    assert ref.score(cm, d, poses, 3, flags=ref.STOP_ON_FAILURE).tolist() == [-3, -4]


# ---- gem_mapgrid_adjust_plan --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from gem_amd import _lib
    return _lib.load()


def adjust(lib, plan, res, cap=None):
    """(rc, count, points)"""
    v = np.ascontiguousarray(plan, np.float64).reshape(-1, 2)
    pv = v.ctypes.data_as(C.POINTER(C.c_double)) if v.size else None
    n = C.c_longlong(-7)
    rc = lib.gem_mapgrid_adjust_plan(pv, v.shape[0], float(res), None, 0, C.byref(n))
    if rc != 0 or cap is None:
        return rc, int(n.value), None
    out = np.full((cap + 3, 2), -1.0, np.float64)
    m = C.c_longlong(-7)
    rc = lib.gem_mapgrid_adjust_plan(pv, v.shape[0], float(res), out.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(m))
    return rc, int(m.value), out


def test_adjust_plan_matches_the_restatement(lib):
    import gem_amd
    rng = np.random.default_rng(7)
    res = 0.05
    plans = {
        "closer than a cell": [(0.0, 0.0), (0.01, 0.02), (0.03, 0.01), (0.04, 0.04)],
        "exactly one resolution apart": [(0.0, 0.0), (res, 0.0), (res, res), (2 * res, res)],
        "a long jump": [(0.1, 0.2), (7.3, -4.1)],
        "one point": [(1.0, 2.0)],
        "empty": [],
        "random": rng.uniform(-3, 3, (40, 2)),
        "large coordinates": rng.uniform(-1, 1, (10, 2)) + 1e6,
    }
    for name, plan in plans.items():
        want = ref.adjust_plan(plan, res)
        rc, count, _ = adjust(lib, plan, res)
        assert rc == 0 and count == want.shape[0], name
        rc, m, got = adjust(lib, plan, res, cap=count)
        assert rc == 0 and m == count and got[:count].tobytes() == want.tobytes(), name
        assert gem_amd.adjust_plan(plan, res).tobytes() == want.tobytes(), name
    assert ref.adjust_plan(plans["closer than a cell"], res).shape[0] == 4
    assert ref.adjust_plan(plans["exactly one resolution apart"], res).shape[0] == 4      # the test is >: nothing inserted
    assert ref.adjust_plan(plans["a long jump"], res).shape[0] == int(np.ceil(np.hypot(7.2, 4.3) / res)) + 1


def test_adjust_plan_cap_and_errors(lib):
    plan = [(0.0, 0.0), (1.0, 0.0)]
    rc, count, _ = adjust(lib, plan, 0.1)
    assert rc == 0 and count == 11
    rc, m, got = adjust(lib, plan, 0.1, cap=5)                           # cap too small: an error, the count still reported
    assert rc != 0 and m == 11 and (got[5:] == -1.0).all() and (got[:5] != -1.0).any()
    for bad_res in (0.0, -1.0, float("nan"), float("inf")):
        assert adjust(lib, plan, bad_res)[0] != 0
    for bad in ([(0.0, float("nan")), (1.0, 0.0)], [(0.0, 0.0), (float("inf"), 0.0)]):
        assert adjust(lib, bad, 0.1)[0] != 0
    assert adjust(lib, [(0.0, 0.0), (1e9, 0.0)], 0.05)[0] != 0            # above GEM_MAPGRID_MAX_POINTS
    assert adjust(lib, [(0.0, 0.0), (1e300, 0.0)], 0.05)[0] != 0          # the squared distance overflows
    n = C.c_longlong(-7)
    assert lib.gem_mapgrid_adjust_plan(None, 3, 0.1, None, 0, C.byref(n)) != 0 and n.value == -7     # NULL with a non-zero count
    assert lib.gem_mapgrid_adjust_plan(None, -1, 0.1, None, 0, C.byref(n)) != 0
    assert lib.gem_mapgrid_adjust_plan(None, 0, 0.1, None, 0, C.byref(n)) == 0 and n.value == 0


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def declared(header):
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(gem_[a-z_0-9]+)\s*\(", text)))


def test_mapgrid_symbols_are_declared_exported_and_bound(lib):
    from gem_amd import _lib
    names = declared(ROOT / "include" / "gem_hip_mapgrid.h")
    assert names == sorted(_lib.MAPGRID_SIGNATURES) == ["gem_costmap_mapgrid_prepare", "gem_costmap_mapgrid_read", "gem_costmap_mapgrid_score",
                                                        "gem_costmap_mapgrid_score_device", "gem_mapgrid_adjust_plan"]
    for n in names:
        assert getattr(lib, n).argtypes == _lib.MAPGRID_SIGNATURES[n][1]
    text = (ROOT / "include" / "gem_hip.h").read_text()
    assert text.index('#include "gem_hip_inflate.h"') < text.index('#include "gem_hip_mapgrid.h"')
    assert lib.gem_abi_version() == 9


def test_constants_match_the_header(tmp_path):
    from gem_amd import _lib
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "gem_hip.h"\nint main(void) { printf("%d %d %d %d %d %d\\n", GEM_MAPGRID_PATH, GEM_MAPGRID_GOAL, '
                   "GEM_MAPGRID_STOP_ON_FAILURE, GEM_MAPGRID_SUM, GEM_MAPGRID_MAX_POINTS, GEM_MAPGRID_MAX_WORDS); return 0; }\n")
    exe = tmp_path / "consts"
    res = subprocess.run(["cc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [_lib.MAPGRID_PATH, _lib.MAPGRID_GOAL, _lib.MAPGRID_STOP_ON_FAILURE, _lib.MAPGRID_SUM, _lib.MAPGRID_MAX_POINTS, _lib.MAPGRID_MAX_WORDS]
    assert got == [ref.PATH, ref.GOAL, ref.STOP_ON_FAILURE, ref.SUM, ref.MAX_POINTS, ref.MAX_WORDS]


def test_python_facade_has_the_mapgrid_calls():
    import gem_amd
    for name in ("prepare_map_grid", "read_map_grid", "score_map_grid"):
        assert callable(getattr(gem_amd.Costmap, name))
    assert callable(gem_amd.adjust_plan)
    with pytest.raises(ValueError):
        gem_amd.adjust_plan([(0.0, 0.0)], 0.0)


def build_mapgrid_check(out: Path) -> Path:
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc", "-std=c++17", "-O2", "-Wall", "-Werror",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "mapgrid_check.cpp"), "-o", str(out),
           f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_mapgrid_facade_builds():
    """gem::Costmap's MapGrid calls compile with hipcc against the installed headers and the library; the host-only plan adjustment is
    checked, and without a GPU the check exits early."""
    import tempfile
    from gem_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as td:
        exe = build_mapgrid_check(Path(td) / "mapgrid_check")
        res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: built)"), res.stdout + res.stderr
