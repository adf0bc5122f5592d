"""CPU tests of the global-plan contract of include/gem_hip_navplan.h: the restatement itself (tests/navplan_ref.py: the heapq Dijkstra
against the order-free sweeps, known answers), the host-only gem_navplan_weights and gem_navplan_host against the restatement on the
geometries the device is tested at, the path's defining property, the error cases and the ABI (symbols, the include line, the Python
and C++ facades).  Every comparison is exact."""
import ctypes as C
import functools
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import navplan_ref as ref  # noqa: E402

GEOMETRIES = {"64x64": (64, 64), "65x65": (65, 65), "130x90": (130, 90), "129x129": (129, 129), "65x3": (65, 3), "1x200": (1, 200), "200x1": (200, 1)}   # size_x, size_y
KINDS = ["empty", "noise", "wall", "blocked"]
INV = -1                                                                 # GEM_ERR_INVALID


@pytest.fixture(scope="module")
def lib():
    from gem_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def default_weights():
    w = ref.weights()
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def scenario(geom, kind):
    """the grid of a geometry: never changed.  empty | 30 % of the cells a random byte 0 .. 255 | two walls at columns 63 - 64 with one
    gap | every cell a random traversable byte and 30 % of them 252, 253 or 254"""
    sx, sy = GEOMETRIES[geom]
    rng = np.random.default_rng(sx * 1000 + sy)
    g = np.zeros((sy, sx), np.uint8)
    if kind == "noise":
        hit = rng.random((sy, sx)) < 0.3
        g[hit] = rng.integers(0, 256, int(hit.sum()), dtype=np.uint8)
    elif kind == "wall":
        gap = sy // 3
        for col in (63, 64):
            if col < sx:
                g[:, col] = 254
                g[gap, col] = 0
        if sx == 1:                                                      # a thin map: the wall lies across it
            g[63:65, 0] = 254
    elif kind == "blocked":
        g = rng.integers(0, 252, (sy, sx), dtype=np.uint8)
        blk = rng.random((sy, sx)) < 0.3
        g[blk] = rng.integers(252, 255, int(blk.sum()), dtype=np.uint8)
    g.setflags(write=False)
    return g


def corner_cells(sx, sy):
    """a cell in each corner tile, one off the rim where the map is wide enough (the rim itself is the outline); the goal is the
    opposite one"""
    xs, ys = (min(1, sx - 1), max(sx - 2, 0)), (min(1, sy - 1), max(sy - 2, 0))
    return [((xs[i], ys[j]), (xs[1 - i], ys[1 - j])) for j in (0, 1) for i in (0, 1)]


@functools.lru_cache(maxsize=None)
def expected(geom, kind):
    """[(start, goal, flags, ref.plan)] of a scenario: computed once, shared by the host-twin and the device tests"""
    g = scenario(geom, kind)
    out = []
    for start, goal in corner_cells(*GEOMETRIES[geom]):
        for flags in (ref.OUTLINE, 0):
            out.append((start, goal, flags, ref.plan(g, default_weights(), flags, start, goal)))
    return out


def special_cases():
    """(name, grid, start, goal, flags): the start on a lethal byte, the goal on one, a goal walled in, start = goal, a start and a goal
    off the map"""
    g = np.zeros((9, 11), np.uint8)
    g[4, 2] = 254
    g[2, 8] = 253
    g[5:8, 5:8] = 254
    g[6, 6] = 0
    g.setflags(write=False)
    return [("start on a lethal byte", g, (2, 4), (9, 7), 0), ("goal on a lethal byte", g, (1, 1), (8, 2), 0),
            ("goal walled in", g, (1, 1), (6, 6), 0), ("start = goal", g, (3, 3), (3, 3), ref.OUTLINE),
            ("start = goal on a lethal byte", g, (2, 4), (2, 4), 0), ("start off the map", g, (-1, 3), (4, 4), 0),
            ("goal off the map", g, (1, 1), (11, 4), ref.OUTLINE), ("start on the outline", g, (0, 4), (9, 7), ref.OUTLINE)]


def serpentine(n=130):
    """a one-cell corridor that runs along every second row: walls of 254 between the rows with the gap alternating left and right"""
    g = np.zeros((n, n), np.uint8)
    for k, y in enumerate(range(1, n, 2)):
        g[y, :] = 254
        g[y, n - 1 if k % 2 == 0 else 0] = 0
    g.setflags(write=False)
    return g


def seam_corridor():
    """100 x 70, tile seam between columns 63 and 64: expensive ground (byte 60) with a cheap corridor (byte 0) that starts left of the
    seam, crosses it, runs on, comes back across it further down and ends left of it -- the left tile's edge improves, the right
    tile's answer comes back and improves the left tile's edge cells a second time"""
    g = np.full((70, 100), 60, np.uint8)
    g[5, 40:90] = 0
    g[5:50, 89] = 0
    g[49, 30:90] = 0
    g.setflags(write=False)
    return g


def host_plan(lib, grid, w, flags, start, goal, cap=None):
    sy, sx = grid.shape
    from gem_amd import _lib
    pot = np.full((sy, sx), -5, np.int32)
    cells = np.full(sx * sy if cap is None else max(cap, 1), -5, np.int32)
    st = _lib.NavplanStatus()
    wv = np.ascontiguousarray(w, np.int32)
    rc = lib.gem_navplan_host(np.ascontiguousarray(grid).ctypes.data_as(C.c_void_p), sx, sy, wv.ctypes.data_as(C.POINTER(C.c_int)), flags,
                              (C.c_int * 2)(*start), (C.c_int * 2)(*goal), pot.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p),
                              cells.size if cap is None else cap, C.byref(st))
    return rc, pot, cells, st


def same_as_ref(want, pot, cells, st, what):
    assert pot.dtype == np.int32 and pot.tobytes() == want["pot"].tobytes(), f"{what}: {int((pot != want['pot']).sum())} potentials differ"
    assert (st.found, st.n_path, st.goal_potential) == (want["found"], want["n_path"], want["goal_potential"]), what
    assert (tuple(st.start_cell), tuple(st.goal_cell)) == (want["start_cell"], want["goal_cell"]), what
    assert cells[:st.n_path].tolist() == want["cells"].tolist(), what


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_dijkstra_equals_the_sweeps_on_random_grids():
    rng = np.random.default_rng(20261020)
    unreached = lethal_start = 0
    for k in range(120):
        sy, sx = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        g = rng.integers(0, 256, (sy, sx)).astype(np.uint8)
        blk = rng.random((sy, sx)) < (0.0, 0.1, 0.3)[k % 3]
        g[blk] = 254
        w = default_weights() if k % 2 else rng.integers(0, 40, 256).astype(np.int32)
        start = (int(rng.integers(0, sx)), int(rng.integers(0, sy)))
        flags = ref.OUTLINE if k % 4 == 0 else 0
        a, b = ref.potential_dijkstra(g, w, flags, start), ref.potential_sweeps(g, w, flags, start)
        assert a.dtype == np.int32 and a.tobytes() == b.tobytes(), (k, g.shape, start)
        assert a[start[1], start[0]] == 0
        unreached += int((a == ref.UNREACHED).any())
        lethal_start += int(w[g[start[1], start[0]]] == 0)
    assert unreached >= 30 and lethal_start >= 3


def test_known_answer_wall_and_scan_order():
    g = np.zeros((5, 7), np.uint8)
    g[1:4, 3] = 254
    U = ref.UNREACHED
    want = np.array([[100, 50, 100, 150, 200, 250, 300], [50, 0, 50, U, 250, 300, 350], [100, 50, 100, U, 300, 350, 400],
                     [150, 100, 150, U, 350, 400, 450], [200, 150, 200, 250, 300, 350, 400]], np.int32)
    for f in (ref.potential_dijkstra, ref.potential_sweeps):
        assert (f(g, default_weights(), 0, (1, 1)) == want).all()
    assert ref.get_path(want, (1, 1), (5, 1)) == [(1, 1), (2, 1), (3, 0), (4, 0), (5, 1)]
    assert ref.NEIGHBOURS == [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def test_weight_table_known_values():
    w = ref.weights()
    assert w[0] == 50 and w[1] == 53 and w[67] == 251 and w[68] == 252 and w[251] == 252
    assert w[252] == 0 and w[253] == 0 and w[254] == 0 and w[255] == 252         # byte 252 is impassable under the defaults
    assert ref.weights(allow_unknown=False)[255] == 0
    assert ref.weights(cost_factor=2.5) is None and ref.weights(cost_factor=0.8) is None


# ---- the host-only entries against it --------------------------------------------------------------------------------------------------
def test_weights_equal_the_reference_and_a_non_integral_factor_is_refused(lib):
    import gem_amd
    cases = [(50, 3.0, 253, True), (50, 3.0, 253, False), (1, 1.0, 254, True), (0, 2.0, 200, True), (66, 0.0, 253, True), (50, 0.5, 101, False)]
    for neutral, factor, lethal, unknown in cases:
        want = ref.weights(neutral, factor, lethal, unknown)
        out = np.full(256, -7, np.int32)
        rc = lib.gem_navplan_weights(neutral, factor, lethal, int(unknown), out.ctypes.data_as(C.POINTER(C.c_int)))
        if want is None:
            assert rc == INV and (out == -7).all(), (neutral, factor, lethal, unknown)
        else:
            assert rc == 0 and out.tobytes() == want.tobytes(), (neutral, factor, lethal, unknown)
            assert gem_amd.nav_weights(neutral, factor, lethal, unknown).tobytes() == want.tobytes()
    assert ref.weights(0, 2.0, 200, True) is None                         # byte 0 would cost nothing: not a weight
    assert ref.weights(50, 0.5, 101, False) is None
    out = np.full(256, -7, np.int32)
    po = out.ctypes.data_as(C.POINTER(C.c_int))
    for bad in ((50, 2.5, 253, 1), (50, float("nan"), 253, 1), (50, float("inf"), 253, 1), (-1, 3.0, 253, 1), (50, 3.0, 0, 1), (50, 3.0, 257, 1)):
        assert lib.gem_navplan_weights(*bad, po) == INV and (out == -7).all(), bad
    assert lib.gem_navplan_weights(50, 3.0, 253, 1, None) == INV
    with pytest.raises(ValueError):
        gem_amd.nav_weights(cost_factor=2.5)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_host_twin_equals_the_reference(lib, geom, kind):
    g = scenario(geom, kind)
    found = 0
    for start, goal, flags, want in expected(geom, kind):
        rc, pot, cells, st = host_plan(lib, g, default_weights(), flags, start, goal)
        assert rc == 0 and st.rounds == 0 and st.chunks == 0
        same_as_ref(want, pot, cells, st, f"{geom} {kind} {start} -> {goal} flags {flags}")
        found += st.found
    if kind in ("empty", "noise") and min(g.shape) > 3:
        assert found == 8


def test_host_twin_special_cases_serpentine_and_corridor(lib):
    for name, g, start, goal, flags in special_cases():
        want = ref.plan(g, default_weights(), flags, start, goal)
        rc, pot, cells, st = host_plan(lib, g, default_weights(), flags, start, goal)
        assert rc == 0, name
        same_as_ref(want, pot, cells, st, name)
    by = {c[0]: ref.plan(c[1], default_weights(), c[4], c[2], c[3]) for c in special_cases()}
    assert by["start on a lethal byte"]["found"] == 1 and by["goal on a lethal byte"]["found"] == 0 and by["goal walled in"]["found"] == 0
    assert by["start = goal"]["n_path"] == 1 and by["start = goal on a lethal byte"]["n_path"] == 1
    assert by["start off the map"]["found"] == 0 and (by["start off the map"]["pot"] == ref.UNREACHED).all()
    assert by["goal off the map"]["found"] == 0 and by["goal off the map"]["goal_cell"] == (-1, -1)
    assert by["start on the outline"]["found"] == 1                       # a source whatever its byte, and wherever it lies
    g = serpentine()
    want = ref.plan(g, default_weights(), 0, (0, 0), (0, 128))
    assert want["found"] == 1 and want["n_path"] > 60 * 130
    rc, pot, cells, st = host_plan(lib, g, default_weights(), 0, (0, 0), (0, 128))
    same_as_ref(want, pot, cells, st, "serpentine")
    g = seam_corridor()
    want = ref.plan(g, default_weights(), 0, (40, 5), (30, 49))
    rc, pot, cells, st = host_plan(lib, g, default_weights(), 0, (40, 5), (30, 49))
    same_as_ref(want, pot, cells, st, "corridor")
    assert {c % 100 for c in want["cells"].tolist()} >= {63, 64, 89}      # the plan crosses the seam and comes back


def tie_case():
    """(grid, weights): random bytes under a table of weights 1 and 2 -- small whole potentials, so that neighbours often tie"""
    g = np.random.default_rng(7).integers(0, 9, (40, 50), dtype=np.uint8)
    g.setflags(write=False)
    return g, (1 + np.arange(256) % 2).astype(np.int32)


def test_path_steps_are_the_first_minimal_neighbour(lib):
    """the path ends at start and goal and every step goes to the first neighbour, in scan order, with the smallest potential.  The
    property needs ties to mean anything.  An empty grid has none (the diagonal neighbour towards the start is the single smallest),
    so the tie case is a grid of random weights 1 and 2."""
    tg, tw = tie_case()
    for g, w, start, goal, flags in ((tg, tw, (2, 4), (44, 32), 0), (tg, tw, (44, 32), (2, 4), ref.OUTLINE),
                                     (np.zeros((40, 50), np.uint8), default_weights(), (3, 4), (44, 33), 0),
                                     (scenario("130x90", "noise"), default_weights(), (1, 1), (128, 88), 0)):
        rc, pot, cells, st = host_plan(lib, g, w, flags, start, goal)
        assert rc == 0 and st.found == 1
        sy, sx = g.shape
        path = [(int(c) % sx, int(c) // sx) for c in cells[:st.n_path]]
        assert path[0] == start and path[-1] == goal
        ties = 0
        for here, prev in zip(path[:0:-1], path[-2::-1]):                # from the goal backwards: here -> prev
            around = [(here[0] + xd, here[1] + yd) for xd, yd in ref.NEIGHBOURS]
            on = [(x, y) for x, y in around if 0 <= x < sx and 0 <= y < sy]
            low = min(int(pot[y, x]) for x, y in on)
            firsts = [c for c in on if pot[c[1], c[0]] == low]
            assert prev == firsts[0] and low < pot[here[1], here[0]]
            ties += len(firsts) > 1
        if g is tg:
            assert ties > 10, ties


def test_host_twin_errors(lib):
    from gem_amd import _lib
    g = np.zeros((6, 8), np.uint8)
    w = default_weights()
    rc, pot, cells, st = host_plan(lib, g, w, 0, (1, 1), (6, 4))
    assert rc == 0 and st.n_path == 6
    rc, pot, cells, st = host_plan(lib, g, w, 0, (1, 1), (6, 4), cap=5)    # cap too small: an error, the status still filled
    assert rc == INV and st.n_path == 6 and st.found == 1 and (cells == -5).all()
    for flags in (2, 4, -1):
        assert host_plan(lib, g, w, flags, (1, 1), (6, 4))[0] == INV
    neg = np.array(w)
    neg[7] = -1
    assert host_plan(lib, g, neg, 0, (1, 1), (6, 4))[0] == INV
    big = np.array(w)
    big[9] = -(-(2 ** 31 - 1) // 48)                                      # the smallest weight with 48 cells * max(w) >= 2^31 - 1
    assert host_plan(lib, g, big, 0, (1, 1), (6, 4))[0] == INV
    big[9] -= 1
    assert host_plan(lib, g, big, 0, (1, 1), (6, 4))[0] == 0
    st = _lib.NavplanStatus()
    wp, gp = np.ascontiguousarray(w).ctypes.data_as(C.POINTER(C.c_int)), g.ctypes.data_as(C.c_void_p)
    s, e = (C.c_int * 2)(1, 1), (C.c_int * 2)(6, 4)
    assert lib.gem_navplan_host(None, 8, 6, wp, 0, s, e, None, None, 0, C.byref(st)) == INV
    assert lib.gem_navplan_host(gp, 8, 6, None, 0, s, e, None, None, 0, C.byref(st)) == INV
    assert lib.gem_navplan_host(gp, 8, 6, wp, 0, None, e, None, None, 0, C.byref(st)) == INV
    assert lib.gem_navplan_host(gp, 8, 6, wp, 0, s, e, None, None, 0, None) == INV
    assert lib.gem_navplan_host(gp, 0, 6, wp, 0, s, e, None, None, 0, C.byref(st)) == INV
    assert lib.gem_navplan_host(gp, 8, -1, wp, 0, s, e, None, None, 0, C.byref(st)) == INV
    assert lib.gem_navplan_host(gp, 8, 6, wp, 0, s, e, None, None, 0, C.byref(st)) == 0 and st.n_path == 6      # no outputs: the status alone


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def declared(header):
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(gem_[a-z_0-9]+)\s*\(", text)))


def test_navplan_symbols_are_declared_exported_and_bound(lib):
    from gem_amd import _lib
    names = declared(ROOT / "include" / "gem_hip_navplan.h")
    assert names == sorted(_lib.NAVPLAN_SIGNATURES) == ["gem_costmap_navplan", "gem_costmap_navplan_read", "gem_costmap_navplan_status", "gem_navplan_host",
                                                        "gem_navplan_weights"]
    for n in names:
        assert getattr(lib, n).argtypes == _lib.NAVPLAN_SIGNATURES[n][1]
    text = (ROOT / "include" / "gem_hip.h").read_text()
    assert text.index('#include "gem_hip_trajgen.h"') < text.index('#include "gem_hip_navplan.h"')
    assert lib.gem_abi_version() == 9
    hdr = (ROOT / "include" / "gem_hip_navplan.h").read_text()
    for word in ("RESTATED FROM MEMORY", "NOT VERIFIED", "convert_offset_", "navfn", "quadratic", "early exit", "outline_map"):
        assert word in hdr, word
    assert '"nav_chunk"' in (ROOT / "include" / "gem_hip_debug.h").read_text()


def test_constants_and_the_status_layout_match_the_header(tmp_path):
    from gem_amd import _lib
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gem_hip.h"\nint main(void) { printf("%d %d %zu %zu %zu %zu\\n", GEM_NAV_OUTLINE, '
                   "GEM_NAV_UNREACHED, sizeof(gem_navplan_status), offsetof(gem_navplan_status, goal_potential), "
                   "offsetof(gem_navplan_status, start_cell), offsetof(gem_navplan_status, goal_cell)); return 0; }\n")
    exe = tmp_path / "consts"
    res = subprocess.run(["cc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.NavplanStatus
    assert got == [_lib.NAV_OUTLINE, _lib.NAV_UNREACHED, C.sizeof(S), S.goal_potential.offset, S.start_cell.offset, S.goal_cell.offset]
    assert got[:2] == [ref.OUTLINE, ref.UNREACHED]


def test_python_facade_has_the_navplan_calls():
    import gem_amd
    for name in ("nav_plan", "nav_status", "read_potential"):
        assert callable(getattr(gem_amd.Costmap, name))
    g = np.zeros((5, 7), np.uint8)
    g[1:4, 3] = 254
    pot, cells, st = gem_amd.nav_plan_host(g, (1, 1), (5, 1), outline=False)
    want = ref.plan(g, default_weights(), 0, (1, 1), (5, 1))
    assert pot.tobytes() == want["pot"].tobytes() and cells.tolist() == want["cells"].tolist() and st["found"] == 1
    assert st["goal_potential"] == 300 and st["start_cell"] == (1, 1) and st["goal_cell"] == (5, 1)


def build_navplan_check(out: Path) -> Path:
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc", "-std=c++17", "-O2", "-Wall", "-Werror",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "navplan_check.cpp"), "-o", str(out),
           f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_navplan_facade_builds():
    """gem::NavPlan and gem::Costmap::navPlan compile with hipcc against the installed headers and the library; the host-only weight
    table and host twin are checked against a hand-derived answer, and without a GPU the check exits early."""
    import tempfile
    from gem_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as td:
        exe = build_navplan_check(Path(td) / "navplan_check")
        res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: built)"), res.stdout + res.stderr
