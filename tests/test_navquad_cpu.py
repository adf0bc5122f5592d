"""CPU tests of the quadratic-potential contract of include/gem_hip_navquad.h: the restatement itself (tests/navquad_ref.py: Jacobi
sweeps against Gauss-Seidel passes in random orders, hand-checked values, the increment's monotonicity), the kernel header's divide-free
quotient (tests/cpp/navquad_check.cpp) against Python's floor on every (hf, dc), the host twin gem_navquad_host -- a heap, a fourth
order -- against the restatement on the geometries and scenarios of test_navplan_cpu.py, the relation to the linear potential, the
error cases, the ABI and what the potential buys the gradient walk.  Every comparison is exact."""
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
import navpath_ref as pref  # noqa: E402
import navplan_ref as lin  # noqa: E402
import navquad_ref as ref  # noqa: E402
from test_navplan_cpu import corner_cells, default_weights, scenario, seam_corridor, serpentine, special_cases  # noqa: E402

INV = -1                                                                 # GEM_ERR_INVALID
GEOMS = {"64x64": (64, 64), "65x65": (65, 65), "130x90": (130, 90)}     # one exact tile, four tiles (three slivers), six tiles
KINDS = ["noise", "wall", "blocked"]


@pytest.fixture(scope="module")
def lib():
    from gem_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def expected(geom, kind):
    """[(start, goal, flags, ref.plan)] of a scenario of test_navplan_cpu.py: two opposite corners, the outline on and off; computed
    once, shared by the host-twin and the device tests"""
    g = scenario(geom, kind)
    pairs = corner_cells(*GEOMS[geom])
    return [(start, goal, flags, ref.plan(g, default_weights(), flags, start, goal)) for (start, goal), flags in
            ((pairs[0], ref.OUTLINE), (pairs[3], 0))]


def odd_cases():
    """(name, grid, start, goal, flags, weights): 1 x 1, the special cases of test_navplan_cpu.py (a start off the map among them), an
    all-blocked map with the start on it and off it, the corridor across a tile seam, a small serpentine, weights 1 and 462"""
    w = default_weights()
    out = [("1 x 1", np.zeros((1, 1), np.uint8), (0, 0), (0, 0), 0, w), ("1 x 1 outlined", np.zeros((1, 1), np.uint8), (0, 0), (0, 0), ref.OUTLINE, w)]
    out += [(name, g, s, e, f, w) for name, g, s, e, f in special_cases()]
    blocked = np.full((20, 30), 254, np.uint8)
    blocked.setflags(write=False)
    out += [("all blocked", blocked, (3, 4), (20, 10), 0, w), ("all blocked, start off the map", blocked, (30, 4), (20, 10), 0, w)]
    out.append(("corridor", seam_corridor(), (40, 5), (30, 49), 0, w))
    out.append(("serpentine 34", serpentine(34), (0, 0), (0, 32), 0, w))
    rng = np.random.default_rng(462)
    g = rng.integers(0, 256, (40, 70), dtype=np.uint8)
    g.setflags(write=False)
    custom = rng.integers(0, 463, 256).astype(np.int32)
    custom[:4] = (1, 462, 0, 1)
    custom.setflags(write=False)
    out.append(("weights 0 .. 462", g, (2, 3), (66, 35), 0, custom))
    return out


def host_quad(lib, grid, w, flags, start, goal, cap=None):
    sy, sx = grid.shape
    from gem_amd import _lib
    pot = np.full((sy, sx), -5, np.int32)
    cells = np.full(sx * sy if cap is None else max(cap, 1), -5, np.int32)
    st = _lib.NavplanStatus()
    wv = np.ascontiguousarray(w, np.int32)
    rc = lib.gem_navquad_host(np.ascontiguousarray(grid).ctypes.data_as(C.c_void_p), sx, sy, wv.ctypes.data_as(C.POINTER(C.c_int)), flags,
                              (C.c_int * 2)(*start), (C.c_int * 2)(*goal), pot.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p),
                              cells.size if cap is None else cap, C.byref(st))
    return rc, pot, cells, st


def same_as_ref(want, pot, cells, st, what):
    assert pot.dtype == np.int32 and pot.tobytes() == want["pot"].tobytes(), f"{what}: {int((pot != want['pot']).sum())} potentials differ"
    assert (st.found, st.n_path, st.goal_potential) == (want["found"], want["n_path"], want["goal_potential"]), what
    assert (tuple(st.start_cell), tuple(st.goal_cell)) == (want["start_cell"], want["goal_cell"]), what
    assert cells[:st.n_path].tolist() == want["cells"].tolist(), what


def four_ways(lib, g, w, flags, start, goal, want, what, seeds=(1, 2, 3)):
    """Jacobi (want), three Gauss-Seidel orders and the host twin's heap: byte for byte"""
    for seed in seeds:
        gs = ref.potential_gauss_seidel(g, w, flags, start, seed)
        assert gs.dtype == np.int32 and gs.tobytes() == want["pot"].tobytes(), f"{what}: Gauss-Seidel order {seed}"
    rc, pot, cells, st = host_quad(lib, g, w, flags, start, goal)
    assert rc == 0 and st.rounds == 0 and st.chunks == 0, what
    same_as_ref(want, pot, cells, st, what)


# ---- 1. hand-checked values -----------------------------------------------------------------------------------------------------------
def test_known_answer_uniform_weight_50():
    g = np.zeros((8, 8), np.uint8)
    w = np.full(256, 50, np.int32)
    want = np.array([[0, 50, 100, 150], [50, 85, 127, 171], [100, 127, 162, 201], [150, 171, 201, 236]], np.int32)
    assert (ref.potential_jacobi(g, w, 0, (0, 0))[:4, :4] == want).all()
    assert (ref.potential_gauss_seidel(g, w, 0, (0, 0), 5)[:4, :4] == want).all()
    assert (lin.potential_dijkstra(g, w, 0, (0, 0))[:4, :4] == 50 * np.add.outer(np.arange(4), np.arange(4))).all()      # 0 .. 300
    assert ref.inc(50, 0) == 35 and ref.inc(50, 15) == 42 and ref.inc(50, 35) == 48 and ref.inc(50, 50) == 50 and ref.inc(50, 10 ** 9) == 50
    assert ref.update(50, 50, ref.UNREACHED, 50, ref.UNREACHED) == 85 and ref.update(50, 100, ref.UNREACHED, ref.UNREACHED, ref.UNREACHED) == 150
    assert ref.update(50, ref.UNREACHED, ref.UNREACHED, ref.UNREACHED, ref.UNREACHED) == ref.UNREACHED


# ---- 2. the increment, and the header's quotient ---------------------------------------------------------------------------------------
def test_increment_is_monotone_with_slope_at_most_one_and_the_header_quotient_is_the_floor(tmp_path):
    exe = tmp_path / "navquad_check"
    res = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", str(ROOT / "tests" / "cpp" / "navquad_check.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout[-2000:] + run.stderr
    lines = run.stdout.split("\n")
    quot = {int(l.split()[0]): [int(v) for v in l.split()[1:]] for l in lines if l and l[0].isdigit()}
    incs = {int(l.split()[1]): [int(v) for v in l.split()[2:]] for l in lines if l.startswith("inc ")}
    assert sorted(quot) == sorted(incs) == list(range(1, ref.MAX_WEIGHT + 1))
    pairs = 0
    for hf in range(1, ref.MAX_WEIGHT + 1):
        floor = [(-2301 * dc * dc + 5307 * dc * hf + 7040 * hf * hf) // (10000 * hf) for dc in range(hf)]
        assert min(-2301 * dc * dc + 5307 * dc * hf + 7040 * hf * hf for dc in range(hf)) >= 0
        assert quot[hf] == floor, hf                                     # the kernel's quotient, no divide, is Python's floor
        f = [ref.inc(hf, dc) for dc in range(hf + 2)]
        assert incs[hf] == f[:hf + 1], hf
        assert f[hf] == hf and f[hf + 1] == hf and min(f) >= 1 and max(f) <= hf, hf
        steps = np.diff(f)
        assert steps.min() >= 0 and steps.max() <= 1, hf                 # monotone, slope at most 1
        pairs += hf
    assert pairs == 462 * 463 // 2 and 10046 * 462 ** 2 < 2 ** 31 <= 10046 * 463 ** 2


# ---- 3. four orders, one potential ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_jacobi_gauss_seidel_and_the_host_twin_agree(lib, geom, kind):
    g = scenario(geom, kind)
    for k, (start, goal, flags, want) in enumerate(expected(geom, kind)):  # (three orders from one corner, one from the other: pure Python)
        four_ways(lib, g, default_weights(), flags, start, goal, want, f"{geom} {kind} {start} -> {goal} flags {flags}", (1, 2, 3) if k == 0 else (4,))
    if kind == "noise":
        assert all(want["found"] == 1 for _, _, _, want in expected(geom, kind))


def test_odd_cases_agree_four_ways(lib):
    by = {}
    for name, g, start, goal, flags, w in odd_cases():
        want = by[name] = ref.plan(g, w, flags, start, goal)
        four_ways(lib, g, w, flags, start, goal, want, name)
    assert by["1 x 1"]["n_path"] == 1 and by["1 x 1"]["pot"].tolist() == [[0]]
    assert by["start on a lethal byte"]["found"] == 1 and by["goal on a lethal byte"]["found"] == 0 and by["goal walled in"]["found"] == 0
    assert by["start off the map"]["found"] == 0 and (by["start off the map"]["pot"] == ref.UNREACHED).all()
    assert by["all blocked"]["found"] == 0 and int((by["all blocked"]["pot"] != ref.UNREACHED).sum()) == 1     # the source alone
    assert (by["all blocked, start off the map"]["pot"] == ref.UNREACHED).all()
    assert by["corridor"]["found"] == 1 and by["serpentine 34"]["found"] == 1 and by["serpentine 34"]["n_path"] > 16 * 30
    assert by["weights 0 .. 462"]["found"] == 1


def test_the_long_serpentine_equals_the_host_twin(lib):
    g = serpentine()
    want = ref.plan(g, default_weights(), 0, (0, 0), (0, 128))
    assert want["found"] == 1 and want["n_path"] > 60 * 130
    rc, pot, cells, st = host_quad(lib, g, default_weights(), 0, (0, 0), (0, 128))
    assert rc == 0
    same_as_ref(want, pot, cells, st, "serpentine")
    assert (pot == lin.potential_dijkstra(g, default_weights(), 0, (0, 0))).all()     # a one-cell corridor has one axis: the linear potential


# ---- 4. against the linear potential ----------------------------------------------------------------------------------------------------
def test_potential_is_at_most_the_linear_one_with_the_same_reached_set():
    lower = 0
    cases = [(scenario(geom, kind), default_weights(), flags, start, want["pot"]) for geom in GEOMS for kind in KINDS
             for start, _, flags, want in expected(geom, kind)]
    cases += [(g, w, flags, start, ref.potential_jacobi(g, w, flags, start)) for _, g, start, _, flags, w in odd_cases()]
    for g, w, flags, start, pot in cases:
        l = lin.potential_dijkstra(g, w, flags, start)
        assert (pot <= l).all() and ((pot == ref.UNREACHED) == (l == ref.UNREACHED)).all()
        lower += int((pot < l).sum())
    assert lower > 10000


# ---- 5. weight 1: the potential still strictly falls --------------------------------------------------------------------------------------
def test_uniform_weight_one_strictly_falls_and_the_grid_path_arrives(lib):
    g = np.zeros((30, 40), np.uint8)
    w = np.ones(256, np.int32)
    want = ref.plan(g, w, 0, (5, 6), (38, 27))
    rc, pot, cells, st = host_quad(lib, g, w, 0, (5, 6), (38, 27))
    assert rc == 0
    same_as_ref(want, pot, cells, st, "w = 1")
    assert st.found == 1 and cells[0] == 6 * 40 + 5 and cells[st.n_path - 1] == 27 * 40 + 38
    p = np.full((32, 42), ref.UNREACHED, np.int64)
    p[1:-1, 1:-1] = pot
    low4 = np.minimum(np.minimum(p[1:-1, :-2], p[1:-1, 2:]), np.minimum(p[:-2, 1:-1], p[2:, 1:-1]))
    away = np.ones((30, 40), bool)
    away[6, 5] = False
    assert (low4[away] < pot[away]).all() and (pot[away] - low4[away] == 1).all()     # inc(1, .) is 1: max(1, .) at work
    assert ref.inc(1, 0) == 1 and (-2301 * 0 + 7040) // 10000 == 0


# ---- 6. the error cases -----------------------------------------------------------------------------------------------------------------
def test_host_twin_errors_and_the_weight_limit(lib):
    from gem_amd import _lib
    g = np.zeros((6, 8), np.uint8)
    w = np.array(default_weights())
    rc, pot, cells, st = host_quad(lib, g, w, 0, (1, 1), (6, 4))
    assert rc == 0 and st.found == 1 and st.n_path == 6
    rc, pot, cells, st = host_quad(lib, g, w, 0, (1, 1), (6, 4), cap=5)    # cap too small: an error, the status still filled
    assert rc == INV and st.n_path == 6 and st.found == 1 and (cells == -5).all()
    for flags in (2, 4, -1):
        assert host_quad(lib, g, w, flags, (1, 1), (6, 4))[0] == INV
    top = w.copy(); top[9] = 462
    assert host_quad(lib, g, top, 0, (1, 1), (6, 4))[0] == 0
    top[9] = 463
    rc, pot, cells, st = host_quad(lib, g, top, 0, (1, 1), (6, 4))
    assert rc == INV and (pot == -5).all()
    neg = w.copy(); neg[7] = -1
    assert host_quad(lib, g, neg, 0, (1, 1), (6, 4))[0] == INV
    st = _lib.NavplanStatus()
    wp, gp = np.ascontiguousarray(w).ctypes.data_as(C.POINTER(C.c_int)), g.ctypes.data_as(C.c_void_p)
    s, e = (C.c_int * 2)(1, 1), (C.c_int * 2)(6, 4)
    assert lib.gem_navquad_host(None, 8, 6, wp, 0, s, e, None, None, 0, C.byref(st)) == INV
    assert lib.gem_navquad_host(gp, 8, 6, None, 0, s, e, None, None, 0, C.byref(st)) == INV
    assert lib.gem_navquad_host(gp, 8, 6, wp, 0, None, e, None, None, 0, C.byref(st)) == INV
    assert lib.gem_navquad_host(gp, 8, 6, wp, 0, s, None, None, None, 0, C.byref(st)) == INV
    assert lib.gem_navquad_host(gp, 8, 6, wp, 0, s, e, None, None, 0, None) == INV
    assert lib.gem_navquad_host(gp, 0, 6, wp, 0, s, e, None, None, 0, C.byref(st)) == INV
    assert lib.gem_navquad_host(gp, 8, -1, wp, 0, s, e, None, None, 0, C.byref(st)) == INV
    assert lib.gem_navquad_host(gp, 8, 6, wp, 0, s, e, None, None, 0, C.byref(st)) == 0 and st.n_path == 6      # no outputs: the status alone
    # the overflow refusal is the linear plan's: 4 * 10^6 cells of weight 462 stay below 2^31 - 1, 4.7 * 10^6 do not
    assert 4000000 * 462 < 2 ** 31 - 1 <= 4700000 * 462


# ---- 7. what it buys the gradient walk ----------------------------------------------------------------------------------------------------
def arrivals(seed, n):
    """(arrived on the linear potential, arrived on the quadratic one) of 60 gradient walks on an n x n noise map"""
    rng = np.random.default_rng(seed)
    grid = np.zeros((n, n), np.uint8)
    m = rng.random((n, n)) < 0.2
    grid[m] = rng.integers(0, 256, m.sum())
    start = (n // 8, n // 8)
    grid[start[1], start[0]] = 0
    w = default_weights()
    pl = lin.potential_dijkstra(grid, w, lin.OUTLINE, start)
    pq = ref.potential_jacobi(grid, w, ref.OUTLINE, start)
    goals = rng.choice(np.argwhere(pl < lin.UNREACHED), 60, replace=False)       # rows (y, x)
    got = []
    for pot in (pl, pq):
        got.append(sum(pref.walk(pot, start, (int(x), int(y)), 8 * n)[1]["status"] == pref.FOUND for y, x in goals))
    return got


def test_more_gradient_walks_arrive_on_the_quadratic_potential():
    """The claim of DESIGN 7w and of the header, no more: on rough maps the walk arrives MORE OFTEN, not always.  The counts are printed
    and written down there; only the inequality is asserted."""
    for seed, n in ((2, 75), (1, 40)):
        linear, quadratic = arrivals(seed, n)
        print(f"gradient walks that arrive, {n} x {n} noise, seed {seed}, 60 goals: linear {linear}, quadratic {quadratic}")
        assert quadratic > linear, (seed, n, linear, quadratic)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def declared(header):
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(gem_[a-z_0-9]+)\s*\(", text)))


def test_navquad_symbols_are_declared_exported_and_bound(lib):
    from gem_amd import _lib
    names = declared(ROOT / "include" / "gem_hip_navquad.h")
    assert names == sorted(_lib.NAVQUAD_SIGNATURES) == ["gem_costmap_navplan_quadratic", "gem_navquad_host"]
    for n in names:
        assert getattr(lib, n).argtypes == _lib.NAVQUAD_SIGNATURES[n][1]
    assert '#include "gem_hip_navquad.h"' in (ROOT / "include" / "gem_hip.h").read_text()
    assert lib.gem_abi_version() == 9 and _lib.NAVQUAD_MAX_WEIGHT == ref.MAX_WEIGHT
    hdr = (ROOT / "include" / "gem_hip_navquad.h").read_text()
    for word in ("GREATEST fixed point", "MONOTONE", "RECALLED FROM MEMORY", "NOT VERIFIED", "462", "max(1, .)", "min(hf, .)", "INVSQRT2", "GEM_NAVPATH_CAP"):
        assert word in hdr, word
    assert "gem_hip_navquad.h" in (ROOT / "include" / "gem_hip_navplan.h").read_text()
    assert '"navquad_passes"' in (ROOT / "include" / "gem_hip_debug.h").read_text()


def test_python_facade_has_the_navquad_calls():
    import gem_amd
    assert callable(gem_amd.Costmap.nav_plan_quadratic) and "nav_quad_host" in gem_amd.__all__
    g = np.zeros((8, 8), np.uint8)
    pot, cells, st = gem_amd.nav_quad_host(g, (0, 0), (3, 3), weights=np.full(256, 50, np.int32), outline=False)
    assert pot[3, 3] == 236 and pot[1, 1] == 85 and cells.tolist() == [0, 9, 18, 27] and st["found"] == 1 and st["goal_potential"] == 236
    with pytest.raises(ValueError):
        gem_amd.nav_quad_host(g, (0, 0), (3, 3), weights=np.full(256, 463, np.int32))


def build_navquad_facade(out: Path) -> Path:
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc", "-std=c++17", "-O2", "-Wall", "-Werror",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "navquad_facade.cpp"), "-o", str(out),
           f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_navquad_facade_builds(tmp_path):
    """gem::Costmap::navPlanQuadratic compiles with hipcc against the installed headers and the library; the host twin is checked
    against the hand-derived potentials, and without a GPU the check exits early."""
    from gem_amd import build
    build.build()
    exe = build_navquad_facade(tmp_path / "navquad_facade")
    res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: built)"), res.stdout + res.stderr
