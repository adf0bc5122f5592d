"""CPU tests of the inflation contract (include/gem_hip_inflate.h) as tests/inflate_ref.py restates it: the library's host-only cost
table against the restatement byte for byte, what indexing the table by squared distance rests on, the error cases of the table call,
known answers written out by hand, the library's brushfire against the exact nearest seed (equal on structured inputs, never closer on
noise), idempotence, the ABI, and the C++ facade check compiling against the headers.  Nothing is launched: without a GPU the C++
check exits early."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import inflate_ref as ref  # noqa: E402

RES = 0.05
RADII = [1, 2, 11, 64, 127]


def params_for(R, res=RES, inscribed=0.12, weight=3.0, inflate_unknown=False):
    """an inflation radius a fifth of a cell short of R cells: ceil gives R"""
    return ref.Params(max(R * res - 0.2 * res, 0.0), inscribed, weight, inflate_unknown)


def lib_table(p, res):
    from gem_amd import _lib
    lib = _lib.load()
    s = _lib.InflationParams(p.inflation_radius, p.inscribed_radius, p.cost_scaling_factor, int(p.inflate_unknown))
    r = C.c_int(-7)
    assert lib.gem_inflation_table(C.byref(s), res, None, C.byref(r)) == 0
    out = np.full(r.value * r.value + 2, 7, np.uint8)                    # one byte behind the table: it must stay
    assert lib.gem_inflation_table(C.byref(s), res, out.ctypes.data_as(C.c_void_p), None) == 0
    assert out[-1] == 7
    return r.value, out[:-1]


# ---- the table --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0] + RADII)
def test_table_equals_the_restatement(R):
    inscribed = [0.0, 0.12, 2.4 * RES, (R + 3) * RES]                    # none, between cells (twice), above the inflation radius
    for ins in inscribed:
        for weight in (0.0, 3.0, 10.0, 55.5):
            p = params_for(R, inscribed=ins, weight=weight)
            want_R, want = ref.table(p, RES)
            got_R, got = lib_table(p, RES)
            assert want_R == R == got_R and got.tobytes() == want.tobytes(), (R, ins, weight)
            assert got[0] == 254 and (got[1:] <= 253).all() and (np.diff(got.astype(int)) <= 0).all()
    if R >= 11:                                                          # every class of cost occurs
        _, t = lib_table(params_for(R), RES)
        assert (t == 253).sum() >= 2 and ((t > 0) & (t < 253)).any()
        assert (lib_table(params_for(R, inscribed=(R + 3) * RES), RES)[1][1:] == 253).all()
        assert 253 not in lib_table(params_for(R, inscribed=0.0), RES)[1]


def test_a_cell_exactly_on_the_inscribed_radius():
    # 0.25 and 0.75 are exact in binary: d = 3 cells is 0.75 m exactly and still inscribed, as is (3, 4) -> 5 cells at 1.25 m
    for ins, on in ((0.75, 9), (1.25, 25)):
        p = ref.Params(2.0, ins, 2.0, False)
        R, got = lib_table(p, 0.25)
        assert R == 8 and got.tobytes() == ref.table(p, 0.25)[1].tobytes()
        assert got[on] == 253 and got[on + 1] < 253 and (got[1:on + 1] == 253).all()


def test_hypot_is_sqrt_up_to_128():
    assert ref.hypot_is_sqrt(128)
    assert "hypot" in (ROOT / "include" / "gem_hip_inflate.h").read_text()


def test_table_error_cases():
    from gem_amd import _lib
    lib = _lib.load()
    nan, inf = float("nan"), float("inf")
    out, r = np.full(16, 7, np.uint8), C.c_int(-7)

    def call(p, res=RES):
        s = None if p is None else C.byref(_lib.InflationParams(*p))
        return lib.gem_inflation_table(s, res, out.ctypes.data_as(C.c_void_p), C.byref(r))

    good = (0.1, 0.05, 3.0, 0)
    assert call(good) == 0 and r.value == 2 and out[0] == 254 and out[5] == 7
    out[:] = 7; r.value = -7
    assert call(None) == _lib.GEM_OK - 1
    for k in range(3):
        for bad in (nan, inf, -inf, -0.5):
            p = list(good); p[k] = bad
            assert call(tuple(p)) == _lib.GEM_OK - 1, (k, bad)
    for res in (0.0, -0.05, nan, inf):
        assert call(good, res) == _lib.GEM_OK - 1, res
    assert call((127.5 * RES, 0.05, 3.0, 0)) == _lib.GEM_OK - 1           # 128 cells
    assert (out == 7).all() and r.value == -7                            # nothing written


def test_the_limit_is_127_cells():
    R, t = lib_table(params_for(127), RES)
    assert R == ref.MAX_CELLS == 127 and t.size == 127 * 127 + 1 == 16130


# ---- known answers ------------------------------------------------------------------------------------------------------------------
ONE_SEED = ref.Params(2.0, 1.0, 1.0, False)
ONE_SEED_WANT = [[0, 0, 92, 0, 0],
                 [0, 166, 253, 166, 0],
                 [92, 253, 254, 253, 92],
                 [0, 166, 253, 166, 0],
                 [0, 0, 92, 0, 0]]


def test_one_seed_by_hand():
    # resolution 1, R = 2, inscribed 1: 254 | d2 1 -> 253 | d2 2 -> 252 e^-(sqrt 2 - 1) = 166.5 | d2 4 -> 252 / e = 92.7 | d2 5: outside
    assert ref.table(ONE_SEED, 1.0)[1].tolist() == [254, 253, 166, 121, 92]
    g = np.zeros((5, 5), np.uint8)
    g[2, 2] = 254
    for f in (ref.inflate_exact, ref.inflate_brushfire):
        assert f(g, ONE_SEED, 1.0).tolist() == ONE_SEED_WANT
    # the rule for 255 and for old costs above the new one
    g[1, 1] = 255; g[2, 3] = 255; g[0, 2] = 200
    want = [row[:] for row in ONE_SEED_WANT]
    want[1][1] = 255; want[0][2] = 200
    for f in (ref.inflate_exact, ref.inflate_brushfire):
        assert f(g, ONE_SEED, 1.0).tolist() == want
        want_u = [row[:] for row in want]
        want_u[1][1] = 166
        assert f(g, ONE_SEED._replace(inflate_unknown=True), 1.0).tolist() == want_u


@pytest.mark.parametrize("at", [0, 3])
def test_three_cells_where_the_brushfire_is_not_exact(at):
    """lethal cells at (2, 2), (3, 0) and (0, 3) relative to p: p's nearest is (2, 2) at squared distance 8, but the brushfire reaches p
    from one of the other two, at 9.  With an inscribed radius of 2.9 cells the exact cost is 253 and the library's lower."""
    g = np.zeros((10, 10), np.uint8)
    for x, y in ((2, 2), (3, 0), (0, 3)):
        g[at + y, at + x] = 254
    p = ref.Params(4.0, 2.9, 1.0, False)
    exact, d_exact = ref.inflate_exact(g, p, 1.0, None, True)
    brush, d_brush = ref.inflate_brushfire(g, p, 1.0, None, True)
    assert d_exact[at, at] == 8 and d_brush[at, at] == 9
    assert exact[at, at] == 253 and brush[at, at] == ref.compute_cost(p, 1.0, 3.0) == 228
    assert (exact != brush).sum() == 1
    text = (ROOT / "include" / "gem_hip_inflate.h").read_text()
    assert "DELIBERATE DIFFERENCE" in text and "(2, 2), (3, 0) and (0, 3)" in text and "NOT verified" in text


# ---- the brushfire against the exact nearest seed -------------------------------------------------------------------------------------
def structured():
    z = lambda: np.zeros((60, 60), np.uint8)                             # noqa: E731
    single = z(); single[30, 31] = 254
    wall = z(); wall[10:50, 20] = 254
    rect = z(); rect[20:30, 15:40] = 254
    ell = z(); ell[10:45, 12] = 254; ell[44, 12:50] = 254
    diag = z(); diag[np.arange(5, 55), np.arange(5, 55)] = 254
    return {"single": single, "wall": wall, "rectangle": rect, "L": ell, "diagonal": diag}


@pytest.mark.parametrize("R", [4, 11])
@pytest.mark.parametrize("name", list(structured()))
def test_brushfire_equals_exact_on_structured_inputs(name, R):
    g = structured()[name]
    g[::7, ::5] = np.where(g[::7, ::5] == 254, 254, 255)                 # some unknown cells, inside and outside the inscribed radius
    for unknown in (False, True):
        p = params_for(R, inflate_unknown=unknown)
        exact, d_exact = ref.inflate_exact(g, p, RES, None, True)
        brush, d_brush = ref.inflate_brushfire(g, p, RES, None, True)
        assert (d_exact == d_brush).all() and exact.tobytes() == brush.tobytes()
        assert (exact != g).sum() > 20


def noise_grid(rng, sx, sy, lethal, unknown=0.1):
    g = rng.integers(0, 253, (sy, sx), dtype=np.uint8)
    u = rng.random((sy, sx))
    g[rng.random((sy, sx)) < unknown] = 255
    g[u < lethal] = 254
    return g


@pytest.mark.parametrize("R", [4, 11])
@pytest.mark.parametrize("lethal", [0.002, 0.05, 0.2])
def test_brushfire_is_never_closer_than_exact_on_noise(lethal, R):
    rng = np.random.default_rng(int(lethal * 1000) + R)
    differ = 0
    for _ in range(3):
        g = noise_grid(rng, 60, 60, lethal)
        for unknown in (False, True):
            p = params_for(R, inflate_unknown=unknown)
            exact, d_exact = ref.inflate_exact(g, p, RES, None, True)
            brush, d_brush = ref.inflate_brushfire(g, p, RES, None, True)
            assert (d_brush >= d_exact).all()                            # (NONE is the largest value: unreached means unreached in both)
            known = g != 255
            assert (brush[known] <= exact[known]).all()
            differ += int((brush != exact).sum())
    print(f"lethal {lethal} R {R}: {differ} of {6 * 3600} cells differ")
    assert differ <= 6 * 36                                              # at most 1 %: the two are the same thing nearly everywhere


# ---- what follows from the contract -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 2, 11])
def test_idempotence_and_seed_invariance(R):
    rng = np.random.default_rng(R)
    g = noise_grid(rng, 75, 75, 0.01)
    for unknown in (False, True):
        p = params_for(R, inflate_unknown=unknown)
        for window in (None, (10, 12, 40, 50), (0, 0, 20, 20), (30, 30, 30, 60)):
            once = ref.inflate_exact(g, p, RES, window)
            assert ((once == 254) == (g == 254)).all()                   # a 254 never appears or disappears
            assert ref.seeds(once, window, R) == ref.seeds(g, window, R)
            assert ref.inflate_exact(once, p, RES, window).tobytes() == once.tobytes()
            if R == 0 or window == (30, 30, 30, 60):
                assert once.tobytes() == g.tobytes()                     # R == 0 and an empty window change nothing
            else:
                assert once.tobytes() != g.tobytes()


def test_window_seeds_are_those_within_R_of_the_window():
    g = np.zeros((40, 40), np.uint8)
    g[20, 5] = 254                                                       # 5 cells left of the window's first column 10
    for R, hit in ((5, True), (4, False)):
        out = ref.inflate_exact(g, params_for(R, inscribed=0.0), RES, (10, 10, 30, 30))
        assert (out.tobytes() != g.tobytes()) == hit
        if hit:
            assert out[20, 0] > 0                                        # cells outside the window change too: every cell of the map
    r = g.copy()
    ref.reset_window(r, 3, 18, 8, 22, 7)
    assert (r[18:22, 3:8] == 7).all() and (r != g).sum() == 20


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def declared(header):
    import re
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(gem_[a-z_0-9]+)\s*\(", text)))


def test_inflate_symbols_are_declared_exported_and_bound():
    from gem_amd import _lib
    lib = _lib.load()
    names = declared(ROOT / "include" / "gem_hip_inflate.h")
    assert names == sorted(_lib.INFLATE_SIGNATURES) == ["gem_costmap_inflate", "gem_costmap_reset_window", "gem_inflation_table"]
    for n in names:
        assert getattr(lib, n).argtypes == _lib.INFLATE_SIGNATURES[n][1]
    assert '#include "gem_hip_inflate.h"' in (ROOT / "include" / "gem_hip.h").read_text()
    assert lib.gem_abi_version() == 9


def test_params_layout_matches_the_header(tmp_path):
    from gem_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gem_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d\\n", '
                   "sizeof(gem_inflation_params), offsetof(gem_inflation_params, inflation_radius), offsetof(gem_inflation_params, inscribed_radius), "
                   "offsetof(gem_inflation_params, cost_scaling_factor), offsetof(gem_inflation_params, inflate_unknown), GEM_INFLATE_MAX_CELLS); "
                   "return 0; }\n")
    exe = tmp_path / "layout"
    res = subprocess.run(["cc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.InflationParams
    assert got == [C.sizeof(S), S.inflation_radius.offset, S.inscribed_radius.offset, S.cost_scaling_factor.offset, S.inflate_unknown.offset,
                   _lib.INFLATE_MAX_CELLS]
    assert got[5] == ref.MAX_CELLS and _lib.COST_INSCRIBED_INFLATED_OBSTACLE == ref.INSCRIBED


def test_python_facade_has_the_inflation_calls():
    import gem_amd
    for name in ("inflate", "reset_window"):
        assert callable(getattr(gem_amd.Costmap, name))
    p = params_for(11)
    R, t = gem_amd.inflation_table(RES, p.inflation_radius, p.inscribed_radius, p.cost_scaling_factor)
    assert R == 11 and t.dtype == np.uint8 and t.tobytes() == ref.table(p, RES)[1].tobytes()
    with pytest.raises(ValueError):
        gem_amd.inflation_table(RES, 128 * RES, 0.1)


def build_inflate_check(out: Path) -> Path:
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc", "-std=c++17", "-O1", "-Wall", "-Werror",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "inflate_check.cpp"), "-o", str(out),
           f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_inflate_facade_builds():
    """gem::InflationParams and gem::Costmap's inflation calls compile with hipcc against the installed headers and the library; the
    host-only table is checked, and without a GPU the check exits early."""
    import tempfile
    from gem_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as td:
        exe = build_inflate_check(Path(td) / "inflate_check")
        res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: built)"), res.stdout + res.stderr
