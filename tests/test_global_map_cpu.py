"""The submap stack (updateGlobalMap, EMg.cpp:773-905) without a GPU: hand-derived known answers for the restatement the GPU tests
compare gem_global_* with (tests/global_ref.py), and that the C++ gem::GlobalMap builds."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))

import global_ref  # noqa: E402

F32 = np.float32
EYE = np.eye(4, dtype=F32)


def recs(*rows):
    """rows of (x, y, z, covariance[, r, intensity, travers])"""
    out = np.zeros(len(rows), global_ref.POINT)
    for p, row in enumerate(rows):
        x, y, z, cov = row[:4]
        r, inten, trav = (row[4:] + (10, 1.0, 0.5)[len(row) - 4:]) if len(row) > 4 else (10, 1.0, 0.5)
        out[p]["x"], out[p]["y"], out[p]["z"], out[p]["covariance"] = x, y, z, cov
        out[p]["r"], out[p]["g"], out[p]["b"], out[p]["a"] = r, r + 1, r + 2, 99
        out[p]["intensity"], out[p]["travers"], out[p]["pad"] = inten, trav, 7.0
    return out


def test_quantisation_in_double_near_cell_borders():
    q = lambda v, res: float(global_ref.quantise(F32(v), res))
    # (double) 0.05f = 0.05000000074505806 lies above the double 0.05: ceil(1.0000000149) = 2 -> 2 * 0.05 - 0.025
    assert q(0.05, 0.05) == float(F32(0.075))
    assert q(0.1, 0.05) == float(F32(0.125))                          # 2.00000003 -> 3
    assert q(-0.05, 0.05) == float(F32(-0.075))                       # ceil(-1.0000000149) = -1 -> -0.05 - 0.025
    assert q(0.0, 0.05) == float(F32(-0.025)) and q(-0.0, 0.05) == float(F32(-0.025))
    # with the handle's float as the quantum 0.05f / 0.05f = 1 exactly: the cell below
    rf = float(F32(0.05))
    assert q(0.05, rf) == float(F32(0.025))
    assert q(0.050000004, rf) == float(F32(0.075))


def test_formula_as_precedence_parses_it():
    # nv = 0.5, ne = 2, ov = 0.25, oe = 4: nv2 = 0.25, ov2 = 0.0625
    # elevation = 0.25 * 4 + (0.0625 * 2) / 0.0625 + 0.25 = 3.25 (a variance-weighted mean would be 3.6)
    # variance  = (0.0625 * 0.25) / 0.0625 + 0.25 = 0.5
    stack = [recs((0.01, 0.01, 4.0, 0.25, 20, 3.0, 0.1)), recs((0.02, 0.02, 2.0, 0.5, 40, 5.0, 0.9))]
    fused = global_ref.pair_step(stack, 0, 1, 0.05)
    assert fused == 1
    for s in stack:
        assert s.shape == (1,) and s[0]["z"] == F32(3.25) and s[0]["covariance"] == F32(0.5)
        assert (s[0]["r"], s[0]["g"], s[0]["b"], s[0]["a"]) == (40, 41, 42, 0)        # new's colour
        assert s[0]["intensity"] == F32(5.0) and s[0]["travers"] == F32(0.9) and s[0]["pad"] == F32(1.0)
        assert s[0]["x"] == F32(0.025) and s[0]["y"] == F32(0.025)


@pytest.mark.parametrize("ov", [0.0, 1.0, -0.5, 1.5, float("nan")])
def test_old_variance_outside_the_open_interval_is_not_fused(ov):
    stack = [recs((0.01, 0.01, 4.0, ov)), recs((0.02, 0.02, 2.0, 0.5, 40, 5.0, 0.9))]
    assert global_ref.pair_step(stack, 0, 1, 0.05) == 0
    assert stack[0][0]["z"] == F32(4.0) and stack[1][0]["z"] == F32(2.0)
    assert stack[1][0]["covariance"] == F32(0.5) and stack[0][0]["r"] == 10


def test_new_variance_is_not_tested():
    stack = [recs((0.01, 0.01, 4.0, 0.5)), recs((0.02, 0.02, 2.0, 0.0))]
    assert global_ref.pair_step(stack, 0, 1, 0.05) == 1
    # nv = 0: elevation = 0 + (0.25 * 2) / 0.25 + 0 = 2, variance = 0
    assert stack[0][0]["z"] == F32(2.0) and stack[0][0]["covariance"] == F32(0.0)


def test_first_record_of_a_duplicate_key_wins_and_order_is_first_occurrence():
    stack = [recs((0.01, 0.01, 1.0, 2.0), (0.2, 0.2, 5.0, 2.0), (0.04, 0.03, 9.0, 2.0), (0.21, 0.22, 8.0, 2.0))]
    stack.append(recs((9.0, 9.0, 0.0, 2.0)))
    global_ref.pair_step(stack, 0, 1, 0.05)
    s = stack[0]
    assert list(s["z"]) == [1.0, 5.0]
    assert list(s["x"]) == [F32(0.025), F32(0.225)]


def test_submap_zero_is_never_transformed_and_n_opt_is_clamped():
    t = np.stack([EYE] * 5)
    t[:, 0, 3] = 1.0                                                   # + 1 m in x for every entry, entry 0 included
    far = np.array([[0, 0], [100, 0], [200, 0], [300, 0], [400, 0]], F32)     # no neighbours: transforms only
    stack = [recs((0.5, 0.5, 1.0, 2.0)), recs((0.5, 0.5, 1.0, 2.0))]
    assert global_ref.loop_closure(stack, 5, t, far, 25.0, 0.05) == 0
    assert stack[0][0]["x"] == F32(0.5) and stack[1][0]["x"] == F32(1.5)
    assert stack[1][0]["pad"] == F32(1.0)                              # row 3 of the matrix: 0, 0, 0, 1
    stack = [recs((0.5, 0.5, 1.0, 2.0)) for _ in range(3)]
    global_ref.loop_closure(stack, 1, t[:1], far[:1], 25.0, 0.05)
    assert all(s[0]["x"] == F32(0.5) and s[0]["pad"] == F32(7.0) for s in stack)


def test_transform_rounds_every_step_in_float():
    m = EYE.copy()
    m[0, 0], m[0, 1], m[0, 3] = F32(0.1), F32(0.2), F32(0.3)
    r = recs((F32(3.0), F32(7.0), F32(1.0), 1.0))
    got = global_ref.transform(r, m)[0]["x"]
    want = F32(F32(3.0) * F32(0.1)) + F32(F32(F32(7.0) * F32(0.2)) + F32(F32(F32(1.0) * F32(0.0)) + F32(0.3)))
    assert got == want


def test_two_list_entries_run_no_step_three_run_two():
    two = [recs((0.01, 0.01, 4.0, 0.5)), recs((0.02, 0.02, 2.0, 0.5))]
    assert global_ref.loop_closure(two, 2, np.stack([EYE] * 2), [[0, 0], [10, 0]], 25.0, 0.05) == 0
    assert two[0][0]["pad"] == F32(7.0)                                # not even re-hashed
    three = [recs((0.01, 0.01, 4.0, 0.5)), recs((0.02, 0.02, 2.0, 0.5)), recs((5.0, 5.0, 1.0, 0.5))]
    # every list is [i, the nearer one, the farther one]: i = 0 -> (0, 1), (0, 2); i = 1 -> (1, 0), (1, 2); i = 2 -> (2, 1), (2, 0)
    assert global_ref.neighbours([[0, 0], [10, 0], [21, 0]], 3, 1, 25.0) == [1, 0, 2]
    assert global_ref.neighbours([[0, 0], [10, 0], [21, 0]], 3, 2, 25.0) == [2, 1, 0]
    assert global_ref.loop_closure(three, 3, np.stack([EYE] * 3), [[0, 0], [10, 0], [21, 0]], 25.0, 0.05) == 2     # (0, 1) and (1, 0)


def test_distance_ties_by_index_and_strict_radius():
    c = [[0, 0], [0, 1], [1, 0], [0, -1], [-1, 0]]
    assert global_ref.neighbours(c, 5, 0, 25.0) == [0, 1, 2, 3, 4]
    assert global_ref.neighbours(c, 5, 1, 25.0) == [1, 0, 2, 4, 3]        # d2 1, 2, 2, 4
    assert global_ref.neighbours([[0, 0], [3, 4], [3, 3.99]], 3, 0, 5.0) == [0, 2]   # 25 is not < 25
    assert global_ref.neighbours([[0, 0], [1, 0]], 2, 0, 0.0) == []


def test_coincident_centre_gives_the_self_step():
    # centres 0 and 1 coincide: the list of i = 1 is [0, 1, 2] and its steps are (1, 1) and (1, 2)
    assert global_ref.neighbours([[0, 0], [0, 0], [5, 0]], 3, 1, 10.0) == [0, 1, 2]
    stack = [recs((50.0, 50.0, 1.0, 2.0)), recs((0.01, 0.01, 2.0, 0.5)), recs((30.0, 30.0, 1.0, 2.0))]
    fused = global_ref.pair_step(stack, 1, 1, 0.05)
    # nv = ov = 0.5, ne = oe = 2: elevation = 0.25 * 2 + (0.25 * 2) / 0.25 + 0.25 = 2.75, variance = 0.0625 / 0.25 + 0.25 = 0.5
    assert fused == 1 and stack[1][0]["z"] == F32(2.75) and stack[1][0]["covariance"] == F32(0.5)


def test_nan_key_is_kept_and_never_matched():
    nan = float("nan")
    stack = [recs((nan, 0.01, 4.0, 0.5), (nan, 0.01, 5.0, 0.5), (0.01, 0.01, 1.0, 0.5)), recs((nan, 0.01, 2.0, 0.5))]
    assert global_ref.pair_step(stack, 0, 1, 0.05) == 0
    assert stack[0].shape == (3,) and list(stack[0]["z"]) == [4.0, 5.0, 1.0] and np.isnan(stack[0]["x"][:2]).all()
    assert stack[1].shape == (1,) and stack[1][0]["z"] == F32(2.0)


def test_infinite_key_matches_itself():
    inf = float("inf")
    stack = [recs((inf, 0.01, 4.0, 0.25)), recs((inf, 0.02, 2.0, 0.5))]
    assert global_ref.pair_step(stack, 0, 1, 0.05) == 1 and stack[0][0]["x"] == F32(inf)


def build_global_facade_check(out: Path) -> Path:
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc", "-std=c++17", "-O1", "-Wall", "-Werror",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "global_facade_check.cpp"), "-o", str(out),
           f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_global_facade_builds():
    """gem::GlobalMap compiles with hipcc against the installed header and the library; without a GPU the check exits early."""
    import tempfile
    from gem_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as td:
        exe = build_global_facade_check(Path(td) / "global_facade_check")
        res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: built)"), res.stdout + res.stderr
