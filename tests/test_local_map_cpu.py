"""The rolling-window local map (updateLocalMap, EMg.cpp:609-767) without a GPU: hand-derived known answers for the restatement the
GPU tests compare gem_local_* with (tests/local_ref.py, driven from the oracle's show()), the record dtype of the Python API against
PointXYZRGBICT, and that the C++ gem::LocalMap builds."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))

import local_ref  # noqa: E402

F32 = np.float32
L, RES = 8, 0.5


def captured(oracle_mod, traver=None, position=(0.0, 0.0), length=L, res=RES):
    """every cell valid (elevation = its linear index / 8, traver 0.5 unless given), captured at `position` with start (0, 0)."""
    m = oracle_mod.OracleMap(length, res)
    c, s = m.pose()[:2]
    assert list(s) == [0, 0]
    m.set_layer("elevation", np.arange(length * length, dtype=F32).reshape(length, length) / 8)
    m.set_layer("traver", np.full((length, length), 0.5, F32) if traver is None else traver)
    m.set_layer("color_r", np.full((length, length), 300)); m.set_layer("color_g", np.full((length, length), 7))
    m.set_layer("color_b", np.full((length, length), 255))
    o = m.show(position=position)
    return local_ref.capture(o, length, length * float(F32(res)), float(F32(res)), position, s)


def cells(out, cap):
    """(ix, iy) buffer indices of spilled records, by their position (x = 1.75 - 0.5 ix at centre 0, start 0)"""
    return [(int(round((1.75 - float(r["x"])) / 0.5)), int(round((1.75 - float(r["y"])) / 0.5))) for r in out]


# current position (the half-width is 2 m: window [c - 2, c + 2]), shift, and the cells that leave it (hand-derived: x, y in
# {1.75, 1.25, ..., -1.75} for ix, iy = 0..7; moving by +0.6 leaves x < -1.4 = ix 7, by -0.6 leaves x > 1.4 = ix 0)
CASES = {
    "+x":  ((0.6, 0.0), (0.6, 0.0), lambda ix, iy: ix == 7),
    "-x":  ((-0.6, 0.0), (-0.6, 0.0), lambda ix, iy: ix == 0),
    "+y":  ((0.0, 0.6), (0.0, 0.6), lambda ix, iy: iy == 7),
    "-y":  ((0.0, -0.6), (0.0, -0.6), lambda ix, iy: iy == 0),
    "++":  ((0.6, 0.6), (0.6, 0.6), lambda ix, iy: ix == 7 or iy == 7),
    "--":  ((-0.6, -0.6), (-0.6, -0.6), lambda ix, iy: ix == 0 or iy == 0),
    "+-":  ((0.6, -0.6), (0.6, -0.6), lambda ix, iy: ix == 7 or iy == 0),
    "-+":  ((-0.6, 0.6), (-0.6, 0.6), lambda ix, iy: ix == 0 or iy == 7),
}


@pytest.mark.parametrize("case", list(CASES))
def test_eight_shift_sign_cases(oracle_mod, case):
    cap = captured(oracle_mod)
    cur, shift, want = CASES[case]
    d = {}
    out, replaced = local_ref.spill(cap, cur, shift, d)
    # iteration order = linear index lin = iy * 8 + ix (column-major)
    expect = [(ix, iy) for iy in range(L) for ix in range(L) if want(ix, iy)]
    assert cells(out, cap) == expect
    assert len(out) == (15 if case[1] in "+-" else 8)                      # both diagonal L-shapes: a row and a column
    assert replaced == 0 and len(d) == len(out)
    r = out[0]
    assert (r["pad"], r["a"], r["r"], r["g"], r["b"]) == (F32(1.0), 0, 300 % 256, 7, 255)
    assert r["travers"] == F32(0.5)


def test_no_move_spills_nothing(oracle_mod):
    cap = captured(oracle_mod)
    assert len(local_ref.spill(cap, (0.6, 0.0), (0.0, 0.0), {})[0]) == 0      # dx == dy == 0: no branch applies
    assert len(local_ref.spill(cap, (0.0, 0.0), (0.6, 0.0), {})[0]) == 0      # inside the window


def test_storage_index_of_elevation(oracle_mod):
    """the record of buffer cell (ix, iy) holds the storage cell [ix][iy]'s elevation (EM.cpp:98-100)"""
    cap = captured(oracle_mod)
    out, _ = local_ref.spill(cap, (0.6, 0.0), (0.6, 0.0), {})
    for r, (ix, iy) in zip(out, cells(out, cap)):
        assert r["z"] == F32((ix * 8 + iy) / 8)


def test_negative_and_nan_traversability_not_spilled(oracle_mod):
    t = np.full((L, L), 0.5, F32)
    t[7, 0] = -0.25             # kept by show (!= -10), not spilled (traver >= 0.0 fails)
    t[7, 1] = np.nan            # dropped by show already
    t[7, 2] = 0.0               # 0.0 >= 0.0: spilled
    t[7, 3] = -0.0              # -0.0 >= 0.0: spilled
    cap = captured(oracle_mod, traver=t)
    assert cap.rec.size == 63
    out, _ = local_ref.spill(cap, (0.6, 0.0), (0.6, 0.0), {})
    assert cells(out, cap) == [(7, iy) for iy in range(2, 8)]


def test_replacement_when_returning(oracle_mod):
    cap = captured(oracle_mod)
    d = {}
    out1, r1 = local_ref.spill(cap, (0.6, 0.0), (0.6, 0.0), d)
    out2, r2 = local_ref.spill(cap, (0.6, 0.6), (0.6, 0.6), d)          # the column ix = 7 again, plus the row iy = 7
    assert (len(out1), r1, len(out2), r2, len(d)) == (8, 0, 15, 8, 15)


def test_export_order_after_reinsert(oracle_mod):
    cap = captured(oracle_mod)
    d = {}
    local_ref.spill(cap, (0.0, 0.6), (0.0, 0.6), d)                       # row iy = 7: ix 0..7
    local_ref.spill(cap, (0.6, 0.0), (0.6, 0.0), d)                       # column ix = 7: (7, 7) re-inserted, goes last
    e = local_ref.export(d)
    got = cells(e, cap)
    assert got == [(ix, 7) for ix in range(7)] + [(7, iy) for iy in range(8)]
    assert len(set(got)) == len(got) == 15


def test_two_cells_one_float_key_far_from_origin(oracle_mod):
    """at x ~ 3e6 the float spacing is 0.25: cells 0.05 m apart round to one key; the later cell wins and counts as replaced"""
    res = 0.05
    far = (3.0e6, 0.0)
    cap = captured(oracle_mod, position=far, res=res)
    out, replaced = local_ref.spill(cap, (far[0] + 0.25, 0.0), (0.25, 0.0), d := {})
    keys = [(float(r["x"]), float(r["y"])) for r in out]
    assert len(out) == 40 and len(set(keys)) == 16                       # columns ux = 3..7 (x < c + 0.05): two float x per row
    assert replaced == len(keys) - len(set(keys)) and len(d) == len(set(keys))


def test_minus_zero_equals_plus_zero():
    d = {}
    rec = np.zeros(2, local_ref.POINT)
    rec["x"] = [F32(-0.0), F32(0.0)]
    for r in rec:
        d[(float(r["x"]), float(r["y"]))] = r.tobytes()
    assert len(d) == 1


def test_point_dtype_matches_pointxyzrgbict():
    from gem_amd import POINT_DTYPE
    assert POINT_DTYPE.itemsize == 32 and POINT_DTYPE == local_ref.POINT
    off = {n: POINT_DTYPE.fields[n][1] for n in POINT_DTYPE.names}
    assert off == {"x": 0, "y": 4, "z": 8, "pad": 12, "b": 16, "g": 17, "r": 18, "a": 19, "covariance": 20, "intensity": 24, "travers": 28}


def build_local_facade_check(out: Path) -> Path:
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc", "-std=c++17", "-O1", "-Wall", "-Werror",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "local_facade_check.cpp"), "-o", str(out),
           f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_local_facade_builds_and_pins_the_record(tmp_path):
    """gem::LocalMap compiles with hipcc against the installed header and the library; without a GPU the check only pins the
    record layout and exits."""
    from gem_amd import build
    build.build()
    exe = build_local_facade_check(tmp_path / "local_facade_check")
    res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: layout)"), res.stdout + res.stderr
