"""CPU tests of the best-trajectory contract of include/gem_hip_critics.h: the restatement itself (tests/critics_ref.py: the library's
loop with its early exit against the contract's loop without it), the host-only gem_critics_select against the restatement bit for bit,
and the ABI (symbols, constants, sizes, the Python and C++ facades).  Every comparison is exact."""
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
import critics_ref as ref  # noqa: E402

N_TABLES = 480


# ---- random score tables ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables():
    """[(critics, scores [n_critics, n_traj])]: 1 - 8 critics, 0 - 200 trajectories; zero scales, zero scores, negatives, NaN externals
    and exact ties (scores and scales are small multiples of 1/4, so sums are exact and collide often).  Never changed."""
    rng = np.random.default_rng(20261019)
    out = []
    for k in range(N_TABLES):
        nc = int(rng.integers(1, 9))
        nt = 0 if k % 40 == 7 else int(rng.integers(1, 201))
        scales = rng.integers(0, 9, nc) / 4.0                            # 0 occurs: a critic that is skipped
        if k % 3 == 0:
            scales[int(rng.integers(0, nc))] = 0.0
        critics = [ref.external(s, j) for j, s in enumerate(scales)]
        levels = int(rng.integers(2, 12))                                # few levels: many exact ties
        s = rng.integers(0, levels, (nc, nt)) / 4.0
        reject = 1.0 if k % 10 == 3 else (0.02, 0.1, 0.4)[k % 3]          # every tenth table: everything rejected
        neg = rng.random((nc, nt)) < reject
        if k % 10 == 3 and nt:
            live = int(np.flatnonzero(scales != 0)[0]) if (scales != 0).any() else 0
            scales[live] = max(scales[live], 0.25)
            critics[live]["scale"] = float(scales[live])
            neg[live, :] = True
        s[neg] = -rng.integers(1, 8, int(neg.sum())).astype(np.float64)
        if k % 7 == 0 and nt:
            s[int(rng.integers(0, nc)), int(rng.integers(0, nt))] = np.nan
        if k % 5 == 0 and nt > 3:                                        # the first trajectories cost most: the winner comes later
            s[:, :3] = np.where(s[:, :3] < 0, s[:, :3], s[:, :3] + 50.0)
        s.setflags(write=False)
        out.append((critics, s))
    return out


def as_c(critics):
    from gem_amd import _lib
    return (_lib.Critic * max(len(critics), 1))(*[_lib.Critic(c["kind"], c["grid"], c["flags"], c["column"], c["scale"], c["xshift"]) for c in critics])


def test_the_early_exit_is_irrelevant():
    """the library's loops with the early exit against best_traj_cost pick the same winner at the same cost as the contract's full sums"""
    seen = {"tie": 0, "all rejected": 0, "empty": 0, "winner not 0": 0, "nan": 0, "zero scale": 0, "cut short": 0}
    for critics, s in tables():
        totals = ref.combine(critics, s)
        best, cost, n_valid = ref.find_best(totals)
        lib_best, lib_cost = ref.library_find_best(critics, s)
        assert (best, np.float64(cost).tobytes()) == (lib_best, np.float64(lib_cost).tobytes())
        nt = s.shape[1]
        seen["empty"] += nt == 0
        seen["all rejected"] += nt > 0 and n_valid == 0
        seen["winner not 0"] += best > 0
        seen["tie"] += best >= 0 and int((totals == cost).sum()) > 1
        seen["nan"] += bool(np.isnan(totals).any())
        seen["zero scale"] += any(c["scale"] == 0 for c in critics)
        # the exit does cut trajectories short: a valid trajectory behind the winner whose first term alone already costs more
        live = [k for k, c in enumerate(critics) if c["scale"] != 0]
        if best >= 0 and cost > 0 and len(live) > 1:
            first = s[live[0]] * critics[live[0]]["scale"]
            seen["cut short"] += bool(((first > cost) & (totals >= 0))[best + 1:].any())
    assert all(v > 0 for v in seen.values()), seen
    assert len(tables()) >= 400


def test_known_answers_of_the_combination():
    cs = [ref.external(2.0, 0), ref.external(0.0, 1), ref.external(1.0, 2)]
    s = np.array([[1.0, 0.5, -2.0, 0.5], [-1.0, -1.0, -1.0, -1.0], [0.0, 1.0, 5.0, 1.0]])
    assert ref.combine(cs, s).tolist() == [2.0, 2.0, -2.0, 2.0] and ref.find_best(ref.combine(cs, s)) == (0, 2.0, 3)
    assert ref.library_find_best(cs, s) == (0, 2.0)
    # a negative score decides even behind a NaN; a NaN alone is not valid; -0.0 is a zero score
    cs = [ref.external(1.0, 0), ref.external(1.0, 1)]
    t = ref.combine(cs, np.array([[np.nan, np.nan, -0.0], [-3.0, 1.0, 2.0]]))
    assert t[0] == -3.0 and np.isnan(t[1]) and t[2] == 2.0 and ref.find_best(t) == (2, 2.0, 1)
    assert ref.find_best([]) == (-1, -1.0, 0) and ref.find_best([-1.0, np.nan]) == (-1, -1.0, 0)
    assert ref.find_best([np.inf, np.inf]) == (0, np.inf, 2)
    assert ref.combine(cs, np.zeros((2, 3)), lens=[0, 2, 3], T=2).tolist() == [-5.0, 0.0, -5.0]


# ---- gem_critics_select -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from gem_amd import _lib
    return _lib.load()


def select(lib, critics, s, want_totals=True, n_critics=None):
    from gem_amd import _lib
    s = np.ascontiguousarray(s, np.float64)
    nt = s.shape[1]
    tot = np.full(nt + 2, -77.0)
    best = _lib.BestTrajectory(-9, -9, -9.0, -9)
    rc = lib.gem_critics_select(as_c(critics), len(critics) if n_critics is None else n_critics, s.ctypes.data_as(C.POINTER(C.c_double)) if s.size else None,
                                nt, tot.ctypes.data_as(C.POINTER(C.c_double)) if want_totals else None, C.byref(best))
    return rc, tot, (best.index, best.cost, best.n_valid, best.reserved)


def test_select_equals_the_restatement_bit_for_bit(lib):
    import gem_amd
    for k, (critics, s) in enumerate(tables()):
        totals = ref.combine(critics, s)
        best, cost, n_valid = ref.find_best(totals)
        rc, tot, got = select(lib, critics, s)
        nt = s.shape[1]
        assert rc == 0 and tot[:nt].tobytes() == totals.tobytes() and tot[nt:].tolist() == [-77.0, -77.0], k
        assert got[0] == best and np.float64(got[1]).tobytes() == np.float64(cost).tobytes() and got[2:] == (n_valid, 0), k
        if k % 16 == 0:
            assert select(lib, critics, s, want_totals=False)[2] == got                # out_total may be NULL
            py = gem_amd.select_trajectory(as_c(critics)[:len(critics)], s)
            assert py[:3] == (best, cost, n_valid)
            assert py[3].tobytes() == totals.tobytes()


def test_select_error_cases(lib):
    from gem_amd import _lib
    s = np.ones((1, 3))
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
        rc, tot, got = select(lib, [ref.external(bad, 0)], s)
        assert rc != 0 and (tot == -77.0).all() and got == (-9, -9.0, -9, -9), bad
        assert select(lib, [ref.external(1.0, 0), ref.external(bad, 1)], np.ones((2, 3)))[0] != 0
    nine = [ref.external(1.0, j) for j in range(9)]
    assert select(lib, nine, np.ones((9, 3)))[0] != 0                       # n_critics 9
    assert select(lib, nine[:8], np.ones((8, 3)))[0] == 0
    assert select(lib, nine[:1], s, n_critics=0)[0] != 0                    # n_critics 0
    best = _lib.BestTrajectory(-9, -9, -9.0, -9)
    one = as_c(nine[:1])
    assert lib.gem_critics_select(one, 1, None, 3, None, C.byref(best)) != 0 and best.index == -9      # NULL with a non-zero count
    assert lib.gem_critics_select(None, 1, s.ctypes.data_as(C.POINTER(C.c_double)), 3, None, C.byref(best)) != 0
    assert lib.gem_critics_select(one, 1, s.ctypes.data_as(C.POINTER(C.c_double)), 3, None, None) != 0
    assert lib.gem_critics_select(one, 1, s.ctypes.data_as(C.POINTER(C.c_double)), -1, None, C.byref(best)) != 0
    assert lib.gem_critics_select(one, 1, None, 0, None, C.byref(best)) == 0 and (best.index, best.cost, best.n_valid) == (-1, -1.0, 0)
    with pytest.raises(ValueError):
        import gem_amd
        gem_amd.select_trajectory([gem_amd.external_critic(-1.0, 0)], s)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def declared(header):
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(gem_[a-z_0-9]+)\s*\(", text)))


def test_critics_symbols_are_declared_exported_and_bound(lib):
    from gem_amd import _lib
    names = declared(ROOT / "include" / "gem_hip_critics.h")
    assert names == sorted(_lib.CRITICS_SIGNATURES) == ["gem_costmap_best_trajectory", "gem_costmap_best_trajectory_device",
                                                        "gem_costmap_mapgrid_prepare_front", "gem_costmap_mapgrid_read_front", "gem_critics_select"]
    for n in names:
        assert getattr(lib, n).argtypes == _lib.CRITICS_SIGNATURES[n][1]
    text = (ROOT / "include" / "gem_hip.h").read_text()
    assert text.index('#include "gem_hip_mapgrid.h"') < text.index('#include "gem_hip_critics.h"')
    hdr = (ROOT / "include" / "gem_hip_critics.h").read_text()
    assert "NOT verified" in hdr and "UNVERIFIED" in hdr
    assert lib.gem_abi_version() == 9


def test_constants_and_sizes_match_the_header(tmp_path):
    from gem_amd import _lib
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "gem_hip.h"\nint main(void) { printf("%d %d %d %d %d %d %d %d %d %d\\n", GEM_CRITIC_OBSTACLE, '
                   "GEM_CRITIC_MAPGRID, GEM_CRITIC_EXTERNAL, GEM_CRITIC_MAX, GEM_CRITIC_GRID_PATH, GEM_CRITIC_GRID_GOAL, GEM_CRITIC_GRID_FRONT, "
                   "GEM_CRITIC_CENTRE_COST, (int)sizeof(gem_critic), (int)sizeof(gem_best_trajectory)); return 0; }\n")
    exe = tmp_path / "consts"
    res = subprocess.run(["cc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [_lib.CRITIC_OBSTACLE, _lib.CRITIC_MAPGRID, _lib.CRITIC_EXTERNAL, _lib.CRITIC_MAX, _lib.CRITIC_GRID_PATH, _lib.CRITIC_GRID_GOAL,
                   _lib.CRITIC_GRID_FRONT, _lib.CRITIC_CENTRE_COST, C.sizeof(_lib.Critic), C.sizeof(_lib.BestTrajectory)]
    assert got == [ref.OBSTACLE, ref.MAPGRID, ref.EXTERNAL, ref.MAX, ref.GRID_PATH, ref.GRID_GOAL, ref.GRID_FRONT, ref.CENTRE_COST, 32, 32]
    assert _lib.CRITIC_CENTRE_COST & (_lib.FOOTPRINT_INSCRIBED_LETHAL | _lib.FOOTPRINT_SUM) == 0


def test_python_facade_has_the_critics_calls():
    import gem_amd
    for name in ("best_trajectory", "prepare_map_grid_front", "read_map_grid_front"):
        assert callable(getattr(gem_amd.Costmap, name))
    c = gem_amd.map_grid_critic(24.0, gem_amd._lib.CRITIC_GRID_FRONT, 0.325, gem_amd._lib.MAPGRID_SUM)
    assert (c.kind, c.grid, c.flags, c.column, c.scale, c.xshift) == (2, 4, 2, 0, 24.0, 0.325)
    c = gem_amd.obstacle_critic(0.01, gem_amd._lib.CRITIC_CENTRE_COST)
    assert (c.kind, c.flags, c.scale) == (1, 4, 0.01)
    c = gem_amd.external_critic(1.0, 3)
    assert (c.kind, c.column, c.scale) == (3, 3, 1.0)
    assert gem_amd.select_trajectory([c], np.array([[3.0, 1.0, -1.0, 1.0]]))[:3] == (1, 1.0, 3)


def build_critics_check(out: Path) -> Path:
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc", "-std=c++17", "-O2", "-Wall", "-Werror",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "critics_check.cpp"), "-o", str(out),
           f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_critics_facade_builds():
    """gem::Critic, gem::selectTrajectory and gem::Costmap's best-trajectory calls compile with hipcc -Wall -Werror against the headers
    and the library; the host-only combination is checked, and without a GPU the check exits early."""
    import tempfile
    from gem_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as td:
        exe = build_critics_check(Path(td) / "critics_check")
        res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: built)"), res.stdout + res.stderr
