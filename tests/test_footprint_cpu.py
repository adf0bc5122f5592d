"""CPU tests of the footprint contract (include/gem_hip_footprint.h) as tests/footprint_ref.py restates it: the closed form of the line
iterator against the iterator's own loop, every sequential form against its vectorised form, the known answers that follow from the
contract's text, the ABI (symbols, struct layout, flags), and the C++ facade check compiling against the headers.  Nothing is
launched: without a GPU the C++ check exits early."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import costmap_ref as cref  # noqa: E402
import footprint_ref as ref  # noqa: E402

EMPTY = [1e30, 1e30, -1e30, -1e30]
ORIGIN = (-3.1, 2.7)
GEOMETRIES = [(75, 75, 0.2), (130, 90, 0.05)]


def noise_map(rng, sx, sy, res, few_253=6):
    """the grids of the GPU tests: bytes uniform in 0 .. 252, 0.4 % of the cells 254, 0.4 % 255, a handful 253"""
    cm = cref.Costmap(sx, sy, res, *ORIGIN)
    cm.grid[:] = rng.integers(0, 253, (sy, sx), dtype=np.uint8)
    u = rng.random((sy, sx))
    cm.grid[u < 0.004] = 254
    cm.grid[(u >= 0.004) & (u < 0.008)] = 255
    cm.grid[rng.integers(0, sy, few_253), rng.integers(0, sx, few_253)] = 253
    return cm


def random_poses(rng, cm, n):
    """uniform over the map's box widened by 10 % on every side, uniform yaw"""
    w, h = cm.size_x * cm.res, cm.size_y * cm.res
    xyt = np.stack([rng.uniform(cm.ox - 0.1 * w, cm.ox + 1.1 * w, n), rng.uniform(cm.oy - 0.1 * h, cm.oy + 1.1 * h, n),
                    rng.uniform(-np.pi, np.pi, n)], axis=1)
    return ref.poses_from_yaw(xyt)


SPECS = {"rectangle": ref.RECTANGLE, "triangle": [[0.7, 0.0], [-0.5, 0.45], [-0.5, -0.45]],
         "16-gon": ref.regular_polygon(16, 0.9), "32-gon": ref.regular_polygon(32, 0.9)}


# ---- the line ---------------------------------------------------------------------------------------------------------------------
def test_closed_form_equals_the_iterator():
    rng = np.random.default_rng(1)
    segs = [tuple(int(v) for v in rng.integers(0, 300, 4)) for _ in range(6000)]
    segs += [tuple(int(v) for v in rng.integers(0, 12, 4)) for _ in range(14000)]          # short ones: every tie of the rounding
    segs += [(5, 5, 5, 5), (0, 0, 0, 9), (0, 9, 0, 0), (3, 4, 11, 4), (11, 4, 3, 4), (2, 2, 9, 9), (9, 9, 2, 2), (9, 2, 2, 9), (0, 0, 1, 0), (7, 3, 7, 4)]
    kinds = set()
    for s in segs:
        dx, dy = abs(s[2] - s[0]), abs(s[3] - s[1])
        kinds.add("cell" if dx == dy == 0 else "dx0" if dx == 0 else "dy0" if dy == 0 else "diag" if dx == dy else "x" if dx > dy else "y")
        a, b = ref.line_iter(*s), ref.line_closed(*s)
        assert a == b, s
        assert a[0] == (s[0], s[1]) and a[-1] == (s[2], s[3]) and len(a) == max(dx, dy) + 1
    assert kinds == {"cell", "dx0", "dy0", "diag", "x", "y"}
    arr = np.asarray(segs, np.int64)
    cx, cy, valid = ref.line_closed_v(arr[:, 0], arr[:, 1], arr[:, 2], arr[:, 3])
    for r, s in enumerate(segs[::37]):
        r *= 37
        assert list(zip(cx[r][valid[r]].tolist(), cy[r][valid[r]].tolist())) == ref.line_closed(*s)


# ---- loop forms against vectorised forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("spec", list(SPECS))
def test_footprint_cost_loop_equals_vectorised(geom, spec):
    rng = np.random.default_rng(geom[0] + len(spec))
    cm = noise_map(rng, *geom)
    poses = random_poses(rng, cm, 300)
    for flags in (0, ref.INSCRIBED_LETHAL):
        got = ref.footprint_cost(cm, poses, SPECS[spec], flags)
        want = [ref.footprint_cost_loop(cm, p, SPECS[spec], flags) for p in poses]
        assert got.tolist() == want
        assert len(set(want)) > 3


def test_transform_forms_agree():
    rng = np.random.default_rng(3)
    poses = random_poses(rng, cref.Costmap(75, 75, 0.2, *ORIGIN), 50)
    wx, wy = ref.transform_v(poses, SPECS["16-gon"])
    for k, p in enumerate(poses):
        assert ref.transform(p, SPECS["16-gon"]) == list(zip(wx[k].tolist(), wy[k].tolist()))


def test_trajectory_forms_agree():
    rng = np.random.default_rng(4)
    for T in (1, 7, 64):
        r = rng.integers(0, 254, (200, T))
        r[rng.random((200, T)) < 0.02] = rng.integers(-3, 0)
        r[0, :] = 5; r[1, :] = 9; r[1, -1] = -2; r[2, 0] = -1; r[2, 1:] = -3
        for flags in (0, ref.SUM):
            a, b = ref.score_trajectories_loop(r, T, flags), ref.score_trajectories(r, T, flags)
            assert a.tolist() == b.tolist()
            assert a[0] == (5 * T if flags else 5) and a[1] == -2 and a[2] == -1


@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}")
def test_fill_loop_equals_set(geom):
    rng = np.random.default_rng(5)
    cm = cref.Costmap(*geom, *ORIGIN)
    poses = random_poses(rng, cm, 200)
    done = 0
    for spec in SPECS.values():
        for p in poses[:60]:
            a, b = cref.Costmap(*geom, *ORIGIN), cref.Costmap(*geom, *ORIGIN)
            ba, bb = list(EMPTY), list(EMPTY)
            oka, okb = ref.clear_footprint(a, p, spec, ba, loop=True), ref.clear_footprint(b, p, spec, bb)
            assert oka == okb and ba == bb and a.grid.tobytes() == b.grid.tobytes()
            assert ba != EMPTY
            done += int(oka)
            if not oka:
                assert (a.grid == 255).all()
    assert done > 50


# ---- known answers ------------------------------------------------------------------------------------------------------------------
def test_known_answers():
    cases = ref.known_answers()
    assert len(cases) > 40
    for name, cm, poses, spec, flags, want in cases:
        assert [ref.footprint_cost_loop(cm, p, spec, flags) for p in poses] == want, name
        assert ref.footprint_cost(cm, poses, spec, flags).tolist() == want, name


def test_clearing_known_answers():
    cm = cref.Costmap(75, 75, 0.2, *ORIGIN)
    mid = (ORIGIN[0] + 7.5, ORIGIN[1] + 7.5, 1.0, 0.0)
    # heading 0: exactly the box of the vertex cells
    cells = [cref.world_to_map(cm, wx, wy) for wx, wy in ref.transform(mid, ref.RECTANGLE)]
    xs, ys = [c[0] for c in cells], [c[1] for c in cells]
    for loop in (False, True):
        cm.reset()
        b = list(EMPTY)
        assert ref.clear_footprint(cm, mid, ref.RECTANGLE, b, loop)
        want = np.full((75, 75), 255, np.uint8)
        want[min(ys):max(ys) + 1, min(xs):max(xs) + 1] = 0
        assert cm.grid.tobytes() == want.tobytes() and (want == 0).sum() == 7 * 5
        assert b == [mid[0] - 0.64, mid[1] - 0.40, mid[0] + 0.64, mid[1] + 0.40]
        # every vertex in one cell: that cell
        cm.reset()
        assert ref.clear_footprint(cm, mid, [[0.001, 0.001], [0.002, 0.001], [0.001, 0.002]], None, loop)
        assert (cm.grid == 0).sum() == 1 and cm.grid[37, 37] == 0
        # fewer than three vertices: nothing written, ok, bounds touched; a vertex off the map: nothing written, not ok, bounds touched
        cm.reset()
        b = list(EMPTY)
        assert ref.clear_footprint(cm, mid, ref.RECTANGLE[:2], b, loop) and (cm.grid == 255).all() and b != EMPTY
        b = list(EMPTY)
        assert not ref.clear_footprint(cm, (ORIGIN[0] + 0.3, mid[1], 1.0, 0.0), ref.RECTANGLE, b, loop)
        assert (cm.grid == 255).all() and b[0] == ORIGIN[0] + 0.3 - 0.64


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def declared(header):
    import re
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(gem_[a-z_0-9]+)\s*\(", text)))


def test_footprint_symbols_are_declared_exported_and_bound():
    from gem_amd import _lib
    lib = _lib.load()
    names = declared(ROOT / "include" / "gem_hip_footprint.h")
    assert names == sorted(_lib.FOOTPRINT_SIGNATURES) and len(names) == 5
    for n in names:
        assert getattr(lib, n).argtypes == _lib.FOOTPRINT_SIGNATURES[n][1]
    hdr = (ROOT / "include" / "gem_hip.h").read_text()
    assert '#include "gem_hip_footprint.h"' in hdr
    assert lib.gem_abi_version() == 9
    assert "NOT verified" in (ROOT / "include" / "gem_hip_footprint.h").read_text()


def test_pose_layout_and_flags_match_the_header(tmp_path):
    from gem_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gem_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d %d %d\\n", '
                   "sizeof(gem_footprint_pose), offsetof(gem_footprint_pose, x), offsetof(gem_footprint_pose, y), "
                   "offsetof(gem_footprint_pose, cos_th), offsetof(gem_footprint_pose, sin_th), GEM_FOOTPRINT_MAX_VERTICES, "
                   "GEM_FOOTPRINT_INSCRIBED_LETHAL, GEM_FOOTPRINT_SUM); return 0; }\n")
    exe = tmp_path / "layout"
    res = subprocess.run(["cc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.FootprintPose
    assert got == [C.sizeof(S), S.x.offset, S.y.offset, S.cos_th.offset, S.sin_th.offset, _lib.FOOTPRINT_MAX_VERTICES,
                   _lib.FOOTPRINT_INSCRIBED_LETHAL, _lib.FOOTPRINT_SUM]
    assert C.sizeof(S) == 32 and (ref.MAX_VERTICES, ref.INSCRIBED_LETHAL, ref.SUM) == tuple(got[5:])


def test_python_facade_has_the_footprint_calls():
    from gem_amd import Costmap
    for name in ("clear_footprint", "footprint_cost", "score_trajectories", "poses_from_yaw"):
        assert callable(getattr(Costmap, name))
    xyt = np.array([[1.0, 2.0, 0.3], [0.0, -1.0, -2.5]])
    assert Costmap.poses_from_yaw(xyt).tobytes() == ref.poses_from_yaw(xyt).tobytes()


def build_footprint_check(out: Path) -> Path:
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc", "-std=c++17", "-O1", "-Wall", "-Werror",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "footprint_check.cpp"), "-o", str(out),
           f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_footprint_facade_builds():
    """gem::FootprintPose and gem::Costmap's footprint calls compile with hipcc against the installed headers and the library;
    without a GPU the check exits early."""
    import tempfile
    from gem_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as td:
        exe = build_footprint_check(Path(td) / "footprint_check")
        res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: built)"), res.stdout + res.stderr
