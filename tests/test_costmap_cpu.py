"""The costmap layers (layers/: PointMapLayer, ElevationMapLayer; costmap_2d restated) without a GPU: hand-computed known answers
for the restatement the GPU tests compare gem_costmap_* with (tests/costmap_ref.py), its literal loops against its vectorised forms,
the struct layout, and that the C++ gem::Costmap builds."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))

import costmap_ref as ref  # noqa: E402
from local_ref import POINT  # noqa: E402

F32 = np.float32
FREE, LETHAL, NOINFO = ref.FREE_SPACE, ref.LETHAL_OBSTACLE, ref.NO_INFORMATION


# ---- worldToMap -------------------------------------------------------------------------------------------------------------------
def test_world_to_map_known_answers():
    cm = ref.Costmap(4, 3, 0.5, origin_x=1.0, origin_y=-2.0)
    assert ref.world_to_map(cm, 1.0, -2.0) == (0, 0)                                  # on the origin: in
    assert ref.world_to_map(cm, 1.0 + 4 * 0.5, -2.0) is None                          # on origin + size * resolution: out
    assert ref.world_to_map(cm, 1.0, -2.0 + 3 * 0.5) is None
    assert ref.world_to_map(cm, 3.0 - 1e-12, -0.5 - 1e-12) == (3, 2)                  # just inside the far corner
    # just below the origin: (int)(-1e-9 / 0.5) would truncate to cell 0; the comparison comes first
    assert ref.world_to_map(cm, 1.0 - 1e-9, -2.0) is None
    assert ref.world_to_map(cm, 1.0, np.nextafter(-2.0, -3.0)) is None
    assert ref.world_to_map(cm, 1.49999, -1.50001) == (0, 0) and ref.world_to_map(cm, 1.5, -1.5) == (1, 1)
    for bad in (np.nan, np.inf, -np.inf):                                              # the contract's deliberate difference
        assert ref.world_to_map(cm, bad, 0.0) is None and ref.world_to_map(cm, 2.0, bad) is None
    assert ref.world_to_map(cm, 1e300, -2.0) is None and ref.world_to_map(cm, 1.0 + 0.5 * 2.0 ** 31, -2.0) is None


def test_world_to_map_vectorised_equals_scalar():
    rng = np.random.default_rng(0)
    cm = ref.Costmap(7, 5, 0.2, origin_x=-0.7, origin_y=0.3)
    wx = np.concatenate([rng.uniform(-1.5, 1.5, 500), [np.nan, np.inf, -np.inf, -0.7, -0.7 + 7 * 0.2, 1e300, -1e300, 0.0]])
    wy = np.concatenate([rng.uniform(-0.5, 2.0, 500), [0.5, 0.5, 0.5, 0.3, 0.3, 0.5, 0.5, np.nan]])
    ok, idx = ref.world_to_map_v(cm, wx, wy)
    for k in range(wx.size):
        m = ref.world_to_map(cm, wx[k], wy[k])
        assert (m is not None) == bool(ok[k])
        if m:
            assert idx[k] == m[1] * cm.size_x + m[0]


# ---- updateOrigin -----------------------------------------------------------------------------------------------------------------
def numbered(sx=5, sy=4, res=0.5, default=NOINFO):
    cm = ref.Costmap(sx, sy, res, 10.0, 20.0, default)
    cm.grid[:] = np.arange(sx * sy, dtype=np.uint8).reshape(sy, sx)
    return cm


@pytest.mark.parametrize("loop", [False, True])
def test_update_origin_known_answers(loop):
    cm = numbered()
    before = cm.grid.copy()
    ref.update_origin(cm, 10.0 - 0.9 * 0.5, 20.0 + 0.9 * 0.5, loop)                   # -0.9 / +0.9 cell: truncates to zero
    assert (cm.ox, cm.oy) == (10.0, 20.0) and np.array_equal(cm.grid, before)
    ref.update_origin(cm, 10.0 + 1.5 * 0.5, 20.0, loop)                               # +1.5 cells moves one
    assert (cm.ox, cm.oy) == (10.5, 20.0)
    assert np.array_equal(cm.grid[:, :4], before[:, 1:]) and (cm.grid[:, 4] == NOINFO).all()
    cm = numbered()
    ref.update_origin(cm, 10.0 - 2 * 0.5, 20.0 + 1 * 0.5, loop)                       # diagonal: two left, one up
    assert (cm.ox, cm.oy) == (9.0, 20.5)
    want = np.full((4, 5), NOINFO, np.uint8)
    want[0:3, 2:5] = before[1:4, 0:3]
    assert np.array_equal(cm.grid, want)
    cm = numbered()
    ref.update_origin(cm, 10.0 + 1 * 0.5, 20.0 - 3 * 0.5, loop)                       # the other diagonal
    want = np.full((4, 5), NOINFO, np.uint8)
    want[3:4, 0:4] = before[0:1, 1:5]
    assert np.array_equal(cm.grid, want)
    for step in ((5, 0), (-5, 0), (0, 4), (7, -9)):                                    # at or beyond the size: everything resets
        cm = numbered(default=FREE)
        ref.update_origin(cm, 10.0 + step[0] * 0.5, 20.0 + step[1] * 0.5, loop)
        assert (cm.grid == FREE).all() and (cm.ox, cm.oy) == (10.0 + step[0] * 0.5, 20.0 + step[1] * 0.5)


def test_roll_to_is_update_origin_about_the_robot():
    a, b = numbered(), numbered()
    ref.roll_to(a, 12.3, 19.1)
    mx, my = (5 - 1 + 0.5) * 0.5, (4 - 1 + 0.5) * 0.5                                  # getSizeInMetersX / Y
    ref.update_origin(b, 12.3 - mx / 2, 19.1 - my / 2)
    assert (a.ox, a.oy) == (b.ox, b.oy) and np.array_equal(a.grid, b.grid)
    assert (a.ox, a.oy) == (10.0 + 2 * 0.5, 20.0 - 3 * 0.5)                            # (12.3 - 1.125 - 10) / 0.5 = 2.35, (19.1 - 0.875 - 20) / 0.5 = -3.55


def test_update_origin_forms_agree_on_random_steps():
    rng = np.random.default_rng(3)
    for _ in range(40):
        a, b = numbered(9, 7, 0.25), numbered(9, 7, 0.25)
        nx, ny = 10.0 + rng.uniform(-3, 3), 20.0 + rng.uniform(-3, 3)
        ref.update_origin(a, nx, ny)
        ref.update_origin(b, nx, ny, loop=True)
        assert np.array_equal(a.grid, b.grid) and (a.ox, a.oy) == (b.ox, b.oy)


# ---- the combination rules ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", [False, True])
def test_merge_rules_on_a_4x4_example(loop):
    layer, master = ref.Costmap(4, 4, 1.0), ref.Costmap(4, 4, 1.0)
    layer.grid[:] = [[FREE, LETHAL, NOINFO, 100]] * 4
    master.grid[:] = np.array([[FREE] * 4, [100] * 4, [LETHAL] * 4, [NOINFO] * 4], np.uint8)
    m = ref.Costmap(4, 4, 1.0); m.grid[:] = master.grid
    ref.merge(layer, m, (0, 0, 4, 4), ref.OVERWRITE, loop)                              # every known layer cell replaces
    assert m.grid.tolist() == [[FREE, LETHAL, FREE, 100], [FREE, LETHAL, 100, 100], [FREE, LETHAL, LETHAL, 100], [FREE, LETHAL, NOINFO, 100]]
    m.grid[:] = master.grid
    ref.merge(layer, m, (0, 0, 4, 4), ref.MAX, loop)                                    # ... only an unknown or smaller master cell
    assert m.grid.tolist() == [[FREE, LETHAL, FREE, 100], [100, LETHAL, 100, 100], [LETHAL, LETHAL, LETHAL, LETHAL], [FREE, LETHAL, NOINFO, 100]]
    m.grid[:] = master.grid
    ref.merge(layer, m, (1, 1, 3, 4), ref.OVERWRITE, loop)                              # a window: columns 1-2, rows 1-3
    assert m.grid.tolist() == [[FREE] * 4, [100, LETHAL, 100, 100], [LETHAL] * 4, [NOINFO, LETHAL, NOINFO, NOINFO]]


# ---- the marking loops ------------------------------------------------------------------------------------------------------------
def records(x, y, travers):
    r = np.zeros(len(x), POINT)
    r["x"], r["y"], r["travers"] = x, y, travers
    return r


def test_point_layer_known_answers():
    cm = ref.Costmap(2, 2, 1.0)
    nan = np.nan
    #           cell (0,0): free then lethal | (1,0): lethal then free | (0,1): exactly the threshold | (1,1): NaN | outside
    r = records([0.1, 0.2, 1.1, 1.2, 0.5, 1.5, 2.0, -0.1], [0.1, 0.2, 0.1, 0.2, 1.5, 1.5, 0.5, 0.5], [0.9, 0.1, 0.1, 0.9, 0.5, nan, 0.9, 0.9])
    b = ref.mark_points(cm, r, 0.5, [1e30, 1e30, -1e30, -1e30])
    assert cm.grid.tolist() == [[LETHAL, FREE], [LETHAL, LETHAL]]                      # travers == thresh is not > thresh: lethal
    assert b == [float(F32(0.1)), float(F32(0.1)), 1.5, 1.5]                           # the refused records touch nothing
    cm2 = ref.Costmap(2, 2, 1.0)
    ref.mark_points(cm2, r[::-1], 0.5)                                                 # reversed: the other record of a cell decides
    assert cm2.grid.tolist() == [[FREE, LETHAL], [LETHAL, LETHAL]]


def test_visual_layer_known_answers():
    # L = 2, res 1, length 2, position (0, 0), start (1, 0): lin -> (ix, iy) = (lin % 2, lin // 2), ux = (ix - 1) % 2, uy = iy;
    # x = 0.5 - ux, y = 0.5 - uy: lin 0 -> (-0.5, 0.5), 1 -> (0.5, 0.5), 2 -> (-0.5, -0.5), 3 -> (0.5, -0.5)
    trav = np.array([0.5, 0.2, np.nan, 0.9], F32)
    g = ref.VisualGeom(2, 2.0, 1.0, (0.0, 0.0), (1, 0))
    px, py, lethal = ref.visual_inputs(trav, g, 0.5)
    assert px.tolist() == [-0.5, 0.5, -0.5, 0.5] and py.tolist() == [0.5, 0.5, -0.5, -0.5]
    assert lethal.tolist() == [False, True, False, False]                              # == thresh is not < thresh; NaN is free
    cm = ref.Costmap(2, 2, 1.0, -1.0, -1.0)
    b = ref.mark_visual(cm, trav, g, 0.5, [1e30, 1e30, -1e30, -1e30])
    assert cm.grid.tolist() == [[FREE, FREE], [FREE, LETHAL]] and b == [-0.5, -0.5, 0.5, 0.5]
    # at traver == thresh the two layers disagree
    one = ref.Costmap(1, 1, 4.0, -2.0, -2.0)
    ref.mark_points(one, records([0.0], [0.0], [0.5]), 0.5)
    assert one.grid[0, 0] == LETHAL
    ref.mark_visual(one, np.array([0.5], F32), ref.VisualGeom(1, 1.0, 1.0, (0.0, 0.0), (0, 0)), 0.5)
    assert one.grid[0, 0] == FREE


def random_cloud(rng, n, cm, thresh=0.5):
    span_x, span_y = cm.size_x * cm.res, cm.size_y * cm.res
    x = cm.ox + rng.uniform(-0.2, 1.2, n) * span_x
    y = cm.oy + rng.uniform(-0.2, 1.2, n) * span_y
    t = rng.uniform(0, 1, n)
    t[rng.random(n) < 0.1] = thresh
    t[rng.random(n) < 0.05] = np.nan
    x[rng.random(n) < 0.02] = np.nan
    y[rng.random(n) < 0.02] = np.inf
    x[rng.random(n) < 0.02] = cm.ox
    y[rng.random(n) < 0.02] = cm.oy + span_y
    return records(x.astype(F32), y.astype(F32), t.astype(F32))


@pytest.mark.parametrize("seed", range(6))
def test_literal_loops_equal_the_vectorised_forms(seed):
    rng = np.random.default_rng(seed)
    sx, sy = int(rng.integers(1, 12)), int(rng.integers(1, 12))
    a = ref.Costmap(sx, sy, 0.2, rng.uniform(-1, 1), rng.uniform(-1, 1), FREE if seed % 2 else NOINFO)
    b = ref.Costmap(sx, sy, 0.2, a.ox, a.oy, a.default)
    for step in range(4):
        r = random_cloud(rng, 400, a)
        nan_start = step == 2                                                          # NaN bounds: std::min / std::max replace them
        b0 = [np.nan] * 4 if nan_start else [1e30, 1e30, -1e30, -1e30]
        ba, bb = ref.mark_points(a, r, 0.5, list(b0)), ref.mark_points(b, r, 0.5, list(b0), loop=True)
        assert np.array_equal(a.grid, b.grid) and ba == bb
        L = 9
        trav = rng.uniform(0, 1, L * L).astype(F32)
        trav[rng.random(L * L) < 0.4] = np.nan
        geom = ref.VisualGeom(L, L * 0.07 + 0.01, 0.07, (a.ox + 0.3, a.oy + 0.2), (int(rng.integers(0, L)), int(rng.integers(0, L))))
        ba = ref.mark_visual(a, trav, geom, 0.5, [1e30, 1e30, -1e30, -1e30])
        bb = ref.mark_visual(b, trav, geom, 0.5, [1e30, 1e30, -1e30, -1e30], loop=True)
        assert np.array_equal(a.grid, b.grid) and ba == bb
        robot = (a.ox + rng.uniform(-1, 3), a.oy + rng.uniform(-1, 3))
        ref.roll_to(a, *robot); ref.roll_to(b, *robot, loop=True)
        assert np.array_equal(a.grid, b.grid) and (a.ox, a.oy) == (b.ox, b.oy)
        ma, mb = ref.Costmap(sx, sy, 0.2, default_value=FREE), ref.Costmap(sx, sy, 0.2, default_value=FREE)
        ma.grid[:] = mb.grid[:] = rng.choice(np.array([FREE, 100, LETHAL, NOINFO], np.uint8), (sy, sx))
        w = (0, 0, sx, sy) if step % 2 else (sx // 3, sy // 3, sx - sx // 4, sy - sy // 4)
        ref.merge(a, ma, w, step % 2); ref.merge(b, mb, w, step % 2, loop=True)
        assert np.array_equal(ma.grid, mb.grid)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------
def test_costmap_config_layout_matches_the_header(tmp_path):
    from gem_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gem_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(gem_costmap_config), offsetof(gem_costmap_config, size_x), offsetof(gem_costmap_config, size_y), "
                   "offsetof(gem_costmap_config, resolution), offsetof(gem_costmap_config, origin_x), offsetof(gem_costmap_config, origin_y), "
                   "offsetof(gem_costmap_config, default_value)); return 0; }\n")
    exe = tmp_path / "layout"
    res = subprocess.run(["cc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.CostmapConfig
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in ("size_x", "size_y", "resolution", "origin_x", "origin_y", "default_value")]
    assert C.sizeof(S) == 40
    assert (_lib.COST_FREE_SPACE, _lib.COST_LETHAL_OBSTACLE, _lib.COST_NO_INFORMATION) == (FREE, LETHAL, NOINFO)


def test_costmap_symbols_are_bound():
    from gem_amd import _lib
    lib = _lib.load()
    names = [n for n in _lib.SIGNATURES if n.startswith("gem_costmap_")]
    assert len(names) == 14 and all(hasattr(lib, n) for n in names)
    assert lib.gem_abi_version() == 9


def build_costmap_facade_check(out: Path) -> Path:
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc", "-std=c++17", "-O1", "-Wall", "-Werror",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "costmap_facade_check.cpp"), "-o", str(out),
           f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_costmap_facade_builds():
    """gem::Costmap compiles with hipcc against the installed header and the library; without a GPU the check exits early."""
    import tempfile
    from gem_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as td:
        exe = build_costmap_facade_check(Path(td) / "costmap_facade_check")
        res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: built)"), res.stdout + res.stderr
