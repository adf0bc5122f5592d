"""CPU tests of the frontier-search contract of include/gem_hip_frontier.h: the restatement itself (tests/frontier_ref.py: the flood fill
against the order-free sweeps, hand-checkable answers), the host-only gem_frontiers_host against the restatement byte for byte on the
geometries and scenes the device is tested at, the error cases and the ABI (symbols, the include line, the Python and C++ facades).
Every comparison is exact.  The potentials come from gem_navplan_host, which test_navplan_cpu.py pins to navplan_ref."""
import ctypes as C
import functools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import frontier_ref as fref  # noqa: E402
import navplan_ref as nref  # noqa: E402
from test_navplan_cpu import GEOMETRIES, corner_cells, declared  # noqa: E402

SCENES = ["disc", "noise", "known", "unknown"]
RES = 0.2
INV = -1                                                                 # GEM_ERR_INVALID
U = fref.UNREACHED


@pytest.fixture(scope="module")
def lib():
    from gem_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def weights_known_only():
    w = nref.weights(allow_unknown=False)
    w.setflags(write=False)
    return w


def potential(grid, start, outline=False):
    """the potential of a plan with allow_unknown = 0 from `start`: gem_navplan_host"""
    import gem_amd
    pot, _cells, _st = gem_amd.nav_plan_host(grid, start, start, weights_known_only(), outline=outline)
    return pot


@functools.lru_cache(maxsize=None)
def scene(geom, kind, corner):
    """(grid, start) of a geometry, never changed.  disc: a known disc around the start inside unknown | noise: 30 % of the cells 255
    and 30 % of the rest a random byte 0 .. 254 | known: no unknown cell | unknown: every cell but the start"""
    sx, sy = GEOMETRIES[geom]
    start = corner_cells(sx, sy)[corner][0]
    rng = np.random.default_rng(sx * 1000 + sy + 17 * corner)
    g = np.zeros((sy, sx), np.uint8)
    if kind == "disc":
        yy, xx = np.mgrid[0:sy, 0:sx]
        r = 0.7 * max(sx, sy)
        g[(xx - start[0]) ** 2 + (yy - start[1]) ** 2 > r * r] = 255
    elif kind == "noise":
        unknown = rng.random((sy, sx)) < 0.3
        some = ~unknown & (rng.random((sy, sx)) < 0.3)
        g[some] = rng.integers(0, 255, int(some.sum()), dtype=np.uint8)
        g[unknown] = 255
    elif kind == "unknown":
        g[:] = 255
    g[start[1], start[0]] = 0
    g.setflags(write=False)
    return g, start


@functools.lru_cache(maxsize=None)
def expected(geom, kind, corner, params=(0.0, 1.0, 1.0)):
    """(grid, start, pot, fref.search) of a scene: computed once, shared by the host-twin and the device tests"""
    g, start = scene(geom, kind, corner)
    pot = potential(g, start)
    pot.setflags(write=False)
    return g, start, pot, fref.search(g, pot, RES, *params)


def diagonal_scene(anti):
    """130 x 130: one frontier whose two bars touch only across the point where four tiles meet: (63, 63) - (64, 64), or on the
    anti-diagonal (64, 63) - (63, 64)"""
    g = np.zeros((130, 130), np.uint8)
    if not anti:
        g[63, 50:64] = 255
        g[64, 64:80] = 255
    else:
        g[63, 64:80] = 255
        g[64, 50:64] = 255
    g.setflags(write=False)
    return g, (1, 1)


def climbing_scene(left):
    """130 x 130: one frontier whose smallest cell lies in an UPPER tile and whose label, having run down across an edge and along
    row 64, reaches another upper tile only by CLIMBING through that tile's corner: from (63, 64) up to (64, 63) into tile (1, 0), the
    root 660 in tile (0, 0); or, `left`, from (64, 64) up to (63, 63) into tile (0, 0), the root 750 in tile (1, 0).  (diagonal_scene's
    smallest cell lies in an upper tile too, so there a label crosses the corner downwards only.)"""
    g = np.zeros((130, 130), np.uint8)
    if not left:
        g[5:71, 10] = 255
        g[64, 10:64] = 255
        g[63, 64:80] = 255
    else:
        g[5:65, 100] = 255
        g[64, 64:101] = 255
        g[63, 50:64] = 255
    g.setflags(write=False)
    return g, (1, 1)


CLIMBING = {False: (660, 135), True: (750, 110)}                         # left: the frontier's root and its cells


def climbing_expected(left):
    """(grid, start, pot, fref.search) of climbing_scene, with what the scene claims asserted"""
    g, start = climbing_scene(left)
    pot = potential(g, start)
    want = fref.search(g, pot, RES)
    four = fref.labels_flood(want["mask"], fref.N4)
    assert want["n_frontiers"] == 1 and len(np.unique(four[want["mask"]])) == 2      # 4-connectivity would not pass
    assert (want["all"][0]["root"], want["all"][0]["size"]) == CLIMBING[left]
    return g, start, pot, want


def serpentine_scene(n=130):
    """a one-cell-wide serpentine of unknown cells through known free space: rows y = 1, 3, 5, ... span x = 1 .. n - 2 and are joined
    at alternating ends"""
    g = np.zeros((n, n), np.uint8)
    rows = list(range(1, n - 2, 2))
    for k, y in enumerate(rows):
        g[y, 1:n - 1] = 255
        if k + 1 < len(rows):
            g[y + 1, n - 2 if k % 2 == 0 else 1] = 255
    g.setflags(write=False)
    return g, (0, 0)


def far_root_scene():
    """130 x 130: a frontier whose smallest cell lies in the top-left tile and whose mass lies in the bottom-right one: a line from
    (5, 5) along row 5 and down column 100 into a comb of columns"""
    g = np.zeros((130, 130), np.uint8)
    g[5, 5:101] = 255
    g[5:127, 100] = 255
    g[126, 100:125] = 255
    for x in range(102, 126, 2):
        g[100:127, x] = 255
    g.setflags(write=False)
    return g, (1, 1)


def pick_scene():
    """41 x 25, the start at (20, 10): two congruent bars at equal potential left and right of it (A, B: 5 cells, access 9 steps = 450),
    a short bar close to the start (C: 3 cells, 7 steps = 350) and a long one far from it (D: 31 cells, 12 steps = 600)"""
    g = np.zeros((25, 41), np.uint8)
    g[8:13, 10] = 255                                                    # A, root (10, 8)
    g[8:13, 30] = 255                                                    # B
    g[2, 19:22] = 255                                                    # C
    g[23, 5:36] = 255                                                    # D
    g.setflags(write=False)
    return g, (20, 10)


def ragged_scene(n=1000, seed=1000):
    """n x n: a known region with a ragged rim around the middle, 20 % of its cells a random byte 0 .. 255, unknown outside"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n, 0:n]
    dx, dy = xx - n / 2, yy - n / 2
    ang = np.arctan2(dy, dx)
    rim = n * (0.33 + 0.07 * np.sin(5 * ang) + 0.03 * np.sin(17 * ang))
    g = np.full((n, n), 255, np.uint8)
    inside = dx * dx + dy * dy < rim * rim
    g[inside] = 0
    hit = inside & (rng.random((n, n)) < 0.2)
    g[hit] = rng.integers(0, 256, int(hit.sum()), dtype=np.uint8)
    g[n // 2, n // 2] = 0
    g.setflags(write=False)
    return g, (n // 2, n // 2)


def thin_scene(n=1000):
    """the same size with ONE long thin frontier: known below a gently waving line, unknown above it"""
    yy, xx = np.mgrid[0:n, 0:n]
    g = np.where(yy > n / 2 + 40 * np.sin(xx / 37.0), 255, 0).astype(np.uint8)
    g.setflags(write=False)
    return g, (n // 2, n // 4)


def frontier_struct(r):
    from gem_amd import _lib
    return _lib.Frontier(r["root"], r["size"], r["sum_x"], r["sum_y"], r["access_potential"], r["access_cell"], r["cost"])


def host_search(lib, grid, pot, res=RES, params=(0.0, 1.0, 1.0), cap=None, labels=True, out=True):
    from gem_amd import _lib
    sy, sx = grid.shape
    g, p = np.ascontiguousarray(grid, np.uint8), np.ascontiguousarray(pot, np.int32)
    lab = np.full((sy, sx), -5, np.int32)
    n = ((sx + 1) // 2) * ((sy + 1) // 2) if cap is None else cap
    rec = (_lib.Frontier * max(n, 1))()
    st = _lib.FrontierStatus()
    prm = _lib.FrontierParams(*params)
    rc = lib.gem_frontiers_host(g.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p), sx, sy, res, C.byref(prm),
                                lab.ctypes.data_as(C.c_void_p) if labels else None, rec if out else None, n, C.byref(st))
    return rc, lab, rec, st


def same_as_ref(want, lab, rec, st, what):
    """labels by tobytes(), the kept records and the winner as the struct's 40 bytes, the counts as integers"""
    assert lab.dtype == np.int32 and lab.tobytes() == want["labels"].tobytes(), f"{what}: {int((lab != want['labels']).sum())} labels differ"
    assert (st.n_cells, st.n_frontiers, st.n_kept, st.best) == (want["n_cells"], want["n_frontiers"], want["n_kept"], want["best"]), what
    for i, r in enumerate(want["kept"]):
        assert bytes(rec[i]) == bytes(frontier_struct(r)), (what, i, r)
    if want["best"] >= 0:
        assert bytes(st.best_frontier) == bytes(frontier_struct(want["best_frontier"])), what
    else:
        assert st.best_frontier.root == -1 and st.best_frontier.size == 0, what


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_flood_fill_equals_the_sweeps_on_random_grids():
    rng = np.random.default_rng(20261020)
    many = diag_only = 0
    for k in range(120):
        sy, sx = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        mask = rng.random((sy, sx)) < (0.15, 0.4, 0.7)[k % 3]
        a, b = fref.labels_flood(mask), fref.labels_sweeps(mask)
        assert a.dtype == np.int32 and a.tobytes() == b.tobytes(), (k, mask.shape)
        assert ((a >= 0) == mask).all() and (a[mask] <= np.nonzero(mask.reshape(-1))[0]).all()
        n8, n4 = len(np.unique(a[mask])), len(np.unique(fref.labels_flood(mask, fref.N4)[mask]))
        many += n8 > 3
        diag_only += n4 > n8
    assert many >= 30 and diag_only >= 30


def test_known_answers_on_9_x_11():
    sy, sx = 9, 11
    cell = lambda x, y: y * sx + x  # noqa: E731
    # a door on each of the four sides: the only reached cell lies left of, right of, above, below the unknown cell (5, 4)
    for xd, yd in fref.N4:
        g = np.zeros((sy, sx), np.uint8)
        g[4, 5] = 255
        pot = np.full((sy, sx), U, np.int32)
        pot[4 + yd, 5 + xd] = 7
        s = fref.search(g, pot, 0.5)
        assert s["n_cells"] == 1 and s["all"] == [{"root": cell(5, 4), "size": 1, "sum_x": 5, "sum_y": 4, "access_potential": 7,
                                                   "access_cell": cell(5 + xd, 4 + yd), "cost": 7.0 - 0.5}]
    # four doors: the smallest potential wins, among equals the smaller cell
    g = np.zeros((sy, sx), np.uint8)
    g[4, 5] = 255
    pot = (10 * (np.arange(sx)[None, :] + np.arange(sy)[:, None])).astype(np.int32)
    s = fref.search(g, pot, 0.5)
    assert s["all"][0]["access_potential"] == 80 and s["all"][0]["access_cell"] == cell(5, 3)      # (5, 3) and (4, 4) tie at 80
    # the start on an unknown byte is no door: (3, 2) has no other reached neighbour; the start itself has the door (1, 2)
    g = np.zeros((sy, sx), np.uint8)
    g[2, 2] = g[2, 3] = 255
    pot = np.full((sy, sx), U, np.int32)
    pot[2, 2] = 0
    pot[2, 1] = 50
    s = fref.search(g, pot, 0.5)
    assert s["mask"].sum() == 1 and s["mask"][2, 2] and s["all"][0]["access_cell"] == cell(1, 2) and s["all"][0]["access_potential"] == 50
    # an unknown cell whose known neighbours are all unreached is no frontier cell
    g = np.zeros((sy, sx), np.uint8)
    g[6, 8] = 255
    pot = np.full((sy, sx), U, np.int32)
    pot[0, 0] = 0
    s = fref.search(g, pot, 0.5)
    assert s["n_cells"] == 0 and s["best"] == -1 and (s["labels"] == -1).all()
    # two cells that touch by a corner are one frontier; a third one two columns on is another
    g = np.zeros((sy, sx), np.uint8)
    g[3, 4] = g[4, 5] = g[4, 7] = 255
    pot = (10 * (np.arange(sx)[None, :] + np.arange(sy)[:, None])).astype(np.int32)
    s = fref.search(g, pot, 0.5, min_frontier_size=1.0, potential_scale=2.0, gain_scale=3.0)
    assert [r["root"] for r in s["all"]] == [cell(4, 3), cell(7, 4)] and s["labels"][4, 5] == cell(4, 3)
    a, b = s["all"]
    assert (a["size"], a["sum_x"], a["sum_y"], a["access_potential"], a["access_cell"]) == (2, 9, 7, 60, cell(4, 2))
    assert a["cost"] == 2.0 * 60 - 3.0 * (2 * 0.5) and b["cost"] == 2.0 * 100 - 3.0 * 0.5
    assert s["n_kept"] == 1 and s["best"] == 0 and s["best_frontier"] is a                        # b is half a metre long: dropped
    assert fref.centroid(a, 0.5, -1.0, 2.0) == (-1.0 + (4.5 + 0.5) * 0.5, 2.0 + (3.5 + 0.5) * 0.5)


def test_special_scenes_are_what_they_claim():
    for anti in (False, True):
        g, start = diagonal_scene(anti)
        mask, _ = fref.classify(g, potential(g, start))
        assert len(np.unique(fref.labels_flood(mask)[mask])) == 1 and len(np.unique(fref.labels_flood(mask, fref.N4)[mask])) == 2
    g, start = serpentine_scene()
    s = fref.search(g, potential(g, start), RES)
    assert s["n_frontiers"] == 1 and s["all"][0]["size"] > 60 * 128 and s["n_cells"] == int((g == 255).sum())
    g, start = far_root_scene()
    s = fref.search(g, potential(g, start), RES)
    assert s["n_frontiers"] == 1 and s["all"][0]["root"] == 5 * 130 + 5
    assert s["all"][0]["sum_x"] / s["all"][0]["size"] > 90 and s["all"][0]["sum_y"] / s["all"][0]["size"] > 64


# ---- the host twin against it ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SCENES)
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_host_twin_equals_the_restatement(lib, geom, kind):
    cells = 0
    for corner in range(4):
        g, start, pot, want = expected(geom, kind, corner)
        rc, lab, rec, st = host_search(lib, g, pot)
        assert rc == 0 and st.rounds == 0 and st.chunks == 0
        same_as_ref(want, lab, rec, st, f"{geom} {kind} corner {corner}")
        cells += st.n_cells
    if kind == "known":
        assert cells == 0
    if kind == "unknown":
        assert cells > 0
    if kind in ("disc", "noise") and min(GEOMETRIES[geom]) > 3:
        assert cells > 0


def test_host_twin_special_scenes_and_the_pick(lib):
    for name, (g, start) in (("diagonal", diagonal_scene(False)), ("anti-diagonal", diagonal_scene(True)), ("serpentine", serpentine_scene()),
                             ("far root", far_root_scene())):
        pot = potential(g, start)
        rc, lab, rec, st = host_search(lib, g, pot)
        assert rc == 0
        same_as_ref(fref.search(g, pot, RES), lab, rec, st, name)
    for left in (False, True):
        g, start, pot, want = climbing_expected(left)
        rc, lab, rec, st = host_search(lib, g, pot)
        assert rc == 0
        same_as_ref(want, lab, rec, st, f"climbing, left {left}")
    g, start = pick_scene()
    pot = potential(g, start)
    winners = {}
    for params in PICK_PARAMS:
        want = fref.search(g, pot, RES, *params)
        rc, lab, rec, st = host_search(lib, g, pot, params=params)
        assert rc == 0
        same_as_ref(want, lab, rec, st, f"pick {params}")
        winners[params] = want["best_frontier"]["root"] if want["best"] >= 0 else None
    check_pick_winners(winners)


PICK_PARAMS = [(0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.7, 1.0, 0.0), (0.0, 1.0, 1000.0), (100.0, 1.0, 1.0), (1.0, 0.0, 0.0)]


def check_pick_winners(winners):
    """the restatement's winners on pick_scene(), derived by hand: with the gain off the close short bar C wins; dropped by
    min_frontier_size (3 cells are 0.6 m) the next cheapest are A and B at equal cost, and the smaller root, A, wins; with the travel
    cost off, or a large gain scale, the long bar D wins; nothing is 100 m long; with both scales 0 every cost is 0 and the smallest
    root wins"""
    A, C_, D = 8 * 41 + 10, 2 * 41 + 19, 23 * 41 + 5
    assert winners[(0.0, 1.0, 0.0)] == C_ and winners[(0.7, 1.0, 0.0)] == A and winners[(0.0, 0.0, 1.0)] == D
    assert winners[(0.0, 1.0, 1000.0)] == D and winners[(100.0, 1.0, 1.0)] is None and winners[(1.0, 0.0, 0.0)] == A
    assert winners[(0.0, 1.0, 0.0)] != winners[(0.0, 0.0, 1.0)]          # a scale pair for which the winner changes


def test_python_twin_and_centroid():
    import gem_amd
    g, start = pick_scene()
    pot = potential(g, start)
    kept, labels, st = gem_amd.frontiers_host(g, pot, RES, 0.7, 1.0, 0.0, origin=(-3.0, 2.0))
    want = fref.search(g, pot, RES, 0.7, 1.0, 0.0)
    assert labels.tobytes() == want["labels"].tobytes() and st["n_kept"] == want["n_kept"] == 3 and st["best"] == want["best"]
    for got, r in zip(kept, want["kept"]):
        assert {k: got[k] for k in r} == r and got["centroid"] == fref.centroid(r, RES, -3.0, 2.0)
    assert st["best_frontier"]["root"] == 8 * 41 + 10 and st["best_frontier"]["centroid"] == (-3.0 + 10.5 * RES, 2.0 + 10.5 * RES)
    with pytest.raises(ValueError):
        gem_amd.frontiers_host(g, pot, RES, -1.0)


def test_host_twin_errors(lib):
    from gem_amd import _lib
    g, start = pick_scene()
    pot = potential(g, start)
    rc, lab, rec, st = host_search(lib, g, pot)
    assert rc == 0 and st.n_kept == 4
    rc, lab, rec, st = host_search(lib, g, pot, cap=3)                    # cap too small: an error, the status still filled
    assert rc == INV and st.n_kept == 4 and st.best_frontier.size > 0 and rec[0].size == 0
    rc, lab, rec, st = host_search(lib, g, pot, labels=False, out=False)  # no outputs: the status alone
    assert rc == 0 and st.n_kept == 4 and st.n_cells == 44
    nan, inf = float("nan"), float("inf")
    for bad in (nan, inf, -inf, -1.0, -1e-300, 1.1e100):
        for k in range(3):
            p = [0.0, 1.0, 1.0]
            p[k] = bad
            assert host_search(lib, g, pot, params=tuple(p))[0] == INV, (bad, k)
    assert host_search(lib, g, pot, params=(1e100, 1e100, 1e100))[0] == 0 and host_search(lib, g, pot, params=(-0.0, 0.0, 0.0))[0] == 0
    for res in (0.0, -0.2, nan, inf):
        assert host_search(lib, g, pot, res=res)[0] == INV
    gp, pp = np.ascontiguousarray(g).ctypes.data_as(C.c_void_p), pot.ctypes.data_as(C.c_void_p)
    prm, st = _lib.FrontierParams(0.0, 1.0, 1.0), _lib.FrontierStatus()
    assert lib.gem_frontiers_host(None, pp, 41, 25, RES, C.byref(prm), None, None, 0, C.byref(st)) == INV
    assert lib.gem_frontiers_host(gp, None, 41, 25, RES, C.byref(prm), None, None, 0, C.byref(st)) == INV
    assert lib.gem_frontiers_host(gp, pp, 41, 25, RES, None, None, None, 0, C.byref(st)) == INV
    assert lib.gem_frontiers_host(gp, pp, 41, 25, RES, C.byref(prm), None, None, 0, None) == INV
    assert lib.gem_frontiers_host(gp, pp, 0, 21, RES, C.byref(prm), None, None, 0, C.byref(st)) == INV
    assert lib.gem_frontiers_host(gp, pp, 41, -1, RES, C.byref(prm), None, None, 0, C.byref(st)) == INV
    assert lib.gem_frontiers_host(gp, pp, 41, 25, RES, C.byref(prm), None, None, 0, C.byref(st)) == 0 and st.n_frontiers == 4


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_frontier_symbols_are_declared_exported_and_bound(lib):
    from gem_amd import _lib
    names = declared(ROOT / "include" / "gem_hip_frontier.h")
    assert names == sorted(_lib.FRONTIER_SIGNATURES) == ["gem_costmap_frontiers", "gem_costmap_frontiers_read", "gem_costmap_navplan_goal",
                                                         "gem_frontiers_host"]
    for n in names:
        assert getattr(lib, n).argtypes == _lib.FRONTIER_SIGNATURES[n][1]
    text = (ROOT / "include" / "gem_hip.h").read_text()
    assert text.index('#include "gem_hip_navplan.h"') < text.index('#include "gem_hip_frontier.h"')
    assert lib.gem_abi_version() == 9
    hdr = (ROOT / "include" / "gem_hip_frontier.h").read_text()
    for word in ("IN THE MANNER OF", "RECALLED FROM MEMORY", "NOT VERIFIED", "DELIBERATELY DEPARTS", "min_distance", "visiting order", "`initial`",
                 "non-increasing costs", "allow_unknown = 0", "CALLER'S business"):
        assert word in hdr, word
    assert '"front_chunk"' in (ROOT / "include" / "gem_hip_debug.h").read_text()


def test_struct_layouts_match_the_header(tmp_path):
    from gem_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gem_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(gem_frontier), offsetof(gem_frontier, sum_x), offsetof(gem_frontier, access_potential), offsetof(gem_frontier, cost), "
                   "sizeof(gem_frontier_status), offsetof(gem_frontier_status, best_frontier), sizeof(gem_frontier_params)); return 0; }\n")
    exe = tmp_path / "layout"
    res = subprocess.run(["cc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    F, S = _lib.Frontier, _lib.FrontierStatus
    assert got == [C.sizeof(F), F.sum_x.offset, F.access_potential.offset, F.cost.offset, C.sizeof(S), S.best_frontier.offset,
                   C.sizeof(_lib.FrontierParams)]
    assert got[0] == 40


def test_python_facade_has_the_frontier_calls():
    import gem_amd
    for name in ("frontiers", "read_frontiers", "nav_plan_to"):
        assert callable(getattr(gem_amd.Costmap, name))
    assert callable(gem_amd.frontiers_host) and "frontiers_host" in gem_amd.__all__


def build_frontier_check(out: Path) -> Path:
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc", "-std=c++17", "-O2", "-Wall", "-Werror",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "frontier_check.cpp"), "-o", str(out),
           f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_frontier_facade_builds():
    """gem::Frontier, gem::FrontierSearch and gem::Costmap::frontiers / readFrontiers / navPlanTo compile with hipcc against the installed
    headers and the library; the host twin is checked against a hand-derived answer, and without a GPU the check exits early."""
    import tempfile
    from gem_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as td:
        exe = build_frontier_check(Path(td) / "frontier_check")
        res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: built)"), res.stdout + res.stderr
