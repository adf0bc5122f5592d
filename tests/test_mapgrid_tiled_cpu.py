"""CPU tests of the tiled MapGrid (gem_costmap_mapgrid_prepare_tiled / _prepare_front_tiled, include/gem_hip_mapgrid_tiled.h):

  1. the protocol's model (tests/mapgrid_tiled_model.py: tiles in a random order, halo cells old or new per edge) byte for byte against
     ref.distance_levels of tests/mapgrid_ref.py on random grids with 0 / 30 / 60 % blocked cells, one to fifty sources, some of them on
     253 / 254 cells, and on the fixed cases of tests/test_mapgrid_tiled_gpu.py: a source at each of the four cells around a tile
     corner, a blocked source, walls on a seam with one gap, the serpentine;
  2. the ABI: sizeof(gem_mapgrid_tiled_status) from a C translation unit that includes gem_hip.h, takes the address of both new symbols
     and links against libgem_hip.so; _lib binds them with the same layout; the facades; the debug key's documentation."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import mapgrid_ref as ref  # noqa: E402
import mapgrid_tiled_model as model  # noqa: E402


def same(grid, sources, rng, tile, what):
    want = ref.distance_levels(grid, sources)
    got, rounds = model.tiled_distance(grid, sources, rng, tile)
    assert got.dtype == np.int32 and got.tobytes() == want.tobytes(), f"{what}: {int((got != want).sum())} cells differ"
    return want, rounds


# ---- 1. the protocol ------------------------------------------------------------------------------------------------------------------
def random_case(rng, k):
    sx, sy = int(rng.integers(1, 201)), int(rng.integers(1, 141))
    share = (0.0, 0.3, 0.6)[k % 3]
    g = rng.integers(0, 253, (sy, sx)).astype(np.uint8)
    blk = rng.random((sy, sx)) < share
    g[blk] = rng.integers(253, 256, int(blk.sum())).astype(np.uint8)
    n = int(rng.integers(1, 51))
    src = [(int(rng.integers(0, sx)), int(rng.integers(0, sy))) for _ in range(n)]
    ys, xs = np.nonzero((g == 253) | (g == 254))
    if k % 2 == 0 and ys.size:
        for j in rng.integers(0, ys.size, 1 + k % 3):
            src.append((int(xs[j]), int(ys[j])))                         # sources on blocked cells
    return g, src


def test_model_equals_the_reference_on_random_grids():
    rng = np.random.default_rng(20261021)
    on_blocked = seams = many_rounds = 0
    for k in range(210):
        g, src = random_case(rng, k)
        tile = (64, 16, 32)[k % 3] if k < 150 else 64                    # the protocol does not depend on the tile size: small tiles, many seams
        on_blocked += any(g[y, x] >= 253 for x, y in src)
        seams += g.shape[0] > tile or g.shape[1] > tile
        _, rounds = same(g, src, rng, tile, f"case {k} {g.shape} tile {tile}")
        many_rounds += rounds > 2
    assert on_blocked >= 50 and seams >= 150 and many_rounds >= 30


def test_a_source_at_each_cell_around_a_tile_corner():
    rng = np.random.default_rng(1)
    for sx, sy in ((128, 128), (130, 70)):
        for kind in ("empty", "noise"):
            g = np.zeros((sy, sx), np.uint8)
            if kind == "noise":
                blk = rng.random((sy, sx)) < 0.3
                g[blk] = rng.integers(253, 256, int(blk.sum())).astype(np.uint8)
                g[62:66, 62:66] = 0
            for cell in ((63, 63), (64, 63), (63, 64), (64, 64)):
                want, _ = same(g, [cell], rng, 64, f"{sx} x {sy} {kind} source {cell}")
                assert want[63, 63] < 3 and want[64, 64] < 3                # the diagonal tile is reached, through one of the four


def test_a_blocked_source_keeps_zero_and_its_neighbours_extend_from_it():
    rng = np.random.default_rng(2)
    for cell in ((63, 10), (64, 10), (10, 63), (10, 64), (0, 0), (129, 69)):    # on both sides of a seam, and in two map corners
        g = np.zeros((70, 130), np.uint8)
        g[cell[1], cell[0]] = 254
        want, _ = same(g, [cell], rng, 64, f"blocked source {cell}")
        assert want[cell[1], cell[0]] == 0 and (want < g.size).all()
    g = np.zeros((70, 130), np.uint8)                                    # a blocked source walled in by blocked cells reaches nothing
    g[9:12, 62:65] = 254
    want, _ = same(g, [(63, 10)], rng, 64, "walled-in blocked source")
    OB, UN = ref.constants(g)
    assert want[10, 63] == 0 and want[10, 62] == OB and want[9, 62] == UN and want[0, 0] == UN


def test_walls_on_the_seams_and_the_serpentine():
    rng = np.random.default_rng(3)
    g = np.zeros((130, 130), np.uint8)
    g[:, 63:65] = 254
    g[40, 63:65] = 0
    want, _ = same(g, [(0, 129)], rng, 64, "wall on columns 63 - 64")
    assert want[40, 64] == 89 + 64 and (want == g.size).any()
    want, _ = same(g.T.copy(), [(129, 0)], rng, 64, "wall on rows 63 - 64")
    assert want[64, 40] == 89 + 64
    n = 130
    g = np.zeros((n, n), np.uint8)
    for y in range(1, n, 2):
        g[y, :] = 254
        g[y, n - 1 if y % 4 == 1 else 0] = 0
    want, rounds = same(g, [(0, 0)], rng, 64, "serpentine")
    assert int(want[want < n * n].max()) == 8514 and rounds > 6             # more rounds than the default chunk of 3 + 3


def test_no_source_converges_at_once():
    g = np.zeros((70, 130), np.uint8)
    got, rounds = model.tiled_distance(g, [], np.random.default_rng(4))
    assert rounds == 0 and (got == g.size + 1).all()


# ---- 2. symbols and layout ------------------------------------------------------------------------------------------------------------
def test_tiled_symbols_and_the_status_layout(tmp_path):
    from gem_amd import _lib, build
    lib = _lib.load()
    src = tmp_path / "tiled.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gem_hip.h"\n'
                   "int main(void) {\n"
                   "    int (*p)(gem_handle*, int, const double*, long long, int, gem_mapgrid_tiled_status*) = &gem_costmap_mapgrid_prepare_tiled;\n"
                   "    int (*f)(gem_handle*, int, const double*, long long, gem_mapgrid_tiled_status*) = &gem_costmap_mapgrid_prepare_front_tiled;\n"
                   '    printf("%d %d %d %d %d %d %d\\n", (int)sizeof(gem_mapgrid_tiled_status), (int)offsetof(gem_mapgrid_tiled_status, started),\n'
                   "           (int)offsetof(gem_mapgrid_tiled_status, goal_cell), (int)offsetof(gem_mapgrid_tiled_status, rounds),\n"
                   "           (int)offsetof(gem_mapgrid_tiled_status, chunks), p != NULL, f != NULL);\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "tiled"
    libdir = build.LIB.parent
    res = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe), f"-L{libdir}", "-lgem_hip",
                          f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.MapGridTiledStatus
    assert got == [C.sizeof(S), S.started.offset, S.goal_cell.offset, S.rounds.offset, S.chunks.offset, 1, 1] and got[0] == 20
    assert sorted(_lib.MAPGRID_TILED_SIGNATURES) == ["gem_costmap_mapgrid_prepare_front_tiled", "gem_costmap_mapgrid_prepare_tiled"]
    for n, (rt, args) in _lib.MAPGRID_TILED_SIGNATURES.items():
        assert getattr(lib, n).argtypes == args and getattr(lib, n).restype == rt
        assert args[-1] == C.POINTER(S)
    text = (ROOT / "include" / "gem_hip.h").read_text()
    assert text.index('#include "gem_hip_critics.h"') < text.index('#include "gem_hip_mapgrid_tiled.h"')
    assert lib.gem_abi_version() == 9                                    # symbols only added


def test_facades_header_text_and_the_debug_key():
    import gem_amd
    for name in ("prepare_map_grid_tiled", "prepare_map_grid_front_tiled"):
        assert callable(getattr(gem_amd.Costmap, name))
    hpp = (ROOT / "include" / "gem" / "gem.hpp").read_text()
    for name in ("struct MapGridTiledStatus", "prepareMapGridTiled(", "prepareMapGridFrontTiled("):
        assert name in hpp
    header = " ".join((ROOT / "include" / "gem_hip_mapgrid.h").read_text().replace("*", " ").split())
    assert "is not provided. GEM_ERR_INVALID" not in header and "gem_costmap_mapgrid_prepare_tiled" in header
    assert "the first host wait of a cycle is the PREPARE" in header
    assert '"mapgrid_chunk"' in (ROOT / "include" / "gem_hip_debug.h").read_text()
    from gem_amd import build
    names = [p.name for p in build.SOURCES + build.HEADERS]
    assert "gem_mapgrid_tiled.hip" in names and "gem_mapgrid_tiled.hpp" in names and "gem_hip_mapgrid_tiled.h" in names
