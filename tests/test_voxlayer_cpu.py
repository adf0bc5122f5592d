"""CPU tests of the VoxelLayer contract (include/gem_hip_voxlayer.h) as tests/voxlayer_ref.py restates it: bresenham3D's own loop against
the closed form of the line, the literal form against the set-function form on every case, the known answers that follow from the
contract's text, the host twin gem_voxlayer_host (through tests/cpp/voxlayer_check.cpp, built with a plain g++) against the numpy
statement on every case of the GPU file, its error cases, and the ABI.  Nothing is launched: without a GPU the C++ check stops after the
host twin.  Every comparison is exact: grids and columns by tobytes(), bounds by == on doubles.

The cases of tests/test_voxlayer_gpu.py are built here (`cases()`), once, and never changed.  The geometries, their noise grids and
random clouds and the sensor helper are tests/test_obstacle_cpu.py's."""
import ctypes as C
import functools
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import costmap_ref as cref  # noqa: E402
import obstacle_ref as oref  # noqa: E402
import voxlayer_ref as ref  # noqa: E402
from test_footprint_cpu import ORIGIN  # noqa: E402
from test_obstacle_cpu import COUNTS, EMPTY, GEOMETRIES, STRIDES, extent, f32, hand_made, packed, sensor, world  # noqa: E402

# the buffer's window is wider than the layer's maximum and reaches below both floors: rays are clipped at the ceiling and at the floor
WINDOW = (-0.4, 2.2)
LAYER_MAX = 1.5
GRIDS = {"z10": (10, 0.2, 0.0), "z1": (1, 0.2, 0.0), "z16": (16, 0.2, -0.3), "z10 low": (10, 0.2, -0.3)}
THRESHOLDS = [(15, 0), (2, 0), (15, 2)]                                  # (unknown, mark)


def voxels(grid, thresholds):
    return ref.Voxels(*GRIDS[grid], *thresholds)


def observation(cm, points, origin, raytrace=0.4, stride=16, **more):
    w, _ = extent(cm)
    o = {"points": packed(points, stride), "origin": origin, "obstacle_range": 0.35 * w, "raytrace_range": raytrace * w,
         "min_obstacle_height": WINDOW[0], "max_obstacle_height": WINDOW[1]}
    o.update(more)
    o["points"].setflags(write=False)
    return o


def steep(cm, origin):
    """the records a sweep over the plane never makes: straight below and above the sensor and nearly so (z-dominant rays, the one
    above beyond the layer's maximum), and one in the sensor's own voxel"""
    ox, oy, oz = origin
    r = cm.res
    return np.asarray([(ox, oy, -0.35), (ox, oy, 2.15), (ox + 0.3 * r, oy - 0.2 * r, -0.2), (ox - 1.2 * r, oy + 0.4 * r, 2.1),
                       (ox + 0.1 * r, oy, oz + 0.01), (ox + 2.5 * r, oy + 1.5 * r, -0.1)], np.float32)


@functools.lru_cache(maxsize=None)
def noise_columns(geom):
    """a geometry's columns: per voxel unknown, marked or free at random, marks sparse (two per column on average); built once"""
    sx, sy, _ = GEOMETRIES[geom]
    rng = np.random.default_rng(sx + 29)
    low = rng.integers(0, 1 << 16, (sy, sx), dtype=np.uint32)
    high = low & rng.integers(0, 1 << 16, (sy, sx), dtype=np.uint32) & rng.integers(0, 1 << 16, (sy, sx), dtype=np.uint32)
    cols = low | (high << np.uint32(16))
    cols.setflags(write=False)
    return cols


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (geometry, Voxels, observations, bounds in): every case of the GPU file, and of the host twin's comparison here"""
    out = {}
    for g, geom in enumerate(GEOMETRIES):
        cm, cloud = world(geom)
        s = sensor(cm)
        whole = np.concatenate([cloud, hand_made(cm, s), steep(cm, s)])
        out[f"{geom} z10 range 0.4 w"] = (geom, voxels("z10", (15, 0)), (observation(cm, whole, s, 0.4),), tuple(EMPTY))
        out[f"{geom} z16 range 2.0 w"] = (geom, voxels("z16", (2, 0)), (observation(cm, whole, s, 2.0),), tuple(EMPTY))
        out[f"{geom} z1 range 0.4 w"] = (geom, voxels("z1", (15, 2)), (observation(cm, whole, (s[0], s[1], 0.1), 0.4),), tuple(EMPTY))
        # sensor positions: in the first and the last voxel, on a voxel boundary, below origin_z (nothing cleared), off the map (likewise)
        w, h = extent(cm)
        spots = {"first voxel": (f32(cm.ox + 0.3 * cm.res), f32(cm.oy + 0.6 * cm.res), -0.25),
                 "last voxel": (f32(cm.ox + w - 0.4 * cm.res), f32(cm.oy + h - 0.7 * cm.res), 1.65),
                 "voxel boundary": (cm.ox + 20 * cm.res, cm.oy + 31 * cm.res, -0.3 + 4 * 0.2),
                 "below origin_z": (s[0], s[1], -0.35),
                 "off the map": (f32(cm.ox - 0.05 * w), f32(cm.oy + 0.5 * h), 0.8)}
        for k, (name, at) in enumerate(spots.items()):
            pts = np.concatenate([cloud[:1500], hand_made(cm, at), steep(cm, at)])
            out[f"{geom} sensor {name}"] = (geom, voxels("z10 low", THRESHOLDS[(g + k) % 3]), (observation(cm, pts, at, 0.4, stride=12),),
                                            (at[0], at[1], at[0], at[1]))
        # two clearing and two marking observations with different origins: the marks of one lie on the rays of another
        a, b = sensor(cm, 0.2, 0.3), sensor(cm, 0.7, 0.55, 1.2)
        out[f"{geom} four observations"] = (geom, voxels("z16", (15, 2)), (
            observation(cm, cloud[:1200], a, 0.5, stride=32, marking=False),
            observation(cm, cloud[1000:2200], b, 0.45, stride=12, clearing=False, obstacle_range=0.5 * w),
            observation(cm, cloud[2000:3300], b, 2.0, stride=16, marking=False),
            observation(cm, cloud[3000:4097], a, 0.4, stride=16, clearing=False, obstacle_range=0.6 * w)), tuple(EMPTY))
    cm, cloud = world("75x75")
    for k, n in enumerate(COUNTS):                                       # counts around a wave and a workgroup, every stride
        for j, stride in enumerate(STRIDES):
            v = voxels(("z10", "z1", "z16")[(k + j) % 3], THRESHOLDS[(k + 2 * j) % 3])
            out[f"75x75 n {n} stride {stride}"] = ("75x75", v, (observation(cm, cloud[:n], sensor(cm), (0.4, 2.0)[k % 2], stride),),
                                                   None if n == 63 else tuple(EMPTY))
    # marks alone at mark_threshold 2, and two records in one cell of the last column whose column holds one mark: the library touches
    # the second record only (the first leaves two marks, not above the threshold), the set function touches both -- the first lies
    # further out, so the two forms' bounds differ (DIFFERING)
    cols, v = noise_columns("75x75"), voxels("z16", (15, 2))
    x = cm.size_x - 1
    y = int(np.flatnonzero(ref.POPCOUNT16[cols[:, x] >> 16] == 1)[0])
    z = [k for k in range(9) if not (int(cols[y, x]) >> (16 + k)) & 1][:2]
    pair = [(cm.ox + (x + 0.99) * cm.res, cm.oy + (y + 0.5) * cm.res, -0.3 + (z[0] + 0.5) * 0.2),
            (cm.ox + (x + 0.2) * cm.res, cm.oy + (y + 0.5) * cm.res, -0.3 + (z[1] + 0.5) * 0.2)]
    out["75x75 marks in order"] = ("75x75", v, (observation(cm, np.concatenate([cloud[:500], np.asarray(pair, np.float32)]), sensor(cm), clearing=False,
                                                            obstacle_range=2.0 * extent(cm)[0]),), tuple(EMPTY))
    cm, cloud = world("300x260")
    for n in (65, 4097):
        out[f"300x260 n {n} stride 32"] = ("300x260", voxels("z10", (15, 2)), (observation(cm, cloud[:n], sensor(cm), 0.4, 32),), tuple(EMPTY))
    return out


def fresh(geom):
    """a geometry's noise grid and noise columns, as copies"""
    cm = cref.Costmap(*GEOMETRIES[geom], *ORIGIN)
    cm.grid[:] = world(geom)[0].grid
    return cm, noise_columns(geom).copy()


@functools.lru_cache(maxsize=None)
def wanted(name):
    """the reference's answer to a case: (grid bytes, column bytes, bounds or None)"""
    geom, vox, observations, bounds = cases()[name]
    cm, cols = fresh(geom)
    b = None if bounds is None else list(bounds)
    ref.observe(cm, cols, vox, list(observations), LAYER_MAX, b)
    return cm.grid.tobytes(), cols.tobytes(), b


# ---- the line -------------------------------------------------------------------------------------------------------------------------
def test_bresenham3d_is_a_prefix_of_the_closed_form():
    rng = np.random.default_rng(3)
    segs = [tuple(int(v) for v in rng.integers(0, 300, 6)) for _ in range(300)]
    segs += [tuple(int(v) for v in rng.integers(0, 9, 6)) for _ in range(6000)]           # short ones: every tie of the rounding
    segs += [tuple(int(v) for v in np.r_[rng.integers(0, 40, 2), rng.integers(0, 16, 1), rng.integers(0, 40, 2), rng.integers(0, 16, 1)])
             for _ in range(1500)]                                                        # a costmap's proportions: 16 voxels high
    segs += [(5, 5, 5, 5, 5, 5), (0, 0, 0, 0, 0, 9), (0, 0, 9, 0, 0, 0), (3, 4, 2, 11, 4, 2), (4, 3, 2, 4, 11, 2),    # zero length, the axes
             (2, 2, 7, 9, 9, 7), (2, 7, 2, 9, 7, 9), (7, 2, 2, 7, 9, 9), (9, 9, 7, 2, 2, 7),                          # |dx| = |dy|, |dx| = |dz|, |dy| = |dz|
             (1, 1, 1, 8, 8, 8), (8, 8, 8, 1, 1, 1), (8, 1, 8, 1, 8, 1), (0, 0, 0, 1, 0, 0), (7, 3, 3, 7, 3, 4)]      # all three equal
    seen, cuts = set(), 0
    for s in segs:
        whole = ref.line_closed(*s)
        d = (s[3] - s[0], s[4] - s[1], s[5] - s[2])
        da = len(whole) - 1
        assert da == max(abs(v) for v in d) and whole[0] == s[:3] and whole[-1] == s[3:]
        assert ref.raytrace_line(*s) == whole                             # no limit: max_length = UINT_MAX
        ad = sorted(abs(v) for v in d)
        seen.add((ref.dominant(*d), ad[2] == ad[1], ad[0] == ad[1]))
        for cell_range in (range(0, da + 2) if da <= 10 else sorted({0, 1, da // 3, da // 2, da - 1, da, da + 1})):
            got = ref.raytrace_line(*s, cell_range)
            end = ref.ray_end(*s, cell_range)
            assert got == whole[:end + 1], (s, cell_range)
            assert end <= min(cell_range, da)
            cuts += end < da
    # every dominant axis; all three deltas equal; the top two equal; and, under each strictly dominant axis, its two minor deltas equal
    assert {k[0] for k in seen} == {0, 1, 2} and (0, True, True) in seen and any(k[1] and not k[2] for k in seen)
    assert {k[0] for k in seen if k[2] and not k[1]} == {0, 1, 2}
    assert cuts > 20000
    # max_length 0 keeps the first voxel alone, a zero-length line is its voxel whatever the range
    assert ref.raytrace_line(3, 4, 5, 9, 4, 5, 0) == [(3, 4, 5)] and ref.raytrace_line(3, 4, 5, 3, 4, 5, 0) == [(3, 4, 5)]
    # the double coordinates enter the length only: fractions change dist, not the voxels
    assert ref.raytrace_line(0.9, 0.0, 0.0, 4.0, 0.0, 0.0, 4) == [(k, 0, 0) for k in range(5)]
    assert ref.raytrace_line(0.0, 0.0, 0.0, 4.9, 0.0, 0.0, 4) == [(k, 0, 0) for k in range(4)]      # scale = 4 / 4.9, (unsigned)(3.26) = 3


# ---- the two forms ----------------------------------------------------------------------------------------------------------------------
def contains(outer, inner):
    return outer[0] <= inner[0] and outer[1] <= inner[1] and outer[2] >= inner[2] and outer[3] >= inner[3]


DIFFERING = "75x75 marks in order"       # mark_threshold 2: the first of two records of a cell that ends lethal does not touch in the library


@pytest.mark.parametrize("name", list(cases()))
def test_literal_form_equals_set_function_form(name):
    geom, vox, observations, bounds = cases()[name]
    observations = list(observations)                                    # every case, its whole clouds
    a, cols_a = fresh(geom)
    b, cols_b = fresh(geom)
    ba, bb = list(EMPTY if bounds is None else bounds), list(EMPTY if bounds is None else bounds)
    ref.observe_loop(a, cols_a, vox, observations, LAYER_MAX, ba)
    ref.observe(b, cols_b, vox, observations, LAYER_MAX, bb)
    assert a.grid.tobytes() == b.grid.tobytes(), int((a.grid != b.grid).sum())
    assert cols_a.tobytes() == cols_b.tobytes(), int((cols_a != cols_b).sum())
    if vox.mark_threshold == 0:
        assert ba == bb
    else:
        assert contains(bb, ba), (ba, bb)                                # the header's one named departure: a superset
        if name == DIFFERING:
            assert ba != bb


def test_the_case_set_holds_every_class():
    """cells of every class of the byte rule and rays of every kind, in the reference's answer: a green run cannot be an empty one"""
    cells = dict.fromkeys(["freed", "unknown", "kept", "lethal", "accepted but not lethal"], 0)
    rays = dict.fromkeys(["z-dominant", "cut by the range", "ceiling", "floor", "left", "bottom", "right", "top"], 0)
    for name, (geom, vox, observations, bounds) in cases().items():
        cm, cols = fresh(geom)
        d = {}
        ref.observe(cm, cols, vox, list(observations), LAYER_MAX, None, detail=d)
        for k in ("freed", "unknown", "kept", "lethal"):
            cells[k] += int(d[k].sum())
        if vox.mark_threshold == 2:
            cells["accepted but not lethal"] += int((d["accepted"] & ~d["lethal"]).sum())
        assert (cm.grid.reshape(-1)[d["freed"]] == 0).all() and (cm.grid.reshape(-1)[d["unknown"]] == 255).all()
        assert (cm.grid.reshape(-1)[d["lethal"]] == 254).all()
        assert (cm.grid.reshape(-1)[d["kept"]] == world(geom)[0].grid.reshape(-1)[d["kept"]]).all()
        for c in d["rays"]:
            if c is None:                                                # the sensor outside the voxel grid: nothing is cleared
                rays["none: sensor outside"] = rays.get("none: sensor outside", 0) + 1
                continue
            ok = c["ok"]
            rays["z-dominant"] += int((ok & (c["axis"] == 2) & (c["da"] > 0)).sum())
            rays["cut by the range"] += int((ok & (c["end"] < c["da"])).sum())
            for k in ("ceiling", "floor", "left", "bottom", "right", "top"):
                rays[k] += int((ok & c[k]).sum())
    print(cells, rays)
    assert all(v >= 5 for v in cells.values()), cells
    assert all(v >= 3 for v in rays.values()), rays


# ---- known answers from the contract's text -------------------------------------------------------------------------------------------
def both(vox, observations, layer_max=2.0, fill=100, columns=ref.UNKNOWN_COLUMN, size=20, res=0.5):
    """the two forms on a plain map, which must agree: (grid, columns, bounds)"""
    out = []
    for fn in (ref.observe_loop, ref.observe):
        cm = cref.Costmap(size, size, res, 0.0, 0.0)
        cm.grid[:] = fill
        cols = np.full((size, size), columns, np.uint32)
        b = list(EMPTY)
        fn(cm, cols, vox, observations, layer_max, b)
        out.append((cm.grid, cols, b))
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    assert out[0][2] == out[1][2] or vox.mark_threshold > 0
    return out[1]


def test_known_answers():
    vox = ref.Voxels(10, 0.2, 0.0, 15, 0)
    at = (5.25, 5.25, 0.9)                                               # voxel (10, 10, 4)
    far = np.array([[9.25, 5.25, 0.9]], np.float32)                      # 4 m along x; shortened by 2 * 0.5 to 8.25: voxel (16, 10, 4)
    g, c, b = both(vox, [{"points": far, "origin": at, "raytrace_range": 100.0, "marking": False}])
    assert np.flatnonzero(g[10] == 0).tolist() == list(range(10, 17)) and (g != 100).sum() == 7
    assert (c[10, 10:17] == (ref.UNKNOWN_COLUMN & ~(1 << 4))).all() and (c != ref.UNKNOWN_COLUMN).sum() == 7
    assert b == [8.25, 5.25, 8.25, 5.25]                                 # the ray's end alone: raytraceFreespace does not touch the sensor
    # unknown_threshold 14: a column with one voxel cleared still has 15 unknown ones and turns NO_INFORMATION
    g, _, _ = both(vox._replace(unknown_threshold=14), [{"points": far, "origin": at, "raytrace_range": 100.0, "marking": False}])
    assert (g[10, 10:17] == 255).all() and (g != 100).sum() == 7
    # a mark: both bits of its voxel, 254; pz below origin_z is lifted to origin_z
    low = np.array([[6.25, 5.25, -0.1]], np.float32)
    g, c, b = both(vox, [{"points": low, "origin": at, "clearing": False, "min_obstacle_height": -1.0}])
    assert g[10, 12] == 254 and c[10, 12] == (ref.UNKNOWN_COLUMN | (1 << 16)) and (g != 100).sum() == 1 and b == [6.25, 5.25, 6.25, 5.25]
    # mark_threshold 1: one marked voxel is not lethal and does not touch; two are, and then BOTH records touch here
    one = np.array([[6.25, 5.25, 0.5]], np.float32)
    two = np.array([[6.25, 5.25, 0.5], [6.3, 5.3, 1.1]], np.float32)
    g, c, b = both(vox._replace(mark_threshold=1), [{"points": one, "origin": at, "clearing": False}])
    assert (g == 100).all() and c[10, 12] == (ref.UNKNOWN_COLUMN | (1 << 18)) and b == EMPTY
    g, c, b = both(vox._replace(mark_threshold=1), [{"points": two, "origin": at, "clearing": False}])
    assert g[10, 12] == 254 and c[10, 12] == (ref.UNKNOWN_COLUMN | (1 << 18) | (1 << 21)) and b == [6.25, 5.25, float(np.float32(6.3)), float(np.float32(5.3))]
    # the overhang: marks in voxel 6 over a ray through voxel 1 of the same cell -- the cell stays lethal, the 2-D layer clears it
    over = (1 << 22) | ref.UNKNOWN_COLUMN
    ground = (5.25, 5.25, 0.3)
    ray = np.array([[9.25, 5.25, 0.3]], np.float32)
    for fn in (ref.observe_loop, ref.observe):
        cm = cref.Costmap(20, 20, 0.5, 0.0, 0.0)
        cm.grid[:] = 100
        cm.grid[10, 13] = 254
        cols = np.full((20, 20), ref.UNKNOWN_COLUMN, np.uint32)
        cols[10, 13] = over
        fn(cm, cols, vox, [{"points": ray, "origin": ground, "raytrace_range": 100.0, "marking": False}], 2.0, None)
        assert cm.grid[10, 13] == 254 and cols[10, 13] == over & ~(1 << 1) and cm.grid[10, 12] == 0 and cm.grid[10, 14] == 0
    flat = cref.Costmap(20, 20, 0.5, 0.0, 0.0)
    flat.grid[:] = 100
    flat.grid[10, 13] = 254
    oref.observe(flat, [{"points": ray, "origin": ground, "raytrace_range": 100.0, "marking": False}], 2.0)
    assert flat.grid[10, 13] == 0
    # the sensor below the grid or off the map clears nothing; marks still land
    for bad in ((5.25, 5.25, -0.1), (-0.25, 5.25, 0.9)):
        g, c, b = both(vox, [{"points": np.array([[0.75, 5.25, 0.5]], np.float32), "origin": bad, "obstacle_range": 10.0}])
        assert (g != 100).sum() == 1 and g[10, 1] == 254 and b == [0.75, 5.25, 0.75, 5.25]
    # a ray leaving through the right edge ends in the last column: map_end_x = (20 - 0.5) * 0.5 = 9.75
    g, _, b = both(vox, [{"points": np.array([[25.0, 5.25, 0.9]], np.float32), "origin": at, "raytrace_range": 100.0, "marking": False}])
    assert np.flatnonzero(g[10] == 0).tolist() == list(range(10, 20)) and b == [9.75, 5.25, 9.75, 5.25]
    # a ray above the layer's maximum ends 0.01 below it
    up = np.array([[5.25, 5.25, 1.9]], np.float32)
    _, c, _ = both(vox._replace(size_z=16), [{"points": up, "origin": (5.25, 5.25, 0.1), "raytrace_range": 100.0, "marking": False, "max_obstacle_height": 3.0}],
                   layer_max=1.0)
    assert c[10, 10] == (ref.UNKNOWN_COLUMN & ~0b11111) and (c != ref.UNKNOWN_COLUMN).sum() == 1            # z-dominant: voxels 0 .. 4 (0.99 m)


# ---- the host twin ------------------------------------------------------------------------------------------------------------------
def build_voxlayer_check(out: Path) -> Path:
    """tests/cpp/voxlayer_check.cpp with a plain g++ against the installed headers and the library"""
    from gem_amd import build
    build.build()
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "voxlayer_check.cpp"),
           "-o", str(out), f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def case_bytes(name):
    geom, vox, observations, bounds = cases()[name]
    sx, sy, res = GEOMETRIES[geom]
    b = EMPTY if bounds is None else bounds
    out = [struct.pack("<IIddddIddIIii4d", sx, sy, res, ORIGIN[0], ORIGIN[1], LAYER_MAX, vox.size_z, vox.z_resolution, vox.origin_z,
                       vox.unknown_threshold, vox.mark_threshold, len(observations), int(bounds is not None), *b),
           world(geom)[0].grid.tobytes(), noise_columns(geom).tobytes()]
    for o in observations:
        p = o["points"]
        flags = (oref.MARKING if oref.field(o, "marking") else 0) | (oref.CLEARING if oref.field(o, "clearing") else 0)
        out.append(struct.pack("<qII7d", p.shape[0], p.shape[1] * 4, flags, *o["origin"], oref.field(o, "obstacle_range"),
                               oref.field(o, "raytrace_range"), oref.field(o, "min_obstacle_height"), oref.field(o, "max_obstacle_height")))
        out.append(p.tobytes())
    return b"".join(out)


def test_the_host_twin_equals_the_numpy_statement(tmp_path):
    exe = build_voxlayer_check(tmp_path / "voxlayer_check")
    res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: built)"), res.stdout + res.stderr
    names = list(cases())
    (tmp_path / "in.bin").write_bytes(struct.pack("<i", len(names)) + b"".join(case_bytes(n) for n in names))
    res = subprocess.run([str(exe), "host", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got, at = (tmp_path / "out.bin").read_bytes(), 0
    for name in names:
        geom, _, _, bounds = cases()[name]
        cells = GEOMETRIES[geom][0] * GEOMETRIES[geom][1]
        rc, = struct.unpack_from("<i", got, at)
        grid, cols = got[at + 4:at + 4 + cells], got[at + 4 + cells:at + 4 + 5 * cells]
        b = list(struct.unpack_from("<4d", got, at + 4 + 5 * cells))
        at += 4 + 5 * cells + 32
        want_grid, want_cols, want_b = wanted(name)
        assert rc == 0 and grid == want_grid and cols == want_cols, (name, rc)
        assert b == (EMPTY if bounds is None else want_b), name
    assert at == len(got)


def test_the_python_host_twin_and_its_error_cases():
    from gem_amd import _lib, voxlayer_host
    for name in ("75x75 z10 range 0.4 w", "130x90 four observations", "75x75 n 0 stride 12", "300x260 sensor first voxel"):
        geom, vox, observations, bounds = cases()[name]
        cm, cols = fresh(geom)
        b = voxlayer_host(cm.grid, cols, GEOMETRIES[geom][2], ORIGIN, vox, list(observations), LAYER_MAX, None if bounds is None else list(bounds))
        assert (cm.grid.tobytes(), cols.tobytes(), b) == wanted(name)
    geom, vox, observations, _ = cases()["75x75 n 65 stride 12"]
    cm, cols = fresh(geom)
    nan, inf = float("nan"), float("inf")
    bad = [vox._replace(size_z=0), vox._replace(size_z=17), vox._replace(z_resolution=0.0), vox._replace(z_resolution=-0.2), vox._replace(z_resolution=nan),
           vox._replace(z_resolution=inf), vox._replace(origin_z=nan), vox._replace(origin_z=-inf), vox._replace(unknown_threshold=17),
           vox._replace(mark_threshold=17)]
    for v in bad:
        with pytest.raises(ValueError):
            voxlayer_host(cm.grid, cols, 0.2, ORIGIN, v, list(observations), LAYER_MAX, list(EMPTY))
    for o in ({**observations[0], "raytrace_range": -1.0}, {**observations[0], "origin": (nan, 0.0, 0.0)}, {**observations[0], "marking": False, "clearing": False}):
        with pytest.raises(ValueError):
            voxlayer_host(cm.grid, cols, 0.2, ORIGIN, vox, [o], LAYER_MAX)
    with pytest.raises(ValueError):
        voxlayer_host(cm.grid, cols, 0.2, ORIGIN, vox, list(observations), nan)
    with pytest.raises(ValueError):
        voxlayer_host(cm.grid, cols, 0.0, ORIGIN, vox, list(observations), LAYER_MAX)
    # a NULL columns, grid, geometry or voxel configuration, straight at the C entry
    lib = _lib.load()
    cfg = _lib.CostmapConfig(75, 75, 0.2, ORIGIN[0], ORIGIN[1], 0)
    vc = _lib.VoxelConfig(*vox)
    gp, cp = cm.grid.ctypes.data_as(C.c_void_p), cols.ctypes.data_as(C.c_void_p)
    inv = _lib.GEM_OK - 1
    assert lib.gem_voxlayer_host(gp, None, C.byref(cfg), C.byref(vc), None, 0, LAYER_MAX, None) == inv
    assert lib.gem_voxlayer_host(None, cp, C.byref(cfg), C.byref(vc), None, 0, LAYER_MAX, None) == inv
    assert lib.gem_voxlayer_host(gp, cp, None, C.byref(vc), None, 0, LAYER_MAX, None) == inv
    assert lib.gem_voxlayer_host(gp, cp, C.byref(cfg), None, None, 0, LAYER_MAX, None) == inv
    assert lib.gem_voxlayer_host(gp, cp, C.byref(cfg), C.byref(vc), None, 1, LAYER_MAX, None) == inv
    assert lib.gem_voxlayer_host(gp, cp, C.byref(cfg), C.byref(vc), None, 0, LAYER_MAX, None) == _lib.GEM_OK
    assert cm.grid.tobytes() == world(geom)[0].grid.tobytes() and cols.tobytes() == noise_columns(geom).tobytes()      # nothing changed by any of them


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def declared(header):
    import re
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(gem_[a-z_0-9]+)\s*\(", text)))


def test_voxlayer_symbols_are_declared_exported_and_bound():
    from gem_amd import _lib
    lib = _lib.load()
    names = declared(ROOT / "include" / "gem_hip_voxlayer.h")
    assert names == sorted(_lib.VOXLAYER_SIGNATURES) and len(names) == 7
    for n in names:
        assert getattr(lib, n).argtypes == _lib.VOXLAYER_SIGNATURES[n][1]
    assert '#include "gem_hip_voxlayer.h"' in (ROOT / "include" / "gem_hip.h").read_text()
    assert lib.gem_abi_version() == 9
    hdr = " ".join((ROOT / "include" / "gem_hip_voxlayer.h").read_text().replace("*", " ").split())
    assert "UNVERIFIED AGAINST THE LIBRARY" in hdr and "NAMED DEPARTURE" in hdr and "NOT PROVIDED" in hdr and "OPEN POINTS" in hdr
    for point in ("popcount <= thr reading of bitsBelowThreshold", "no touch of the sensor", "getSizeInMetersX for map_end", "2 resolution shortening",
                  "sqrt where the library may call hypot"):
        assert point in hdr, point


def test_voxel_config_layout_matches_the_header(tmp_path):
    from gem_amd import _lib
    fields = ["size_z", "z_resolution", "origin_z", "unknown_threshold", "mark_threshold"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gem_hip.h"\nint main(void) { printf("%zu ' + "%zu " * len(fields) + '\\n", '
                   "sizeof(gem_voxel_config), " + ", ".join(f"offsetof(gem_voxel_config, {f})" for f in fields) + "); return 0; }\n")
    exe = tmp_path / "layout"
    res = subprocess.run(["cc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.VoxelConfig
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]


def test_python_facade_has_the_voxel_calls():
    from gem_amd import Costmap
    for name in ("attach_voxels", "detach_voxels", "read_voxels", "write_voxels", "voxel_observe"):
        assert callable(getattr(Costmap, name))
