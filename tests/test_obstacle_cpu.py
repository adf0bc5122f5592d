"""CPU tests of the ObstacleLayer contract (include/gem_hip_obstacle.h) as tests/obstacle_ref.py restates it: the sequential form against
the vectorised one, raytraceLine's own loop against the closed form of the line, the known answers that follow from the contract's
text, the host twin gem_obstacle_host (through tests/cpp/obstacle_check.cpp, built with a plain g++) against the numpy statement on
every case of the GPU file, and the ABI (symbols, struct layout, flags).  Nothing is launched: without a GPU the C++ check stops
after the host twin.  Every comparison is exact: grids by tobytes(), bounds by == on doubles.

The cases of tests/test_obstacle_gpu.py are built here (`cases()`), once, and never changed."""
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
import footprint_ref as fref  # noqa: E402
import obstacle_ref as ref  # noqa: E402
from test_footprint_cpu import ORIGIN, noise_map  # noqa: E402

EMPTY = [1e30, 1e30, -1e30, -1e30]
# 75 x 75 and 130 x 90 keep the bitmaps in LDS, 300 x 260 is above kCostLdsCells (8192 cells): the kernels' one size switch
GEOMETRIES = {"75x75": (75, 75, 0.2), "130x90": (130, 90, 0.05), "300x260": (300, 260, 0.1)}
COUNTS = [0, 1, 63, 64, 65, 4097]
STRIDES = [12, 16, 32]
WINDOW = (0.0, 2.0)
LAYER_MAX = 1.5


def f32(v):
    """the nearest float32, as a Python float: a sensor there can be met exactly by a record (a == 0, b == 0)"""
    return float(np.float32(v))


def extent(cm):
    return cm.size_x * cm.res, cm.size_y * cm.res


def sensor(cm, fx=0.37, fy=0.61, z=0.8):
    w, h = extent(cm)
    return (f32(cm.ox + fx * w), f32(cm.oy + fy * h), z)


def random_cloud(rng, cm, n):
    """x / y uniform over the map's box widened by 30 % per side, z uniform in [-0.5, 2.5]; float32 [n, 3]"""
    w, h = extent(cm)
    return np.stack([rng.uniform(cm.ox - 0.3 * w, cm.ox + 1.3 * w, n), rng.uniform(cm.oy - 0.3 * h, cm.oy + 1.3 * h, n),
                     rng.uniform(-0.5, 2.5, n)], axis=1).astype(np.float32)


def hand_made(cm, origin):
    """the records a random draw never makes: NaN and +-inf in x, y or z; a point equal to the origin; a == 0 and b == 0 rays leaving
    through each side (and staying inside); rays through all four corners, and the corners themselves"""
    w, h = extent(cm)
    ox, oy, oz = origin
    nan, inf = float("nan"), float("inf")
    mid = (cm.ox + 0.5 * w, cm.oy + 0.5 * h)
    rows = []
    for bad in (nan, inf, -inf):
        rows += [(bad, mid[1], 1.0), (mid[0], bad, 1.0), (mid[0], mid[1], bad), (bad, bad, 1.0), (bad, oy, 1.0), (ox, bad, 1.0)]
    rows.append((ox, oy, oz))
    rows.append((ox, oy, 1.0))
    for far in (0.1, 0.6, 2.0):                                          # a == 0: straight up and down; b == 0: left and right
        rows += [(ox, oy + far * h, 1.0), (ox, oy - far * h, 1.0), (ox + far * w, oy, 1.0), (ox - far * w, oy, 1.0)]
    corners = [(cm.ox, cm.oy), (cm.ox + w, cm.oy), (cm.ox, cm.oy + h), (cm.ox + w, cm.oy + h)]
    for cx, cy in corners:
        rows.append((cx, cy, 1.0))
        for t in (0.5, 0.999, 1.0, 1.001, 3.0):
            rows.append((ox + t * (cx - ox), oy + t * (cy - oy), 1.0))
    return np.asarray(rows, np.float32)


def packed(points, stride, seed=0):
    """[n, 3] -> float32 [n, stride / 4]: x, y, z first, the rest of a record whatever another field left there"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    out = np.random.default_rng(seed).uniform(-9.0, 9.0, (p.shape[0], stride // 4)).astype(np.float32)
    out[:, :3] = p
    return out


def observation(cm, points, origin, raytrace=0.4, stride=16, **more):
    w, _ = extent(cm)
    o = {"points": packed(points, stride), "origin": origin, "obstacle_range": 0.35 * w, "raytrace_range": raytrace * w,
         "min_obstacle_height": WINDOW[0], "max_obstacle_height": WINDOW[1]}
    o.update(more)
    o["points"].setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def world(geom):
    """a geometry's noise grid and its 4097 random records: built once, never changed"""
    rng = np.random.default_rng(GEOMETRIES[geom][0] + 17)
    cm = noise_map(rng, *GEOMETRIES[geom])
    cloud = random_cloud(rng, cm, max(COUNTS))
    cm.grid.setflags(write=False)
    cloud.setflags(write=False)
    return cm, cloud


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (geometry, observations, bounds in): every case of the GPU file, and of the host twin's comparison here"""
    out = {}
    for geom in GEOMETRIES:
        cm, cloud = world(geom)
        s = sensor(cm)
        whole = np.concatenate([cloud, hand_made(cm, s)])
        for raytrace in (0.4, 2.0):
            out[f"{geom} range {raytrace} w"] = (geom, (observation(cm, whole, s, raytrace),), tuple(EMPTY))
        # sensor positions: in cell (0, 0), in cell (sx - 1, sy - 1), on a cell boundary, off the map (nothing cleared, marks still land)
        w, h = extent(cm)
        spots = {"first cell": (f32(cm.ox + 0.3 * cm.res), f32(cm.oy + 0.6 * cm.res), 0.8),
                 "last cell": (f32(cm.ox + w - 0.4 * cm.res), f32(cm.oy + h - 0.7 * cm.res), 0.8),
                 "cell boundary": (cm.ox + 20 * cm.res, cm.oy + 31 * cm.res, 0.8),
                 "off the map": (f32(cm.ox - 0.05 * w), f32(cm.oy + 0.5 * h), 0.8)}
        for name, at in spots.items():
            pts = np.concatenate([cloud[:1500], hand_made(cm, at)])
            out[f"{geom} sensor {name}"] = (geom, (observation(cm, pts, at, 0.4, stride=12),), (at[0], at[1], at[0], at[1]))
        # two clearing and two marking observations with different origins: the marks of one lie on the rays of another
        a, b = sensor(cm, 0.2, 0.3), sensor(cm, 0.7, 0.55)
        out[f"{geom} four observations"] = (geom, (
            observation(cm, cloud[:1200], a, 0.5, stride=32, marking=False),
            observation(cm, cloud[1000:2200], b, 0.45, stride=12, clearing=False, obstacle_range=0.5 * w),
            observation(cm, cloud[2000:3300], b, 2.0, stride=16, marking=False),
            observation(cm, cloud[3000:4097], a, 0.4, stride=16, clearing=False, obstacle_range=0.6 * w)), tuple(EMPTY))
    cm, cloud = world("75x75")
    for k, n in enumerate(COUNTS):                                       # counts around a wave and a workgroup, every stride
        for stride in STRIDES:
            out[f"75x75 n {n} stride {stride}"] = ("75x75", (observation(cm, cloud[:n], sensor(cm), (0.4, 2.0)[k % 2], stride),), None if n == 63 else tuple(EMPTY))
    cm, cloud = world("300x260")
    for n in (65, 4097):
        out[f"300x260 n {n} stride 32"] = ("300x260", (observation(cm, cloud[:n], sensor(cm), 0.4, 32),), tuple(EMPTY))
    return out


@functools.lru_cache(maxsize=None)
def wanted(name):
    """the reference's answer to a case: (grid bytes, bounds or None)"""
    geom, observations, bounds = cases()[name]
    cm = cref.Costmap(*GEOMETRIES[geom], *ORIGIN)
    cm.grid[:] = world(geom)[0].grid
    b = None if bounds is None else list(bounds)
    ref.observe(cm, list(observations), LAYER_MAX, b)
    return cm.grid.tobytes(), b


# ---- the two forms of the statement ---------------------------------------------------------------------------------------------------
def small(name):
    """a case cut down to what the sequential form walks in a second or two: every hand-made record and the first random ones"""
    geom, observations, bounds = cases()[name]
    cut = []
    for o in observations:
        p = o["points"]
        keep = np.r_[0:min(250, len(p)), max(len(p) - 60, 0):len(p)]
        cut.append({**o, "points": p[np.unique(keep)]})
    return geom, cut, bounds


@pytest.mark.parametrize("name", [n for n in cases() if "stride" not in n or " n 65 " in n])
def test_loop_form_equals_vectorised_form(name):
    geom, observations, bounds = small(name)
    a, b = cref.Costmap(*GEOMETRIES[geom], *ORIGIN), cref.Costmap(*GEOMETRIES[geom], *ORIGIN)
    a.grid[:] = world(geom)[0].grid
    b.grid[:] = a.grid
    ba, bb = (None, None) if bounds is None else (list(bounds), list(bounds))
    ref.observe_loop(a, observations, LAYER_MAX, ba)
    ref.observe(b, observations, LAYER_MAX, bb)
    assert a.grid.tobytes() == b.grid.tobytes(), int((a.grid != b.grid).sum())
    assert ba == bb
    if "off the map" in name:
        assert not ((a.grid == 0) & (world(geom)[0].grid != 0)).any() and (a.grid != world(geom)[0].grid).any()   # nothing cleared, marks landed
    else:
        assert ((a.grid == 0) & (world(geom)[0].grid != 0)).sum() > 20


def test_raytrace_line_is_a_prefix_of_the_closed_form():
    rng = np.random.default_rng(2)
    segs = [tuple(int(v) for v in rng.integers(0, 300, 4)) for _ in range(400)]
    segs += [tuple(int(v) for v in rng.integers(0, 12, 4)) for _ in range(19590)]       # short ones: every tie of the rounding
    segs += [(5, 5, 5, 5), (0, 0, 0, 9), (0, 9, 0, 0), (3, 4, 11, 4), (11, 4, 3, 4), (2, 2, 9, 9), (9, 9, 2, 2), (9, 2, 2, 9), (0, 0, 1, 0), (7, 3, 7, 4)]
    assert len(segs) == 20000
    cuts = 0
    for s in segs:
        whole = fref.line_closed(*s)
        da = len(whole) - 1
        assert ref.raytrace_line(*s) == whole                             # no limit: max_length = UINT_MAX
        ranges = range(0, da + 2) if da <= 24 else sorted({0, 1, da // 3, da // 2, da - 1, da, da + 1})
        for cell_range in ranges:
            got = ref.raytrace_line(*s, cell_range)
            end = ref.ray_end(*s, cell_range)
            assert got == whole[:end + 1], (s, cell_range)
            assert end <= min(cell_range, da)                             # never beyond the range in steps of the dominant axis
            cuts += end < da
    assert cuts > 50000


# ---- known answers from the contract's text -------------------------------------------------------------------------------------------
def plain(sx=20, sy=20, res=0.5, fill=100):
    cm = cref.Costmap(sx, sy, res, 0.0, 0.0)
    cm.grid[:] = fill
    return cm


def both(cm, observations, layer_max=2.0, bounds=None):
    """the two forms on copies of cm, which must agree: (grid, bounds)"""
    a, b = plain(cm.size_x, cm.size_y, cm.res), plain(cm.size_x, cm.size_y, cm.res)
    a.grid[:] = cm.grid; b.grid[:] = cm.grid
    ba, bb = (None, None) if bounds is None else (list(bounds), list(bounds))
    ref.observe_loop(a, observations, layer_max, ba)
    ref.observe(b, observations, layer_max, bb)
    assert a.grid.tobytes() == b.grid.tobytes() and ba == bb
    return a.grid, ba


def test_known_answers():
    cm = plain()
    at = (5.25, 5.25, 0.5)                                               # cell (10, 10)
    pts = np.array([[9.25, 5.25, 0.5]], np.float32)                      # cell (18, 10), 4 m = 8 cells away
    # range 0 clears the origin cell only; its bounds are the origin alone (s = 0)
    g, b = both(cm, [{"points": pts, "origin": at, "raytrace_range": 0.0, "marking": False}], bounds=EMPTY)
    assert (g != 100).sum() == 1 and g[10, 10] == 0 and b == [5.25, 5.25, 5.25, 5.25]
    # the default 3 m = 6 cells: cells 10 .. 16 of the row, and the touched point 3 m along the ray
    g, b = both(cm, [{"points": pts, "origin": at, "marking": False}], bounds=EMPTY)
    assert np.flatnonzero(g[10] == 0).tolist() == list(range(10, 17)) and (g != 100).sum() == 7 and b == [5.25, 5.25, 8.25, 5.25]
    # a long range: the whole ray, end cell included
    g, _ = both(cm, [{"points": pts, "origin": at, "raytrace_range": 100.0, "marking": False}])
    assert np.flatnonzero(g[10] == 0).tolist() == list(range(10, 19))
    # a point in the origin's cell has dist == 0: scale 1, that cell alone, whatever the range
    near = np.array([[5.3, 5.4, 0.5]], np.float32)
    for r in (0.0, 3.0):
        g, _ = both(cm, [{"points": near, "origin": at, "raytrace_range": r, "marking": False}])
        assert (g != 100).sum() == 1 and g[10, 10] == 0
    assert ref.ray_end(10, 10, 10, 10, 0) == 0 and ref.raytrace_line(10, 10, 10, 10, 0) == [(10, 10)]
    # sq == range^2 is not marked, the next float below is: 3-4-5 in the plane, the sensor's height
    edge = np.array([[5.25 + 3.0, 5.25 + 4.0, 0.5]], np.float32)
    g, _ = both(cm, [{"points": edge, "origin": at, "obstacle_range": 5.0, "clearing": False}])
    assert (g != 100).sum() == 0
    g, _ = both(cm, [{"points": edge, "origin": at, "obstacle_range": float(np.nextafter(5.0, 6.0)), "clearing": False}])
    assert g[18, 16] == 254 and (g != 100).sum() == 1
    # z on either edge of the window is kept, the next float outside is dropped, for both uses; NaN is dropped
    lo, hi = np.float32(0.25), np.float32(1.75)
    for z, kept in ((lo, True), (hi, True), (np.nextafter(lo, np.float32(-9)), False), (np.nextafter(hi, np.float32(9)), False), (np.float32("nan"), False)):
        p = np.array([[6.25, 5.25, z]], np.float32)
        g, _ = both(cm, [{"points": p, "origin": at, "min_obstacle_height": float(lo), "max_obstacle_height": float(hi)}], layer_max=9.0)
        assert ((g != 100).sum() == 3 and g[10, 12] == 254 and g[10, 10] == g[10, 11] == 0) if kept else (g == 100).all(), (z, kept)
    # the layer's maximum: only marking looks at it
    g, _ = both(cm, [{"points": np.array([[6.25, 5.25, 1.0]], np.float32), "origin": at}], layer_max=0.9)
    assert g[10, 10:13].tolist() == [0, 0, 0] and (g != 100).sum() == 3
    # clears before marks whatever the order of the observations: a cell marked by one and crossed by a ray of the other ends as 254
    m = {"points": np.array([[7.25, 5.25, 0.5]], np.float32), "origin": at, "clearing": False}
    c = {"points": pts, "origin": at, "marking": False}
    for order in ([m, c], [c, m]):
        g, _ = both(cm, order)
        assert g[10, 14] == 254 and g[10, 13] == 0 and g[10, 15] == 0
    # the sensor off the map: nothing cleared, nothing touched by clearing, marks still land
    g, b = both(cm, [{"points": np.array([[0.75, 5.25, 0.5]], np.float32), "origin": (-0.25, 5.25, 0.5)}], bounds=EMPTY)
    assert (g != 100).sum() == 1 and g[10, 1] == 254 and b == [0.75, 5.25, 0.75, 5.25]
    # a ray leaving through the right edge is clipped to map_end_x - .001: the last column, and the bounds from the clipped point
    g, b = both(cm, [{"points": np.array([[25.0, 5.25, 0.5]], np.float32), "origin": at, "raytrace_range": 100.0, "marking": False}], bounds=EMPTY)
    assert np.flatnonzero(g[10] == 0).tolist() == list(range(10, 20)) and b == [5.25, 5.25, 5.25 + ((10.0 - .001) - 5.25) * 1.0, 5.25]
    assert ref.cell_distance(3.0, 0.5) == 6 and ref.cell_distance(3.01, 0.5) == 7 and ref.cell_distance(float("inf"), 0.5) == ref.UINT_MAX


def test_the_random_cloud_holds_every_class():
    """the shares the issue lists, in the reference's answer: no class of records can go untested unnoticed"""
    for geom in GEOMETRIES:
        cm, cloud = world(geom)
        near = ref.classes(cm, observation(cm, cloud, sensor(cm), 0.4), LAYER_MAX)
        print(geom, {k: f"{100 * v:.1f} %" for k, v in near.items()})
        for name in ("no clip, full", "no clip, cut", "one clip, full", "one clip, cut", "two clips, cut", "marked", "too high", "too far",
                     "outside the window"):
            assert near[name] >= 0.02, (geom, name, near[name])
        far = ref.classes(cm, observation(cm, cloud, sensor(cm), 2.0), LAYER_MAX)
        assert far["no clip, cut"] == far["one clip, cut"] == far["two clips, cut"] == 0.0        # with 2 w every ray is full
        assert far["no clip, full"] >= 0.2 and far["one clip, full"] >= 0.3 and far["two clips, full"] >= 0.02
    # the four observations: cells marked by one and crossed by a ray of another
    for geom in GEOMETRIES:
        _, observations, _ = cases()[f"{geom} four observations"]
        base = world(geom)[0]
        cleared = cref.Costmap(*GEOMETRIES[geom], *ORIGIN)
        cleared.grid[:] = 100
        ref.observe(cleared, [o for o in observations if not ref.field(o, "marking")], LAYER_MAX)
        final = np.frombuffer(wanted(f"{geom} four observations")[0], np.uint8).reshape(base.grid.shape)
        assert ((cleared.grid == 0) & (final == 254)).sum() >= 5


# ---- the host twin ------------------------------------------------------------------------------------------------------------------
def build_obstacle_check(out: Path) -> Path:
    """tests/cpp/obstacle_check.cpp with a plain g++ against the installed headers and the library"""
    from gem_amd import build
    build.build()
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "obstacle_check.cpp"),
           "-o", str(out), f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def case_bytes(name):
    geom, observations, bounds = cases()[name]
    sx, sy, res = GEOMETRIES[geom]
    b = EMPTY if bounds is None else bounds
    out = [struct.pack("<IIddddii4d", sx, sy, res, ORIGIN[0], ORIGIN[1], LAYER_MAX, len(observations), int(bounds is not None), *b),
           world(geom)[0].grid.tobytes()]
    for o in observations:
        p = o["points"]
        flags = (ref.MARKING if ref.field(o, "marking") else 0) | (ref.CLEARING if ref.field(o, "clearing") else 0)
        out.append(struct.pack("<qII7d", p.shape[0], p.shape[1] * 4, flags, *o["origin"], ref.field(o, "obstacle_range"),
                               ref.field(o, "raytrace_range"), ref.field(o, "min_obstacle_height"), ref.field(o, "max_obstacle_height")))
        out.append(p.tobytes())
    return b"".join(out)


def test_the_host_twin_equals_the_numpy_statement(tmp_path):
    exe = build_obstacle_check(tmp_path / "obstacle_check")
    res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: built)"), res.stdout + res.stderr
    names = list(cases())
    (tmp_path / "in.bin").write_bytes(struct.pack("<i", len(names)) + b"".join(case_bytes(n) for n in names))
    res = subprocess.run([str(exe), "host", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got, at = (tmp_path / "out.bin").read_bytes(), 0
    for name in names:
        geom, _, bounds = cases()[name]
        cells = GEOMETRIES[geom][0] * GEOMETRIES[geom][1]
        rc, = struct.unpack_from("<i", got, at)
        grid = got[at + 4:at + 4 + cells]
        b = list(struct.unpack_from("<4d", got, at + 4 + cells))
        at += 4 + cells + 32
        want_grid, want_b = wanted(name)
        assert rc == 0 and grid == want_grid, (name, rc)
        assert b == (EMPTY if bounds is None else want_b), name
    assert at == len(got)


def test_the_python_host_twin():
    from gem_amd import obstacle_host
    for name in ("75x75 range 0.4 w", "130x90 four observations", "75x75 n 0 stride 12"):
        geom, observations, bounds = cases()[name]
        grid = world(geom)[0].grid.copy()
        b = obstacle_host(grid, GEOMETRIES[geom][2], ORIGIN, list(observations), LAYER_MAX, None if bounds is None else list(bounds))
        assert (grid.tobytes(), b) == wanted(name)
    with pytest.raises(ValueError):
        obstacle_host(grid, 0.2, ORIGIN, [{"points": np.zeros((1, 3), np.float32), "origin": (0, 0, 0), "raytrace_range": -1.0}])


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def declared(header):
    import re
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(gem_[a-z_0-9]+)\s*\(", text)))


def test_obstacle_symbols_are_declared_exported_and_bound():
    from gem_amd import _lib
    lib = _lib.load()
    names = declared(ROOT / "include" / "gem_hip_obstacle.h")
    assert names == sorted(_lib.OBSTACLE_SIGNATURES) and len(names) == 3
    for n in names:
        assert getattr(lib, n).argtypes == _lib.OBSTACLE_SIGNATURES[n][1]
    assert '#include "gem_hip_obstacle.h"' in (ROOT / "include" / "gem_hip.h").read_text()
    assert lib.gem_abi_version() == 9
    hdr = (ROOT / "include" / "gem_hip_obstacle.h").read_text()
    assert "NOT verified" in hdr and "NAMED DEPARTURES" in hdr and "NOT PROVIDED" in hdr
    assert '"obstacle_direct"' in (ROOT / "include" / "gem_hip_debug.h").read_text()


def test_observation_layout_and_flags_match_the_header(tmp_path):
    from gem_amd import _lib
    fields = ["points", "n", "point_step", "flags", "origin", "obstacle_range", "raytrace_range", "min_obstacle_height", "max_obstacle_height"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gem_hip.h"\nint main(void) { printf("%zu ' + "%zu " * len(fields) + '%d %d %d\\n", '
                   "sizeof(gem_observation), " + ", ".join(f"offsetof(gem_observation, {f})" for f in fields) +
                   ", GEM_OBS_MARKING, GEM_OBS_CLEARING, GEM_OBS_MAX); return 0; }\n")
    exe = tmp_path / "layout"
    res = subprocess.run(["cc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.Observation
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields] + [_lib.OBS_MARKING, _lib.OBS_CLEARING, _lib.OBS_MAX]
    assert C.sizeof(S) == 80 and (ref.MARKING, ref.CLEARING, ref.MAX_OBSERVATIONS) == tuple(got[-3:])


def test_python_facade_has_the_observe_call():
    from gem_amd import Costmap, api
    assert callable(Costmap.observe)
    pts = np.arange(12, dtype=np.float32).reshape(3, 4)
    obs, keep, dev = api._observations([{"points": pts, "origin": (1, 2, 3), "marking": False}])
    assert not dev and obs[0].n == 3 and obs[0].point_step == 16 and obs[0].flags == ref.CLEARING and list(obs[0].origin) == [1.0, 2.0, 3.0]
    assert (obs[0].obstacle_range, obs[0].raytrace_range, obs[0].min_obstacle_height, obs[0].max_obstacle_height) == (2.5, 3.0, 0.0, 2.0)
    with pytest.raises(ValueError):
        api._observations([{"points": np.zeros((3, 2), np.float32), "origin": (0, 0, 0)}])
