"""Footprints on the device costmap (gem_costmap_clear_footprint, gem_costmap_footprint_cost*, gem_costmap_score_trajectories*) against
the restatement of tests/footprint_ref.py.  Every comparison is exact: pose and trajectory costs as integers, grids by tobytes(), bounds
by == on doubles.

  1. pose costs on 75 x 75 @ 0.2, 130 x 90 @ 0.05 and 1000 x 1000 @ 0.2 noise grids, four specs (so every lane-group width of the
     kernel, 8, 16, 32 and 64 lanes), both values of the inscribed flag, n = 1, 63, 64, 65, 4097; the known answers of the CPU file;
  2. trajectories: T = 1, 7, 64, 100, 1 / 65 / 513 of them, max and sum, with and without the per-pose output;
  3. clearing behind a mark that only enqueued, all eight headings, off the map, a sliver, fewer than three vertices, a triangle over
     more than 900 columns (several column chunks), a merge afterwards;
  4. the device-pointer forms with torch tensors, and no allocation in a second identical loop;
  5. the error cases (GEM_ERR_INVALID, grid and outputs unchanged);
  6. the C++ facade (tests/cpp/footprint_check.cpp) as a child process."""
import ctypes as C
import functools
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gem_amd import ElevationMap, _lib

sys.path.insert(0, str(Path(__file__).resolve().parent))
import costmap_ref as cref  # noqa: E402
import footprint_ref as ref  # noqa: E402
from test_costmap_gpu import lattice_cloud  # noqa: E402
from test_footprint_cpu import EMPTY, ORIGIN, SPECS, build_footprint_check, noise_map, random_poses  # noqa: E402
from test_local_map_gpu import HEADINGS  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
GEOMETRIES = {"75x75": (75, 75, 0.2), "130x90": (130, 90, 0.05), "1000x1000": (1000, 1000, 0.2)}
COUNTS = [1, 63, 64, 65, 4097]
THRESH = 0.5
INV = _lib.GEM_OK - 1


@pytest.fixture(scope="module")
def emap():
    m = ElevationMap(32, 0.05)
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def world(geom):
    """the noise grid of a geometry and 4097 poses over its widened box: built once, never changed"""
    rng = np.random.default_rng(GEOMETRIES[geom][0])
    sx, sy, _ = GEOMETRIES[geom]
    cm = noise_map(rng, *GEOMETRIES[geom], few_253=max(6, sx * sy // 1000))
    poses = random_poses(rng, cm, max(COUNTS))
    cm.grid.setflags(write=False)
    poses.setflags(write=False)
    return cm, poses


@functools.lru_cache(maxsize=None)
def wanted(geom, spec, flags):
    cm, poses = world(geom)
    return ref.footprint_cost(cm, poses, SPECS[spec], flags)


def device_copy(m, cm):
    dev = m.costmap(cm.size_x, cm.size_y, cm.res, cm.ox, cm.oy)
    dev.write(cm.grid)
    return dev


# ---- 1. pose costs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", list(SPECS))
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_pose_costs(emap, geom, spec):
    cm, poses = world(geom)
    dev = device_copy(emap, cm)
    try:
        for flags in (0, ref.INSCRIBED_LETHAL):
            want = wanted(geom, spec, flags)
            shares = [float((want == v).mean()) for v in (-3, -2, -1)] + [float((want >= 0).mean())]
            print(f"{geom} {spec} flags {flags}: -3 / -2 / -1 / >= 0 = " + " / ".join(f"{100 * s:.1f} %" for s in shares))
            if spec == "rectangle" and flags == 0:
                assert min(shares) >= 0.02, shares                       # no class can go untested unnoticed
            for n in COUNTS:
                got = dev.footprint_cost(poses[:n], SPECS[spec], flags)
                assert got.dtype == np.int32 and got.tolist() == want[:n].tolist(), (n, int((got != want[:n]).sum()))
        assert (wanted(geom, spec, 0) != wanted(geom, spec, ref.INSCRIBED_LETHAL)).any()          # (the flag decides some pose)
        # yaw poses take the same road: math.cos / math.sin element by element
        xyt = np.stack([poses[:65, 0], poses[:65, 1], np.arctan2(poses[:65, 3], poses[:65, 2])], axis=1)
        assert dev.footprint_cost(xyt, SPECS[spec]).tolist() == ref.footprint_cost(cm, ref.poses_from_yaw(xyt), SPECS[spec]).tolist()
    finally:
        dev.close()


def test_known_answers_on_the_device(emap):
    for name, cm, poses, spec, flags, want in ref.known_answers():
        dev = device_copy(emap, cm)
        try:
            assert dev.footprint_cost(np.asarray(poses, np.float64), spec, flags).tolist() == want, name
        finally:
            dev.close()


# ---- 2. trajectories ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trajectory_world():
    """a grid with few enough negative cells that long trajectories still get through, and a pool of poses inside it with their costs"""
    rng = np.random.default_rng(11)
    cm = cref.Costmap(75, 75, 0.2, *ORIGIN)
    cm.grid[:] = rng.integers(0, 253, (75, 75), dtype=np.uint8)
    u = rng.random((75, 75))
    cm.grid[u < 0.0005] = 254
    cm.grid[(u >= 0.0005) & (u < 0.001)] = 255
    n = 513 * 100
    xyt = np.stack([rng.uniform(cm.ox + 0.8, cm.ox + 14.2, n), rng.uniform(cm.oy + 0.8, cm.oy + 14.2, n), rng.uniform(-np.pi, np.pi, n)], axis=1)
    pool = ref.poses_from_yaw(xyt)
    cost = ref.footprint_cost(cm, pool, ref.RECTANGLE, 0)
    assert 0.005 < (cost < 0).mean() < 0.2
    cm.grid.setflags(write=False)
    return cm, pool, cost


@pytest.mark.parametrize("n_traj", [1, 65, 513])
@pytest.mark.parametrize("T", [1, 7, 64, 100])
def test_trajectories(emap, T, n_traj):
    cm, pool, cost = trajectory_world()
    n = n_traj * T
    poses, c = pool[:n].copy(), cost[:n]
    bad, good = pool[np.flatnonzero(cost < 0)[:2]], pool[np.flatnonzero(cost >= 0)[:2 * T]]
    poses[:T] = good[:T]; poses[T - 1] = bad[0]                            # trajectory 0: only its last pose is negative
    if n_traj > 1:
        poses[T:2 * T] = good[T:2 * T]; poses[T] = bad[1]                   # trajectory 1: its first pose is
    each = ref.footprint_cost(cm, poses, ref.RECTANGLE, 0)
    assert (each[:T - 1] >= 0).all() and each[T - 1] < 0 and (n_traj == 1 or each[T] < 0)
    dev = device_copy(emap, cm)
    try:
        assert dev.footprint_cost(poses, ref.RECTANGLE).tolist() == each.tolist()
        for flags in (0, ref.SUM):
            want = ref.score_trajectories(each, T, flags)
            assert want.tolist() == ref.score_trajectories_loop(each, T, flags).tolist()
            assert want[0] == each[T - 1] and (n_traj == 1 or want[1] == each[T])
            if n_traj >= 65 and T <= 64:
                assert (want < 0).any() and (want >= 0).any()
            got = dev.score_trajectories(poses, T, ref.RECTANGLE, flags)
            assert got.dtype == np.int32 and got.tolist() == want.tolist()
            got, got_each = dev.score_trajectories(poses, T, ref.RECTANGLE, flags, pose_costs=True)
            assert got.tolist() == want.tolist() and got_each.tolist() == each.tolist()
        if T > 1:                                                         # the sum is not the maximum
            assert ref.score_trajectories(each, T, ref.SUM).tolist() != ref.score_trajectories(each, T, 0).tolist() or n_traj == 1
    finally:
        dev.close()


# ---- 3. clearing --------------------------------------------------------------------------------------------------------------------
def clear_both(dev, cm, pose, spec, bounds):
    want_b = list(bounds)
    want_ok = ref.clear_footprint(cm, pose, spec, want_b)
    ok, b = dev.clear_footprint(pose, spec, list(bounds))
    assert ok == want_ok and b == want_b, (ok, want_ok, b, want_b)
    return ok


def same_grid(dev, cm):
    got = dev.read()
    assert got.tobytes() == cm.grid.tobytes(), f"{int((got != cm.grid).sum())} cells differ"


@pytest.mark.parametrize("geom", ["75x75", "130x90"])
def test_clearing_behind_an_enqueued_mark(emap, geom):
    sx, sy, res = GEOMETRIES[geom]
    rng = np.random.default_rng(sx)
    cm = cref.Costmap(sx, sy, res, *ORIGIN)
    dev = emap.costmap(sx, sy, res, *ORIGIN)
    centre = np.array([cm.ox + 0.5 * sx * res, cm.oy + 0.5 * sy * res])
    try:
        cleared = 0
        for k, d in enumerate(HEADINGS):
            pts = lattice_cloud(rng, 20000, cm)
            yaw = math.atan2(d[1], d[0]) + 0.01 * k
            at = centre + 0.3 * k * res * np.array(d, float)
            pose = (float(at[0]), float(at[1]), math.cos(yaw), math.sin(yaw))
            for spec in (ref.RECTANGLE, SPECS["16-gon"] if k % 2 else SPECS["triangle"]):
                cref.mark_points(cm, pts, THRESH)
                before = int((cm.grid != 0).sum())
                dev.mark_points(pts, THRESH, None)                        # only enqueued; nothing waits before the clear
                assert clear_both(dev, cm, pose, spec, EMPTY)
                cleared += before - int((cm.grid != 0).sum())
                same_grid(dev, cm)
            # (x, y, theta) is the same call
            ok, b = dev.clear_footprint((pose[0], pose[1], yaw), ref.RECTANGLE, list(EMPTY))
            assert ok and b[0] < pose[0] < b[2] and ref.clear_footprint(cm, pose, ref.RECTANGLE)
            same_grid(dev, cm)
        assert cleared > 100                                              # the clears removed lethal cells of the marks
    finally:
        dev.close()


def test_clearing_edge_cases(emap):
    cm = cref.Costmap(75, 75, 0.2, *ORIGIN)
    cm.grid[:] = world("75x75")[0].grid
    dev = device_copy(emap, cm)
    mid = (cm.ox + 7.5, cm.oy + 7.5)
    try:
        # partly off the map: nothing written, not ok, the bounds still touched (clear_both compares them)
        for x, y in ((cm.ox + 0.3, mid[1]), (mid[0], cm.oy + 14.9), (cm.ox - 5.0, cm.oy - 5.0)):
            assert not clear_both(dev, cm, (x, y, math.cos(0.4), math.sin(0.4)), ref.RECTANGLE, [0.0, 1e30, -1e30, 0.0])
            same_grid(dev, cm)
        # fewer than three vertices: ok, nothing written
        for n in (0, 1, 2):
            assert clear_both(dev, cm, (mid[0], mid[1], 1.0, 0.0), ref.RECTANGLE[:n], EMPTY)
            same_grid(dev, cm)
        # slivers: thinner than a cell, along a row, along a column, along the diagonal; every vertex in one cell
        sliver = [[-2.0, 0.0], [2.0, 0.01], [2.0, -0.01]]
        for yaw in (0.0, math.pi / 2, math.pi / 4, 2.0):
            before = cm.grid.copy()
            assert clear_both(dev, cm, (mid[0] + 0.03, mid[1] + 0.07, math.cos(yaw), math.sin(yaw)), sliver, EMPTY)
            assert 10 <= int((before != cm.grid).sum()) <= 80
            same_grid(dev, cm)
        assert clear_both(dev, cm, (cm.ox + 1.0, cm.oy + 1.0, 1.0, 0.0), [[0.001, 0.001], [0.002, 0.001], [0.001, 0.002]], EMPTY)
        same_grid(dev, cm)
        # the heading-0 rectangle in the corner: the box of its vertex cells, the map's first column and row included
        assert clear_both(dev, cm, (cm.ox + 0.65, cm.oy + 0.41, 1.0, 0.0), ref.RECTANGLE, EMPTY)
        assert (cm.grid[0:5, 0:7] == 0).all()
        same_grid(dev, cm)
    finally:
        dev.close()


def test_clearing_a_wide_triangle_then_merging(emap):
    cm = cref.Costmap(1000, 1000, 0.2, *ORIGIN)
    cm.grid[:] = world("1000x1000")[0].grid
    master = cref.Costmap(1000, 1000, 0.2, *ORIGIN, cref.FREE_SPACE)
    master.grid[:] = np.random.default_rng(3).choice(np.array([0, 100, 254, 255], np.uint8), (1000, 1000))
    dev, dmaster = device_copy(emap, cm), device_copy(emap, master)
    try:
        wide = [[-95.0, -20.0], [95.5, -31.0], [3.0, 60.0]]               # more than 900 columns: several column chunks of the kernel
        pose = (cm.ox + 100.0, cm.oy + 100.0, math.cos(0.05), math.sin(0.05))
        cells = [cref.world_to_map(cm, *w) for w in ref.transform(pose, wide)]
        assert max(c[0] for c in cells) - min(c[0] for c in cells) > 900
        before = int((cm.grid != 0).sum())
        b = [pose[0], pose[1], pose[0], pose[1]]
        assert clear_both(dev, cm, pose, wide, b)
        assert before - int((cm.grid != 0).sum()) > 150000
        same_grid(dev, cm)
        # ObstacleLayer::updateCosts: the footprint first, then the combination rule
        window = (20, 30, 990, 700)
        cref.merge(cm, master, window, cref.MAX)
        dev.merge(dmaster, window, cref.MAX)
        same_grid(dmaster, master)
        same_grid(dev, cm)
    finally:
        dev.close(); dmaster.close()


# ---- 4. device pointers ---------------------------------------------------------------------------------------------------------------
def test_device_pointer_forms_and_a_second_loop_allocates_nothing(emap):
    import torch
    cm, poses = world("130x90")
    big, big_poses = world("1000x1000")
    dev, dbig = device_copy(emap, cm), device_copy(emap, big)
    T = 17
    n = (poses.shape[0] // T) * T
    d_poses = torch.from_numpy(poses[:n].copy()).to("cuda:0")
    d_big = torch.from_numpy(big_poses[:n].copy()).to("cuda:0")

    def loop():
        out = []
        for spec in ("rectangle", "16-gon"):
            for flags in (0, ref.INSCRIBED_LETHAL, ref.SUM):
                a = dev.footprint_cost(d_poses, SPECS[spec], flags)       # only enqueued: nothing is read before the synchronize below
                t, each = dev.score_trajectories(d_poses, T, SPECS[spec], flags, pose_costs=True)
                t2 = dbig.score_trajectories(d_big, T, SPECS[spec], flags)
                emap.synchronize()
                h_t, h_each = dev.score_trajectories(poses[:n], T, SPECS[spec], flags, pose_costs=True)
                assert a.dtype == torch.int32 and a.cpu().numpy().tolist() == h_each.tolist() == each.cpu().numpy().tolist()
                assert t.cpu().numpy().tolist() == h_t.tolist()
                assert t2.cpu().numpy().tolist() == dbig.score_trajectories(big_poses[:n], T, SPECS[spec], flags).tolist()
                assert h_each.tolist() == wanted("130x90", spec, flags & ref.INSCRIBED_LETHAL)[:n].tolist()
                out.append(h_t.tolist())
        return out

    try:
        first = loop()
        a1 = emap.debug_get("arena_allocations")
        second = loop()
        assert emap.debug_get("arena_allocations") == a1 and first == second
        with pytest.raises(ValueError):
            dev.footprint_cost(d_poses.float(), SPECS["rectangle"])
    finally:
        dev.close(); dbig.close()


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------------
def test_error_cases_leave_grid_and_outputs_unchanged():
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    cm, poses = world("75x75")
    dev = device_copy(m, cm)
    n, T = 64, 8
    p = np.ascontiguousarray(poses[:n])
    pp = p.ctypes.data_as(C.c_void_p)
    spec = np.ascontiguousarray(ref.RECTANGLE, np.float64)
    sp = spec.ctypes.data_as(C.POINTER(C.c_double))
    out, traj = np.full(n, 77, np.int32), np.full(n // T, 77, np.int32)
    po, pt = out.ctypes.data_as(C.c_void_p), traj.ctypes.data_as(C.c_void_p)
    b, ok = (C.c_double * 4)(*EMPTY), C.c_int(55)
    one = _lib.FootprintPose(cm.ox + 7.5, cm.oy + 7.5, 1.0, 0.0)
    nan, inf = float("nan"), float("inf")

    def cost(id_=None, poses_=pp, n_=n, spec_=sp, nv=4, flags=0, out_=po, entry="gem_costmap_footprint_cost"):
        return getattr(lib, entry)(h, dev.id if id_ is None else id_, poses_, n_, spec_, nv, flags, out_)

    def score(id_=None, poses_=pp, nt=n // T, T_=T, spec_=sp, nv=4, flags=0, each_=po, traj_=pt, entry="gem_costmap_score_trajectories"):
        return getattr(lib, entry)(h, dev.id if id_ is None else id_, poses_, nt, T_, spec_, nv, flags, each_, traj_)

    def clear(id_=None, pose_=one, spec_=sp, nv=4):
        return lib.gem_costmap_clear_footprint(h, dev.id if id_ is None else id_, C.byref(pose_) if pose_ is not None else None, spec_, nv, b, C.byref(ok))

    def unchanged():
        got = dev.read()
        assert got.tobytes() == cm.grid.tobytes()
        assert (out == 77).all() and (traj == 77).all() and list(b) == EMPTY and ok.value == 55

    bad_specs = []
    for v in (nan, inf, -inf):
        s = spec.copy(); s[2, 1] = v
        bad_specs.append(s)
    try:
        assert cost() == 0 and out.tolist() == ref.footprint_cost(cm, p, ref.RECTANGLE).tolist()       # (the arguments are good ones)
        assert score() == 0 and clear(pose_=_lib.FootprintPose(cm.ox - 9.0, cm.oy, 1.0, 0.0)) == 0 and ok.value == 0
        out[:] = 77; traj[:] = 77; ok.value = 55
        for i in range(4):
            b[i] = EMPTY[i]
        for e in ("", "_device"):
            fc, st = "gem_costmap_footprint_cost" + e, "gem_costmap_score_trajectories" + e
            for bad in (-1, 5, 8, 1 << 20):                               # a bad id
                assert cost(id_=bad, entry=fc) == INV and score(id_=bad, entry=st) == INV
            assert cost(n_=-1, entry=fc) == INV and score(nt=-1, entry=st) == INV
            assert cost(n_=(1 << 31) - 1, entry=fc) == INV                # above 2^31 - 2
            assert score(nt=(1 << 31) // T, entry=st) == INV and score(nt=1 << 40, entry=st) == INV
            for bad_T in (0, -1, (1 << 20) + 1):
                assert score(T_=bad_T, entry=st) == INV
            for nv in (-1, 33):
                assert cost(nv=nv, entry=fc) == INV and score(nv=nv, entry=st) == INV
            for s in bad_specs:
                q = s.ctypes.data_as(C.POINTER(C.c_double))
                assert cost(spec_=q, entry=fc) == INV and score(spec_=q, entry=st) == INV
            for flags in (4, 8, 1 << 30, -1):
                assert cost(flags=flags, entry=fc) == INV and score(flags=flags, entry=st) == INV
            assert cost(poses_=None, entry=fc) == INV and cost(out_=None, entry=fc) == INV and cost(spec_=None, entry=fc) == INV
            assert score(poses_=None, entry=st) == INV and score(traj_=None, entry=st) == INV and score(spec_=None, entry=st) == INV
        unchanged()
        for bad in (-1, 5, 8):
            assert clear(id_=bad) == INV
        assert clear(nv=-1) == INV and clear(nv=33) == INV and clear(spec_=None) == INV and clear(pose_=None) == INV
        for s in bad_specs:
            assert clear(spec_=s.ctypes.data_as(C.POINTER(C.c_double))) == INV
        for bad_pose in ((nan, 0.0, 1.0, 0.0), (0.0, inf, 1.0, 0.0), (0.0, 0.0, nan, 0.0), (0.0, 0.0, 1.0, -inf)):
            assert clear(pose_=_lib.FootprintPose(*bad_pose)) == INV
        unchanged()
        # zero counts are fine with NULL arrays, and a non-finite pose simply answers -3
        assert cost(poses_=None, n_=0, out_=None) == 0 and score(poses_=None, nt=0, each_=None, traj_=None) == 0
        q = p.copy(); q[0, 0] = nan; q[1, 1] = inf; q[2, 2] = nan; q[3, 3] = -inf
        assert dev.footprint_cost(q[:4], ref.RECTANGLE).tolist() == [-3, -3, -3, -3]
        # a handle with a communicator
        w = ElevationMap(32, 0.05)
        w.comm_init_loopback(9534, 1, 0, tile_strips=False)
        assert w._lib.gem_costmap_footprint_cost(w._h, 0, pp, n, sp, 4, 0, po) == INV
        assert w._lib.gem_costmap_clear_footprint(w._h, 0, C.byref(one), sp, 4, b, C.byref(ok)) == INV
        unchanged()
        w.close()
    finally:
        dev.close()
        m.close()


# ---- 6. the C++ facade ----------------------------------------------------------------------------------------------------------------
def test_cpp_footprint_facade(tmp_path):
    exe = build_footprint_check(tmp_path / "footprint_check")
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
