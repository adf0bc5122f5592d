"""The VoxelGrid pre-filter on the device, against the numpy restatement of its contract (tests/voxel_ref.py) and the oracle:

  1. gem_voxel_device: centroids, rgb, m and the NaN tail bit for bit -- a C2 sweep, random clouds with duplicates, non-finite
     values in every coordinate, one voxel of 100k points, every point its own voxel, n = 0 / 1, tails around the workgroup size,
     2^22 points, every field kind, overflow and empty stages, both launch presets, chains;
  2. gem_add_voxel / gem_add_voxel_device over a sequence of frames with moves and variance updates: the oracle's map of the
     filtered cloud, on every pipeline;
  3. voxel_device -> colorize_device -> add_device against the oracle's colorize and fuse of the filtered cloud;
  4. gem_reserve, then a stream of voxel frames of varying n: no arena allocation, maps exact;
  5. the C++ gem::VoxelGrid (tests/cpp/voxel_facade_check.cpp) as a child process."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gem_amd import ElevationMap, GemError, VoxelStage, _lib, synth

sys.path.insert(0, str(Path(__file__).resolve().parent))
import voxel_ref as vr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
F32 = np.float32
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def corrupt(rng, xyzi, fraction):
    out = xyzi.copy()
    hit = np.flatnonzero(rng.random(out.shape[0]) < fraction)
    col = rng.integers(0, 4, hit.size)
    val = np.array([NAN, INF, -INF], F32)[rng.integers(0, 3, hit.size)]
    for c in range(3):
        out[hit[(col == c) | (col == 3)], c] = val[(col == c) | (col == 3)]
    return out


def check(m, xyzi, stages, rgb=None, name=""):
    import torch
    d = torch.from_numpy(xyzi).cuda()
    dr = torch.from_numpy(rgb.view(np.int32)).cuda() if rgb is not None else None
    out, rgb_out, count = m.voxel_device(stages, d, dr)
    ex, er, em = vr.voxel(xyzi, rgb, stages)
    k = int(count.item())
    assert k == em, (name, k, em)
    got = out.cpu().numpy()
    assert np.array_equal(bits(got), bits(ex)), f"{name}: {(bits(got) != bits(ex)).any(axis=1).sum()} points differ"
    if rgb is not None:
        assert np.array_equal(rgb_out.cpu().numpy().view(np.uint32), er), name
    return k


def cases():
    rng = np.random.default_rng(17)
    out = []
    wl = synth.config_c2()
    sweep = wl.clouds[0]
    out.append(("c2_sweep", sweep, VoxelStage.filter_launch()))
    out.append(("c2_kitti", sweep, VoxelStage.filter_kitti_launch()))
    out.append(("c2_plain", sweep, [VoxelStage(0.05)]))
    rc = synth.random_cloud(5, 60_000, 20.0)
    out.append(("random_dups", rc, [VoxelStage(0.1)]))
    out.append(("random_corrupt", corrupt(rng, rc, 0.2), [VoxelStage(0.1, "z", -0.5, 0.5)]))
    one = np.concatenate([rng.uniform(0.0, 0.099, (100_000, 3)), rng.uniform(0, 255, (100_000, 1))], 1).astype(F32)
    out.append(("one_voxel_100k", one, [VoxelStage(0.1)]))
    grid = np.stack(np.meshgrid(np.arange(40), np.arange(40), np.arange(20), indexing="ij"), -1).reshape(-1, 3)
    own = np.concatenate([grid * 0.1 + 0.05, rng.uniform(0, 9, (grid.shape[0], 1))], 1).astype(F32)
    out.append(("own_voxels", own[rng.permutation(own.shape[0])], [VoxelStage(0.1)]))
    for n in (0, 1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 8193):
        c = corrupt(rng, rng.normal(0, 3, (n, 4)).astype(F32), 0.2)
        out.append((f"n{n}", c, [VoxelStage(0.25)]))
    fld = rng.normal(0, 8, (30_000, 4)).astype(F32)
    fld[rng.random(30_000) < 0.1, 3] = NAN
    for f in ("x", "y", "z", "intensity"):
        out.append((f"field_{f}", fld, [VoxelStage(0.2, f, -3.0, 0.1)]))
        out.append((f"field_{f}_neg", fld, [VoxelStage(0.2, f, -3.0, 0.1, True)]))
    out.append(("overflow", corrupt(rng, rng.normal(0, 500, (20_000, 4)).astype(F32), 0.1), [VoxelStage(1e-4)]))
    out.append(("empty", fld, [VoxelStage(0.2, "x", 1e6, 2e6)]))
    out.append(("all_nan", np.full((3000, 4), NAN, F32), [VoxelStage(0.2)]))
    out.append(("chain_overflow_then_grid", fld, [VoxelStage(1e-4), VoxelStage(0.5, "y", -5, 5), VoxelStage(1e-4), VoxelStage(1.0)]))
    out.append(("chain_empty_then", fld, [VoxelStage(0.2, "x", 1e6, 2e6), VoxelStage(0.5)]))
    return out


@pytest.mark.one_pipeline
def test_voxel_device_matches_numpy():
    m = ElevationMap(64, 0.1)
    rng = np.random.default_rng(3)
    for name, xyzi, stages in cases():
        for with_rgb in (False, True):
            rgb = rng.integers(0, 1 << 24, xyzi.shape[0]).astype(np.uint32) if with_rgb else None
            check(m, xyzi, stages, rgb, name)
    big = corrupt(rng, rng.normal(0, 6, (1 << 22, 4)).astype(F32), 0.05)       # (extent within the int32 voxel count)
    k = check(m, big, [VoxelStage(0.1)], None, "2^22")
    assert 0 < k < big.shape[0]
    m.close()


@pytest.mark.one_pipeline
def test_voxel_device_rejects_bad_parameters():
    import torch
    m = ElevationMap(64, 0.1)
    d = torch.zeros((10, 4), dtype=torch.float32, device="cuda")
    for bad in ([VoxelStage(0.0)], [VoxelStage(-1.0)], [VoxelStage(float("inf"))], [VoxelStage(float("nan"))]):
        with pytest.raises(GemError):
            m.voxel_device(bad, d)
    p = VoxelStage(0.1).to_struct()
    p.field = 5
    with pytest.raises(GemError):
        m.voxel_device([p], d)
    arr = (_lib.VoxelParams * 5)(*([VoxelStage(0.1).to_struct()] * 5))
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.empty_like(d)
    for ns in (0, 5):                                          # GEM_ERR_INVALID
        assert m._lib.gem_voxel_device(m._h, arr, ns, 10, d.data_ptr(), None, out.data_ptr(), None, count.data_ptr()) == -1
    m.close()


def frames(n_steps=4):
    wl = synth.config_c2()
    T = wl.frames[0].T.astype(np.float64)
    rng = np.random.default_rng(23)
    out = []
    for step in range(n_steps):
        Ts = T.copy()
        Ts[0, 3] += 0.07 * step
        Ts[1, 3] -= 0.04 * step
        cloud = synth.lidar_sweep(rng, Ts) if step else wl.clouds[0]
        out.append((synth._frame_for(Ts, wl.frames[0].model), cloud))
    return wl.length, wl.resolution, out


@pytest.mark.parametrize("preset", ["filter", "kitti"])
def test_add_voxel_map_parity(oracle_mod, preset):
    import torch
    stages = VoxelStage.filter_launch() if preset == "filter" else VoxelStage.filter_kitti_launch()
    L, res, seq = frames()
    rng = np.random.default_rng(5)
    host, host_rgb, dev, dev_rgb = (ElevationMap(L, res) for _ in range(4))
    ref, ref_rgb = oracle_mod.OracleMap(L, res), oracle_mod.OracleMap(L, res)
    everyone = (host, host_rgb, dev, dev_rgb, ref, ref_rgb)
    for step, (f, cloud) in enumerate(seq):
        n = cloud.shape[0]
        rgb = (rng.integers(0, 3, (n, 3)) * 100).astype(np.uint32)
        packed = (rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]
        for m in everyone:
            m.move(np.array([0.05 * step, -0.03 * step, 0.0], F32))
            if step:
                m.mapvar_update(1e-5)
        fx, fc, k = vr.voxel(cloud, packed, stages)
        assert 0 < k < n
        host.add_voxel(f, stages, cloud)
        host_rgb.add_voxel(f, stages, cloud, rgb=packed)
        dev.add_voxel(f, stages, torch.from_numpy(cloud).cuda())
        dev_rgb.add_voxel(f, stages, torch.from_numpy(cloud).cuda(), rgb=torch.from_numpy(packed.view(np.int32)).cuda())
        ref.add(f, fx[:k])
        ref_rgb.add(f, fx[:k], rgb=fc[:k])
        for name in ("elevation", "variance", "intensity", "color_r", "color_g", "color_b"):
            for who, m, twin in (("host", host, ref), ("device", dev, ref), ("host rgb", host_rgb, ref_rgb), ("device rgb", dev_rgb, ref_rgb)):
                want, got = twin.layer(name), m.layer(name)
                bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
                assert bad.size == 0, f"{who} step {step} {name}: {bad.size} cells differ from the oracle's map of the filtered cloud"
    assert (ref.layer("elevation") != -10).sum() > 1000
    for m in (host, host_rgb, dev, dev_rgb):
        m.close()


def test_voxel_colorize_add_device(oracle_mod):
    """the node's order with the nodelets dropped: voxel -> gem_colorize_device -> gem_add_device on the padded cloud"""
    import torch
    L, res, seq = frames(3)
    stages = VoxelStage.filter_launch()
    rng = np.random.default_rng(31)
    img = rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)
    P = np.array([[160.0, 0.0, 160.0, 0.0], [0.0, 160.0, 120.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
    P = P @ np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0], [0, 0, 0, 1]], np.float64)       # camera looking along +x
    gpu, ref = ElevationMap(L, res), oracle_mod.OracleMap(L, res)
    d_img = torch.from_numpy(img).cuda()
    for step, (f, cloud) in enumerate(seq):
        for m in (gpu, ref):
            m.move(np.array([0.05 * step, 0.0, 0.0], F32))
        out, _, count = gpu.voxel_device(stages, torch.from_numpy(cloud).cuda(), sync=False)
        rgb, out = gpu.colorize(P, d_img, out)
        gpu.add(f, out, rgb=rgb)                                   # (device tensors: gem_add_device)
        fx, _, k = vr.voxel(cloud, None, stages)
        o = oracle_mod.colorize(P, img, fx[:k])
        assert 0 < o["count"] < k
        ref.add(f, o["xyzi"], rgb=o["rgb"])
        gpu.synchronize()
        assert int(count.item()) == k
        got_rgb = rgb.cpu().numpy().view(np.uint32)
        assert np.array_equal(got_rgb[:k], o["rgb"]) and (got_rgb[k:] == 0).all()
        assert np.array_equal(bits(out.cpu().numpy()[:k]), bits(o["xyzi"]))
        for name in ("elevation", "variance", "intensity", "color_r", "color_g", "color_b"):
            assert np.array_equal(bits(gpu.layer(name)), bits(ref.layer(name))), f"step {step} {name}"
    gpu.close()


def test_reserve_then_voxel_stream_allocates_nothing(oracle_mod):
    import torch
    L, res, seq = frames(2)
    stages = VoxelStage.filter_kitti_launch()
    rng = np.random.default_rng(8)
    gpu, ref = ElevationMap(L, res), oracle_mod.OracleMap(L, res)
    gpu.reserve(200_000)
    before = gpu.debug_get("arena_allocations")
    grew = []
    f, base = seq[0]
    for i, n in enumerate((131_072, 90_000, 150_000, 4097, 1, 0, 120_000)):
        cloud = base[rng.permutation(base.shape[0])[:n]] if n <= base.shape[0] else np.concatenate([base, base[:n - base.shape[0]]])
        if i % 2:
            gpu.add_voxel(f, stages, torch.from_numpy(np.ascontiguousarray(cloud)).cuda())
        else:
            gpu.add_voxel(f, stages, cloud)
        fx, _, k = vr.voxel(cloud, None, stages)
        ref.add(f, fx[:k])
        out, _, count = gpu.voxel_device(stages, torch.from_numpy(np.ascontiguousarray(cloud)).cuda()) if n else (None, None, None)
        if n:
            assert int(count.item()) == k
        grew.append(gpu.debug_get("arena_allocations") - before)
    assert grew[-1] == 0, f"allocations after each frame: {grew}"
    for name in ("elevation", "variance", "intensity"):
        assert np.array_equal(bits(gpu.layer(name)), bits(ref.layer(name))), name
    gpu.close()


@pytest.mark.one_pipeline
def test_cpp_voxel_facade(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc"
    exe = tmp_path / "voxel_facade_check"
    lib = ROOT / "gem_amd" / "lib"
    subprocess.run([hipcc, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "voxel_facade_check.cpp"),
                    "-o", str(exe), "-L", str(lib), "-lgem_hip", f"-Wl,-rpath,{lib}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
