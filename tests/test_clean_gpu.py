"""cleanPointCloud (SensorProcessorBase.cpp:89) on the device, against the numpy reference (tests/clean_ref.py) and the oracle:

  1. gem_clean_device: kept XYZI, rgb, orig and count bit for bit, for organised clouds with holes, every non-finite value in every
     coordinate, the PassThrough limits and their neighbours, tails around the workgroup size, n = 0 and 2^24 points;
  2. gem_process_points_raw: the kept points' outputs = Process_points on the cleaned cloud with the kept indices (all four models);
  3. gem_add_raw / gem_add_raw_device / gem_add_aos_raw over a sequence of frames with moves in between: the map of fusing the
     cleaned cloud with its indices, on every pipeline;
  4. REMOVE_NAN fuses with no pass of its own (gem_hip.h): a cloud full of non-finite values, filter on and off, window at +-inf;
  5. gem_add_raw / gem_add_voxel from host arrays with rgb through both staging branches (the pinned buffer and the arena), = the
     device calls and the oracle; the Python twin's checks of device rgb / orig_index;
  6. the C++ processors' processRaw (tests/cpp/clean_facade_check.cpp) as a child process."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gem_amd import ElevationMap, RejectFilter, SensorModel, _lib, synth

sys.path.insert(0, str(Path(__file__).resolve().parent))
import clean_ref  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
NAN, INF = np.float32(np.nan), np.float32(np.inf)
STEREO = lambda: SensorModel(2, (0.1, 0.001, 380.0, 1.0, 0.002, 0.001, 30.0), original_width=640)
PT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1"),
               ("covariance", "<f4"), ("intensity", "<f4"), ("travers", "<f4")])          # PointXYZRGBICT


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def params(mode, z_min=-np.inf, z_max=np.inf):
    p = _lib.CleanParams()
    p.mode, p.z_min, p.z_max = int(mode), float(z_min), float(z_max)
    return p


def corrupt(rng, xyzi, fraction):
    """non-finite values in random points: NaN / +inf / -inf in one coordinate, or in all three"""
    out = xyzi.copy()
    hit = np.flatnonzero(rng.random(out.shape[0]) < fraction)
    col = rng.integers(0, 4, hit.size)
    val = np.array([NAN, INF, -INF], F32)[rng.integers(0, 3, hit.size)]
    for c in range(3):
        out[hit[(col == c) | (col == 3)], c] = val[(col == c) | (col == 3)]
    return out


# ---- 1. the compaction itself ------------------------------------------------------------------------------------------------
def clean_cases():
    rng = np.random.default_rng(41)
    cases = []
    W, H = 640, 480                                             # organised depth image: NaN pixels and whole NaN rows
    img = np.concatenate([rng.normal(0, 2, (H * W, 2)), rng.uniform(0.05, 6.0, (H * W, 1)), rng.uniform(0, 255, (H * W, 1))], 1).astype(F32)
    img[rng.random(H * W) < 0.2, :3] = NAN
    img.reshape(H, W, 4)[100:108, :, :3] = NAN
    img.reshape(H, W, 4)[:, 600:, 2] = NAN
    cases.append(("organised", img, clean_ref.REMOVE_NAN, -np.inf, np.inf))
    _, zlo, zhi = clean_ref.params_for_model(1, 0.2, 3.25)
    cases.append(("organised_d435", img, clean_ref.PASSTHROUGH_Z, zlo, zhi))
    special = []
    for c in range(3):                                          # +-inf and NaN in each coordinate alone, between finite points
        for v in (NAN, INF, -INF):
            p = np.array([1.0, -2.0, 0.5, 7.0], F32); p[c] = v
            special += [p, np.array([0.1 * len(special), 0.2, 0.3, 1.0], F32)]
    special = np.array(special, F32)
    cases.append(("special", special, clean_ref.REMOVE_NAN, -np.inf, np.inf))
    edge = []
    for lo, hi in ((zlo, zhi), clean_ref.params_for_model(1)[1:]):
        for z in (lo, hi, np.nextafter(lo, -INF), np.nextafter(lo, INF), np.nextafter(hi, -INF), np.nextafter(hi, INF), F32(-0.0), F32(0.0),
                  F32(-1e-45), F32(np.finfo(F32).max), F32(1.0)):
            edge.append([0.5, 0.5, z, 3.0])
        edge.append([NAN, 0.5, 1.0, 3.0])                       # finite z, NaN x
        edge.append([0.5, INF, 1.0, 3.0])
    edge = np.array(edge, F32)
    cases.append(("edges_d435", edge, clean_ref.PASSTHROUGH_Z, zlo, zhi))
    cases.append(("edges_defaults", edge, clean_ref.PASSTHROUGH_Z) + tuple(clean_ref.params_for_model(1)[1:]))
    finite = rng.normal(0, 3, (70_000, 4)).astype(F32)
    cases.append(("no_nan_identity", finite, clean_ref.REMOVE_NAN, -np.inf, np.inf))
    cases.append(("none_keeps_all", img, clean_ref.NONE, -np.inf, np.inf))
    cases.append(("all_nan", np.full((5000, 4), NAN, F32), clean_ref.REMOVE_NAN, -np.inf, np.inf))
    for n in (0, 1, 63, 64, 65, 255, 257, 1023, 1024, 1025, 2049):
        c = corrupt(rng, rng.normal(0, 3, (n, 4)).astype(F32), 0.3)
        cases.append((f"n{n}", c, clean_ref.REMOVE_NAN, -np.inf, np.inf))
    return cases


@pytest.mark.one_pipeline
def test_clean_device_matches_numpy():
    import torch
    m = ElevationMap(64, 0.1)
    rng = np.random.default_rng(3)
    cases = clean_cases()
    big = corrupt(rng, rng.normal(0, 5, (1 << 24, 4)).astype(F32), 0.25)
    cases.append(("2^24", big, clean_ref.REMOVE_NAN, -np.inf, np.inf))
    for name, xyzi, mode, lo, hi in cases:
        for with_rgb in (False, True):
            n = xyzi.shape[0]
            rgb = rng.integers(0, 1 << 24, n).astype(np.uint32) if with_rgb else None
            d = torch.from_numpy(xyzi).cuda()
            dr = torch.from_numpy(rgb.view(np.int32)).cuda() if with_rgb else None
            p = params(mode, lo, hi)
            out, rgb_out, orig, count = m.clean_device(p, d, dr)
            ex, er, eo = clean_ref.clean(xyzi, rgb, mode, p.z_min, p.z_max)
            k = int(count.item())
            assert k == eo.size, (name, k, eo.size)
            assert np.array_equal(orig[:k].cpu().numpy(), eo), name
            assert np.array_equal(bits(out[:k].cpu().numpy()), bits(ex)), name
            if with_rgb:
                assert np.array_equal(rgb_out[:k].cpu().numpy().view(np.uint32), er), name
            if name == "2^24":
                break
    assert clean_ref.clean(big)[2].size < big.shape[0]
    m.close()


# ---- raw workloads ------------------------------------------------------------------------------------------------------------
def raw_workload(model: str, seed: int = 7):
    """(raw XYZI cloud, its frame's sensor -> map transform, sensor model, map length, resolution, map position).
    laser: a C2 velodyne sweep with a quarter of its points made non-finite; the camera models: the C3 depth image ORGANISED --
    640 x 480, NaN where no ray hit, a few non-finite values more -- with depths to 12 m, beyond the d435's 3.25 m cutoff."""
    rng = np.random.default_rng(seed)
    if model == "laser":
        wl = synth.config_c2()
        return corrupt(rng, wl.clouds[0], 0.25), wl.frames[0].T.astype(np.float64), wl.frames[0].model, wl.length, wl.resolution, np.zeros(3, F32)
    wl = synth.config_c3(structured_light=(model == "structured_light"))
    raw = np.full((640 * 480, 4), NAN, F32)
    raw[:, 3] = rng.uniform(1, 255, raw.shape[0])
    raw[wl.orig_index] = wl.clouds[0]
    raw = corrupt(rng, raw, 0.02)
    sm = {"structured_light": wl.frames[0].model, "stereo": STEREO(), "perfect": SensorModel.perfect()}[model]
    return raw, wl.frames[0].T.astype(np.float64), sm, wl.length, wl.resolution, wl.map_position


def frame_at(T, sm, step):
    Ts = T.copy()
    Ts[0, 3] += 0.05 * step
    Ts[1, 3] -= 0.03 * step
    return synth._frame_for(Ts, sm)


# ---- 2. Process_points on a raw cloud ---------------------------------------------------------------------------------------------
@pytest.mark.one_pipeline
@pytest.mark.parametrize("model", ["laser", "structured_light", "stereo", "perfect"])
def test_process_points_raw(oracle_mod, model):
    raw, T, sm, L, res, pos = raw_workload(model)
    f = frame_at(T, sm, 0)
    cp = sm.clean_params()
    kx, _, kept = clean_ref.clean(raw, None, cp.mode, cp.z_min, cp.z_max)
    assert 0 < kept.size < raw.shape[0]
    if model == "structured_light":
        assert kept.size < clean_ref.clean(raw)[2].size            # the cutoffs drop finite points too
    gpu, ref = ElevationMap(L, res), oracle_mod.OracleMap(L, res)
    for m in (gpu, ref):
        m.move(pos)
    g = gpu.process_points_raw(f, raw[:, 0], raw[:, 1], raw[:, 2])
    assert g["n_kept"] == kept.size and np.array_equal(g["orig"], kept)
    e = gpu.process_points(f, kx[:, 0], kx[:, 1], kx[:, 2], orig_index=kept)           # the cleaned cloud, on the device
    o = ref.process_points(f, kx[:, 0], kx[:, 1], kx[:, 2], orig_index=kept)
    for k in ("index", "var", "x_ts", "y_ts", "height"):
        assert np.array_equal(g[k].view(np.uint32), e[k].view(np.uint32)), k
    assert np.array_equal(g["index"], o["index"])
    for k in ("x_ts", "y_ts", "height"):
        assert np.array_equal(g[k], o[k]), k
    acc = o["index"] >= 0
    assert acc.sum() > 1000
    if model == "laser":
        assert np.array_equal(g["var"], o["var"])
    else:                                                          # double pow() / sqrt() may differ in the last ulp (test_parity_gpu)
        v, w = g["var"][acc].astype(np.float64), o["var"][acc].astype(np.float64)
        assert np.max(np.abs(v - w) / np.maximum(np.abs(w), 1e-30)) <= 1e-5
    gpu.close()


# ---- 3. the fused path on raw clouds ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["laser", "structured_light", "stereo", "perfect"])
def test_add_raw_map_parity(oracle_mod, model):
    import torch
    raw, T, sm, L, res, pos = raw_workload(model, seed=11)
    rng = np.random.default_rng(5)
    n = raw.shape[0]
    rgb = (rng.integers(0, 3, (n, 3)) * 100).astype(np.uint32)
    packed = (rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]
    pts = np.zeros(n, PT)
    pts["x"], pts["y"], pts["z"], pts["intensity"] = raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 3]
    pts["r"], pts["g"], pts["b"], pts["a"], pts["pad"] = rgb[:, 0], rgb[:, 1], rgb[:, 2], 255, 1.0
    cp = sm.clean_params()
    kx, kc, kept = clean_ref.clean(raw, packed, cp.mode, cp.z_min, cp.z_max)
    host, dev, dev_rgb, aos, cln, cln0 = (ElevationMap(L, res) for _ in range(6))
    ref = oracle_mod.OracleMap(L, res)
    d_raw, d_rgb = torch.from_numpy(raw).cuda(), torch.from_numpy(packed.view(np.int32)).cuda()
    everyone = (host, dev, dev_rgb, aos, cln, cln0, ref)
    for step in range(3):
        for m in everyone:
            m.move(np.asarray(pos, F32) + np.array([0.1 * step, -0.05 * step, 0.0], F32))
            if step:
                m.mapvar_update(1e-5)
        f = frame_at(T, sm, step)
        host.add_raw(f, raw, rgb=packed)
        dev.add_raw(f, d_raw)                                       # colourless: the one-launch-per-frame path where it applies
        dev_rgb.add_raw(f, d_raw, rgb=d_rgb)
        aos.add_aos_raw(f, pts)
        cln.add(f, kx, rgb=kc, orig_index=kept)
        cln0.add(f, kx, orig_index=kept)                           # the colourless twin of cln, for `dev`
        ref.add(f, kx, rgb=kc, orig_index=kept)
        for name in ("elevation", "variance", "intensity", "color_r", "color_g", "color_b"):
            for who, m, twin in (("add_raw", host, cln), ("add_aos_raw", aos, cln), ("add_raw_device rgb", dev_rgb, cln), ("add_raw_device", dev, cln0)):
                want, got = twin.layer(name), m.layer(name)
                bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
                assert bad.size == 0, f"{who} step {step} {name}: {bad.size} cells differ from the cleaned cloud's map"
        e, eo = cln.layer("elevation"), ref.layer("elevation")
        assert np.array_equal(e == -10, eo == -10)
        if model == "laser":
            for name in ("elevation", "variance", "intensity", "color_r", "color_g", "color_b"):
                assert np.array_equal(cln.layer(name), ref.layer(name)), name
        else:                                                       # double pow() / sqrt() in the camera models: north_star's 1e-5
            for name in ("elevation", "variance"):
                g, o = cln.layer(name).astype(np.float64), ref.layer(name).astype(np.float64)
                assert np.max(np.abs(g - o) / np.maximum(np.abs(o), 1e-30)) <= 1e-5, name
    assert host.stats()["points_in"] == n                           # raw points
    assert (ref.layer("elevation") != -10).sum() > 1000
    for m in (host, dev, dev_rgb, aos, cln, cln0):
        m.close()


def test_reserve_then_no_allocation_for_raw_clouds(oracle_mod):
    """gem_reserve covers the raw-cloud entries as it covers gem_add*: after reserve(n) a stream of structured-light frames (d435
    cutoffs: the masked copy) and of compactions of up to n raw points -- smaller ones first -- allocates nothing, and the map is the
    map of the cleaned clouds."""
    import torch
    raw, T, sm, L, res, pos = raw_workload("structured_light", seed=13)
    n = raw.shape[0]
    cp = sm.clean_params()
    gpu, cln = ElevationMap(L, res), ElevationMap(L, res)
    gpu.reserve(n)
    before = gpu.debug_get("arena_allocations")
    assert before > 0
    d_raw = torch.from_numpy(raw).cuda()
    for m in (gpu, cln):
        m.move(pos)
    for step, m_pts in enumerate((20_000, n, n, 60_000)):
        f = frame_at(T, sm, step)
        part = raw[:m_pts]
        kx, _, kept = clean_ref.clean(part, None, cp.mode, cp.z_min, cp.z_max)
        if step % 2:
            gpu.add_raw(f, d_raw[:m_pts])
        else:
            gpu.add_raw(f, part)
        cln.add(f, kx, orig_index=kept)
        g = gpu.process_points_raw(f, part[:, 0], part[:, 1], part[:, 2])
        assert g["n_kept"] == kept.size and np.array_equal(g["orig"], kept)
        _, _, orig, count = gpu.clean_device(cp, d_raw[:m_pts])
        assert int(count.item()) == kept.size and np.array_equal(orig[:kept.size].cpu().numpy(), kept)
    for name in ("elevation", "variance"):
        assert np.array_equal(gpu.layer(name).view(np.uint32), cln.layer(name).view(np.uint32)), name
    assert gpu.debug_get("arena_allocations") == before, "a raw-cloud call inside the reserved bounds allocated"
    gpu.close(); cln.close()


# ---- 4. REMOVE_NAN needs no pass ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filter_on", [False, True])
def test_remove_nan_fuse_needs_no_pass(oracle_mod, filter_on):
    """Projection rejects every point with a non-finite coordinate (h is NaN or +-inf), even with the height window at +-inf and
    with the reject filter on or off: gem_add_raw with REMOVE_NAN is gem_add on the raw cloud, and that must be the cleaned map."""
    import torch
    rng = np.random.default_rng(17 + filter_on)
    c = synth.random_cloud(19, 80_000, 5.5)
    raw = corrupt(rng, c, 0.4)
    raw[::97, :3] = np.array([INF, -INF, 0.5], F32)               # h = T[8] inf + T[9] (-inf) + ...: NaN or +-inf in any pose
    f = synth._frame_for(synth.pose_matrix(0.2, -0.1, 0.4, 0.3, 0.05, -0.02), SensorModel.velodyne(), RejectFilter.reference() if filter_on else None)
    f.lower, f.upper = -np.inf, np.inf
    kx, _, kept = clean_ref.clean(raw)
    assert kept.size < 0.7 * raw.shape[0]
    host, dev = ElevationMap(110, 0.1), ElevationMap(110, 0.1)
    ref = oracle_mod.OracleMap(110, 0.1)
    d = torch.from_numpy(raw).cuda()
    for _ in range(2):
        host.add_raw(f, raw); dev.add_raw(f, d); ref.add(f, kx)
        for name in ("elevation", "variance", "intensity"):
            o = ref.layer(name)
            assert np.array_equal(host.layer(name), o), name
            assert np.array_equal(dev.layer(name), o), name
    assert (ref.layer("elevation") != -10).sum() > 1000
    host.close(); dev.close()


# ---- 5. the host entries' two staging branches ----------------------------------------------------------------------------------
@pytest.mark.parametrize("copy_threads", [0, 4])
def test_host_raw_and_voxel_through_staging_and_arena(oracle_mod, copy_threads):
    """gem_add_raw (d435 cut-offs, PASSTHROUGH_Z) and gem_add_voxel (filter_launch) from host arrays with rgb, on clouds of at least
    128 KB (with copy threads: read in place from a half of the pinned staging buffer) and of less (copied into the arena), and one
    n = 0 call behind a variance update: every layer bit for bit the map of the same calls from device tensors and the oracle's."""
    import torch
    from gem_amd import VoxelStage
    import voxel_ref as vr
    raw, T, _, L, res, pos = raw_workload("structured_light", seed=19)
    d435, laser = SensorModel.realsense_d435(), SensorModel.velodyne()
    cp = d435.clean_params()
    wl = synth.config_c2()
    sweep, stages = wl.clouds[0], VoxelStage.filter_launch()
    rng = np.random.default_rng(29)
    raw_host, raw_dev = ElevationMap(L, res), ElevationMap(L, res)
    vox_host, vox_dev = ElevationMap(wl.length, wl.resolution), ElevationMap(wl.length, wl.resolution)
    raw_ref, vox_ref = oracle_mod.OracleMap(L, res), oracle_mod.OracleMap(wl.length, wl.resolution)
    gpus = (raw_host, raw_dev, vox_host, vox_dev)
    for m in gpus:
        m.debug_set("copy_threads", copy_threads)
    for m in (raw_host, raw_dev, raw_ref):
        m.move(pos)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def colours(n):
        rgb = (rng.integers(0, 3, (n, 3)) * 100).astype(np.uint32)
        return (rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]

    # XYZI + rgb: 20 bytes a point, 60 000 and the 131 072 of the sweep above 128 KB, 3 000 below
    for step, (n_raw, n_vox) in enumerate(((60_000, sweep.shape[0]), (3_000, 3_000), (0, 0), (60_000, sweep.shape[0]), (3_000, 3_000))):
        if step:
            for m in gpus + (raw_ref, vox_ref):
                m.mapvar_update(1e-5)
        part, c_raw = raw[rng.permutation(raw.shape[0])[:n_raw]], colours(n_raw)
        cloud, c_vox = sweep[rng.permutation(sweep.shape[0])[:n_vox]], colours(n_vox)
        f_raw, f_vox = frame_at(T, laser, step), frame_at(wl.frames[0].T.astype(np.float64), wl.frames[0].model, step)
        raw_host.add_raw(f_raw, part, rgb=c_raw, clean=d435)
        raw_dev.add_raw(f_raw, dev(part), rgb=dev(c_raw.view(np.int32)), clean=d435)
        kx, kc, kept = clean_ref.clean(part, c_raw, cp.mode, cp.z_min, cp.z_max)
        raw_ref.add(f_raw, kx, rgb=kc, orig_index=kept)
        vox_host.add_voxel(f_vox, stages, cloud, rgb=c_vox)
        vox_dev.add_voxel(f_vox, stages, dev(cloud), rgb=dev(c_vox.view(np.int32)))
        fx, fc, k = vr.voxel(cloud, c_vox, stages)
        vox_ref.add(f_vox, fx[:k], rgb=fc[:k])
        for who, m, ref in (("add_raw host", raw_host, raw_ref), ("add_raw device", raw_dev, raw_ref),
                            ("add_voxel host", vox_host, vox_ref), ("add_voxel device", vox_dev, vox_ref)):
            for name in ("elevation", "variance", "intensity", "color_r", "color_g", "color_b"):
                bad = np.flatnonzero(bits(m.layer(name)) != bits(ref.layer(name)))
                assert bad.size == 0, f"{who} step {step} {name}: {bad.size} cells differ from the oracle"
    assert (raw_ref.layer("elevation") != -10).sum() > 1000 and (vox_ref.layer("elevation") != -10).sum() > 1000
    for m in gpus:
        m.close()


@pytest.mark.one_pipeline
def test_device_colours_and_indices_must_cover_the_cloud():
    """add / add_raw / add_voxel of a device cloud: an rgb or orig_index tensor shorter than the cloud or not on its device is a
    ValueError before anything is enqueued (the kernels would read past its end); longer ones are read up to n"""
    import torch
    from gem_amd import VoxelStage
    m = ElevationMap(64, 0.1)
    f = synth._frame_for(np.eye(4), SensorModel.velodyne())
    d = torch.from_numpy(synth.random_cloud(3, 100, 2.0)).cuda()
    short, on_host = torch.zeros(99, dtype=torch.int32, device=d.device), torch.zeros(100, dtype=torch.int32)
    for bad in (short, on_host):
        for call in (lambda: m.add(f, d, rgb=bad), lambda: m.add(f, d, orig_index=bad), lambda: m.add_raw(f, d, rgb=bad),
                     lambda: m.add_voxel(f, [VoxelStage(0.1)], d, rgb=bad)):
            with pytest.raises(ValueError):
                call()
    assert m.stats()["points_in"] == 0
    longer = torch.zeros(101, dtype=torch.int32, device=d.device)
    m.add(f, d, rgb=longer, orig_index=longer)
    m.synchronize()
    assert m.stats()["points_in"] == 100
    m.close()


# ---- 6. the C++ processors ------------------------------------------------------------------------------------------------------
@pytest.mark.one_pipeline            # (a C++ child process: the fixture's knobs never reach it)
def test_cpp_process_raw_on_gpu(tmp_path):
    from test_clean_cpu import build_clean_facade_check
    exe = build_clean_facade_check(tmp_path)
    res = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
