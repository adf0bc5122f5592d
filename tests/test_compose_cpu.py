"""tests/compose_ref.py -- the restatement of gem_local_compose's contract (include/gem_hip.h) -- against hand-derived answers, and
its node-scale path (cKDTree candidates + a per-row proof) against the O(n^2) definition, bit for bit.  No GPU."""
import math
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import compose_ref  # noqa: E402
from local_ref import POINT  # noqa: E402

F32, F64 = np.float32, np.float64
SQRT2F = 1.41421353816986083984375          # sqrtf(2.0f) = 0x3FB504F3, as a double


def cloud(xyz, travers=0.5):
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    r = np.zeros(xyz.shape[0], POINT)
    r["x"], r["y"], r["z"], r["pad"], r["travers"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 1.0, travers
    return r


def patch(n=5, z=0.0):
    return [(float(i), float(j), z) for j in range(n) for i in range(n)]


def test_flat_patch_by_hand():
    """5 x 5 points at unit spacing, mean_k = 4.  An interior point has four neighbours at 1; an edge point three at 1 and then a
    diagonal at sqrtf(2); a corner two at 1, one diagonal, and then a point at 2.  Sums in ascending order, in double."""
    rec = cloud(patch())
    *_, dist = compose_ref.compose(rec, mean_k=4, stddev_mul=100.0, brute=True)
    exp = np.empty((5, 5), F32)
    exp[:, :] = F32(((1.0 + 1.0) + 1.0 + 1.0) / 4.0)
    exp[0, :] = exp[-1, :] = exp[:, 0] = exp[:, -1] = F32((((1.0 + 1.0) + 1.0) + SQRT2F) / 4.0)
    exp[0, 0] = exp[0, -1] = exp[-1, 0] = exp[-1, -1] = F32((((1.0 + 1.0) + SQRT2F) + 2.0) / 4.0)
    assert dist.tobytes() == exp.reshape(-1).tobytes()
    road, obstacle, removed, thr, _ = compose_ref.compose(rec, mean_k=4, stddev_mul=100.0, brute=True)
    assert removed == 0 and road.shape[0] == 25 and obstacle.shape[0] == 0 and road.tobytes() == rec.tobytes()
    # the threshold from the hand-derived distances, as a Python loop
    s = q = 0.0
    for d in exp.reshape(-1):
        s += float(d)
        q += float(F32(d * d))
    assert thr == s / 25 + 100.0 * math.sqrt((q - s * s / 25) / 24)


def test_single_spike_is_removed():
    pts = patch()
    pts[12] = (2.0, 2.0, 10.0)
    rec = cloud(pts)
    road, obstacle, removed, thr, dist = compose_ref.compose(rec, mean_k=4, stddev_mul=1.0, brute=True)
    # the spike's four nearest are its lattice neighbours, each sqrtf(1 + 100) away
    assert dist[12] == F32(4.0 * float(np.sqrt(F32(101.0))) / 4.0)
    assert removed == 1 and road.shape[0] == 24 and not (road["z"] == 10.0).any()
    assert road.tobytes() == np.delete(rec, 12).tobytes()


def test_point_exactly_on_the_threshold_is_kept():
    """Four far-apart pairs at unit distance, mean_k = 1: every distance is exactly 1, sum = 8, sq_sum = 8, variance = 0, so the
    threshold is exactly 1 for any multiplier and `<=` keeps all eight points (`<` would remove all of them)."""
    pts = []
    for k in range(4):
        pts += [(100.0 * k, 0.0, 0.0), (100.0 * k + 1.0, 0.0, 0.0)]
    rec = cloud(pts)
    road, _, removed, thr, dist = compose_ref.compose(rec, mean_k=1, stddev_mul=2.5, brute=True)
    assert (dist == F32(1.0)).all() and thr == 1.0
    assert removed == 0 and road.shape[0] == 8


def test_float_product_in_sq_sum_differs_from_a_double_product():
    d = np.array([0.1, 0.2, 0.3, 0.7], F32)
    s = qf = qd = 0.0
    for v in d:
        s += float(v)
        qf += float(F32(v * v))
        qd += float(v) * float(v)
    exp_f = s / 4 + 1.0 * math.sqrt((qf - s * s / 4) / 3)
    exp_d = s / 4 + 1.0 * math.sqrt((qd - s * s / 4) / 3)
    assert exp_f != exp_d
    assert compose_ref.threshold(d, 1.0) == exp_f == 0.5879955549101679
    assert compose_ref.threshold(d, 1.0, float_product=False) == exp_d == 0.5879955581444736


def test_the_two_sqrt_forms_give_different_distances():
    """The query at the origin with neighbours at d2 = 2, 6, 10 (exact in float), mean_k = 3: the sum of three float-rounded roots and
    the sum of three double roots round to different floats."""
    rec = cloud([(0, 0, 0), (1, 1, 0), (2, 1, 1), (3, 1, 0)])
    *_, df = compose_ref.compose(rec, mean_k=3, brute=True)
    *_, dd = compose_ref.compose(rec, mean_k=3, sqrt_double=True, brute=True)
    sf = (float(np.sqrt(F32(2))) + float(np.sqrt(F32(6)))) + float(np.sqrt(F32(10)))
    sd = (math.sqrt(2.0) + math.sqrt(6.0)) + math.sqrt(10.0)
    assert df[0] == F32(sf / 3) and dd[0] == F32(sd / 3) and df[0] != dd[0]
    assert df[0].view(np.uint32) == dd[0].view(np.uint32) + 1


def test_small_clouds_remove_nothing():
    for n in (0, 1, 4):
        rec = cloud(patch()[:n], travers=1.0)
        road, obstacle, removed, thr, dist = compose_ref.compose(rec, mean_k=4)
        assert removed == 0 and road.shape[0] == n and obstacle.shape[0] == 0 and thr == math.inf and np.isinf(dist).all()
    rec = cloud(patch()[:5])                       # n = mean_k + 1: defined
    assert math.isfinite(compose_ref.compose(rec, mean_k=4, brute=True)[3])


def test_travers_equal_to_the_threshold_is_an_obstacle():
    rec = cloud(patch())
    rec["travers"][:] = 0.75
    rec["travers"][3] = 0.25
    rec["travers"][7] = np.nextafter(F32(0.25), F32(1))
    road, obstacle, removed, *_ = compose_ref.compose(rec, mean_k=4, stddev_mul=100.0, travers_threshold=0.25, brute=True)
    assert removed == 0 and obstacle.shape[0] == 1 and obstacle[0].tobytes() == rec[3].tobytes() and road.shape[0] == 24
    rec["travers"][5] = np.nan                     # (a capture holds none) neither list
    road, obstacle, removed, *_ = compose_ref.compose(rec, mean_k=4, stddev_mul=100.0, travers_threshold=0.25, brute=True)
    assert removed == 0 and obstacle.shape[0] == 1 and road.shape[0] == 23


def test_accumulate_is_the_sequential_sum():
    rng = np.random.default_rng(3)
    d = rng.uniform(0.01, 3.0, 5000).astype(F32)
    s = q = 0.0
    for v in d:
        s += float(v)
        q += float(F32(v * v))
    assert compose_ref.ordered_sums(d) == (s, q)


def lattice_cloud(L, res, centre, seed, occupied=1.0, step=0.0, rough=0.05):
    """a capture-like cloud: float positions of an L x L lattice around `centre`, random heights, optionally sparse or with a step"""
    rng = np.random.default_rng(seed)
    u = np.arange(L)
    x = ((centre[0] + 0.5 * L * res - 0.5 * res) + res * (-u).astype(F64)).astype(F32)
    y = ((centre[1] + 0.5 * L * res - 0.5 * res) + res * (-u).astype(F64)).astype(F32)
    X, Y = np.meshgrid(x, y, indexing="ij")
    Z = rng.normal(0.0, rough, (L, L)).astype(F32)
    Z[L // 2:, :] += F32(step)
    keep = rng.random((L, L)) < occupied
    return np.stack([X[keep], Y[keep], Z[keep]], axis=1).astype(F32)


def test_candidate_path_equals_brute_force():
    """The cKDTree path is identical to the definition: dense, sparse (rows that need the fallback), a 2 m step, positions so far out
    that neighbouring cells share a float coordinate; both sqrt forms; several mean_k."""
    cases = [dict(L=128, res=0.05, centre=(0.0, 0.0), seed=1),
             dict(L=96, res=0.05, centre=(3.0, -2.0), seed=2, occupied=0.05),
             dict(L=96, res=0.05, centre=(0.3, 0.1), seed=3, step=2.0),
             dict(L=64, res=0.05, centre=(2.0e4, -2.0e4), seed=4),
             dict(L=64, res=0.05, centre=(1.0e6, -1.0e6), seed=5)]
    for c in cases:
        xyz = lattice_cloud(**c)
        for mean_k, sd in ((20, False), (1, True), (32, False)):
            st = {}
            fast = compose_ref.distances(xyz, mean_k, sd, workers=4, stats=st)
            brute = compose_ref.distances_brute(xyz, mean_k, sd)
            assert fast.tobytes() == brute.tobytes(), (c, mean_k, sd, st)
    # ... and with so few candidates that most rows fail their proof and take the fallback
    xyz = lattice_cloud(L=48, res=0.05, centre=(0.0, 0.0), seed=6)
    st = {}
    fast = compose_ref.distances(xyz, 20, candidates=21, workers=2, stats=st)
    assert st["brute_rows"] > 0 and fast.tobytes() == compose_ref.distances_brute(xyz, 20).tobytes()


def build_compose_facade_check(out: Path) -> Path:
    libdir = ROOT / "gem_amd" / "lib"
    cmd = ["/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else "hipcc", "-std=c++17", "-O1", "-Wall", "-Werror",
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "compose_facade_check.cpp"), "-o", str(out),
           f"-L{libdir}", "-lgem_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def test_compose_facade_builds():
    """gem::LocalMap::compose compiles with hipcc against the installed header and the library; without a GPU the check exits early."""
    import tempfile
    from gem_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as td:
        exe = build_compose_facade_check(Path(td) / "compose_facade_check")
        res = subprocess.run([str(exe), "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK (no GPU: built)"), res.stdout + res.stderr
