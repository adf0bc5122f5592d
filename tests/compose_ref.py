"""numpy restatement of gem_local_compose (include/gem_hip.h): pcl::StatisticalOutlierRemoval<Anypoint> with setMeanK(mean_k) and
setStddevMulThresh(stddev_mul), as pointCloudtoOctomap applies it to the grid cloud of prevMap_ (EMg.cpp:1146-1170), and the split of
the survivors by travers.  PCL is not available here: the statement is written down from PCL >= 1.10
filters/impl/statistical_outlier_removal.hpp and FLANN's L2_Simple<float>, in our own words.

  d2         for point i and every point j, i included: ((dx*dx) + (dy*dy)) + (dz*dz), every operation rounded in float32 (numpy
             float32 arrays round each operation and never fuse a product into a sum).
  distance   the mean_k + 1 smallest d2 of point i, ascending; entry 0 is the query (or a coincident point), 0 either way.
             dist_sum (double) = 0; for k = 1 .. mean_k in that order dist_sum += s(d2[k]); distance[i] = float32(dist_sum / mean_k).
             s() is (double)sqrtf(d2) by default and sqrt((double)d2) with sqrt_double.  Equal d2 values give the same sum whichever
             point supplied them: no tie rule is needed.
  threshold  double sum = sq_sum = 0; for i in order: sum += distance[i]; sq_sum += float32(distance[i] * distance[i]) (a FLOAT
             product, widened when added).  mean = sum / n; variance = (sq_sum - sum * sum / n) / (n - 1);
             threshold = mean + stddev_mul * sqrt(variance), in double.
  filter     i survives iff (double)distance[i] <= threshold; survivors keep their order.
  split      a survivor with (double)travers > travers_threshold -> road; else one with travers <= travers_threshold (not NaN) ->
             obstacle.
  n <= mean_k   (undefined in the reference: it reads past its search result) nothing is removed, distances and threshold are +inf.

Two exact paths to the distances: distances_brute() is the definition, O(n^2); distances() takes candidate sets from a cKDTree in
double, recomputes d2 in float32 from the candidates, PROVES per row that the set was sufficient and falls back to brute force for
the rows where it cannot.  tests/test_compose_cpu.py pins the two to identical bits."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
# relative error bound of the float32 d2 against the exact one: three roundings per squared term (difference, product) and two sums,
# < 8 * 2^-24; the proof below uses 1e-6 (and an absolute 1e-30 for results in the subnormal range)
D2_REL, D2_ABS = 1e-6, 1e-30


def _mean_from_sorted(d2_sorted, mean_k, sqrt_double):
    """d2_sorted: [m, mean_k + 1] float32 ascending -> float32 [m]"""
    acc = np.zeros(d2_sorted.shape[0], F64)
    with np.errstate(invalid="ignore"):
        for k in range(1, mean_k + 1):
            col = d2_sorted[:, k]
            acc = acc + (np.sqrt(col.astype(F64)) if sqrt_double else np.sqrt(col).astype(F64))
        return (acc / F64(mean_k)).astype(F32)


def _d2(q, p):
    """q: [m, 1, 3] or [m, 3] broadcastable against p, float32 -> float32 d2"""
    dx, dy, dz = q[..., 0] - p[..., 0], q[..., 1] - p[..., 1], q[..., 2] - p[..., 2]
    return ((dx * dx) + (dy * dy)) + (dz * dz)


def _smallest(d2, mean_k):
    """the mean_k + 1 smallest of each row, ascending"""
    part = np.partition(d2, mean_k, axis=1)[:, :mean_k + 1]
    return np.sort(part, axis=1)


def distances_brute(xyz, mean_k, sqrt_double=False, rows=None, chunk=256):
    """The definition.  xyz: [n, 3] float32, n > mean_k; rows: the points to answer (default all)."""
    xyz = np.ascontiguousarray(xyz, F32)
    rows = np.arange(xyz.shape[0]) if rows is None else np.asarray(rows)
    out = np.empty(rows.shape[0], F32)
    for a in range(0, rows.shape[0], chunk):
        r = rows[a:a + chunk]
        out[a:a + chunk] = _mean_from_sorted(_smallest(_d2(xyz[r][:, None, :], xyz[None, :, :]), mean_k), mean_k, sqrt_double)
    return out


def distances(xyz, mean_k, sqrt_double=False, candidates=64, workers=8, stats=None):
    """The same values at node scale.  Candidates: the min(candidates, n) nearest points by a cKDTree on the float coordinates widened
    to double.  A point outside the candidate set is at least as far as the farthest candidate (distance `far`, exact up to double
    rounding), so its float32 d2 is >= far^2 * (1 - D2_REL) - D2_ABS; if that exceeds the largest kept float32 d2 of the row, nothing
    outside the set can enter the row's mean_k + 1 smallest, and the row is proven.  Other rows are answered by brute force."""
    from scipy.spatial import cKDTree
    xyz = np.ascontiguousarray(xyz, F32)
    n = xyz.shape[0]
    k = min(max(candidates, mean_k + 1), n)
    far, idx = cKDTree(xyz.astype(F64)).query(xyz.astype(F64), k=k, workers=workers)
    far, idx = far.reshape(n, k), idx.reshape(n, k)
    out = np.empty(n, F32)
    proven = np.zeros(n, bool)
    for a in range(0, n, 1 << 15):
        sl = slice(a, min(n, a + (1 << 15)))
        kept = _smallest(_d2(xyz[sl][:, None, :], xyz[idx[sl]]), mean_k)
        out[sl] = _mean_from_sorted(kept, mean_k, sqrt_double)
        proven[sl] = (k == n) | (far[sl, -1] ** 2 * (1.0 - D2_REL) - D2_ABS > kept[:, -1].astype(F64))
    rest = np.flatnonzero(~proven)
    if rest.size:
        out[rest] = distances_brute(xyz, mean_k, sqrt_double, rows=rest)
    if stats is not None:
        stats["brute_rows"] = int(rest.size)
    return out


def ordered_sums(dist, float_product=True):
    """sum and sq_sum in index order.  np.add.accumulate on float64 is the sequential recurrence (tests pin it to a Python loop)."""
    d = np.asarray(dist, F32)
    if d.size == 0:
        return 0.0, 0.0
    sq = (d * d).astype(F64) if float_product else d.astype(F64) * d.astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.add.accumulate(d.astype(F64))[-1]), float(np.add.accumulate(sq)[-1])


def threshold(dist, stddev_mul, float_product=True):
    n = len(dist)
    s, q = ordered_sums(dist, float_product)
    mean = s / n
    variance = (q - s * s / n) / (n - 1)
    root = math.sqrt(variance) if variance >= 0.0 else math.nan           # sqrt of a negative double is NaN (inf and NaN pass through)
    return mean + stddev_mul * root


def compose(rec, mean_k=20, stddev_mul=1.0, travers_threshold=0.0, sqrt_double=False, brute=False, workers=8):
    """rec: the capture's records (local_ref.POINT) in order -> (road, obstacle, removed, threshold, distances)"""
    n = rec.shape[0]
    if n <= mean_k:
        dist, thr = np.full(n, np.inf, F32), math.inf
    else:
        xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(F32)
        dist = distances_brute(xyz, mean_k, sqrt_double) if brute else distances(xyz, mean_k, sqrt_double, workers=workers)
        thr = threshold(dist, stddev_mul)
    keep = dist.astype(F64) <= thr
    t = rec["travers"].astype(F64)
    road = keep & (t > travers_threshold)
    obstacle = keep & ~road & (t <= travers_threshold)
    return rec[road], rec[obstacle], int(n - keep.sum()), thr, dist
