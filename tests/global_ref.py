"""numpy + dict restatement of the submap stack (globalMap_: the new-keyframe branch of ElevationMapping::updateLocalMap,
EMg.cpp:630-687, and updateGlobalMap, :773-905), the semantics include/gem_hip.h pins for gem_global_*.

The stack is a Python list of POINT arrays.  A hashed submap is a dict from the key -- a pair of Python floats, or ("nan", position)
for a record whose key has a NaN, so that it never equals anything -- to (record, position of the key's first record); dicts keep
insertion order, which is the device's export order: the first occurrence of each key.

The dict forms are the definition.  hash_fast / pair_step_fast (loop_closure(..., fast=True)) are the same on arrays -- the first
record of a key by a stable np.unique on the key's bits, NaN keys kept apart -- fast enough for submaps of a million records;
tests/test_vectorised_refs_cpu.py pins the two forms to identical bytes."""
import numpy as np

import local_ref

POINT = local_ref.POINT
F32 = np.float32


def push_local(stack: list, local: dict, cap: local_ref.Capture) -> int:
    """globalMap_.push_back(*out_pc + *grid_pc): the local map's export, then the capture's grid cloud."""
    stack.append(np.concatenate([local_ref.export(local), local_ref.grid_cloud(cap)]))
    return len(stack) - 1


def push(stack: list, points) -> int:
    stack.append(np.asarray(points, POINT).copy())
    return len(stack) - 1


def transform(rec: np.ndarray, m) -> np.ndarray:
    """x' = x*m00 + (y*m01 + (z*m02 + m03)) and rows 1, 2, 3 into y, z, pad, every step rounded in float; m is M[row][col]."""
    m = np.asarray(m, F32).reshape(4, 4)
    out = rec.copy()
    x, y, z = rec["x"], rec["y"], rec["z"]
    with np.errstate(invalid="ignore", over="ignore"):
        for row, f in enumerate(("x", "y", "z", "pad")):
            out[f] = x * m[row, 0] + (y * m[row, 1] + (z * m[row, 2] + m[row, 3]))
    return out


def neighbours(centres, n: int, i: int, radius: float) -> list:
    """the j in [0, n) with d2 = dx*dx + dy*dy (float, neighbour minus i) < (float)(radius * radius), ascending (d2, j)"""
    c = np.asarray(centres, F32).reshape(-1, 2)
    r2 = F32(float(radius) * float(radius))
    hits = []
    for j in range(n):
        dx, dy = F32(c[j, 0] - c[i, 0]), F32(c[j, 1] - c[i, 1])
        d2 = F32(F32(dx * dx) + F32(dy * dy))
        if d2 < r2:
            hits.append((float(d2), j))
    return [j for _, j in sorted(hits)]


def quantise(v, res: float) -> np.ndarray:
    """pointCloudtoHash's coordinate (EMg.cpp:1184-1185): (float)(ceil((double) v / res) * res - res / 2.0)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.ceil(np.asarray(v, np.float64) / res) * res - res / 2.0).astype(F32)


def hash_cloud(rec: np.ndarray, res: float) -> dict:
    """pointCloudtoHash: the first record of a key keeps it (unordered_map::insert)"""
    kx, ky = quantise(rec["x"], res), quantise(rec["y"], res)
    out = {}
    for p in range(rec.shape[0]):
        r = rec[p].copy()
        r["x"], r["y"] = kx[p], ky[p]
        key = ("nan", p) if np.isnan(kx[p]) or np.isnan(ky[p]) else (float(kx[p]), float(ky[p]))
        if key not in out:
            out[key] = r
    return out


def fuse(new: np.void, old: np.void) -> np.void:
    """EMg.cpp:862-863 as C++ precedence parses them, in double; colour, intensity and travers from new"""
    nv, ne = float(new["covariance"]), float(new["z"])
    ov, oe = float(old["covariance"]), float(old["z"])
    nv2, ov2 = nv * nv, ov * ov
    r = new.copy()
    r["z"] = F32(((nv2 * oe) + ((ov2 * ne) / ov2)) + nv2)
    r["covariance"] = F32(((ov2 * nv2) / ov2) + nv2)
    return r


def export(h: dict) -> np.ndarray:
    """localHashtoPointCloud: x, y the key, pad 1, a 0, the stored intensity; first-occurrence order"""
    out = np.array(list(h.values()), POINT) if h else np.zeros(0, POINT)
    out["pad"], out["a"] = 1.0, 0
    return out


def pair_step(stack: list, i: int, k: int, res: float) -> int:
    old, new = hash_cloud(stack[i], res), hash_cloud(stack[k], res)
    fused = 0
    for key, nr in new.items():
        if key[0] == "nan" or key not in old:
            continue
        orr = old[key]
        if F32(0) < orr["covariance"] < F32(1):
            f = fuse(nr, orr)
            new[key] = f
            old[key] = f
            fused += 1
    stack[k] = export(new)
    stack[i] = export(old)
    return fused


def hash_fast(rec: np.ndarray, res: float):
    """export(hash_cloud(rec, res)) on arrays, with the entries' keys (local_key's bits) and which of them are NaN keys"""
    kx, ky = quantise(rec["x"], res), quantise(rec["y"], res)
    nan = np.isnan(kx) | np.isnan(ky)
    bits = local_ref.key_bits(kx, ky)
    real = np.flatnonzero(~nan)
    _, first = np.unique(bits[real], return_index=True)                   # stable: the first occurrence of every key
    keep = np.sort(np.concatenate([real[first], np.flatnonzero(nan)]))
    out = rec[keep].copy()
    out["x"], out["y"], out["pad"], out["a"] = kx[keep], ky[keep], 1.0, 0
    return out, bits[keep], nan[keep]


def pair_step_fast(stack: list, i: int, k: int, res: float) -> int:
    """pair_step on arrays"""
    old, okey, onan = hash_fast(stack[i], res)
    new, nkey, nnan = hash_fast(stack[k], res)
    oreal, nreal = np.flatnonzero(~onan), np.flatnonzero(~nnan)
    _, oi, ni = np.intersect1d(okey[oreal], nkey[nreal], assume_unique=True, return_indices=True)
    oi, ni = oreal[oi], nreal[ni]
    oc = old["covariance"][oi]
    hit = (F32(0) < oc) & (oc < F32(1))
    oi, ni = oi[hit], ni[hit]
    nv, ne = new["covariance"][ni].astype(np.float64), new["z"][ni].astype(np.float64)
    ov, oe = old["covariance"][oi].astype(np.float64), old["z"][oi].astype(np.float64)
    f = new[ni].copy()
    with np.errstate(all="ignore"):
        nv2, ov2 = nv * nv, ov * ov
        f["z"] = (((nv2 * oe) + ((ov2 * ne) / ov2)) + nv2).astype(F32)
        f["covariance"] = (((ov2 * nv2) / ov2) + nv2).astype(F32)
    new[ni] = f
    old[oi] = f
    stack[k] = new
    stack[i] = old
    return int(ni.size)


def loop_closure(stack: list, n_opt: int, transforms, centres, radius: float = 25.0, resolution: float = 0.0,
                 map_resolution: float = None, fast: bool = False) -> int:
    """updateGlobalMap's body; transforms M[row][col] per submap (entry 0 ignored).  Returns the fused count."""
    n = min(n_opt, len(stack))
    res = float(resolution) if resolution > 0 else float(F32(map_resolution))
    for i in range(1, n):
        stack[i] = transform(stack[i], np.asarray(transforms)[i])
    fused = 0
    for i in range(n):
        lst = neighbours(centres, n, i, radius)
        if len(lst) > 2:
            for k in lst[1:]:
                fused += (pair_step_fast if fast else pair_step)(stack, i, k, res)
    return fused


def export_all(stack: list) -> np.ndarray:
    return np.concatenate(stack) if stack else np.zeros(0, POINT)


def same(a: np.ndarray, b: np.ndarray) -> bool:
    """bit for bit, except that a NaN x or y equals any NaN (the payload of a NaN key is the platform's)"""
    if a.shape != b.shape:
        return False
    a, b = a.copy(), b.copy()
    for f in ("x", "y"):
        na, nb = np.isnan(a[f]), np.isnan(b[f])
        if not np.array_equal(na, nb):
            return False
        a[f][na] = 0.0; b[f][nb] = 0.0
    return a.tobytes() == b.tobytes()
