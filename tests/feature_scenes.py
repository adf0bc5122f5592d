"""Scenes, oracle-derived bounds and the comparison rules of the traversability-stage edge tests
(tests/test_map_feature_edges_gpu.py on the device, tests/test_map_feature.py for everything that needs the oracle alone).

Kernel and oracle replay the same float operations in the same order; the only licensed difference is that a double
sin / cos / atan2 / acos of the device library and of glibc may round to adjacent floats.  `bound(scene)` measures what
that licence is worth for one scene, on the oracle alone: the largest slope change over K oracle runs whose four trig
wrappers move their result one float up or down at random (OracleMap.map_feature(nudge=(seed, 3))), times 2 -- K random
draws do not reach the worst combination of up to 9 x 5 nudges per cell; a real defect (a swapped pivot, a wrong sign, a
missed wrap) moves slopes by 1e-2 and more.  No number in the rules below is chosen by hand.

Every scene carries a precondition on the oracle's masks / rotation counts, so that a scene cannot silently stop covering
the case it was written for.
"""
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

F32 = np.float32
EMPTY = F32(-10.0)
NUDGE_ONE_IN = 3
SLOPE_ABS = 2e-3                 # the project's catch-all slope tolerance (tests/test_map_feature.py): no scene's bound may exceed it
LAYERS = ("rough", "slope", "traver")


def terrain(L, res, seed=0, amp=0.4):
    """The terrain family of tests/test_map_feature.py (slope + waves + noise, 15 % holes, a gap, a step)."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(L) * res, np.arange(L) * res, indexing="ij")
    z = 0.6 * x + 0.15 * y + amp * np.sin(2 * np.pi * x / (9 * res)) * np.cos(2 * np.pi * y / (7 * res)) + rng.normal(0, 0.01, (L, L))
    z[rng.random((L, L)) < 0.15] = -10.0
    z[:, L // 2: L // 2 + 3] = -10.0
    z[L // 3: L // 3 + 1, :] += 0.5
    return z.astype(F32)


def dense(L, res, seed, ax=0.6, ay=0.15, amp=0.4, noise=0.01):
    """The same family without holes."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(L) * res, np.arange(L) * res, indexing="ij")
    z = ax * x + ay * y + amp * np.sin(2 * np.pi * x / (9 * res)) * np.cos(2 * np.pi * y / (7 * res)) + rng.normal(0, noise, (L, L))
    return z.astype(F32)


@dataclass
class Scene:
    name: str
    L: int
    res: float
    z: np.ndarray
    move: Optional[tuple] = None                 # position handed to move() before the elevation is set
    start: Optional[tuple] = None                # (sx, sy) the move must reach (None entries: any)
    K: int = 8                                   # nudged oracle runs behind bound()
    pre: Optional[Callable] = None               # pre(scene, Eval): asserts what the scene must reach
    note: str = ""
    cache: dict = field(default_factory=dict, repr=False)


@dataclass
class Eval:
    out: dict                                    # the plain oracle's rough / slope / traver
    rot: np.ndarray                              # rotations per cell, 255 = not fitted
    start: tuple
    bound: float

    @property
    def fitted(self):
        return self.rot != 255

    @property
    def rotating(self):
        return (self.rot != 255) & (self.rot > 0)


def prepare(m, scene):
    """Brings a map (device or oracle) into the scene's state."""
    if scene.move is not None:
        m.move(np.array(scene.move, F32))
    s = tuple(int(v) for v in m.pose()[1])
    if scene.start is not None:
        for want, got in zip(scene.start, s):
            assert want is None or want == got, f"{scene.name}: start index {s}, wanted {scene.start}"
    m.set_layer("elevation", scene.z)
    return s


def evaluate(om, scene) -> Eval:
    """Plain oracle run + rotation counts + the scene's bound (K nudged runs), cached on the scene."""
    if "eval" in scene.cache:
        return scene.cache["eval"]
    ref = om.OracleMap(scene.L, scene.res)
    start = prepare(ref, scene)
    out = ref.map_feature()
    rot = ref.feature_rotations()
    worst = 0.0
    for k in range(scene.K):
        ref.set_layer("traver", np.full((scene.L, scene.L), EMPTY))
        n = ref.map_feature(nudge=(1000 + k, NUDGE_ONE_IN))
        assert np.array_equal(ref.feature_rotations() == 255, rot == 255)
        assert _same_bits(n["rough"], out["rough"]), f"{scene.name}: the nudge moved a roughness"
        still = (rot == 0)
        assert _same_bits(n["slope"][still], out["slope"][still]), f"{scene.name}: the nudge moved a cell that does not rotate"
        d = np.abs(n["slope"].astype(np.float64) - out["slope"].astype(np.float64))
        d = d[np.isfinite(d)]
        if d.size:
            worst = max(worst, float(d.max()))
    ref.close()
    ev = Eval(out, rot, start, 2.0 * worst)
    scene.cache["eval"] = ev
    return ev


def check_precondition(om, scene) -> Eval:
    bind_plain(om, scene)
    ev = evaluate(om, scene)
    if scene.pre is not None:
        scene.pre(scene, ev)
    return ev


def _same_bits(a, b) -> bool:
    a = np.ascontiguousarray(a, F32); b = np.ascontiguousarray(b, F32)
    both_nan = np.isnan(a) & np.isnan(b)                    # (a NaN's payload and sign are not part of the contract)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | both_nan))


def traver_from(slope, rough):
    """GPU:653 in numpy: float32(0.5 (1 - double(S) / 0.6) + 0.5 (1 - double(R) / 0.2))."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (0.5 * (1.0 - slope.astype(np.float64) / 0.6) + 0.5 * (1.0 - rough.astype(np.float64) / 0.2)).astype(F32)


def compare(g, ev: Eval, scene, slope_abs: float) -> dict:
    """The six rules, applied to the device's layers `g` against the oracle's `ev`.  Returns the scene's row of
    profiles/map_feature_edges.txt."""
    o, name = ev.out, scene.name
    fitted, rotating = ev.fitted, ev.rotating
    print(f"[{name}] bound {ev.bound:.3e}  fitted {int(fitted.sum())}  rotating {int(rotating.sum())}  max rotations "
          f"{int(ev.rot[fitted].max()) if fitted.any() else 0}")
    assert ev.bound <= slope_abs, f"{name}: the oracle-derived bound {ev.bound:.3e} is looser than SLOPE_ABS"
    # 1. masks
    assert np.array_equal(g["traver"] == EMPTY, o["traver"] == EMPTY), f"{name}: sets of unfitted cells differ"
    for k in LAYERS:
        assert np.array_equal(np.isnan(g[k]), np.isnan(o[k])), f"{name}: NaN masks differ in {k}"
        assert np.array_equal(np.isposinf(g[k]), np.isposinf(o[k])) and np.array_equal(np.isneginf(g[k]), np.isneginf(o[k])), \
            f"{name}: inf masks differ in {k}"
    # 2. roughness: no library call, bit-identical
    fin = np.isfinite(o["rough"])
    assert _same_bits(g["rough"][fin], o["rough"][fin]), f"{name}: roughness differs in {int((g['rough'][fin] != o['rough'][fin]).sum())} cells"
    # 3. traver follows from the device's own slope and roughness
    t = traver_from(g["slope"], g["rough"])
    ok = fitted & np.isfinite(g["traver"]) & np.isfinite(t)
    assert _same_bits(g["traver"][ok], t[ok]), f"{name}: traver is not 0.5 (1 - slope / 0.6) + 0.5 (1 - rough / 0.2) of the device's layers"
    assert _same_bits(g["traver"][~fitted], o["traver"][~fitted]) and not g["slope"][~fitted].any() and not g["rough"][~fitted].any(), \
        f"{name}: a cell without a fit was written"
    # 4. cells that do not rotate
    still = fitted & ~rotating
    assert _same_bits(g["slope"][still], o["slope"][still]), f"{name}: slope differs in a cell that does not rotate"
    # 5. cells that rotate: within the licence
    gs, os_ = g["slope"][rotating].astype(np.float64), o["slope"][rotating].astype(np.float64)
    finite = np.isfinite(os_)
    diff = np.abs(gs[finite] - os_[finite])
    worst = float(diff.max()) if diff.size else 0.0
    unequal = int((g["slope"][rotating][finite] != o["slope"][rotating][finite]).sum())
    row = {"scene": name, "fitted": int(fitted.sum()), "rotating": int(rotating.sum()), "not_bit_equal": unequal,
           "max_abs_slope_diff": worst, "bound": ev.bound}
    print(f"[{name}] cells not bit-equal {unequal}  max |slope_gpu - slope_ref| {worst:.3e}")
    assert worst <= ev.bound, f"{name}: slope differs by {worst:.3e}, the trigonometry licenses {ev.bound:.3e}"
    # 6. share of the rotating cells that agree bit for bit
    if diff.size:
        assert 1.0 - unequal / diff.size >= 0.999, f"{name}: {unequal} of {diff.size} rotating cells are not bit-equal"
    return row


# ---- float32 replay of the covariance and of the pivot scan (numpy scalars, the reference's order) ------------------------
def covariance_replay(z, res, start=(0, 0)):
    """(n [L, L], a [L, L, 6] = a00 a11 a22 a01 a02 a12) of every cell with more than 7 valid window cells, float32, in the
    reference's order (GPU:583-635).  For small maps only: a Python loop."""
    L = z.shape[0]
    r = F32(res)
    n_out = np.zeros((L, L), np.int32); a_out = np.zeros((L, L, 6), F32)
    for cx in range(L):
        for cy in range(L):
            if z[cx, cy] == EMPTY:
                continue
            px, py, pz = [], [], []
            ex0, ey0 = (cx + L - start[0]) % L, (cy + L - start[1]) % L
            for i in range(-2, 3):
                for j in range(-2, 3):
                    if 0 <= ex0 + i < L and 0 <= ey0 + j < L:
                        sx_, sy_ = (cx + i + L) % L, (cy + j + L) % L
                        if z[sx_, sy_] != EMPTY:
                            px.append(F32(sx_) * r); py.append(F32(sy_) * r); pz.append(F32(z[sx_, sy_]))
            n = len(px)
            n_out[cx, cy] = n
            if n <= 7:
                continue
            mx = my = mz = F32(0)
            for k in range(n):
                mx = F32(mx + px[k]); my = F32(my + py[k]); mz = F32(mz + pz[k])
            mx = F32(mx / F32(n)); my = F32(my / F32(n)); mz = F32(mz / F32(n))
            a = [F32(0)] * 6
            for k in range(n):
                dx, dy, dz = F32(px[k] - mx), F32(py[k] - my), F32(pz[k] - mz)
                for q, (u, v) in enumerate(((dx, dx), (dy, dy), (dz, dz), (dx, dy), (dx, dz), (dy, dz))):
                    a[q] = F32(a[q] + F32(u * v))
            a_out[cx, cy] = a
    return n_out, a_out


def pivot_replay(m):
    """The pivot scan of computerEigenvalue on a row-major 3x3 float32 matrix (GPU:85-103): (row, col) of the pivot, or None
    when the loop ends.  The start value is the SIGNED m[0][1]; a later entry wins only when its magnitude is strictly greater."""
    m = np.asarray(m, F32).reshape(3, 3)
    best, row, col = m[0, 1], 0, 1
    for i in range(3):
        for j in range(3):
            d = np.abs(m[i, j])
            if i != j and d > best:
                best, row, col = d, i, j
    if best < F32(0.01):
        return None
    return row, col


def jacobi_replay(m, strict=True):
    """computerEigenvalue (GPU:66-187) on float32 numpy scalars, trigonometry in double (libm) and rounded: (nCount, pivots,
    eigenvector of the smallest eigenvalue).  strict=False replaces the scan's > by >= (what a wrong restatement would do)."""
    import math
    a = np.array(m, F32).reshape(3, 3); v = np.eye(3, dtype=F32)
    count, pivots = 0, []
    while True:
        best, p, q = a[0, 1], 0, 1
        for i in range(3):
            for j in range(3):
                d = np.abs(a[i, j])
                if i != j and (d > best if strict else d >= best):
                    best, p, q = d, i, j
        if best < F32(0.01) or count > 30:
            break
        count += 1; pivots.append((p, q))
        app, apq, aqq = a[p, p], a[p, q], a[q, q]
        ang = F32(0.5 * float(F32(math.atan2(float(F32(-2) * apq), float(aqq - app)))))
        sn, cs = F32(math.sin(float(ang))), F32(math.cos(float(ang)))
        sn2, cs2 = F32(math.sin(float(F32(2) * ang))), F32(math.cos(float(F32(2) * ang)))
        a[p, p] = app * cs * cs + aqq * sn * sn + F32(2) * apq * cs * sn
        a[q, q] = app * sn * sn + aqq * cs * cs - F32(2) * apq * cs * sn
        a[p, q] = a[q, p] = F32(0.5 * float(aqq - app) * float(sn2) + float(apq * cs2))
        r = 3 - p - q
        for u, w in (((r, p), (r, q)), ((p, r), (q, r))):              # column pair, then row pair (GPU:129-151)
            t = a[u]; a[u] = a[w] * sn + t * cs; a[w] = a[w] * cs - t * sn
        for i in range(3):
            t = v[i, p]; v[i, p] = v[i, q] * sn + t * cs; v[i, q] = v[i, q] * cs - t * sn
    k = 0
    for i in (1, 2):
        if a[k, k] > a[i, i]:
            k = i
    return count, pivots, v[:, k].copy()


def window_counts(z, start=(0, 0)):
    """Valid cells in every cell's 5x5 window (clipped in unrolled coordinates, read with the storage wrap), from the hole mask."""
    L = z.shape[0]
    valid = np.roll(z != EMPTY, (-start[0], -start[1]), (0, 1)).astype(np.int32)      # unrolled
    pad = np.zeros((L + 4, L + 4), np.int32); pad[2:-2, 2:-2] = valid
    n = sum(pad[i:i + L, j:j + L] for i in range(5) for j in range(5))
    return np.roll(n, (start[0], start[1]), (0, 1))


# ---- preconditions -----------------------------------------------------------------------------------------------------------
def _tiles(mask):
    """Rotating cells per 16x16 storage tile (the kernel's jn)."""
    L = mask.shape[0]; t = (L + 15) // 16
    pad = np.zeros((16 * t, 16 * t), np.int32); pad[:L, :L] = mask
    return pad.reshape(t, 16, t, 16).sum((1, 3))


def pre_rotating_share(share):
    def pre(sc, ev):
        assert ev.rotating.mean() >= share, f"{sc.name}: only {ev.rotating.mean():.3f} of the cells rotate"
    return pre


def pre_full_tile(sc, ev):
    jn = _tiles(ev.rotating)
    assert (jn[1:-1, 1:-1] == 256).any(), f"{sc.name}: no interior tile in which all 256 cells rotate"


def pre_island(sc, ev):
    jn = _tiles(ev.rotating)
    part = np.argwhere((jn > 0) & (jn < 64))
    assert len(part) == 1 and (jn > 0).sum() == 1, f"{sc.name}: rotating cells per tile {jn.tolist()}"
    r, c = part[0]
    assert jn[r - 1, c] == 0 and jn[r + 1, c] == 0 and jn[r, c - 1] == 0 and jn[r, c + 1] == 0


def pre_tie_plain(sc, ev):
    _, a = covariance_replay(sc.z, sc.res)
    inner = a[2:-2, 2:-2].reshape(-1, 6)
    assert inner.shape[0] == 144
    assert np.all(inner[:, 3] == 0) and np.all(np.abs(inner[:, 4]) == np.abs(inner[:, 5])) and np.all(np.abs(inner[:, 4]) >= F32(0.01)), \
        f"{sc.name}: |a02| == |a12| with a01 == 0 does not hold in every interior cell"
    assert ev.rotating[2:-2, 2:-2].all()


def pre_tie_holes(sc, ev):
    n, a = covariance_replay(sc.z, sc.res)
    f = (n > 7) & (sc.z != EMPTY)
    a = a[f]
    a01, m02, m12 = a[:, 3], np.abs(a[:, 4]), np.abs(a[:, 5])
    assert (a01 > 0).any() and (a01 < 0).any(), f"{sc.name}: a01 has one sign only"
    tie = (np.abs(a01) >= F32(0.01)) & ((np.abs(a01) == m02) | (np.abs(a01) == m12))
    assert tie.any(), f"{sc.name}: no tie in magnitude between a01 and a02 / a12"
    top = tie & (((np.abs(a01) == m02) & (m02 >= m12)) | ((np.abs(a01) == m12) & (m12 >= m02)))
    assert top.any(), f"{sc.name}: no tie that decides the pivot"
    assert np.array_equal(f, ev.fitted)


def pre_near_flat(sc, ev):
    s = ev.out["slope"][ev.rotating]
    assert s.size > 100 and s.max() < 1.5e-3, f"{sc.name}: {s.size} rotating cells, largest slope {s.max() if s.size else 0:.3e}"
    assert (s > 0).any()


def pre_many_rotations(sc, ev):
    assert ev.rot[ev.fitted].max() >= 8, f"{sc.name}: at most {ev.rot[ev.fitted].max()} rotations"


def pre_fitted(count):
    def pre(sc, ev):
        assert ev.fitted.sum() > count, f"{sc.name}: {ev.fitted.sum()} fitted cells"
    return pre


def pre_seven_eight(sc, ev):
    n = window_counts(sc.z)
    valid = sc.z != EMPTY
    assert (valid & (n == 7)).sum() >= 12 and (valid & (n == 8)).sum() >= 12, \
        f"{sc.name}: {(valid & (n == 7)).sum()} windows of 7, {(valid & (n == 8)).sum()} of 8"
    assert np.array_equal(valid & (n > 7), ev.fitted), f"{sc.name}: p_n > 7 is not what decides the fit"


def pre_minus_ten(cell):
    def pre(sc, ev):
        r, c = cell
        assert sc.z[r, c] == EMPTY and ev.rot[r, c] == 255 and ev.out["traver"][r, c] == EMPTY
        n = window_counts(sc.z)
        assert n[r, c + 1] == 24 and n[r + 1, c] == 24 and ev.fitted[r, c + 1] and ev.fitted.sum() == sc.L * sc.L - 1
    return pre


def pre_start(sc, ev):
    sx, sy = ev.start
    L = sc.L
    assert ev.fitted[sx % L, sy % L], f"{sc.name}: the unrolled corner cell is not fitted"
    n = window_counts(sc.z, ev.start)
    assert n[sx % L, sy % L] == 9 and np.array_equal((sc.z != EMPTY) & (n > 7), ev.fitted)


def pre_small(sc, ev):
    L = sc.L
    n = window_counts(sc.z, ev.start)
    assert np.array_equal((sc.z != EMPTY) & (n > 7), ev.fitted), f"{sc.name}: fitted cells are not those with more than 7 window cells"
    if L <= 2:
        assert not ev.fitted.any()
    if L == 3 and not (sc.z == EMPTY).any():
        assert ev.fitted.all()


def nonfinite_cells():
    """(row, col, value) of the non-finite heights put into terrain(64, 0.1, 1): one NaN, +inf and -inf inside, a NaN on the map's
    rim and a NaN next to a hole."""
    return [(10, 10, np.nan), (20, 40, np.inf), (45, 12, -np.inf), (0, 25, np.nan), (50, 36, np.nan)]


def pre_nonfinite(sc, ev):
    o = ev.out
    for k in ("rough", "traver"):
        assert np.isnan(o[k]).any() and np.isinf(o[k]).any(), f"{sc.name}: no NaN / inf in {k}"
    assert sc.z[50, 35] == EMPTY                                   # the NaN next to a hole (the gap of the terrain)
    far = np.ones((sc.L, sc.L), bool)
    for r, c, _ in nonfinite_cells():
        far[max(0, r - 2): r + 3, max(0, c - 2): c + 3] = False
    plain = sc.cache["plain"]
    for k in LAYERS:
        assert np.isfinite(o[k][far]).all() and _same_bits(o[k][far], plain.out[k][far]), f"{sc.name}: a non-finite height reached further than 2 cells in {k}"
    assert (~far & ev.fitted).sum() > 60


# ---- the scenes ------------------------------------------------------------------------------------------------------------------
def _plane(L, res, ax, ay):
    x, y = np.meshgrid(np.arange(L, dtype=np.float64) * res, np.arange(L, dtype=np.float64) * res, indexing="ij")
    return ax * x + ay * y


TIE_HOLES = (0, 4, 13, 17, 18, 19, 23, 24)        # cells (row * 5 + col) of a 5x5 tile, repeated with period 5; chosen on the replay


def _tie_holes(z):
    """Holes of period 5, found by trying patterns on covariance_replay until a01 takes both signs and its magnitude ties
    bit for bit with that of a02 or a12 (pre_tie_holes), in at least one cell as the largest entry of the scan."""
    z = z.copy()
    for c in TIE_HOLES:
        z[c // 5::5, c % 5::5] = EMPTY
    return z


def _seven_eight():
    z = terrain(64, 0.1, 1)
    z[37:, :] = EMPTY                                              # three empty rows, then the hand-made patch
    rng = np.random.default_rng(7)
    k = 0
    for r in (41, 47, 53, 59):
        for c in range(1, 62, 6):
            blob = (0.5 * np.arange(3)[:, None] * 0.1 + 0.3 * np.arange(3)[None, :] * 0.1 + rng.normal(0, 0.02, (3, 3)) + 1.0).astype(F32)
            blob[0, 0] = EMPTY                                     # 8 cells: fitted
            if k % 2:
                blob[2, 1] = EMPTY                                 # 7 cells: not fitted
            z[r:r + 3, c:c + 3] = blob
            k += 1
    return z


def core_scenes():
    out = []
    out.append(Scene("terrain64", 64, 0.1, terrain(64, 0.1, 1), pre=pre_rotating_share(0.3)))
    out.append(Scene("terrain75_moved", 75, 0.2, terrain(75, 0.2, 2), move=(1.3, -0.7, 0), pre=pre_rotating_share(0.3)))
    out.append(Scene("terrain200", 200, 0.05, terrain(200, 0.05, 3), pre=pre_rotating_share(0.3)))
    out.append(Scene("steep_plane_full_tiles", 64, 0.1, _plane(64, 0.1, 2.0, 1.5).astype(F32), pre=pre_full_tile))
    z = np.full((64, 64), 0.25, F32); z[21:24, 20:24] = 1.25
    out.append(Scene("island_in_flat", 64, 0.1, z, pre=pre_island))
    for tag, (ax, ay) in (("x+y", (1, 1)), ("-x-y", (-1, -1)), ("x-y", (1, -1))):
        p = _plane(16, 0.125, ax, ay).astype(F32)
        out.append(Scene(f"tie[{tag}]", 16, 0.125, p, pre=pre_tie_plain))
        out.append(Scene(f"tie_holes[{tag}]", 16, 0.125, _tie_holes(p), pre=pre_tie_holes))
    rng = np.random.default_rng(11)
    out.append(Scene("near_flat", 64, 1.0, (_plane(64, 1.0, 3e-4, 1e-4) + rng.normal(0, 1e-3, (64, 64))).astype(F32), pre=pre_near_flat))
    rng = np.random.default_rng(12)
    out.append(Scene("res1000_moved", 64, 1000.0, (_plane(64, 1000.0, 0.5, 0.2) + rng.normal(0, 10.0, (64, 64))).astype(F32),
                     move=(7000.0, -5000.0, 0), start=(64 - 7, 5), pre=pre_many_rotations))
    t = terrain(64, 0.1, 1)
    out.append(Scene("terrain+1e4", 64, 0.1, np.where(t == EMPTY, EMPTY, t + F32(1e4)).astype(F32), pre=pre_fitted(3000)))
    out.append(Scene("terrain*1e3", 64, 0.1, np.where(t == EMPTY, EMPTY, t * F32(1e3)).astype(F32), pre=pre_fitted(3000)))
    plain = Scene("terrain64_for_nonfinite", 64, 0.1, _nonfinite_base())
    nf = plain.z.copy()
    for r, c, v in nonfinite_cells():
        nf[r, c] = v
    sc = Scene("nonfinite", 64, 0.1, nf, pre=pre_nonfinite)
    sc.cache["plain_scene"] = plain
    out.append(sc)
    p = (_plane(32, 0.1, 0.3, -0.2) + 1.0).astype(F32); p[12, 17] = EMPTY
    out.append(Scene("minus_ten_is_a_hole", 32, 0.1, p, pre=pre_minus_ten((12, 17))))
    out.append(Scene("seven_eight", 64, 0.1, _seven_eight(), pre=pre_seven_eight))
    return out


def _nonfinite_base():
    z = terrain(64, 0.1, 1)
    for r, c, _ in nonfinite_cells():
        z[r, c] = F32(1.0) if z[r, c] == EMPTY else z[r, c]       # the cells that will hold the non-finite heights are valid
    z[50, 35] = EMPTY
    return z


def start_scenes():
    out = []
    for L in (16, 17, 31, 33, 75):
        res = 0.1
        for axis in (0, 1):
            for k, target in enumerate(sorted({0, 1, 2, 15, 16, 17, L - 2, L - 1})):
                if target >= L:
                    continue
                other = (3 * L // 7 + 5 * k + axis) % L
                s = (target, other) if axis == 0 else (other, target)
                # start = -shift mod L (Move): a move of -s cells from the origin
                mv = (-s[0] * res, -s[1] * res, 0.0)
                z = dense(L, res, 300 + L + k)
                rng = np.random.default_rng(L * 16 + k)
                holes = rng.random((L, L)) < 0.08
                holes[np.ix_([(s[0] + d) % L for d in range(3)], [(s[1] + d) % L for d in range(3)])] = False    # the corner's 3x3 window
                z[holes] = EMPTY
                out.append(Scene(f"start[L{L},sx{s[0]},sy{s[1]}]", L, res, z, move=mv, start=s, pre=pre_start))
    return out


def small_scenes():
    out = []
    for L in range(1, 7):
        for moved in (False, True):
            for holes in (False, True):
                rng = np.random.default_rng(L * 4 + 2 * moved + holes)
                z = (_plane(L, 0.25, 0.8, -0.5) + rng.normal(0, 0.02, (L, L)) + 0.5).astype(F32)
                if holes:
                    z[rng.integers(0, L), rng.integers(0, L)] = EMPTY
                s = ((L + 1) // 2 % L, (L - 1) % L) if moved else (0, 0)
                mv = (-s[0] * 0.25, -s[1] * 0.25, 0.0) if moved else None
                out.append(Scene(f"small[L{L},{'moved' if moved else 'unmoved'},{'holes' if holes else 'full'}]", L, 0.25, z,
                                 move=mv, start=s, pre=pre_small))
    return out


def big_scene():
    return Scene("terrain1025", 1025, 0.05, terrain(1025, 0.05, 4), K=2, pre=pre_rotating_share(0.3))


def bind_plain(om, scene):
    """The non-finite scene compares against the same scene without the non-finite heights."""
    if "plain_scene" in scene.cache and "plain" not in scene.cache:
        scene.cache["plain"] = evaluate(om, scene.cache["plain_scene"])


_ALL = None


def all_scenes():
    global _ALL
    if _ALL is None:
        _ALL = core_scenes() + start_scenes() + small_scenes() + [big_scene()]
    return _ALL
