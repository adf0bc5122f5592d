"""octomap 1.8 / 1.9 ColorOcTree insertion, restated (include/gem_hip.h, gem_octree_build) -- twice.

build_literal()  a pointer tree that follows the library's functions one for one: updateNode / updateNodeRecurs / expandNode /
                 pruneNode / integrateNodeColor / updateInnerOccupancy / writeData.  Slow, and the thing everything else is pinned to.
build_array()    the form the device takes: keys, a stable sort by Morton key, leaves, every leaf's largest full aligned block (k*),
                 one walker per block, inner nodes by level from the sorted terminals, the stream by offsets.

Records are PointXYZRGBICT (32 bytes: x y z at 0 4 8, b g r a bytes at 16).  octomap itself is not needed (and not here).
"""
from __future__ import annotations

import math
from bisect import bisect_left

import numpy as np

DEPTH = 16
MAXVAL = 32768
RECORD = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1"),
                   ("covariance", "<f4"), ("intensity", "<f4"), ("travers", "<f4")])
assert RECORD.itemsize == 32
WHITE = (255, 255, 255)


class Params:
    """gem_octree_params: zeros in the three probabilities select octomap's defaults."""

    def __init__(self, resolution, prob_hit=0.0, clamp_min=0.0, clamp_max=0.0):
        self.resolution = float(resolution)
        self.hit = np.float32(math.log(0.7 / 0.3)) if prob_hit == 0.0 else np.float32(math.log(prob_hit / (1.0 - prob_hit)))
        self.cmin = np.float32(math.log(0.1192 / 0.8808)) if clamp_min == 0.0 else np.float32(math.log(clamp_min / (1.0 - clamp_min)))
        self.cmax = np.float32(math.log(0.971 / 0.029)) if clamp_max == 0.0 else np.float32(math.log(clamp_max / (1.0 - clamp_max)))
        self.prob_hit = prob_hit
        if not (math.isfinite(self.resolution) and self.resolution > 0.0):
            raise ValueError("resolution")
        if prob_hit != 0.0 and not prob_hit > 0.5:
            raise ValueError("prob_hit")
        # f(n): the value of a leaf after n hits; S: the first n with f(n) >= cmax
        self.f = [np.float32(0.0)]
        while not self.f[-1] >= self.cmax:
            if len(self.f) > 64:
                raise ValueError("no saturation within 64 steps")
            v = np.float32(min(max(np.float32(self.f[-1] + self.hit), self.cmin), self.cmax))
            if not v > self.f[-1]:
                raise ValueError("values not strictly increasing")
            self.f.append(v)
        self.S = len(self.f) - 1
        if self.S < 1:
            raise ValueError("clamp_max <= 0")
        self.p = [blend_p(v) for v in self.f]


def blend_p(value):
    return 1.0 - 1.0 / (1.0 + math.exp(float(value)))


def blend(prev, c, p):
    """one channel of integrateNodeColor: (uint8_t)((double)prev * p + (double)c * (0.99 - p))"""
    return int(float(prev) * p + float(c) * (0.99 - p)) & 255


def axis_key(coord, rf):
    """(int)floor(rf * (double)coord) + 32768, or None (out of range / not finite)"""
    c = float(coord)
    if not math.isfinite(c):
        return None
    k = math.floor(rf * c) + MAXVAL
    return int(k) if 0 <= k < 2 * MAXVAL else None


def point_key(rec, rf):
    k = (axis_key(rec["x"], rf), axis_key(rec["y"], rf), axis_key(rec["z"], rf))
    return None if None in k else k


def morton(k):
    m = 0
    for d in range(DEPTH):
        m |= (((k[0] >> d) & 1) | (((k[1] >> d) & 1) << 1) | (((k[2] >> d) & 1) << 2)) << (3 * d)
    return m


def rgb_of(rec):
    return (int(rec["r"]), int(rec["g"]), int(rec["b"]))


def make_cloud(xyz, rgb):
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    rgb = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
    out = np.zeros(xyz.shape[0], dtype=RECORD)
    out["x"], out["y"], out["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out["r"], out["g"], out["b"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    out["pad"] = 1.0
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the literal form
# ---------------------------------------------------------------------------------------------------------------------------------
class Node:
    __slots__ = ("value", "color", "children")

    def __init__(self):
        self.value = np.float32(0.0)
        self.color = WHITE
        self.children = None

    def has_children(self):
        return self.children is not None and any(c is not None for c in self.children)

    def color_set(self):
        return self.color != WHITE

    def average_child_color(self):
        s, c = [0, 0, 0], 0
        if self.children is not None:
            for ch in self.children:
                if ch is not None and ch.color_set():
                    s = [s[i] + ch.color[i] for i in range(3)]
                    c += 1
        if c:
            return tuple((v // c) & 255 for v in s)
        return WHITE


class LiteralTree:
    def __init__(self, params):
        self.P = params
        self.root = None
        self.stats = dict(points_in=0, points_keyed=0, prunes=0, expands=0, prunes_level=[0] * (DEPTH + 1))

    def search(self, m):
        if self.root is None:
            return None
        n = self.root
        for d in range(DEPTH - 1, -1, -1):
            pos = (m >> (3 * d)) & 7
            if n.children is not None and n.children[pos] is not None:
                n = n.children[pos]
            elif not n.has_children():
                return n                      # a pruned leaf above depth 16
            else:
                return None
        return n

    def update_node(self, m):
        leaf = self.search(m)
        if leaf is not None and leaf.value >= self.P.cmax:
            return
        created_root = False
        if self.root is None:
            self.root = Node()
            created_root = True
        self._recurs(self.root, created_root, m, 0)

    def _recurs(self, node, just_created, m, depth):
        if depth == DEPTH:
            node.value = np.float32(min(max(np.float32(node.value + self.P.hit), self.P.cmin), self.P.cmax))
            return
        pos = (m >> (3 * (DEPTH - 1 - depth))) & 7
        created = False
        if node.children is None or node.children[pos] is None:
            if not node.has_children() and not just_created:
                node.children = []
                for _ in range(8):                # expandNode: the children copy value and colour
                    c = Node()
                    c.value, c.color = node.value, node.color
                    node.children.append(c)
                self.stats["expands"] += 1
            else:
                if node.children is None:
                    node.children = [None] * 8
                node.children[pos] = Node()
                created = True
        self._recurs(node.children[pos], created, m, depth + 1)
        if self._prune(node):
            self.stats["prunes"] += 1
            self.stats["prunes_level"][DEPTH - depth] += 1
        else:
            node.value = max(c.value for c in node.children if c is not None)

    def _prune(self, node):
        ch = node.children
        if ch is None or any(c is None for c in ch) or any(c.has_children() for c in ch):
            return False
        if any(not (c.value == ch[0].value) for c in ch):
            return False
        node.value, node.color = ch[0].value, ch[0].color
        if node.color_set():
            node.color = node.average_child_color()
        node.children = None
        return True

    def integrate_color(self, m, rgb):
        n = self.search(m)
        if n is None:
            return
        if not n.color_set():
            n.color = tuple(rgb)
        else:
            p = blend_p(n.value)
            n.color = tuple(blend(n.color[i], rgb[i], p) for i in range(3))

    def insert(self, cloud):
        rf = 1.0 / self.P.resolution
        for rec in cloud:
            self.stats["points_in"] += 1
            k = point_key(rec, rf)
            if k is None:
                continue
            self.stats["points_keyed"] += 1
            m = morton(k)
            self.update_node(m)
            self.integrate_color(m, rgb_of(rec))

    def update_inner(self):
        if self.root is not None:
            self._inner(self.root)

    def _inner(self, node):
        if not node.has_children():
            return
        for c in node.children:
            if c is not None:
                self._inner(c)
        node.value = max(c.value for c in node.children if c is not None)
        node.color = node.average_child_color()

    def stream(self):
        out = bytearray()
        nodes = leaves = pruned = 0
        stack = [(self.root, 0)] if self.root is not None else []
        while stack:
            n, d = stack.pop()
            mask = 0
            if n.children is not None:
                for i, c in enumerate(n.children):
                    if c is not None:
                        mask |= 1 << i
            out += np.float32(n.value).tobytes() + bytes([n.color[0], n.color[1], n.color[2], mask])
            nodes += 1
            if mask == 0:
                if d == DEPTH:
                    leaves += 1
                else:
                    pruned += 1
            for i in range(7, -1, -1):
                if mask & (1 << i):
                    stack.append((n.children[i], d + 1))
        self.stats.update(nodes=nodes, leaves_depth16=leaves, pruned_leaves=pruned, bytes=len(out))
        return bytes(out)


def build_literal(cloud, params):
    """(stream bytes, stats) of pointCloudtoOctomap's loop + updateInnerOccupancy + fullMapToMsg"""
    t = LiteralTree(params)
    t.insert(cloud)
    t.update_inner()
    data = t.stream()
    return data, t.stats


# ---------------------------------------------------------------------------------------------------------------------------------
# the array form
# ---------------------------------------------------------------------------------------------------------------------------------
def sorted_leaves(cloud, params):
    """keys of the valid records, stably sorted: (order, keys sorted, leaf starts, leaf keys)"""
    rf = 1.0 / params.resolution
    keys, pos = [], []
    for i, rec in enumerate(cloud):
        k = point_key(rec, rf)
        if k is not None:
            keys.append(morton(k))
            pos.append(i)
    order = sorted(range(len(keys)), key=lambda j: keys[j])          # stable
    skey = [keys[j] for j in order]
    spos = [pos[j] for j in order]
    starts = [j for j in range(len(skey)) if j == 0 or skey[j] != skey[j - 1]]
    return skey, spos, starts


def leaf_kstar(lkeys, max_level=3):
    """the largest k <= max_level for which the aligned block of 8^k leaves around each leaf is all there"""
    n = len(lkeys)
    ks = [0] * n
    for i, key in enumerate(lkeys):
        for k in range(1, max_level + 1):
            sz = 8 ** k
            base = key & ~(sz - 1)
            j = i - (key - base)
            if j >= 0 and j + sz - 1 < n and lkeys[j] == base and lkeys[j + sz - 1] == base + sz - 1:
                ks[i] = k
            else:
                break
    return ks


def walk_single(params, colors):
    """k* = 0: the leaf's records in order -> (count, colour)"""
    cnt, col = 0, WHITE
    for rgb in colors:
        cnt = min(cnt + 1, params.S)
        col = tuple(rgb) if col == WHITE else tuple(blend(col[i], rgb[i], params.p[cnt]) for i in range(3))
    return cnt, col


def _avg(cols):
    s = [c for c in cols if c != WHITE]
    if not s:
        return WHITE
    return tuple((sum(c[i] for c in s) // len(s)) & 255 for i in range(3))


def walk_block(params, K, events):
    """One block of 8^K leaves (K = 1, 2), every leaf hit at least once; events = [(leaf slot, rgb)] in input order.
    Returns per leaf slot (term, count, colour): term 0 = the leaf is a node, k = the slot is the base of a block pruned at level k,
    255 = covered by one.  State as the device keeps it: leaves L[64], mids M[8] (level 1), top T (level 2); for K = 1 only
    octet 0 is populated and the top never prunes (its other children are not there)."""
    S = params.S
    L = [None] * 64                    # [cnt, col] or None
    M = [None] * 8                     # [cnt, col, has_children]
    T = None                           # [cnt, col, has_children]
    top = K == 2

    def blend_into(node, rgb):
        node[1] = tuple(rgb) if node[1] == WHITE else tuple(blend(node[1][i], rgb[i], params.p[node[0]]) for i in range(3))

    for slot, rgb in events:
        o = slot >> 3
        # search
        if top and T is not None and not T[2]:
            s = T
        elif M[o] is not None and not M[o][2]:
            s = M[o]
        elif M[o] is not None and L[slot] is not None:
            s = L[slot]
        else:
            s = None
        if s is None or s[0] < S:
            # updateNodeRecurs
            fresh_t = False
            if top:
                if T is None:
                    T = [0, WHITE, False]
                    fresh_t = True
            fresh_m = False
            if M[o] is None:
                if top and not T[2] and not fresh_t:           # the top is pruned: expand it
                    for q in range(8):
                        M[q] = [T[0], T[1], False]
                else:
                    M[o] = [0, WHITE, False]
                    fresh_m = True
                if top:
                    T[2] = True
            if L[slot] is None:
                if not M[o][2] and not fresh_m:                # the mid is pruned: expand it
                    for q in range(8):
                        L[o * 8 + q] = [M[o][0], M[o][1]]
                else:
                    L[slot] = [0, WHITE]
                M[o][2] = True
            L[slot][0] = min(L[slot][0] + 1, S)
            ch = L[o * 8:o * 8 + 8]
            if all(c is not None for c in ch) and all(c[0] == ch[0][0] for c in ch):
                M[o][0], M[o][1], M[o][2] = ch[0][0], ch[0][1], False
                if M[o][1] != WHITE:
                    M[o][1] = _avg([c[1] for c in ch])
                for q in range(8):
                    L[o * 8 + q] = None
                if top and all(m is not None and not m[2] for m in M) and all(m[0] == M[0][0] for m in M):
                    T[0], T[1], T[2] = M[0][0], M[0][1], False
                    if T[1] != WHITE:
                        T[1] = _avg([m[1] for m in M])
                    M = [None] * 8
        # integrateNodeColor: search again
        if top and T is not None and not T[2]:
            blend_into(T, rgb)
        elif not M[o][2]:
            blend_into(M[o], rgb)
        else:
            blend_into(L[slot], rgb)
    out = [None] * (8 ** K)
    if top and not T[2]:
        out = [(255, 0, WHITE)] * 64
        out[0] = (2, T[0], T[1])
        return out
    for o in range(8 ** (K - 1)):
        if not M[o][2]:
            for q in range(8):
                out[o * 8 + q] = (255, 0, WHITE)
            out[o * 8] = (1, M[o][0], M[o][1])
        else:
            for q in range(8):
                out[o * 8 + q] = (0, L[o * 8 + q][0], L[o * 8 + q][1])
    return out


def fallback_terminals(params, lkeys, events):
    """k* >= 3: the literal tree over these leaves' records in input order; returns (term, value-count, colour) per leaf in key order"""
    t = LiteralTree(params)
    for m, rgb in events:
        t.update_node(m)
        t.integrate_color(m, rgb)
    out = []

    def rec(n, d):
        if not n.has_children():
            lvl = DEPTH - d
            cnt = params.f.index(n.value)
            out.append((lvl, cnt, n.color))
            out.extend([(255, 0, WHITE)] * (8 ** lvl - 1))
            return
        for c in n.children:
            if c is not None:
                rec(c, d + 1)

    if t.root is not None:
        rec(t.root, 0)
    assert len(out) == len(lkeys)
    return out


def regroup(cloud, params, by="block"):
    """the cloud stably reordered by group: 'block' = every leaf's largest full aligned block, 'leaf' = the leaf alone"""
    skey, spos, starts = sorted_leaves(cloud, params)
    lkeys = [skey[s] for s in starts]
    ks = leaf_kstar(lkeys, max_level=DEPTH) if by == "block" else [0] * len(lkeys)
    ends = starts[1:] + [len(skey)]
    groups = {}
    for i, key in enumerate(lkeys):
        g = key >> (3 * ks[i])
        groups.setdefault((ks[i], g), []).extend(spos[starts[i]:ends[i]])
    idx = []
    for g in groups.values():
        idx.extend(sorted(g))
    return cloud[np.asarray(idx, dtype=np.int64)] if idx else cloud[:0]


def build_array(cloud, params):
    skey, spos, starts = sorted_leaves(cloud, params)
    stats = dict(points_in=len(cloud), points_keyed=len(skey), leaves_depth16=0, pruned_leaves=0, nodes=0, bytes=0,
                 coupled_blocks=[0, 0, 0], fallback_points=0)
    if not skey:
        return b"", stats
    lkeys = [skey[s] for s in starts]
    ends = starts[1:] + [len(skey)]
    nl = len(lkeys)
    ks = leaf_kstar(lkeys)
    cols = [rgb_of(cloud[p]) for p in spos]
    term = [None] * nl
    i = 0
    fb_leaves = []
    while i < nl:
        k = ks[i]
        if k == 0:
            cnt, col = walk_single(params, cols[starts[i]:ends[i]])
            term[i] = (0, cnt, col)
            i += 1
        elif k <= 2:
            sz = 8 ** k
            ev = sorted((spos[j], q, cols[j]) for q in range(sz) for j in range(starts[i + q], ends[i + q]))
            term[i:i + sz] = walk_block(params, k, [(q, c) for _, q, c in ev])
            stats["coupled_blocks"][k - 1] += 1
            i += sz
        else:
            stats["coupled_blocks"][2] += 1
            fb_leaves.extend(range(i, i + 512))
            i += 512
    if fb_leaves:
        ev = sorted((spos[j], lkeys[i], cols[j]) for i in fb_leaves for j in range(starts[i], ends[i]))
        stats["fallback_points"] = len(ev)
        for i, t in zip(fb_leaves, fallback_terminals(params, [lkeys[i] for i in fb_leaves], [(m, c) for _, m, c in ev])):
            term[i] = t
    # terminals in key order
    tk, tl, tv, tc = [], [], [], []
    for i in range(nl):
        if term[i][0] != 255:
            tk.append(lkeys[i]); tl.append(term[i][0]); tv.append(params.f[term[i][1]]); tc.append(term[i][2])
    nt = len(tk)
    # first new depth of every terminal, offsets
    d0 = [0] * nt
    for j in range(1, nt):
        x = tk[j] ^ tk[j - 1]
        d0[j] = DEPTH - (x.bit_length() - 1) // 3
    off = [0] * (nt + 1)
    for j in range(nt):
        off[j + 1] = off[j] + (DEPTH - tl[j]) - d0[j] + 1
    val = [None] * off[nt]
    col = [None] * off[nt]
    msk = [0] * off[nt]
    for j in range(nt):
        D = DEPTH - tl[j]
        val[off[j] + D - d0[j]] = tv[j]
        col[off[j] + D - d0[j]] = tc[j]
    for d in range(DEPTH - 1, -1, -1):
        sh = 3 * (DEPTH - 1 - d)
        for j in range(nt):
            if not (d0[j] <= d < DEPTH - tl[j]):
                continue
            prefix = tk[j] >> (sh + 3)
            v, cs, m = None, [], 0
            for c in range(8):
                lo = ((prefix << 3) | c) << sh
                q = bisect_left(tk, lo, j)
                if q < nt and tk[q] < lo + (1 << sh):
                    at = off[q] + (d + 1 - d0[q])
                    m |= 1 << c
                    v = val[at] if v is None else max(v, val[at])
                    cs.append(col[at])
            at = off[j] + d - d0[j]
            val[at], col[at], msk[at] = v, _avg(cs), m
    out = bytearray()
    for a in range(off[nt]):
        out += np.float32(val[a]).tobytes() + bytes([col[a][0], col[a][1], col[a][2], msk[a]])
    stats["nodes"] = off[nt]
    stats["bytes"] = len(out)
    stats["leaves_depth16"] = sum(1 for t in tl if t == 0)
    stats["pruned_leaves"] = sum(1 for t in tl if t != 0)
    return bytes(out), stats


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded scenes
# ---------------------------------------------------------------------------------------------------------------------------------
def scene_elevation(L, res, kind, seed=0):
    """Heights of an L x L map with 1 - 2 cm of noise.  'rolling': a smooth surface.  'steps': plateaus 0.6 m apart, the half of the
    map with column index >= L / 2 raised by 0.1 m.  Where a surface runs along the boundary between the two layers of a 2 x 2 x 2
    block of tree leaves the noise fills both layers, which is what makes full blocks (and prunes, once the leaves saturate) on a
    height map; the boundaries that qualify are the ODD multiples of the tree's resolution, so the plateaus at 0.6 k serve a 0.2 m
    tree and the raised ones at 0.6 k + 0.1 a 0.1 m tree."""
    rng = np.random.default_rng(seed)
    u = (0.5 * L - 0.5 - np.arange(L, dtype=np.float64)) * res
    X, Y = np.meshgrid(u, u, indexing="xy")
    if kind == "rolling":
        return 0.4 * np.sin(X * 0.9) * np.cos(Y * 0.7) + rng.normal(0.0, 0.02, X.shape)
    Z = 0.6 * np.floor((X + Y * 0.35) / 1.7) + rng.normal(0.0, 0.01, X.shape)
    Z[:, L // 2:] += 0.1
    return Z


def lattice_scene(L, res, kind, seed=0):
    """a capture-like cloud: one record per cell of scene_elevation's map on the lattice of a map centred at 0, row-major"""
    rng = np.random.default_rng(seed + 1000)
    u = (0.5 * L - 0.5 - np.arange(L, dtype=np.float64)) * res
    X, Y = np.meshgrid(u, u, indexing="xy")
    Z = scene_elevation(L, res, kind, seed)
    rgb = rng.integers(0, 255, size=(L * L, 3), dtype=np.uint8)
    return make_cloud(np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1), rgb)


def dense_block(levels, res, hits=2, seed=0, base=(3, -5, 2), extra=0):
    """`hits` rounds over one aligned block of 8^levels leaves, every round hitting every leaf once in a seeded order (the block
    collapses at the end of a round and the next round's first point expands it), with `extra` points elsewhere merged in"""
    rng = np.random.default_rng(seed)
    side = 2 ** levels
    b = np.array(base, dtype=np.int64) * side
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 3)
    pts = np.concatenate([g[rng.permutation(len(g))] for _ in range(hits)])
    xyz = (pts + b + 0.5) * res
    if extra:
        other = rng.uniform(-4.0, 4.0, size=(extra, 3))
        where = np.zeros(len(xyz) + extra, dtype=bool)
        where[rng.choice(len(where), size=extra, replace=False)] = True
        merged = np.empty((len(where), 3))
        merged[where], merged[~where] = other, xyz
        xyz = merged
    rgb = rng.integers(0, 255, size=(len(xyz), 3), dtype=np.uint8)
    return make_cloud(xyz, rgb)
