"""numpy / dict restatement of the rolling-window local map (ElevationMapping::updateLocalMap, EMg.cpp:609-767; visualPointMap,
:520-530), the semantics include/gem_hip.h pins for gem_local_*.  Driven from OracleMap.show()'s `visual` output and its geometry;
the local map is a Python dict keyed by the float pair ((float) x, (float) y): `del d[k]; d[k] = v` is the reference's erase +
insert, and the dict's order is the device's export order (last write).  Python floats compare -0.0 == 0.0 and hash them alike.

The reference hashes GridPoint by its bit pattern, so under libstdc++ -0.0 and +0.0 would be two keys there; the device (local_key)
and this restatement take them as one.  A capture's positions are never -0.0, so no result depends on it.

spill() / export() over a dict are the definition.  LocalMap + spill_fast() are the same map on arrays (the key as its float bits,
-0.0 as +0.0; the positions of a capture are finite), fast enough for node-sized maps; tests/test_vectorised_refs_cpu.py pins the two
forms to identical bytes."""
import numpy as np

# PointXYZRGBICT (include/gem/gem.hpp:40)
POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1"),
                  ("covariance", "<f4"), ("intensity", "<f4"), ("travers", "<f4")])


class Capture:
    """visualMap_ as map_.show() leaves it: the kept cells' records in grid_map's iteration order, their linear indices, the geometry."""

    def __init__(self, rec, lin, L, map_length, resolution, position, start):
        self.rec, self.lin, self.L = rec, lin, int(L)
        self.res = float(resolution)
        self.off = 0.5 * float(map_length) - 0.5 * self.res
        self.px, self.py = float(position[0]), float(position[1])
        self.sx, self.sy = int(start[0]), int(start[1])

    def positions(self):
        """grid_map's getPositionFromIndex in double (the formula of k_show_emit): (p + off) - res * unwrapped index."""
        ix, iy = self.lin % self.L, self.lin // self.L
        ux, uy = (ix - self.sx) % self.L, (iy - self.sy) % self.L
        x = (self.px + self.off) + self.res * (-ux).astype(np.float64)
        y = (self.py + self.off) + self.res * (-uy).astype(np.float64)
        return x, y


def capture(show_out, L, map_length, resolution, position, start) -> Capture:
    """show_out: OracleMap.show()'s dict; the geometry it was called with; start = the map's start index at that time."""
    v = np.asarray(show_out["visual"], np.float32).reshape(9, L * L)      # elevation variance rough slope traver r g b intensity
    lin = np.flatnonzero(~np.isnan(v[4]))                                  # kept cells hold their traversability, the others NaN
    cap = Capture(None, lin, L, map_length, resolution, position, start)
    x, y = cap.positions()
    rec = np.zeros(lin.size, POINT)
    rec["x"], rec["y"], rec["z"], rec["pad"] = x.astype(np.float32), y.astype(np.float32), v[0][lin], 1.0
    for f, l in (("r", 5), ("g", 6), ("b", 7)):
        rec[f] = v[l][lin].astype(np.int32).astype(np.uint8)                 # float -> int -> uint8, as k_show_emit
    rec["covariance"], rec["intensity"], rec["travers"] = v[1][lin], v[8][lin], v[4][lin]
    cap.rec = rec
    return cap


def grid_cloud(cap: Capture) -> np.ndarray:
    """gridMaptoPointCloud (EMg.cpp:1198-1224)."""
    return cap.rec.copy()


def spill_mask(prev: Capture, current_position, position_shift) -> np.ndarray:
    """The selection of EMg.cpp:724-733 over the previous capture's records."""
    cx, cy = float(np.float32(current_position[0])), float(np.float32(current_position[1]))
    dx, dy = np.float32(position_shift[0]), np.float32(position_shift[1])
    half = prev.L * prev.res / 2                                           # length_ * resolution_ / 2, double
    x, y = prev.positions()
    lo_x, hi_x, lo_y, hi_y = cx - half, cx + half, cy - half, cy + half
    sel = (((x < lo_x) | (y < lo_y)) & bool(dx > 0 and dy > 0)) \
        | (((x > hi_x) | (y > hi_y)) & bool(dx < 0 and dy < 0)) \
        | (((x < lo_x) | (y > hi_y)) & bool(dx > 0 and dy < 0)) \
        | (((x > hi_x) | (y < lo_y)) & bool(dx < 0 and dy > 0)) \
        | ((x < lo_x) & bool(dx > 0 and dy == 0)) \
        | ((x > hi_x) & bool(dx < 0 and dy == 0)) \
        | ((y < lo_y) & bool(dy > 0 and dx == 0)) \
        | ((y > hi_y) & bool(dy < 0 and dx == 0))
    return sel & (prev.rec["travers"].astype(np.float64) >= 0.0)          # elevation != -10 holds for every captured cell


def spill(prev: Capture, current_position, position_shift, local: dict):
    """The body of the "Local mapping" block (EMg.cpp:715-764): (records pushed to visualCloud_, count of replaced keys)."""
    out = prev.rec[spill_mask(prev, current_position, position_shift)].copy()
    replaced = 0
    for r in out:
        key = (float(r["x"]), float(r["y"]))
        if key in local:
            del local[key]                                                 # erase + insert: the key moves to the end
            replaced += 1
        local[key] = r.tobytes()
    return out, replaced


def export(local: dict) -> np.ndarray:
    """localHashtoPointCloud (EMg.cpp:1124-1140) in the device's order: last write."""
    return np.frombuffer(b"".join(local.values()), POINT).copy() if local else np.zeros(0, POINT)


def key_bits(x, y) -> np.ndarray:
    """the key of (x, y) as local_key builds it: x's float bits | y's << 32, -0.0 taken as +0.0"""
    x = np.where(np.asarray(x, np.float32) == 0, np.float32(0), x).astype(np.float32)
    y = np.where(np.asarray(y, np.float32) == 0, np.float32(0), y).astype(np.float32)
    return x.view(np.uint32).astype(np.uint64) | (y.view(np.uint32).astype(np.uint64) << np.uint64(32))


class LocalMap:
    """The local map of spill() on arrays: the live records in last-write order and their keys."""

    def __init__(self):
        self.rec, self.key = np.zeros(0, POINT), np.zeros(0, np.uint64)

    def __len__(self):
        return int(self.key.size)

    def clear(self):
        self.__init__()


def spill_fast(prev: Capture, current_position, position_shift, local: LocalMap):
    """spill() on a LocalMap: the last record of a key within the spill is its write, every key the spill writes moves to the end in
    the order of those last records, and the replaced count is the records minus the keys the map did not hold."""
    out = prev.rec[spill_mask(prev, current_position, position_shift)].copy()
    n = out.size
    if n == 0:
        return out, 0
    k = key_bits(out["x"], out["y"])
    uniq, first_rev = np.unique(k[::-1], return_index=True)               # first in reverse = last in order
    last = np.sort(n - 1 - first_rev)
    added = int(np.count_nonzero(~np.isin(uniq, local.key, assume_unique=True)))
    stay = ~np.isin(local.key, uniq, assume_unique=True)
    local.rec = np.concatenate([local.rec[stay], out[last]])
    local.key = np.concatenate([local.key[stay], k[last]])
    return out, n - added


def export_fast(local: LocalMap) -> np.ndarray:
    return local.rec.copy()
