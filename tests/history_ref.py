"""numpy restatement of the history cloud (visualCloud_ of ElevationMapping: EMg.cpp:750-760 push_back, :788 clear, :894-897 rebuild,
:524-526 visualPointMap), the semantics include/gem_hip_history.h pins for gem_history_* and gem_costmap_mark_history.

The history is a plain list of records.  Its box table and the culling rule are stated here once more, independently of the device
code; the mark itself is costmap_ref.mark_points over the whole list, which knows nothing of blocks: that culled blocks change neither
the grid nor the bounds is what the tests establish."""
import numpy as np

import costmap_ref
from local_ref import POINT

BLOCK = 4096                                                 # records per block (kCostChunk: the inputs of one mark workgroup)
EMPTY_BOX = (np.inf, np.inf, -np.inf, -np.inf)


class History:
    """visualCloud_: records in history order"""

    def __init__(self):
        self.rec = np.zeros(0, POINT)

    def append(self, points):                                # visualCloud_.push_back(pt), one spill or one caller's cloud
        self.rec = np.concatenate([self.rec, np.asarray(points, POINT)])

    def reset_from(self, submaps):                           # visualCloud_.clear(); visualCloud_ += globalMap_[i] for every i
        self.rec = np.concatenate([np.zeros(0, POINT)] + [np.asarray(s, POINT) for s in submaps])

    def clear(self):
        self.rec = np.zeros(0, POINT)

    def export(self, grid_cloud=None):                       # savingMap | visualPointMap: visualCloud_ + grid_pc
        return self.rec.copy() if grid_cloud is None else np.concatenate([self.rec, np.asarray(grid_cloud, POINT)])

    def __len__(self):
        return int(self.rec.shape[0])


def n_blocks(n):
    return (int(n) + BLOCK - 1) // BLOCK


def box_of(x, y):
    """{min_x, min_y, max_x, max_y} as float32 over one block's coordinates: NaN ignored (fminf / fmaxf), +-inf taking part, a block
    without a coordinate {+inf, +inf, -inf, -inf}.  Literal fold, one record at a time."""
    b = [np.float32(v) for v in EMPTY_BOX]
    for vx, vy in zip(np.asarray(x, np.float32), np.asarray(y, np.float32)):
        if not np.isnan(vx):
            b[0], b[2] = min(b[0], vx), max(b[2], vx)
        if not np.isnan(vy):
            b[1], b[3] = min(b[1], vy), max(b[3], vy)
    return tuple(float(v) for v in b)


def boxes(rec):
    """the table of a log: [n_blocks, 4] float32; block b covers records [4096 b, min(4096 (b + 1), len))"""
    n = rec.shape[0]
    out = np.empty((n_blocks(n), 4), np.float32)
    inf = np.float32(np.inf)
    for b in range(out.shape[0]):
        x, y = rec["x"][b * BLOCK:(b + 1) * BLOCK], rec["y"][b * BLOCK:(b + 1) * BLOCK]
        out[b] = (np.fmin.reduce(x, initial=inf), np.fmin.reduce(y, initial=inf), np.fmax.reduce(x, initial=-inf), np.fmax.reduce(y, initial=-inf))
    return out


def cull_exact(cm):
    """the geometries for which the rule below is exact (and applied): the far limits resolve in double, |limit| <= 2^51 res"""
    lx, ly = cm.ox + (cm.size_x + 1) * cm.res, cm.oy + (cm.size_y + 1) * cm.res
    return abs(lx) <= cm.res * 2.0 ** 51 and abs(ly) <= cm.res * 2.0 ** 51


def culled(cm, box):
    """the rule, in double with the floats widened and the costmap's geometry after rolling: box = (min_x, min_y, max_x, max_y)"""
    min_x, min_y, max_x, max_y = (float(v) for v in box)
    return (not (max_x >= cm.ox) or not (max_y >= cm.oy) or not (min_x < cm.ox + (cm.size_x + 1) * cm.res)
            or not (min_y < cm.oy + (cm.size_y + 1) * cm.res))


def culled_blocks(cm, rec, cull=True):
    """[n_blocks] bool: the blocks a mark of `rec` skips"""
    t = boxes(rec)
    if not cull or not cull_exact(cm):
        return np.zeros(t.shape[0], bool)
    return np.array([culled(cm, t[b]) for b in range(t.shape[0])], bool)


def mark_history(cm, hist, thresh, bounds=None):
    """PointMapLayer::updateBounds over the history: costmap_ref.mark_points over every record, in order"""
    return costmap_ref.mark_points(cm, hist.rec, thresh, bounds)
