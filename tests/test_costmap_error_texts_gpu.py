"""The texts of the costmap family's shared failures (gem_last_error), byte for byte: the lookup of a costmap that is not there, through one
entry point of each translation unit (gem_capi_costmap / _inflate / _footprint / _mapgrid / _critics / _navplan / _frontier .cpp), and the
read-backs of a plan and of a frontier search before either was made, on a 4 x 4 costmap.  The codes are the other tests'."""
import ctypes as C

import pytest

from gem_amd import ElevationMap, _lib

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]
INV = _lib.GEM_OK - 1


def test_the_shared_failures_keep_their_texts():
    m = ElevationMap(32, 0.05)
    lib, h = m._lib, m._h
    st = _lib.NavplanStatus()
    lookups = {                                                          # id 7: inside 0 .. 7, never created on this handle
        "gem_costmap_reset": lambda: lib.gem_costmap_reset(h, 7),
        "gem_costmap_reset_window": lambda: lib.gem_costmap_reset_window(h, 7, 0, 0, 1, 1),
        "gem_costmap_footprint_cost": lambda: lib.gem_costmap_footprint_cost(h, 7, None, 0, None, 0, 0, None),
        "gem_costmap_mapgrid_read_front": lambda: lib.gem_costmap_mapgrid_read_front(h, 7, None, None, None),
        "gem_costmap_best_trajectory": lambda: lib.gem_costmap_best_trajectory(h, 7, None, 0, None, None, 0, 1, None, 0, None, 0, None, None),
        "gem_costmap_navplan_status": lambda: lib.gem_costmap_navplan_status(h, 7, C.byref(st)),
        "gem_costmap_frontiers_read": lambda: lib.gem_costmap_frontiers_read(h, 7, None, 0, None),
    }
    try:
        for name, call in lookups.items():
            assert call() == INV, name
            assert lib.gem_last_error(h).decode() == f"{name}: no such costmap"
        dev = m.costmap(4, 4, 0.05, 0.0, 0.0, 0)
        try:
            assert lib.gem_costmap_navplan_read(h, dev.id, None, None, 0) == INV
            assert lib.gem_last_error(h).decode() == "gem_costmap_navplan_read: no plan was made"
            assert lib.gem_costmap_frontiers_read(h, dev.id, None, 0, None) == INV
            assert lib.gem_last_error(h).decode() == "gem_costmap_frontiers_read: no search was made, or a plan was made since"
        finally:
            dev.close()
    finally:
        m.close()
