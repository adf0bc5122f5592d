#!/usr/bin/env python3
"""Randomised soak of the device costmap family: random chains of gem_amd.api.Costmap operations on two to four costmaps of one
handle, every step compared exactly with the chained numpy references of tests/*_ref.py (test infrastructure: this tool is a test, not
the product).  What single-feature tests cannot reach is what lives BETWEEN calls: the scratch arenas all of a handle's costmaps share
(a small map runs in what a large one left), the cached inflation table, the two grids a roll flips between, the generation numbers that
decide what is refused as stale, and the id a destroyed map hands to the next one.

    python tools/fuzz_costmap.py [--seconds 60] [--seed 2] [--backend device|reference|host] [--profile base|full]
Prints one line per scenario and a final summary; exit code 1 on the first mismatch (seed, step, op and arguments are printed, and
`scenario(seed, profile=...)` reproduces it alone).

Two profiles.  "base" draws from OPS and GEOMS: the costmap family as it was when the soak was written, and exactly the scenarios it
drew then (tests/test_fuzz_costmap_cpu.py, tests/test_fuzz_costmap_gpu.py).  "full" draws from FULL_OPS and FULL_GEOMS: the same ops and
besides them the voxel layer (attach_voxels, detach_voxels, write_voxels, read_voxels, voxel_observe), the tiled MapGrid
(prepare_map_grid_tiled, prepare_map_grid_front_tiled), rollout_best and dwa_best, on the same maps and on 513 x 66, 70 x 520 and
1 x 4100 (tests/test_fuzz_costmap_full_cpu.py, tests/test_fuzz_costmap_full_gpu.py).  Its random stream is another one: a seed's full
scenario is not its base scenario with ops added.

The model.  Per device costmap the scenario keeps a costmap_ref.Costmap (grid and origin) and what the ABI promises beyond the grid:
the last plan (potential, path cells, status) and whether it is fresh, the last search and whether it is fresh, the three MapGrid
grids and whether each is fresh.  The freshness rules are those of the headers:
  - a roll that moves the map makes plans, searches and grids stale (gem_hip_navplan.h, gem_hip_frontier.h, gem_hip_mapgrid.h,
    gem_hip_critics.h);
  - an observe call with at least one observation does the same (gem_hip_obstacle.h: "An observe call counts as a change of the grid");
  - creating the map anew does (the same three headers);
  - a new plan invalidates the last search, another goal on the plan's potential keeps it (gem_hip_frontier.h);
  - marks, writes, merges, inflation and resets leave everything as it is: keeping grid and plan consistent is the caller's business.
A finding about the headers themselves: gem_hip_navplan.h, gem_hip_frontier.h, gem_hip_mapgrid.h and gem_hip_critics.h name the roll
and the re-creation only; that an observe call makes their results stale too is said in gem_hip_obstacle.h alone.  They do not
contradict each other, and the model follows the union.
Reads are issued whatever the model says: a stale or missing result must be refused (GemError, and through the C entry the caller's
buffer untouched), a fresh one must equal the reference result computed WHEN THE PLAN / SEARCH / GRID WAS MADE -- not one recomputed
from the current grid, because marks after a plan do not invalidate it.

The full profile's model adds the rules of gem_hip_voxlayer.h, gem_hip_mapgrid_tiled.h, gem_hip_rollout.h and gem_hip_trajgen.h:
  - a fresh attach is all UNKNOWN_COLUMN; reset makes every column unknown; reset_window, write, merge, inflate, clear_footprint, marks
    and the 2-D observe leave the columns alone; a roll that moves the map moves the columns by the same overlap rule and fills the rest
    with unknown; a map created anew has no voxels, whatever the map had whose id it took;
  - voxel_observe with at least one observation makes plans, searches and grids stale, as observe does; with none it changes nothing;
  - every voxel entry on a map without voxels, and attach_voxels on a map that has them, is refused (through the C read entry with the
    caller's buffer untouched);
  - the tiled prepares write the slots, status words and generation of the capped ones: a capped PATH followed by a tiled GOAL leaves
    both fresh, either may be read, scored or handed to best_trajectory, dwa_best and rollout_best;
  - the capped prepares refuse a map above their cap with nothing changed: a grid the tiled form left fresh stays readable and equal;
  - rollout_best needs PATH and GOAL fresh and dwa_best every grid its critics name: issued whatever the model says, refused when stale
    or missing with the prefilled outputs untouched, answered from the bytes AS THEY ARE and the grids AS THEY WERE PREPARED.
Findings about the headers, resolved by the code.  (1) "512 x 512" in gem_hip_mapgrid.h is an example: the capped prepare's cap is
ceil(size_x / 64) * size_y <= GEM_MAPGRID_MAX_WORDS, so 513 x 66 (594 words) and 70 x 520 (1040) are ACCEPTED by it and both forms are
drawn there; only 1 x 4100 (4100 words), added for the purpose, is refused.  (2) gem_hip_mapgrid.h's list of refusals named the roll
and the re-creation only, gem_hip_voxlayer.h and gem_hip_rollout.h "rolled or was observed": the code takes a new generation in both
observe entries (gem_capi_obstacle.cpp, gem_capi_voxlayer.cpp), and gem_hip_mapgrid.h, gem_hip_critics.h, gem_hip_navplan.h and
gem_hip_frontier.h now say so.  (3) gem_hip_trajgen.h says nothing about staleness of its own: dwa_best's grids pass
gem_costmap_best_trajectory's test (gem_hip_critics.h), which is what the model applies.

Compared after every step: the whole grid of the map that was touched (both maps of a merge) by tobytes() and its origin by ==; bounds,
potentials, path cells, status integers, frontier records, distances, scores and the winner by ==.  Every fifth step and at the end all
maps of the handle are compared: an op on map A must not have touched map B.  On a map with voxels the whole column grid is compared
by tobytes() wherever the bytes are; voxel_observe's bounds by ==; the tiled prepares' distances, started and goal cell (rounds depends
on timing and is not compared); the rollout's 64 answer bytes, costs and ahead, DWA's totals and winner by their bytes.  There are no
tolerances.

Left out, because they need elevation-side state (a capture, a submap stack, a history log) that this scenario does not build:
mark_grid_cloud, mark_visual, mark_global and mark_history.  backend="reference" drives the model alone:
tests/test_fuzz_costmap_cpu.py and tests/test_fuzz_costmap_full_cpu.py use it to assert, without a GPU, that the committed seeds cover
what the soak is meant to cover.  backend="host" is the same and besides compares, along the chain, the library's host twins that the
Python module binds (gem_navplan_host, gem_frontiers_host, gem_obstacle_host, gem_inflation_table; in the full profile also
gem_voxlayer_host, gem_rollout_plan / gem_rollout_host and gem_trajgen_plan / gem_trajgen_generate) with the model: the model's own
code is exercised against the library before any GPU visit.
"""
import argparse
import ctypes as C
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import costmap_ref as cref  # noqa: E402
import critics_ref as cr  # noqa: E402
import footprint_ref as fref  # noqa: E402
import frontier_ref as frref  # noqa: E402
import inflate_ref as iref  # noqa: E402
import mapgrid_ref as mref  # noqa: E402
import navplan_ref as nref  # noqa: E402
import obstacle_ref as oref  # noqa: E402
import rollout_ref as rref  # noqa: E402
import trajgen_ref as tref  # noqa: E402
import voxlayer_ref as vref  # noqa: E402

F32 = np.float32
# name -> (size_x, size_y).  kNavTile = 64: 63, 64, 65 and 129 wide or high; kCostLdsCells = 8192: 90 x 91 = 8190 below, 91 x 91 = 8281
# above; a strip, a 1 x N map; the largest about 130 x 129
GEOMS = {"63x64": (63, 64), "64x64": (64, 64), "65x65": (65, 65), "129x63": (129, 63), "40x129": (40, 129), "90x91": (90, 91),
         "91x91": (91, 91), "130x129": (130, 129), "65x3": (65, 3), "1x70": (1, 70)}
LARGE = ["129x63", "90x91", "91x91", "130x129", "130x129"]
SMALL = ["63x64", "64x64", "65x65", "40x129", "65x3", "1x70", "65x3"]
RESOLUTIONS = [0.05, 0.1, 0.2]
EMPTY_BOUNDS = [1e30, 1e30, -1e30, -1e30]
DEBUG_DEFAULTS = {"nav_chunk": 0, "front_chunk": 0, "obstacle_direct": 1}
SLOTS = (mref.PATH, mref.GOAL, cr.GRID_FRONT)
ARENA_OPS = ("inflate", "observe", "frontiers", "nav_plan")          # the ops whose scratch comes from arenas all of a handle's costmaps share
# op -> weight of a free draw (a maker is besides followed by its reads, an arena op by the same op on a smaller map: next_op)
OPS = {"write": 3, "write_window": 3, "reset": 3, "reset_window": 4, "roll": 7, "mark_points": 5, "observe": 7, "clear_footprint": 3,
       "merge": 4, "inflate": 7, "footprint_cost": 3, "score_trajectories": 3, "prepare_map_grid": 7, "prepare_map_grid_front": 4,
       "read_map_grid": 4, "score_map_grid": 3, "nav_plan": 9, "read_potential": 4, "nav_plan_to": 3, "frontiers": 6, "read_frontiers": 4,
       "best_trajectory": 4, "recreate": 3}

# ---- the full profile: tables of its own (tests/test_fuzz_costmap_cpu.py asserts that the base seeds see all of GEOMS and of OPS) ----------
# GEOMS plus two maps past 512 cells in one direction each -- nine tiles across with a seam at 64 / 65 the other way, and the transpose --
# kept narrow so that the numpy references stay fast.  A finding: the capped prepare's limit is not a side of 512 but
# ceil(size_x / 64) * size_y <= GEM_MAPGRID_MAX_WORDS = 4096 (gem_hip_mapgrid.h says so; "512 x 512" is its example), so both of these
# are ACCEPTED by gem_costmap_mapgrid_prepare, and both forms are drawn on them.  The third, 1 x 4100, is the cheapest map that is above
# the cap (one word a row, 4100 rows): there the capped entries must be refused.
FULL_GEOMS = dict(GEOMS, **{"513x66": (513, 66), "70x520": (70, 520), "1x4100": (1, 4100)})
LONG = ["513x66", "70x520", "1x4100"]
FULL_LARGE = LARGE + ["513x66", "70x520", "513x66", "70x520", "1x4100", "1x4100"]
FULL_DEBUG_DEFAULTS = dict(DEBUG_DEFAULTS, mapgrid_chunk=0)
FULL_ARENA_OPS = ARENA_OPS + ("voxel_observe", "prepare_map_grid_tiled", "dwa_best", "rollout_best")
PLANNER_OPS = ("dwa_best", "rollout_best")                             # their arenas are sized by trajectories / candidates, not by cells
# the references of nav_plan and frontiers walk every cell in Python: on a LONG map such a draw is moved to another map of the handle
# with probability LONG_AWAY (the maps stay; the ops still occur there)
HEAVY_ON_LONG, LONG_AWAY = ("nav_plan", "frontiers"), 0.7
# OPS with its weights, and the new ops: voxel_observe heaviest (its shares need calls on columns with a history), the planners light
# because they also follow the prepares, the stale events and their own echoes (next_op_full)
FULL_OPS = dict(OPS, attach_voxels=4, detach_voxels=2, write_voxels=4, read_voxels=4, voxel_observe=20, prepare_map_grid_tiled=9,
                prepare_map_grid_front_tiled=4, rollout_best=6, dwa_best=5)
VOXEL_OPS = ("attach_voxels", "detach_voxels", "write_voxels", "read_voxels", "voxel_observe")
MAPGRID_MAX_WORDS = 4096


def capped_fits(cm):
    """gem_costmap_mapgrid_prepare's cap: the bit plane of the map, rows padded to words of 64 cells, in one workgroup's LDS"""
    return -(-cm.size_x // 64) * cm.size_y <= MAPGRID_MAX_WORDS


def rolled(a, cell_ox, cell_oy, fill):
    """Costmap2D::updateOrigin's copy: out(x, y) = a(x + cell_ox, y + cell_oy) where that lies in the map, fill elsewhere"""
    sy, sx = a.shape
    out = np.full_like(a, fill)
    x0, x1, y0, y1 = max(0, -cell_ox), min(sx, sx - cell_ox), max(0, -cell_oy), min(sy, sy - cell_oy)
    if x1 > x0 and y1 > y0:
        out[y0:y1, x0:x1] = a[y0 + cell_oy:y1 + cell_oy, x0 + cell_ox:x1 + cell_ox]
    return out


class Map:
    """one costmap: the device object (None with the reference backend), the reference grid and the model beyond the grid"""

    def __init__(self, role, geom, res, origin, default):
        self.role, self.geom = role, geom
        sx, sy = FULL_GEOMS[geom]
        self.cm = cref.Costmap(sx, sy, res, origin[0], origin[1], default)
        self.dev = None
        self.vox = self.cols = None      # full profile: a voxlayer_ref.Voxels and the columns uint32 [size_y, size_x]; None without voxels
        self.missing = "never"           # why a result that is None is none: never made, or lost in a re-creation
        self.forget()

    def forget(self):
        self.plan = None                 # {"pot", "cells", "found", "n_path", "goal_potential", "start_cell", "goal_cell", "start", "fresh"}
        self.search = None               # frontier_ref.search's dict + "fresh"
        self.grids = {s: None for s in SLOTS}       # slot -> {"dist", "started", "goal_cell", "fresh"}
        self.infl_key = None

    def stale(self, cause=None):
        for r in [self.plan, self.search] + list(self.grids.values()):
            if r is not None:
                if r["fresh"]:
                    r["cause"] = cause
                r["fresh"] = False

    @property
    def cells(self):
        return self.cm.size_x * self.cm.size_y

    def name(self):
        return f"{self.role}:{self.geom}@{self.cm.res}"


def is_fresh(r):
    return r is not None and r["fresh"]


class Scenario:
    def __init__(self, seed, backend, profile="base"):
        assert profile in ("base", "full"), profile
        self.seed, self.backend, self.device = seed, backend, backend == "device"
        self.full = profile == "full"
        self.rng = np.random.default_rng([seed, 0xC057] if not self.full else [seed, 0xC057, 0xF011])
        self.small_next = False                                          # full profile: the echo of a planner draws a smaller set
        self.probe_next = self.stale_probe = False                       # full profile: the next planner call finds its grids as they are
        self.trace, self.maps, self.follow, self.echo = [], [], None, None
        self.emap = self.lib = self.h = None
        self.GemError = RuntimeError
        self.host = backend == "host"                                    # the model, and the library's host twins chained beside it (no device)
        if self.device or self.host:
            import gem_amd
            self.gem = gem_amd
        if self.device:
            self.emap = gem_amd.ElevationMap(32, 0.05)
            self.lib, self.h, self.GemError = self.emap._lib, self.emap._h, gem_amd.GemError

    # ---- drawing -------------------------------------------------------------------------------------------------------------------
    def pick(self, seq):
        return seq[int(self.rng.integers(len(seq)))]

    def chance(self, p):
        return bool(self.rng.random() < p)

    def origin(self):
        return (float(self.rng.uniform(-4.0, 4.0)) + 0.0137, float(self.rng.uniform(-4.0, 4.0)) - 0.0291)     # no multiple of a resolution

    def window(self, cm):
        if self.chance(0.3):
            return None
        x0, y0 = int(self.rng.integers(0, cm.size_x)), int(self.rng.integers(0, cm.size_y))
        x1, y1 = int(self.rng.integers(x0 + 1, cm.size_x + 1)), int(self.rng.integers(y0 + 1, cm.size_y + 1))
        return (x0, y0, x1, y1)

    def scene(self, cm):
        """a grid with free space to plan through, lethal cells to inflate and clear, and unknown space to have frontiers against"""
        sx, sy, rng = cm.size_x, cm.size_y, self.rng
        g = np.zeros((sy, sx), np.uint8)
        hit = rng.random((sy, sx)) < 0.10
        g[hit] = rng.integers(1, 253, int(hit.sum()), dtype=np.uint8)
        g[rng.random((sy, sx)) < 0.04] = 254
        g[rng.random((sy, sx)) < 0.01] = 253
        kind = int(rng.integers(3))
        if kind < 2:                                                     # known inside a ragged blob, unknown outside
            yy, xx = np.mgrid[0:sy, 0:sx]
            cx, cy = rng.uniform(0.2, 0.8) * sx, rng.uniform(0.2, 0.8) * sy
            rad = rng.uniform(0.35, 0.8) * max(sx, sy)
            ang = np.arctan2(yy - cy, xx - cx)
            g[(xx - cx) ** 2 + (yy - cy) ** 2 > (rad * (1.0 + 0.2 * np.sin(5 * ang))) ** 2] = 255
        else:
            g[rng.random((sy, sx)) < 0.08] = 255
        return g

    def world(self, cm, cell, frac=(0.5, 0.5)):
        return (cm.ox + (cell[0] + frac[0]) * cm.res, cm.oy + (cell[1] + frac[1]) * cm.res)

    def some_cell(self, cm, want=None):
        """a random cell; with `want` (a bool grid) one of its cells where there is any within a few draws"""
        for _ in range(12):
            c = (int(self.rng.integers(cm.size_x)), int(self.rng.integers(cm.size_y)))
            if want is None or want[c[1], c[0]]:
                break
        return c

    def off_map_point(self, cm):
        side = int(self.rng.integers(4))
        x, y = self.world(cm, (cm.size_x // 2, cm.size_y // 2))
        ext_x, ext_y = cm.size_x * cm.res, cm.size_y * cm.res
        return [(cm.ox - 0.7 * cm.res, y), (cm.ox + ext_x + 0.7 * cm.res, y), (x, cm.oy - 0.7 * cm.res), (x, cm.oy + ext_y + 0.7 * cm.res)][side]

    def poses(self, cm, n):
        rng = self.rng
        ext_x, ext_y = cm.size_x * cm.res, cm.size_y * cm.res
        xyt = np.stack([cm.ox + rng.uniform(-0.08, 1.08, n) * ext_x, cm.oy + rng.uniform(-0.08, 1.08, n) * ext_y, rng.uniform(-math.pi, math.pi, n)], 1)
        return fref.poses_from_yaw(xyt)

    def spec(self, cm, allow_centre=False):
        r = cm.res
        opts = [[[-3 * r, -2 * r], [-3 * r, 2 * r], [3 * r, 2 * r], [3 * r, -2 * r]], [[-8 * r, -5 * r], [-8 * r, 5 * r], [8 * r, 5 * r], [8 * r, -5 * r]],
                fref.regular_polygon(5, 4.2 * r), [[-1.2 * r, -0.4 * r], [0.0, 1.3 * r], [1.4 * r, -0.6 * r]]]
        if allow_centre:
            opts.append([[0.0, 0.0], [r, 0.0]])
        k = int(self.rng.integers(len(opts)))
        return k, opts[k]

    # ---- the device side -----------------------------------------------------------------------------------------------------------
    def debug(self, key, value):
        if self.device:
            self.emap.debug_set(key, int(value))

    def create(self, mp):
        if self.device:
            cm = mp.cm
            mp.dev = self.emap.costmap(cm.size_x, cm.size_y, cm.res, cm.ox, cm.oy, cm.default)

    def same_grid(self, mp, what=""):
        if not self.device:
            return
        got = mp.dev.read()
        geo = mp.dev.geometry()
        assert (geo["origin_x"], geo["origin_y"]) == (mp.cm.ox, mp.cm.oy), f"{what}{mp.name()}: origin {(geo['origin_x'], geo['origin_y'])}, want {(mp.cm.ox, mp.cm.oy)}"
        if got.tobytes() != mp.cm.grid.tobytes():
            bad = np.flatnonzero(got.reshape(-1) != mp.cm.grid.reshape(-1))
            raise AssertionError(f"{what}{mp.name()}: {bad.size} cells differ, first {bad[:6].tolist()}, device {got.reshape(-1)[bad[:6]].tolist()} "
                                 f"reference {mp.cm.grid.reshape(-1)[bad[:6]].tolist()}")
        if mp.vox is not None:                                           # the voxel columns next to the bytes
            cols = mp.dev.read_voxels()
            if cols.tobytes() != mp.cols.tobytes():
                bad = np.flatnonzero(cols.reshape(-1) != mp.cols.reshape(-1))
                raise AssertionError(f"{what}{mp.name()}: {bad.size} voxel columns differ, first {bad[:6].tolist()}, device "
                                     f"{[hex(v) for v in cols.reshape(-1)[bad[:6]].tolist()]} reference {[hex(v) for v in mp.cols.reshape(-1)[bad[:6]].tolist()]}")

    def refused(self, fn, what):
        try:
            fn()
        except self.GemError:
            return
        raise AssertionError(f"{what}: the device answered where the model says stale or never made")

    def raw_refused(self, mp, entry, *head):
        """the C entry with the caller's buffer prefilled: refused, and the buffer as it was"""
        out = np.full((mp.cm.size_y, mp.cm.size_x), -7, np.int32)
        p = out.ctypes.data_as(C.c_void_p)
        started, goal = C.c_int(-7), (C.c_int * 2)(-7, -7)
        fn = getattr(self.lib, entry)
        if entry == "gem_costmap_navplan_read":
            rc = fn(self.h, mp.dev.id, p, None, 0)
        elif entry == "gem_costmap_frontiers_read":
            rc = fn(self.h, mp.dev.id, None, 0, p)
        elif entry == "gem_costmap_voxels_read":                         # (the buffer's words read as columns: the same size)
            rc = fn(self.h, mp.dev.id, 0, 0, mp.cm.size_x, mp.cm.size_y, p, mp.cm.size_x)
        else:
            rc = fn(self.h, mp.dev.id, *head, p, C.byref(started), goal)
        assert rc != 0, f"{entry}: answered {rc} where the model says stale or never made"
        assert (out == -7).all() and started.value == -7 and tuple(goal) == (-7, -7), f"{entry}: refused, but the caller's buffers were written"

    def to_device(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def log(self, mp, op, **info):
        self.trace.append(dict(step=self.step, map=mp.role, geom=mp.geom, cells=mp.cells, op=op, **info))

    # ---- ops: grid ------------------------------------------------------------------------------------------------------------------
    def op_write(self, mp):
        g = self.scene(mp.cm)
        self.log(mp, "write")
        mp.cm.grid[:] = g
        if self.device:
            mp.dev.write(g)

    def op_write_window(self, mp):
        w = self.window(mp.cm) or (0, 0, mp.cm.size_x, mp.cm.size_y)
        shape = (w[3] - w[1], w[2] - w[0])
        v = self.rng.choice(np.array([0, 0, 0, 0, 100, 252, 253, 254, 254, 255], np.uint8), shape)
        self.log(mp, "write_window", window=w)
        mp.cm.grid[w[1]:w[3], w[0]:w[2]] = v
        if self.device:
            mp.dev.write(v, w)

    def op_reset(self, mp):
        self.log(mp, "reset", **self.vox_info(mp))
        mp.cm.reset()
        if mp.cols is not None:
            mp.cols[:] = vref.UNKNOWN_COLUMN
        if self.device:
            mp.dev.reset()

    def op_reset_window(self, mp):
        w = self.window(mp.cm) or (0, 0, mp.cm.size_x, mp.cm.size_y)
        self.log(mp, "reset_window", window=w)
        iref.reset_window(mp.cm.grid, *w, mp.cm.default)
        if self.device:
            mp.dev.reset_window(*w)

    def op_roll(self, mp):
        cm, rng = mp.cm, self.rng
        kind = self.pick(["zero", "few", "few", "few", "negative", "negative", "far"])

        def step(size):
            if kind == "zero":
                return 0
            if kind == "far":
                return int(size + rng.integers(1, 4)) * (1 if self.chance(0.5) else -1)
            k = int(rng.integers(0, max(min(size, 9), 1)))                 # 0 .. 8 below the size: one axis may stand still
            return -k if kind == "negative" else k

        def frac(k):                                                     # truncation toward zero gives k back
            return k + 0.3 if k > 0 else (k - 0.3 if k < 0 else (0.3 if self.chance(0.5) else -0.3))
        kx, ky = step(cm.size_x), step(cm.size_y)
        new = (cm.ox + frac(kx) * cm.res, cm.oy + frac(ky) * cm.res)
        form = self.pick(["update_origin", "roll_to"])
        if form == "roll_to":
            mx, my = cm.size_in_meters()
            robot = (new[0] + mx / 2, new[1] + my / 2)
            moved = cref.origin_step(cm, robot[0] - mx / 2, robot[1] - my / 2)
        else:
            moved = cref.origin_step(cm, *new)
        self.log(mp, "roll", form=form, kind=kind, moved=moved, size=(cm.size_x, cm.size_y), **self.vox_info(mp))
        if form == "roll_to":
            cref.roll_to(cm, *robot)
        else:
            cref.update_origin(cm, *new)
        if moved != (0, 0):
            mp.stale("roll")
            if mp.cols is not None:                                      # the columns move with the bytes, the rest unknown
                mp.cols = rolled(mp.cols, moved[0], moved[1], vref.UNKNOWN_COLUMN)
        if self.device:
            mp.dev.roll_to(*robot) if form == "roll_to" else mp.dev.update_origin(*new)

    def op_mark_points(self, mp):
        cm, rng = mp.cm, self.rng
        n = int(self.pick([0, 1, 63, 64, 65, 500, 4097]))
        ext_x, ext_y = cm.size_x * cm.res, cm.size_y * cm.res
        pts = np.zeros(n, POINT_DTYPE)
        pts["x"] = (cm.ox + rng.uniform(-0.15, 1.15, n) * ext_x).astype(F32)
        pts["y"] = (cm.oy + rng.uniform(-0.15, 1.15, n) * ext_y).astype(F32)
        t = rng.uniform(0.2, 0.8, n)
        t[rng.random(n) < 0.04] = np.nan
        t[rng.random(n) < 0.03] = 0.5
        pts["travers"] = t.astype(F32)
        if n >= 63:                                                      # on the edges, off the map, not a number
            mid = self.world(cm, (cm.size_x // 2, cm.size_y // 2))
            special = [(cm.ox, cm.oy), (cm.ox + ext_x, mid[1]), (mid[0], cm.oy + ext_y), (cm.ox - 0.01, mid[1]), (mid[0], cm.oy - 0.01),
                       (np.nan, mid[1]), (mid[0], np.inf), (float(np.nextafter(F32(cm.ox), F32(-1e9))), mid[1])]
            at = rng.choice(n, len(special), replace=False)
            for i, (x, y) in zip(at, special):
                pts["x"][i], pts["y"][i] = x, y
        bounds = None if self.chance(0.5) else list(EMPTY_BOUNDS)
        on_device = self.chance(0.4)
        self.log(mp, "mark_points", n=n, bounds=bounds is not None, on_device=on_device)
        want = cref.mark_points(cm, pts, 0.5, None if bounds is None else list(bounds))
        if self.device:
            src = self.to_device(pts.view(np.uint8).reshape(-1, 32)) if on_device else pts
            got = mp.dev.mark_points(src, 0.5, None if bounds is None else list(bounds))
            assert got == want, f"bounds {got}, want {want}"

    def op_observe(self, mp):
        cm, rng = mp.cm, self.rng
        ext_x, ext_y = cm.size_x * cm.res, cm.size_y * cm.res
        reach = max(ext_x, ext_y)
        n_obs = int(self.pick([0, 1, 1, 1, 2, 2, 3]))
        width = int(self.pick([3, 4, 8]))
        obs, on_map = [], []
        for _ in range(n_obs):
            n = int(self.pick([0, 1, 63, 64, 65, 200, 500]))
            inside = self.chance(0.85)
            s = self.world(cm, self.some_cell(cm), (float(rng.uniform(0.05, 0.95)), float(rng.uniform(0.05, 0.95)))) if inside else self.off_map_point(cm)
            on_map.append(inside)
            a, r = rng.uniform(-math.pi, math.pi, n), rng.uniform(0.0, 1.3, n) * reach
            p = np.zeros((n, width), F32)
            p[:, 0], p[:, 1], p[:, 2] = s[0] + r * np.cos(a), s[1] + r * np.sin(a), rng.uniform(-0.2, 2.3, n)
            p[rng.random(n) < 0.02, 0] = np.nan
            mark, clear = self.pick([(True, True), (True, True), (False, True), (False, True), (True, False)])
            obs.append({"points": p, "origin": (s[0], s[1], float(rng.uniform(0.2, 1.5))), "marking": mark, "clearing": clear,
                        "raytrace_range": float(self.pick([0.3 * reach, 0.3 * reach, 3.0, math.inf])),
                        "obstacle_range": float(self.pick([2.5, 0.5 * reach, math.inf]))})
        layer_max = float(self.pick([2.0, 1.0, math.inf]))
        direct = int(rng.integers(2))
        bounds = None if self.chance(0.5) else list(EMPTY_BOUNDS)
        on_device = self.chance(0.4)
        before = cm.grid.copy()
        want = oref.observe(cm, obs, layer_max, None if bounds is None else list(bounds))
        if self.host:
            twin = before.copy()
            got = self.gem.obstacle_host(twin, cm.res, (cm.ox, cm.oy), obs, layer_max, None if bounds is None else list(bounds))
            assert got == want and twin.tobytes() == cm.grid.tobytes(), f"gem_obstacle_host: bounds {got}, want {want}; {int((twin != cm.grid).sum())} cells differ"
        self.log(mp, "observe", n_obs=n_obs, n=[len(o["points"]) for o in obs], on_map=on_map, direct=direct, on_device=on_device,
                 ranges=[o["raytrace_range"] for o in obs], flags=[(o["marking"], o["clearing"]) for o in obs], bounds=bounds is not None,
                 changed=bool((before != cm.grid).any()), cleared_lethal=bool(((before == 254) & (cm.grid != 254)).any()))
        if n_obs:
            mp.stale("observe")
        if self.device:
            self.debug("obstacle_direct", direct)
            dobs = [{**o, "points": self.to_device(o["points"])} for o in obs] if on_device else obs
            got = mp.dev.observe(dobs, layer_max, None if bounds is None else list(bounds))
            assert got == want, f"bounds {got}, want {want}"

    def op_clear_footprint(self, mp):
        cm = mp.cm
        pose = tuple(float(v) for v in self.poses(cm, 1)[0])
        k, spec = self.spec(cm)
        bounds = None if self.chance(0.5) else list(EMPTY_BOUNDS)
        self.log(mp, "clear_footprint", pose=pose, spec=k, bounds=bounds is not None)
        wb = None if bounds is None else list(bounds)
        ok = fref.clear_footprint(cm, pose, spec, wb)
        if self.device:
            got = mp.dev.clear_footprint(pose, spec, None if bounds is None else list(bounds))
            assert got == (ok, wb), f"(ok, bounds) {got}, want {(ok, wb)}"

    def op_merge(self, mp):
        layer, master = self.maps[0], self.maps[1]                       # the pair of one geometry
        w = self.window(layer.cm)
        mode = int(self.rng.integers(2))
        self.log(layer, "merge", window=w, mode=mode)
        cref.merge(layer.cm, master.cm, w or (0, 0, layer.cm.size_x, layer.cm.size_y), mode)
        if self.device:
            layer.dev.merge(master.dev, w, mode)
        return [layer, master]

    def op_inflate(self, mp):
        cm, r = mp.cm, mp.cm.res
        radii = self.pick([(3 * r - 0.05 * r, 2 * r + 0.05 * r), (3 * r - 0.05 * r, 2 * r + 0.05 * r), (5 * r, 1.2 * r)])
        p = iref.Params(radii[0], radii[1], float(self.pick([3.0, 10.0])), self.chance(0.5))
        again = float(self.rng.random())
        if mp.infl_key is not None and again < 0.7:                      # the cached table: the same key again, or only the factor changed
            p = iref.Params(mp.infl_key[0], mp.infl_key[1], mp.infl_key[2] if again < 0.35 else 13.0 - mp.infl_key[2], p.inflate_unknown)
        w = self.window(cm)
        key = tuple(p[:3])
        self.log(mp, "inflate", params=tuple(p), window=w, same_key=None if mp.infl_key is None else mp.infl_key == key,
                 seeds=int((cm.grid == 254).sum()))
        mp.infl_key = key
        if self.host:
            R, tab = self.gem.inflation_table(cm.res, *p[:3])
            assert (R, tab.tobytes()) == (iref.table(p, cm.res)[0], iref.table(p, cm.res)[1].tobytes()), "gem_inflation_table differs"
        cm.grid[:] = iref.inflate_exact(cm.grid, p, cm.res, w)
        if self.device:
            mp.dev.inflate(p.inflation_radius, p.inscribed_radius, p.cost_scaling_factor, p.inflate_unknown, w)
        self.follow = (mp, ["inflate", "inflate", "mark_points", "write_window"])     # the cached table meets the next key on the same map

    # ---- ops: footprints ------------------------------------------------------------------------------------------------------------
    def op_footprint_cost(self, mp):
        cm = mp.cm
        n = int(self.pick([1, 63, 64, 65, 200]))
        poses = self.poses(cm, n)
        k, spec = self.spec(cm, allow_centre=True)
        flags = int(self.rng.integers(2)) * fref.INSCRIBED_LETHAL
        on_device = self.chance(0.4)
        self.log(mp, "footprint_cost", n=n, spec=k, flags=flags, on_device=on_device)
        want = fref.footprint_cost(cm, poses, spec, flags)
        if self.device:
            if on_device:
                got = mp.dev.footprint_cost(self.to_device(poses), spec, flags)
                self.emap.synchronize()
                got = got.cpu().numpy()
            else:
                got = mp.dev.footprint_cost(poses, spec, flags)
            assert got.tolist() == want.tolist(), f"{int((got != want).sum())} pose costs differ"

    def op_score_trajectories(self, mp):
        cm = mp.cm
        T, nt = int(self.pick([1, 3, 5])), int(self.pick([1, 13, 64, 65]))
        poses = self.poses(cm, nt * T)
        k, spec = self.spec(cm)
        flags = int(self.rng.integers(4))
        self.log(mp, "score_trajectories", n_traj=nt, T=T, spec=k, flags=flags)
        each = fref.footprint_cost(cm, poses, spec, flags & fref.INSCRIBED_LETHAL)
        want = fref.score_trajectories(each, T, flags & fref.SUM)
        if self.device:
            got, got_each = mp.dev.score_trajectories(poses, T, spec, flags, pose_costs=True)
            assert got_each.tolist() == each.tolist() and got.tolist() == want.tolist(), "trajectory or pose costs differ"

    # ---- ops: MapGrid and the critics -------------------------------------------------------------------------------------------------
    def plan_points(self, cm):
        n = int(self.pick([0, 1, 2, 3, 6]))
        known = cm.grid != 255
        pts = [self.world(cm, self.some_cell(cm, known), (float(self.rng.uniform(0.1, 0.9)), float(self.rng.uniform(0.1, 0.9)))) for _ in range(n)]
        if n >= 2 and self.chance(0.2):
            pts[int(self.rng.integers(n))] = self.off_map_point(cm)
        return pts

    def op_prepare_map_grid(self, mp):
        cm = mp.cm
        plan = self.plan_points(cm)
        which = int(self.pick([mref.PATH, mref.GOAL, mref.PATH | mref.GOAL, mref.PATH | mref.GOAL]))
        if not capped_fits(cm):                                          # (a map of the full profile alone)
            return self.capped_refused(mp, "prepare_map_grid", lambda: mp.dev.prepare_map_grid(plan, which))
        want = mref.grids(cm, plan)
        for slot, name in ((mref.PATH, "path"), (mref.GOAL, "goal")):
            if which & slot:
                mp.grids[slot] = {"dist": want[name], "started": want["started"], "goal_cell": want["goal_cell"], "fresh": True, "form": "capped"}
        self.log(mp, "prepare_map_grid", n=len(plan), which=which, started=want["started"], **self.forms_info(mp))
        if self.device:
            mp.dev.prepare_map_grid(plan, which)
        self.follow = (mp, ["read_map_grid", "score_map_grid", "best_trajectory"] + (["rollout_best", "dwa_best"] if self.full else []))

    def op_prepare_map_grid_front(self, mp):
        cm = mp.cm
        plan = self.plan_points(cm)
        if not capped_fits(cm):
            return self.capped_refused(mp, "prepare_map_grid_front", lambda: mp.dev.prepare_map_grid_front(plan))
        want = mref.grids(cm, plan)
        mp.grids[cr.GRID_FRONT] = {"dist": want["goal"], "started": want["started"], "goal_cell": want["goal_cell"], "fresh": True, "form": "capped"}
        self.log(mp, "prepare_map_grid_front", n=len(plan), started=want["started"], **self.forms_info(mp))
        if self.device:
            mp.dev.prepare_map_grid_front(plan)
        self.follow = (mp, ["read_map_grid", "best_trajectory"] + (["dwa_best"] if self.full else []))

    def forms_info(self, mp):
        """full profile: whether the map's fresh grids were made by both forms of the prepare (shared slots, status words, generation)"""
        if not self.full:
            return {}
        forms = {g["form"] for g in mp.grids.values() if is_fresh(g)}
        return {"mixed": forms == {"capped", "tiled"}}

    def same_map_grid(self, mp, slot):
        """a fresh grid read back: distances, started and the goal cell as they were prepared"""
        g = mp.grids[slot]
        dist, started, goal = mp.dev.read_map_grid_front() if slot == cr.GRID_FRONT else mp.dev.read_map_grid(slot)
        assert (started, goal) == (g["started"], g["goal_cell"]), f"(started, goal) {(started, goal)}, want {(g['started'], g['goal_cell'])}"
        assert dist.tobytes() == g["dist"].tobytes(), f"{int((dist != g['dist']).sum())} distances differ"

    def capped_refused(self, mp, op, call):
        """the capped prepare on a map above GEM_MAPGRID_MAX_WORDS: refused, nothing enqueued and nothing changed (gem_hip_mapgrid.h), so
        a grid the tiled prepare left fresh stays readable and equal"""
        fresh = [s for s in SLOTS if is_fresh(mp.grids[s])]
        self.log(mp, op, refused=True, kept=len(fresh))
        if self.device:
            self.refused(call, op + " above the cap")
            for s in fresh:
                self.same_map_grid(mp, s)

    def op_prepare_map_grid_tiled(self, mp):
        cm = mp.cm
        plan = self.plan_points(cm)
        which = int(self.pick([mref.PATH, mref.GOAL, mref.PATH | mref.GOAL, mref.PATH | mref.GOAL]))
        if self.small_next and is_fresh(mp.grids[mref.PATH]) != is_fresh(mp.grids[mref.GOAL]):        # (before a planner: the missing one)
            which = mref.GOAL if is_fresh(mp.grids[mref.PATH]) else mref.PATH
        chunk = int(self.pick([0, 0, 1, 3]))
        want = mref.grids(cm, plan)
        for slot, name in ((mref.PATH, "path"), (mref.GOAL, "goal")):
            if which & slot:
                mp.grids[slot] = {"dist": want[name], "started": want["started"], "goal_cell": want["goal_cell"], "fresh": True, "form": "tiled"}
        self.log(mp, "prepare_map_grid_tiled", n=len(plan), which=which, started=want["started"], chunk=chunk, **self.forms_info(mp))
        if self.device:
            self.debug("mapgrid_chunk", chunk)
            st = mp.dev.prepare_map_grid_tiled(plan, which)              # rounds depends on timing and is not compared
            assert (st["started"], st["goal_cell"]) == (want["started"], want["goal_cell"]), f"status {st}, want {(want['started'], want['goal_cell'])}"
            for slot in (mref.PATH, mref.GOAL):
                if which & slot:
                    self.same_map_grid(mp, slot)
        self.follow = (mp, ["read_map_grid", "score_map_grid", "best_trajectory", "rollout_best", "rollout_best", "dwa_best", "prepare_map_grid"]
                       if capped_fits(cm) else ["prepare_map_grid", "prepare_map_grid_front", "read_map_grid", "rollout_best"])

    def op_prepare_map_grid_front_tiled(self, mp):
        cm = mp.cm
        plan = self.plan_points(cm)
        chunk = int(self.pick([0, 0, 1, 3]))
        want = mref.grids(cm, plan)
        mp.grids[cr.GRID_FRONT] = {"dist": want["goal"], "started": want["started"], "goal_cell": want["goal_cell"], "fresh": True, "form": "tiled"}
        self.log(mp, "prepare_map_grid_front_tiled", n=len(plan), started=want["started"], chunk=chunk, **self.forms_info(mp))
        if self.device:
            self.debug("mapgrid_chunk", chunk)
            st = mp.dev.prepare_map_grid_front_tiled(plan)
            assert (st["started"], st["goal_cell"]) == (want["started"], want["goal_cell"]), f"status {st}, want {(want['started'], want['goal_cell'])}"
            self.same_map_grid(mp, cr.GRID_FRONT)
        self.follow = (mp, ["read_map_grid", "best_trajectory", "dwa_best", "prepare_map_grid"])

    def op_read_map_grid(self, mp):
        slot = int(self.pick(SLOTS))
        g = mp.grids[slot]
        self.log(mp, "read_map_grid", slot=slot, fresh=is_fresh(g))
        if not self.device:
            return
        read = (lambda: mp.dev.read_map_grid_front()) if slot == cr.GRID_FRONT else (lambda: mp.dev.read_map_grid(slot))
        if not is_fresh(g):
            self.refused(read, "read_map_grid")
            if slot == cr.GRID_FRONT:
                self.raw_refused(mp, "gem_costmap_mapgrid_read_front")
            else:
                self.raw_refused(mp, "gem_costmap_mapgrid_read", slot)
            return
        dist, started, goal = read()
        assert (started, goal) == (g["started"], g["goal_cell"]), f"(started, goal) {(started, goal)}, want {(g['started'], g['goal_cell'])}"
        assert dist.tobytes() == g["dist"].tobytes(), f"{int((dist != g['dist']).sum())} distances differ"

    def op_score_map_grid(self, mp):
        cm = mp.cm
        slot = int(self.pick([mref.PATH, mref.GOAL]))
        g = mp.grids[slot]
        T, nt = int(self.pick([1, 3, 5])), int(self.pick([1, 13, 64, 65]))
        poses = self.poses(cm, nt * T)
        xshift = float(self.pick([0.0, 0.0, 1.5 * cm.res]))
        flags = int(self.rng.integers(4))
        self.log(mp, "score_map_grid", slot=slot, fresh=is_fresh(g), n_traj=nt, T=T, xshift=xshift, flags=flags)
        if not is_fresh(g):
            if self.device:
                self.refused(lambda: mp.dev.score_map_grid(slot, poses, T, xshift, flags), "score_map_grid")
            return
        want = mref.score(cm, g["dist"], poses, T, xshift, flags)
        if self.device:
            got = mp.dev.score_map_grid(slot, poses, T, xshift, flags)
            assert got.tolist() == want.tolist(), f"{int((got != want).sum())} scores differ"

    def op_best_trajectory(self, mp):
        cm, rng = mp.cm, self.rng
        fresh = [s for s in SLOTS if is_fresh(mp.grids[s])]
        other = [s for s in SLOTS if s not in fresh]
        critics = []
        if self.chance(0.8) or not fresh:
            critics.append(cr.obstacle(float(self.pick([0.01, 1.0])), int(self.pick([0, fref.INSCRIBED_LETHAL, fref.SUM, cr.CENTRE_COST, 7]))))
        for s in fresh:
            if self.chance(0.7):
                critics.append(cr.map_grid(float(self.pick([1.0, 24.0, 0.0])), s, float(self.pick([0.0, 1.5 * cm.res])), int(rng.integers(4))))
        if not critics:
            critics.append(cr.obstacle(1.0, 0))
        refusal = bool(other) and self.chance(0.15)
        if refusal:                                                      # a critic whose grid is stale or was never prepared
            critics.append(cr.map_grid(1.0, self.pick(other)))
        ext = None
        T, nt = int(self.pick([1, 3, 5])), int(self.pick([1, 7, 64, 65]))
        if self.chance(0.4):
            ext = rng.integers(-1, 6, (1, nt)).astype(np.float64) * 0.75
            critics.insert(0, cr.external(float(self.pick([1.0, 0.5])), 0))
        order = rng.permutation(len(critics))
        critics = [critics[i] for i in order]
        lens = None if self.chance(0.5) else rng.integers(1, T + 1, nt).astype(np.int32)
        poses = self.poses(cm, nt * T)
        k, spec = self.spec(cm)
        self.log(mp, "best_trajectory", critics=[(c["kind"], c["grid"], c["flags"], c["scale"]) for c in critics], n_traj=nt, T=T, spec=k,
                 lens=lens is not None, refusal=refusal)
        as_c = None
        if self.device:
            L = self.gem._lib
            as_c = [L.Critic(c["kind"], c["grid"], c["flags"], c["column"], c["scale"], c["xshift"]) for c in critics]
        if refusal:
            if self.device:
                self.refused(lambda: mp.dev.best_trajectory(as_c, poses, T, spec, ext, lens, totals=True), "best_trajectory")
            return
        table = cr.score_table(cm, {s: mp.grids[s]["dist"] for s in fresh}, critics, poses, T, spec, ext, lens)
        totals = cr.combine(critics, table, lens, T)
        best = cr.find_best(totals)
        if self.device:
            i, cost, n_valid, tot = mp.dev.best_trajectory(as_c, poses, T, spec, ext, lens, totals=True)
            assert tot.tobytes() == totals.tobytes(), f"{int((tot.view(np.uint64) != totals.view(np.uint64)).sum())} totals differ"
            assert (i, np.float64(cost).tobytes(), n_valid) == (best[0], np.float64(best[1]).tobytes(), best[2]), f"winner {(i, cost, n_valid)}, want {best}"

    # ---- ops: the global plan and the frontiers -------------------------------------------------------------------------------------
    def same_status(self, st, want, what):
        got = (st["found"], st["n_path"], st["goal_potential"], tuple(st["start_cell"]), tuple(st["goal_cell"]))
        exp = (want["found"], want["n_path"], want["goal_potential"], tuple(want["start_cell"]), tuple(want["goal_cell"]))
        assert got == exp, f"{what}: status {got}, want {exp}"

    def op_nav_plan(self, mp, for_search=False):
        """for_search: the plan the header advises a search to work from (allow_unknown = 0, here without the outline either)"""
        cm = mp.cm
        chunk = int(self.pick([0, 0, 1, 3]))
        known_only = for_search or self.chance(0.4)
        w = nref.weights(allow_unknown=not known_only)
        flags = nref.OUTLINE if not for_search and self.chance(0.4) else 0
        passable = w[cm.grid] > 0
        sw = self.world(cm, self.some_cell(cm, passable)) if self.chance(0.93) else self.off_map_point(cm)
        gw = sw if self.chance(0.3) else (self.world(cm, self.some_cell(cm, passable)) if self.chance(0.93) else self.off_map_point(cm))
        sc, gc = cref.world_to_map(cm, *sw), cref.world_to_map(cm, *gw)
        want = nref.plan(cm.grid, w, flags, sc, gc)
        if self.host and sc is not None and gc is not None:              # (the twin takes cells: it has no off-the-map point)
            pot, cells, st = self.gem.nav_plan_host(cm.grid, sc, gc, w, outline=bool(flags))
            self.same_status(st, want, "gem_navplan_host")
            assert pot.tobytes() == want["pot"].tobytes() and cells.tolist() == want["cells"].tolist(), "gem_navplan_host: potential or path differ"
        self.log(mp, "nav_plan", chunk=chunk, known_only=known_only, flags=flags, start=sc, goal=gc, found=want["found"], n_path=want["n_path"])
        mp.plan = dict(want, start=sc, fresh=True)
        mp.search = None                                                 # a search carries the plan it was made from
        if self.device:
            self.debug("nav_chunk", chunk)
            path, st = mp.dev.nav_plan(sw, gw, w, outline=bool(flags))
            self.same_status(st, want, "nav_plan")
            assert path.tobytes() == nref.centres(want["cells"], cm.size_x, cm.res, cm.ox, cm.oy).tobytes(), "the path's world points differ"
        self.follow = (mp, ["read_potential", "frontiers", "frontiers", "nav_plan_to"])

    def op_read_potential(self, mp):
        p = mp.plan
        self.log(mp, "read_potential", fresh=is_fresh(p))
        if not self.device:
            return
        if not is_fresh(p):
            self.refused(lambda: mp.dev.read_potential(), "read_potential")
            self.raw_refused(mp, "gem_costmap_navplan_read")
            return
        pot, cells = mp.dev.read_potential()
        assert pot.tobytes() == p["pot"].tobytes(), f"{int((pot != p['pot']).sum())} potentials differ"
        assert cells.tolist() == np.asarray(p["cells"]).tolist(), "the path's cells differ"
        self.same_status(mp.dev.nav_status(), p, "nav_status")

    def op_nav_plan_to(self, mp):
        cm, p = mp.cm, mp.plan
        gw = self.world(cm, self.some_cell(cm)) if self.chance(0.93) else self.off_map_point(cm)
        gc = cref.world_to_map(cm, *gw)
        self.log(mp, "nav_plan_to", fresh=is_fresh(p), goal=gc)
        if not is_fresh(p):
            if self.device:
                self.refused(lambda: mp.dev.nav_plan_to(gw), "nav_plan_to")
            return
        path = nref.get_path(p["pot"], p["start"], gc)                   # one walk on the plan's potential, which stays
        on = nref.on_map(cm.grid, gc)
        p.update(cells=np.array([y * cm.size_x + x for x, y in path], np.int32), found=int(bool(path)), n_path=len(path),
                 goal_potential=int(p["pot"][gc[1], gc[0]]) if on else nref.UNREACHED, goal_cell=tuple(gc) if on else (-1, -1))
        if self.device:
            xy, st = mp.dev.nav_plan_to(gw)
            self.same_status(st, p, "nav_plan_to")
            assert xy.tobytes() == nref.centres(p["cells"], cm.size_x, cm.res, cm.ox, cm.oy).tobytes(), "the path's world points differ"
        self.follow = (mp, ["read_potential", "read_frontiers"])

    def op_frontiers(self, mp):
        cm, p = mp.cm, mp.plan
        chunk = int(self.pick([0, 0, 1, 3]))
        params = (float(self.pick([0.0, 0.0, 0.0, 2 * cm.res, 4 * cm.res])), float(self.pick([1.0, 0.001])), float(self.pick([1.0, 0.0, 3.0])))
        unknown = int((cm.grid == 255).sum())
        if (unknown == 0 or unknown == cm.grid.size) and self.chance(0.8):         # mostly a search has known and unknown space to find an edge between
            self.op_write(mp)
            self.same_grid(mp)
        if not is_fresh(p) and self.chance(0.75):                        # ... and a plan to work from
            self.op_nav_plan(mp, for_search=True)
            p = mp.plan
        if not is_fresh(p):
            self.log(mp, "frontiers", fresh=False, chunk=chunk)
            if self.device:
                self.debug("front_chunk", chunk)
                self.refused(lambda: mp.dev.frontiers(*params), "frontiers")
            return
        want = frref.search(cm.grid, p["pot"], cm.res, *params)          # the bytes as they are now against the plan's potential
        if self.host:
            kept, labels, st = self.gem.frontiers_host(cm.grid, p["pot"], cm.res, *params, origin=(cm.ox, cm.oy))
            assert (st["n_cells"], st["n_frontiers"], st["n_kept"], st["best"]) == (want["n_cells"], want["n_frontiers"], want["n_kept"], want["best"]), st
            assert labels.tobytes() == want["labels"].tobytes() and [{k: f[k] for k in r} for f, r in zip(kept, want["kept"])] == want["kept"], \
                "gem_frontiers_host: labels or kept list differ"
        self.log(mp, "frontiers", fresh=True, chunk=chunk, params=params, n_frontiers=want["n_frontiers"], n_kept=want["n_kept"])
        mp.search = dict(want, fresh=True, origin=(cm.ox, cm.oy))
        if self.device:
            self.debug("front_chunk", chunk)
            st = mp.dev.frontiers(*params)
            got = (st["n_cells"], st["n_frontiers"], st["n_kept"], st["best"])
            exp = (want["n_cells"], want["n_frontiers"], want["n_kept"], want["best"])
            assert got == exp, f"status {got}, want {exp}"
            if want["best"] >= 0:
                b = want["best_frontier"]
                assert {k: st["best_frontier"][k] for k in b} == b, f"the winner {st['best_frontier']}, want {b}"
                assert st["best_frontier"]["centroid"] == frref.centroid(b, cm.res, cm.ox, cm.oy), "the winner's centroid"
            else:
                assert st["best_frontier"] is None, st
        self.follow = (mp, ["read_frontiers", "read_frontiers", "nav_plan_to"])

    def op_read_frontiers(self, mp):
        cm, s = mp.cm, mp.search
        self.log(mp, "read_frontiers", fresh=is_fresh(s))
        if not self.device:
            return
        if not is_fresh(s):
            self.refused(lambda: mp.dev.read_frontiers(), "read_frontiers")
            self.raw_refused(mp, "gem_costmap_frontiers_read")
            return
        kept, labels = mp.dev.read_frontiers()
        assert labels.tobytes() == s["labels"].tobytes(), f"{int((labels != s['labels']).sum())} labels differ"
        assert len(kept) == len(s["kept"]) and [{k: f[k] for k in r} for f, r in zip(kept, s["kept"])] == s["kept"], "the kept list differs"
        assert [f["centroid"] for f in kept] == [frref.centroid(r, cm.res, cm.ox, cm.oy) for r in s["kept"]], "the centroids differ"

    # ---- ops of the full profile: the voxel layer ---------------------------------------------------------------------------------------
    def vox_info(self, mp):
        """full profile: whether the map carries voxels, and columns that are not the unknown one"""
        if not self.full:
            return {}
        return {"voxels": mp.vox is not None, "vox_known": mp.cols is not None and bool((mp.cols != vref.UNKNOWN_COLUMN).any())}

    def no_voxels(self, mp, op, call, raw=False):
        """a voxel entry on a map without voxels: refused, and through the C entry the caller's buffer as it was"""
        self.log(mp, op, refused=True)
        if self.device:
            self.refused(call, op + " on a map without voxels")
            if raw:
                self.raw_refused(mp, "gem_costmap_voxels_read")

    def op_attach_voxels(self, mp):
        vox = vref.Voxels(int(self.pick([10, 10, 10, 16, 16, 16, 1])), float(self.pick([0.2, 0.1])), float(self.pick([0.0, 0.0, -0.4])),
                          int(self.pick([15, 15, 16, 0])), int(self.pick([0, 0, 2])))
        attach = lambda: mp.dev.attach_voxels(*vox)
        if mp.vox is not None:                                           # voxels attached twice: refused, the first grid stays
            self.log(mp, "attach_voxels", refused=True, twice=True)
            if self.device:
                self.refused(attach, "attach_voxels on a map that has voxels")
            return
        self.log(mp, "attach_voxels", refused=False, config=tuple(vox))
        mp.vox, mp.cols = vox, np.full((mp.cm.size_y, mp.cm.size_x), vref.UNKNOWN_COLUMN, np.uint32)
        if self.device:
            attach()
        if self.step >= 0:
            self.follow = (mp, ["write_voxels", "write_voxels", "voxel_observe", "voxel_observe", "read_voxels"])

    def op_detach_voxels(self, mp):
        if mp.vox is None:
            return self.no_voxels(mp, "detach_voxels", lambda: mp.dev.detach_voxels())
        self.log(mp, "detach_voxels", refused=False)
        mp.vox = mp.cols = None
        if self.device:
            mp.dev.detach_voxels()
            self.refused(lambda: mp.dev.read_voxels(), "read_voxels after detach_voxels")

    def columns(self, vox, shape):
        """random columns a VoxelLayer could hold: marked voxels inside size_z are "not known free" too; the bits above size_z stay as
        reset leaves them; whole unknown and whole free columns among them"""
        rng = self.rng
        zmask = (1 << vox.size_z) - 1
        marked = (rng.integers(0, 1 << 16, shape) & rng.integers(0, 1 << 16, shape) & zmask).astype(np.uint32)
        marked[rng.random(shape) < 0.3] = 0
        low = ((rng.integers(0, 1 << 16, shape) & rng.integers(0, 1 << 16, shape)).astype(np.uint32) | marked | np.uint32(0xFFFF & ~zmask))
        cols = (marked << np.uint32(16)) | low
        kind = rng.random(shape)
        cols[kind < 0.15] = vref.UNKNOWN_COLUMN
        cols[kind > 0.9] = np.uint32(0xFFFF & ~zmask)
        return cols.astype(np.uint32)

    def op_write_voxels(self, mp):
        cm = mp.cm
        w = self.window(cm)
        if mp.vox is None:
            ww = w or (0, 0, cm.size_x, cm.size_y)
            zeros = np.zeros((ww[3] - ww[1], ww[2] - ww[0]), np.uint32)
            return self.no_voxels(mp, "write_voxels", lambda: mp.dev.write_voxels(zeros, w))
        ww = w or (0, 0, cm.size_x, cm.size_y)
        v = self.columns(mp.vox, (ww[3] - ww[1], ww[2] - ww[0]))
        self.log(mp, "write_voxels", refused=False, window=w)
        mp.cols[ww[1]:ww[3], ww[0]:ww[2]] = v
        if self.device:
            mp.dev.write_voxels(v, w)
        self.follow = (mp, ["voxel_observe", "voxel_observe", "read_voxels", "roll", "reset", "recreate"])

    def op_read_voxels(self, mp):
        cm = mp.cm
        w = self.window(cm) or (0, 0, cm.size_x, cm.size_y)
        if mp.vox is None:
            return self.no_voxels(mp, "read_voxels", lambda: mp.dev.read_voxels(w), raw=True)
        self.log(mp, "read_voxels", refused=False, window=w)
        if self.device:
            got = mp.dev.read_voxels(w)
            assert got.tobytes() == np.ascontiguousarray(mp.cols[w[1]:w[3], w[0]:w[2]]).tobytes(), f"{int((got != mp.cols[w[1]:w[3], w[0]:w[2]]).sum())} columns of the window differ"

    def voxel_observations(self, cm, vox):
        """observations as op_observe builds them, with the third dimension: sensors inside, above and below the voxel range and off the
        map, returns through the whole height of the range and beyond it"""
        rng = self.rng
        ext_x, ext_y = cm.size_x * cm.res, cm.size_y * cm.res
        reach = min(max(ext_x, ext_y), 140 * cm.res)
        top = vox.origin_z + vox.size_z * vox.z_resolution
        n_obs = int(self.pick([0, 1, 1, 1, 2, 2, 3]))
        width = int(self.pick([3, 4, 8]))                                # records of 12, 16 and 32 bytes
        obs, info = [], []
        for _ in range(n_obs):
            n = int(self.pick([0, 1, 63, 64, 65, 200, 200, 500, 500]))
            where = self.pick(["inside"] * 8 + ["off"])
            s = self.world(cm, self.some_cell(cm), (float(rng.uniform(0.05, 0.95)), float(rng.uniform(0.05, 0.95)))) if where == "inside" else self.off_map_point(cm)
            height = self.pick(["inside"] * 7 + ["above", "below"])
            sz = {"inside": vox.origin_z + float(rng.uniform(0.05, 0.95)) * (top - vox.origin_z), "above": top + 0.3, "below": vox.origin_z - 0.3}[height]
            a, r = rng.uniform(-math.pi, math.pi, n), rng.uniform(0.0, 1.3, n) * reach
            p = np.zeros((n, width), F32)
            p[:, 0], p[:, 1] = s[0] + r * np.cos(a), s[1] + r * np.sin(a)
            p[:, 2] = np.where(rng.random(n) < 0.7, rng.uniform(vox.origin_z, top, n), rng.uniform(vox.origin_z - 0.3, max(top, 1.0) + 0.4, n))
            p[rng.random(n) < 0.02, 0] = np.nan
            mark, clear = self.pick([(True, True), (True, True), (True, True), (False, True), (False, True), (True, False)])
            obs.append({"points": p, "origin": (s[0], s[1], sz), "marking": mark, "clearing": clear,
                        "raytrace_range": float(self.pick([0.3 * reach, 0.3 * reach, 3.0, math.inf])),
                        "obstacle_range": float(self.pick([2.5, 0.5 * reach, math.inf])),
                        "min_obstacle_height": float(self.pick([0.0, 0.0, -1.0])), "max_obstacle_height": float(self.pick([2.0, 2.0, 0.8]))})
            info.append((n, where, height, mark, clear))
        return obs, info

    def op_voxel_observe(self, mp):
        cm = mp.cm
        if mp.vox is None and (self.small_next or self.chance(0.85)):    # mostly the call has voxels to work on; its echo always
            self.op_attach_voxels(mp)
            self.follow = None
            if self.chance(0.7):
                self.op_write_voxels(mp)
                self.follow = None
        if mp.vox is None:
            sensor = self.world(cm, self.some_cell(cm))
            one = [{"points": np.zeros((1, 3), F32), "origin": (sensor[0], sensor[1], 0.5)}]
            return self.no_voxels(mp, "voxel_observe", lambda: mp.dev.voxel_observe(one, 2.0, list(EMPTY_BOUNDS)))
        vox = mp.vox
        obs, info = self.voxel_observations(cm, vox)
        layer_max = float(self.pick([2.0, 1.0, math.inf]))
        bounds = None if self.chance(0.5) else list(EMPTY_BOUNDS)
        on_device = self.chance(0.4)
        before, cols_before = cm.grid.copy(), mp.cols.copy()
        detail = {}
        want = vref.observe(cm, mp.cols, vox, obs, layer_max, None if bounds is None else list(bounds), detail=detail)
        if self.host:
            twin, twin_cols = before.copy(), cols_before.copy()
            got = self.gem.voxlayer_host(twin, twin_cols, cm.res, (cm.ox, cm.oy), tuple(vox), obs, layer_max, None if bounds is None else list(bounds))
            assert got == want, f"gem_voxlayer_host: bounds {got}, want {want}"
            assert twin.tobytes() == cm.grid.tobytes() and twin_cols.tobytes() == mp.cols.tobytes(), \
                f"gem_voxlayer_host: {int((twin != cm.grid).sum())} cells and {int((twin_cols != mp.cols).sum())} columns differ"
        gone = (cols_before >> np.uint32(16)) & ~(mp.cols >> np.uint32(16))
        self.log(mp, "voxel_observe", refused=False, n_obs=len(obs), obs=info, on_device=on_device, bounds=bounds is not None, config=tuple(vox),
                 late=bool(bounds is not None and vox.mark_threshold > 0 and any(o["marking"] and len(o["points"]) for o in obs)),
                 changed=bool((before != cm.grid).any()), cleared_marked=bool(gone.any()), lethal=bool(detail["lethal"].any()))
        if obs:
            mp.stale("voxel_observe")
        if self.device:
            dobs = [{**o, "points": self.to_device(o["points"])} for o in obs] if on_device else obs
            got = mp.dev.voxel_observe(dobs, layer_max, None if bounds is None else list(bounds))
            assert got == want, f"bounds {got}, want {want}"
        self.follow = (mp, ["voxel_observe", "roll", "reset", "read_voxels"])

    # ---- ops of the full profile: the two local planners -----------------------------------------------------------------------------------
    def planner_pose(self, cm, want=None):
        """(x, y, theta) on the map (with `want`, on one of its cells), on a blocked cell or just off the map"""
        kind = self.pick(["on"] * 7 + ["blocked", "off"])
        if kind == "off":
            x, y = self.off_map_point(cm)
        else:
            sel = cm.grid >= 253 if kind == "blocked" else want
            x, y = self.world(cm, self.some_cell(cm, sel), (float(self.rng.uniform(0.1, 0.9)), float(self.rng.uniform(0.1, 0.9))))
        return kind, (x, y, float(self.rng.uniform(-math.pi, math.pi)))

    def grids_for_planner(self, mp):
        """mostly a planner finds PATH and GOAL fresh: the missing ones are prepared first, by either form"""
        if all(is_fresh(mp.grids[s]) for s in (mref.PATH, mref.GOAL)) or not (self.small_next or self.chance(0.8)):
            return
        keep = self.small_next
        self.small_next = True                                           # (the tiled form then prepares the missing one alone)
        if capped_fits(mp.cm) and self.chance(0.5):
            self.op_prepare_map_grid(mp)
            if not all(is_fresh(mp.grids[s]) for s in (mref.PATH, mref.GOAL)):
                self.op_prepare_map_grid_tiled(mp)
        else:
            self.op_prepare_map_grid_tiled(mp)
        self.small_next, self.follow = keep, None
        self.same_grid(mp)

    def lost_grids(self, mp, op):
        """whether `op` has just made PATH or GOAL stale, or a re-creation has taken them"""
        gs = [mp.grids[s] for s in (mref.PATH, mref.GOAL)]
        return mp.missing == "recreate" if op == "recreate" else any(g is not None and not g["fresh"] and g.get("cause") == op for g in gs)

    def why_refused(self, mp, slots):
        """the cause a planner is refused for: what made the first grid that is not fresh stale, or why there is none"""
        for s in slots:
            g = mp.grids[s]
            if not is_fresh(g):
                return mp.missing if g is None else g.get("cause")
        return None

    ROLLOUT_SETS = [dict(vx_samples=2, vtheta_samples=2, holonomic_robot=0, y_vels=()),                    # 4 + 2 + 0 + 1 = 7 candidates
                    dict(vx_samples=2, vtheta_samples=3, holonomic_robot=1, y_vels=(-2.0, 2.0)),           # 6 + 2 + 3 + 2 + 1 = 14
                    dict(vx_samples=3, vtheta_samples=4, holonomic_robot=1, y_vels=(1.5,)),                # 12 + 2 + 4 + 1 + 1 = 20
                    dict(vx_samples=3, vtheta_samples=4, holonomic_robot=0, y_vels=())]                    # 12 + 4 + 1 = 17

    def op_rollout_best(self, mp):
        cm, rng, r = mp.cm, self.rng, mp.cm.res
        small, probe = self.small_next, self.stale_probe
        if not probe:
            self.grids_for_planner(mp)
        base = self.ROLLOUT_SETS[0] if small else self.pick(self.ROLLOUT_SETS)
        cfg = dict(rref.DEFAULTS, **base)
        cfg["y_vels"] = tuple(v * r for v in base["y_vels"])
        cfg.update(sim_time=float(self.pick([1.0, 0.6])), sim_granularity=float(self.pick([r, 0.6 * r])), angular_sim_granularity=float(self.pick([0.2, 0.35])),
                   sim_period=0.1, max_vel_x=5.0 * r, min_vel_x=r, backup_vel=-1.0 * r, heading_lookahead=float(self.pick([2.0 * r, 3.25 * r])),
                   acc_lim_x=25.0 * r, acc_lim_y=25.0 * r, dwa=int(rng.integers(2)), pdist_scale=float(self.pick([0.6, 0.0])),
                   occdist_scale=float(self.pick([0.01, 0.2])))
        path, goal = mp.grids[mref.PATH], mp.grids[mref.GOAL]
        reach = None if not (is_fresh(path) and is_fresh(goal)) else (path["dist"] < cm.grid.size) & (goal["dist"] < cm.grid.size) & (cm.grid < 253)
        kind, pos = self.planner_pose(cm, reach)
        if self.chance(0.2):
            cfg["final_goal"] = self.world(cm, self.some_cell(cm))
        vel = (float(rng.uniform(0.0, 4.0)) * r, float(self.pick([0.0, 0.0, r])), float(rng.uniform(-0.5, 0.5)))
        state = int(self.pick([0, 0, 0, rref.ESCAPING, rref.STUCK_LEFT, rref.STUCK_RIGHT | rref.STUCK_LEFT_STRAFE, rref.STUCK_RIGHT_STRAFE | rref.ESCAPING,
                               rref.ESCAPING | rref.STUCK_LEFT | rref.STUCK_RIGHT, rref.ESCAPING | rref.STUCK_LEFT | rref.STUCK_RIGHT]))     # (the last: the strafes decide, stage 2)
        if state == (rref.ESCAPING | rref.STUCK_LEFT | rref.STUCK_RIGHT) and not small and not cfg["holonomic_robot"]:
            cfg.update(holonomic_robot=1, y_vels=(-2.0 * r, 2.0 * r))     # no forward candidates and no rotation may win: the strafes decide
        k, spec = self.spec(cm, allow_centre=True)
        spec = [] if self.chance(0.5) else spec                          # a point robot: a footprint seldom fits between these scenes' obstacles
        flags = int(rng.integers(2)) * fref.INSCRIBED_LETHAL
        costs, device = self.chance(0.6), self.chance(0.4)
        n_cand = len(rref.candidates(cfg, pos, vel, state))
        plan = self.gem.rollout_plan(cfg, pos, vel, state) if (self.device or self.host) else None
        if plan is not None:
            assert plan.n_cand == n_cand, f"gem_rollout_plan: {plan.n_cand} candidates, want {n_cand}"
        cause = self.why_refused(mp, (mref.PATH, mref.GOAL))
        info = dict(n_cand=n_cand, pose=kind, state=state, flags=flags, spec=k if spec else -1, costs=costs, device=device, small=small)
        if cause is not None:
            self.log(mp, "rollout_best", refused=True, cause=cause, **info)
            if self.device:
                self.refused(lambda: mp.dev.rollout_best(plan, pos, vel, state, spec, flags, costs=costs, device=device), "rollout_best")
                self.raw_rollout_refused(mp, plan, pos, vel, state, spec, flags)
            return
        want = rref.evaluate_all(cm, path["dist"], goal["dist"], cfg, pos, vel, state, spec, flags)     # the grids as they were prepared
        ans = want["answer"]
        if self.host:
            t_ans, t_cost, t_ahead, _ = self.gem.rollout_host(plan, pos, vel, cm.grid, cm.res, (cm.ox, cm.oy), path["dist"], goal["dist"], spec, flags)
            assert t_cost.tobytes() == want["cost"].tobytes() and t_ahead.tobytes() == want["ahead"].tobytes(), "gem_rollout_host: costs or ahead differ"
            assert t_ans["bytes"] == ans["bytes"], f"gem_rollout_host: answer {t_ans}, want {ans}"
        self.log(mp, "rollout_best", refused=False, cause=None, stage=ans["stage"], valid=bool(ans["raw_cost"] >= 0),
                 all_rejected=bool((want["cost"] < 0).all()), **info)
        if self.device:
            got = mp.dev.rollout_best(plan, pos, vel, state, spec, flags, costs=costs, device=device)
            if device:
                self.emap.synchronize()                                  # the 64 bytes are read after the wait
                got = tuple(t.cpu().numpy() for t in got) if costs else got.cpu().numpy()
            g_ans, g_cost, g_ahead = got if costs else (got, None, None)
            if device:
                g_ans = self.gem.rollout_answer(g_ans)
            if costs:
                assert g_cost.tobytes() == want["cost"].tobytes(), f"{int((g_cost.view(np.uint64) != want['cost'].view(np.uint64)).sum())} costs differ"
                assert g_ahead.tobytes() == want["ahead"].tobytes(), f"{int((g_ahead != want['ahead']).sum())} ahead values differ"
            assert g_ans["bytes"] == ans["bytes"], f"answer {g_ans}, want {ans}"

    def raw_rollout_refused(self, mp, plan, pos, vel, state, spec, flags):
        """the C entries with the outputs prefilled, host form and device form: refused, and the buffers as they were"""
        import torch
        L, nc = self.gem._lib, int(plan.n_cand)
        d3 = lambda v: (C.c_double * 3)(*[float(x) for x in v])
        sp = np.ascontiguousarray(spec, np.float64).reshape(-1, 2)
        spp = sp.ctypes.data_as(C.POINTER(C.c_double)) if sp.size else None
        cost, ahead = np.full(nc, -77.0), np.full(nc, -7, np.int32)
        best = L.RolloutBest(-9, -9, -9, -9.0, -9.0, -9.0, -9.0, -9.0, -9)
        rc = self.lib.gem_costmap_rollout_best(self.h, mp.dev.id, C.byref(plan), d3(pos), d3(vel), state, spp, sp.shape[0], flags,
                                               cost.ctypes.data_as(C.c_void_p), ahead.ctypes.data_as(C.c_void_p), C.byref(best))
        assert rc != 0, f"gem_costmap_rollout_best: answered {rc} where the model says stale or never made"
        assert (cost == -77.0).all() and (ahead == -7).all() and (best.index, best.stage, best.cost, best.reserved1) == (-9, -9, -9.0, -9), \
            "gem_costmap_rollout_best: refused, but the caller's buffers were written"
        d_cost = torch.full((nc,), -77.0, dtype=torch.float64, device="cuda:0")
        d_ahead = torch.full((nc,), -7, dtype=torch.int32, device="cuda:0")
        d_best = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda:0")
        rc = self.lib.gem_costmap_rollout_best_device(self.h, mp.dev.id, C.byref(plan), d3(pos), d3(vel), state, spp, sp.shape[0], flags,
                                                      C.c_void_p(d_cost.data_ptr()), C.c_void_p(d_ahead.data_ptr()), C.c_void_p(d_best.data_ptr()))
        assert rc != 0, f"gem_costmap_rollout_best_device: answered {rc} where the model says stale or never made"
        self.emap.synchronize()
        assert bool((d_cost.cpu() == -77.0).all()) and bool((d_ahead.cpu() == -7).all()) and bool((d_best.cpu() == 0xEE).all()), \
            "gem_costmap_rollout_best_device: refused, but the caller's buffers were written"

    DWA_SAMPLES = [(1, 1, 1), (2, 1, 3), (3, 2, 3), (4, 3, 5), (6, 3, 9)]  # 1 .. 162 trajectories and more (a list that crosses zero gains one)

    def op_dwa_best(self, mp):
        cm, rng, r = mp.cm, self.rng, mp.cm.res
        small, probe = self.small_next, self.stale_probe
        if not probe:
            self.grids_for_planner(mp)
        vs = self.pick(self.DWA_SAMPLES[:2]) if small else self.pick(self.DWA_SAMPLES)
        limits = dict(max_vel_x=5.5 * r, min_vel_x=float(self.pick([0.0, -1.0 * r])), max_vel_y=r, min_vel_y=-1.0 * r, max_vel_theta=1.0,
                      min_vel_theta=float(self.pick([0.4, -1.0])), max_vel_trans=float(self.pick([5.5 * r, -1.0])), min_vel_trans=float(self.pick([r, -1.0])),
                      acc_lim_x=25.0 * r, acc_lim_y=25.0 * r, acc_lim_theta=3.2)
        config = dict(sim_time=float(self.pick([1.0, 1.7, 0.5])), sim_granularity=float(self.pick([r, 0.5 * r])), angular_sim_granularity=float(self.pick([0.1, 0.3])),
                      sim_period=float(self.pick([0.05, 0.2])), use_dwa=bool(rng.integers(2)), discretize_by_time=self.chance(0.2),
                      continued_acceleration=self.chance(0.3), oscillation_flags=int(self.pick([0, 0, 0, 16, 16, 1 | 8, 63])), vsamples=vs)
        if config["discretize_by_time"]:
            config["sim_granularity"] = float(self.pick([0.1, 0.25]))    # (then a time: sim_time / sim_granularity steps)
        fresh = [s for s in SLOTS if is_fresh(mp.grids[s])]
        other = [s for s in SLOTS if s not in fresh]
        reach = None
        if mref.GOAL in fresh:
            reach = (mp.grids[mref.GOAL]["dist"] < cm.grid.size) & (cm.grid < 253)
        kind, pos = self.planner_pose(cm, reach)
        vel = (float(rng.uniform(0.0, 4.0)) * r, float(self.pick([0.0, 0.0, 0.5 * r])), float(rng.uniform(-0.5, 0.5)))
        goal = self.world(cm, self.some_cell(cm))
        critics = []
        if self.chance(0.8) or not fresh:
            critics.append(cr.obstacle(float(self.pick([0.01, 1.0])), int(self.pick([0, fref.INSCRIBED_LETHAL, fref.SUM, cr.CENTRE_COST, 7]))))
        for s in fresh:
            if self.chance(0.7):
                critics.append(cr.map_grid(float(self.pick([1.0, 24.0, 0.0])), s, float(self.pick([0.0, 1.5 * r])), int(rng.integers(4))))
        if not critics:
            critics.append(cr.obstacle(1.0, 0))
        for column in (0, 1):                                            # the generated columns: oscillation, twirling
            if self.chance(0.6):
                critics.insert(int(rng.integers(len(critics) + 1)), cr.external(float(self.pick([1.0, 0.5])), column))
        refusal = bool(other) and (probe or self.chance(0.3))
        cause = None
        if refusal:                                                      # a critic whose grid is stale or was never prepared
            slot = self.pick(other)
            critics.append(cr.map_grid(1.0, slot))
            cause = self.why_refused(mp, (slot,))
        k, spec = self.spec(cm)
        if self.chance(0.5):
            k, spec = -1, []                                             # a point robot: a footprint seldom fits between these scenes' obstacles
        totals, device = self.chance(0.7), self.chance(0.4)
        ls = tref.lists(limits, config, pos, vel, goal)
        T0 = max(tref.max_steps(limits, config, ls), 1)
        T = T0 + int(self.pick([0, 0, 2]))                               # sometimes two spare pose slots
        poses, lens, ext, vels = tref.generate(limits, config, pos, vel, goal, T)
        nt = int(lens.size)
        plan = as_c = None
        if self.device or self.host:
            plan = self.gem.trajgen_plan(limits, config, pos, vel, goal)
            assert (int(plan.n_traj), max(int(plan.max_steps), 1)) == (nt, T0), f"gem_trajgen_plan: {plan.n_traj} trajectories of {plan.max_steps} steps, want {nt} of {T0}"
            L = self.gem._lib
            as_c = [L.Critic(c["kind"], c["grid"], c["flags"], c["column"], c["scale"], c["xshift"]) for c in critics]
        if self.host:
            t_poses, t_lens, t_ext, t_vels = self.gem.generate_trajectories(plan, pos, vel, T)
            assert t_lens.tobytes() == lens.tobytes() and t_ext.tobytes() == ext.tobytes() and t_vels.tobytes() == vels.tobytes() and \
                t_poses.tobytes() == poses.tobytes(), "gem_trajgen_generate: trajectories differ"
        info = dict(n_traj=nt, T=T, pose=kind, critics=[(c["kind"], c["grid"], c["column"]) for c in critics], spec=k, totals=totals, device=device, small=small)
        if refusal:
            self.log(mp, "dwa_best", refused=True, cause=cause, **info)
            if self.device:
                self.refused(lambda: mp.dev.dwa_best(as_c, plan, pos, vel, T, spec, totals=totals, device=device), "dwa_best")
                self.raw_dwa_refused(mp, as_c, plan, pos, vel, T, spec)
            return
        table = cr.score_table(cm, {s: mp.grids[s]["dist"] for s in fresh}, critics, poses, T, spec, ext, lens)
        tot = cr.combine(critics, table, lens, T)
        best = cr.find_best(tot)
        self.log(mp, "dwa_best", refused=False, cause=None, n_valid=best[2], **info)
        if self.device:
            got = mp.dev.dwa_best(as_c, plan, pos, vel, T, spec, totals=totals, device=device)
            if device:
                import torch
                self.emap.synchronize()
                b = (got[0] if totals else got).cpu()
                i, cost, n_valid = int(b[0]), float(b.view(torch.float64)[2]), int(b[1])
                assert int(b[3]) == 0, f"the answer's reserved word {int(b[3])}"
                g_tot = got[1].cpu().numpy() if totals else None
            else:
                i, cost, n_valid = got[:3]
                g_tot = got[3] if totals else None
            if totals:
                assert g_tot.tobytes() == tot.tobytes(), f"{int((g_tot.view(np.uint64) != tot.view(np.uint64)).sum())} totals differ"
            assert (i, np.float64(cost).tobytes(), n_valid) == (best[0], np.float64(best[1]).tobytes(), best[2]), f"winner {(i, cost, n_valid)}, want {best}"
            if best[0] >= 0:                                             # the winner's command from the index alone
                assert np.array(self.gem.trajectory_velocity(plan, vel, best[0]), np.float32).tobytes() == vels[best[0]].tobytes(), "the winner's velocity"

    def raw_dwa_refused(self, mp, as_c, plan, pos, vel, T, spec):
        """gem_costmap_dwa_best with the outputs prefilled: refused, and the buffers as they were"""
        L, nt = self.gem._lib, int(plan.n_traj)
        f3 = lambda v: (C.c_float * 3)(*[float(x) for x in np.asarray(v, np.float32)])
        cs = (L.Critic * len(as_c))(*as_c)
        sp = np.ascontiguousarray(spec, np.float64).reshape(-1, 2)
        tot = np.full(max(nt, 1), -77.0)
        best = L.BestTrajectory(-9, -9, -9.0, -9)
        rc = self.lib.gem_costmap_dwa_best(self.h, mp.dev.id, cs, len(as_c), C.byref(plan), f3(pos), f3(vel), T,
                                           sp.ctypes.data_as(C.POINTER(C.c_double)) if sp.size else None, sp.shape[0], tot.ctypes.data_as(C.c_void_p), C.byref(best))
        assert rc != 0, f"gem_costmap_dwa_best: answered {rc} where the model says stale or never made"
        assert (tot == -77.0).all() and (best.index, best.n_valid, best.cost, best.reserved) == (-9, -9, -9.0, -9), \
            "gem_costmap_dwa_best: refused, but the caller's buffers were written"

    # ---- ops: a map goes and another takes its id ---------------------------------------------------------------------------------------
    def op_recreate(self, mp):
        group = self.maps[:2] if mp.role in ("layer", "master") else [mp]
        geom = self.pick([g for g in (FULL_GEOMS if self.full else GEOMS) if g != mp.geom])
        res, origin = float(self.pick(RESOLUTIONS)), self.origin()
        old = [(g.geom, g.cells) for g in group]
        had_voxels = sum(g.vox is not None for g in group)
        ids = sorted(g.dev.id for g in group) if self.device else []
        if self.device:
            for g in group:
                g.dev.close()
        for g in group:
            new = Map(g.role, geom, res, origin, g.cm.default)
            g.geom, g.cm = new.geom, new.cm
            g.forget()
            g.vox = g.cols = None                                        # gem_costmap_destroy frees the columns: the new map has no voxels
            g.missing = "recreate"
            self.create(g)
        self.log(mp, "recreate", old=old, group=len(group), **({"had_voxels": had_voxels} if self.full else {}))
        if self.device and self.full:
            for g in group:                                              # ... not those of the map whose id it took
                self.refused(lambda: g.dev.read_voxels(), "read_voxels on a map created anew")
                self.raw_refused(g, "gem_costmap_voxels_read")
        if self.device:
            assert sorted(g.dev.id for g in group) == ids, f"ids {sorted(g.dev.id for g in group)}, want the old ones {ids}"
            for g in group:                                              # everything of the old map is gone
                self.refused(lambda: g.dev.read_potential(), "read_potential on a map created anew")
                self.refused(lambda: g.dev.read_frontiers(), "read_frontiers on a map created anew")
                self.refused(lambda: g.dev.read_map_grid(mref.PATH), "read_map_grid on a map created anew")
                self.raw_refused(g, "gem_costmap_navplan_read")
                self.raw_refused(g, "gem_costmap_frontiers_read")
                self.raw_refused(g, "gem_costmap_mapgrid_read", mref.GOAL)
                self.raw_refused(g, "gem_costmap_mapgrid_read_front")
        for g in group:                                                  # something to work on
            g.cm.grid[:] = self.scene(g.cm)
            if self.device:
                g.dev.write(g.cm.grid)
        return group

    # ---- the scenario -----------------------------------------------------------------------------------------------------------------
    def open_maps(self):
        rng = self.rng
        big_pair = self.chance(0.5)
        pair = self.pick(LARGE if big_pair else SMALL)
        res, origin = float(self.pick(RESOLUTIONS)), self.origin()
        self.maps = [Map("layer", pair, res, origin, 255), Map("master", pair, res, origin, 0)]
        for k in range(int(self.pick([0, 1, 1, 2, 2]))):                         # singles: first of the other size class, so sizes alternate
            pool = (SMALL if big_pair else LARGE) if k == 0 else (LARGE if big_pair else SMALL)
            self.maps.append(Map(f"single{k}", self.pick(pool), float(self.pick(RESOLUTIONS)), self.origin(), int(self.pick([255, 0]))))
        self.step = -1
        for mp in self.maps:
            self.create(mp)
            self.op_write(mp)
            self.same_grid(mp, "after the opening write: ")

    def next_op(self):
        if self.echo is not None:                                        # the same op on a smaller map: it runs in the arenas the larger one left
            op, cells = self.echo
            self.echo = None
            smaller = [m for m in self.maps if m.cells < cells]
            if smaller and self.chance(0.3):
                self.follow = None
                return self.pick(smaller), op
        if self.follow is not None:
            mp, ops = self.follow
            self.follow = None
            if self.chance(0.65) and mp in self.maps:
                return mp, self.pick(ops)
        names = list(OPS)
        wts = np.array([OPS[n] for n in names], np.float64)
        return self.pick(self.maps), names[int(self.rng.choice(len(names), p=wts / wts.sum()))]

    def open_maps_full(self):
        """as open_maps, from the full profile's pools; about half of the maps open with voxels attached"""
        big_pair = self.chance(0.5)
        pair = self.pick(FULL_LARGE if big_pair else SMALL)
        res, origin = float(self.pick(RESOLUTIONS)), self.origin()
        self.maps = [Map("layer", pair, res, origin, 255), Map("master", pair, res, origin, 0)]
        for k in range(int(self.pick([0, 1, 1, 2, 2]))):
            pool = (SMALL if big_pair else FULL_LARGE) if k == 0 else (FULL_LARGE if big_pair else SMALL)
            self.maps.append(Map(f"single{k}", self.pick(pool), float(self.pick(RESOLUTIONS)), self.origin(), int(self.pick([255, 0]))))
        self.step = -1
        for mp in self.maps:
            self.create(mp)
            self.op_write(mp)
            if self.chance(0.5):                                         # ... and with columns that have something to clear
                self.op_attach_voxels(mp)
                self.op_write_voxels(mp)
                self.follow = None
            self.same_grid(mp, "after the opening write: ")

    def next_op_full(self):
        self.small_next = False
        probe, self.probe_next, self.stale_probe = self.probe_next, False, False
        if self.echo is not None:                                        # the same op again in the arenas the larger call left
            op, cells = self.echo
            self.echo = None
            new = op in FULL_ARENA_OPS[len(ARENA_OPS):]
            pool = self.maps if op in PLANNER_OPS else [m for m in self.maps if m.cells < cells]
            if pool and self.chance((0.7 if op == "voxel_observe" else 0.5) if new else 0.3):
                self.follow = None
                self.small_next = new
                return self.pick(pool), op
        if self.follow is not None:
            mp, ops = self.follow
            self.follow = None
            if self.chance(0.65) and mp in self.maps:
                self.stale_probe = probe                                 # a planner directly behind what made its grids stale
                return mp, self.pick(ops)
        names = list(FULL_OPS)
        wts = np.array([FULL_OPS[n] for n in names], np.float64)
        mp, op = self.pick(self.maps), names[int(self.rng.choice(len(names), p=wts / wts.sum()))]
        others = [m for m in self.maps if m.geom not in LONG]
        if op in HEAVY_ON_LONG and mp.geom in LONG and others and self.chance(LONG_AWAY):
            mp = self.pick(others)
        return mp, op

    def run(self):
        self.open_maps_full() if self.full else self.open_maps()
        steps = int(self.rng.integers(20, 31))
        for self.step in range(steps):
            mp, op = self.next_op_full() if self.full else self.next_op()
            at = len(self.trace)
            try:
                touched = getattr(self, "op_" + op)(mp) or [mp]
                self.echo = (op, mp.cells) if op in (FULL_ARENA_OPS if self.full else ARENA_OPS) else None
                if self.full and op in ("roll", "observe", "voxel_observe", "recreate") and self.lost_grids(mp, op) and self.chance(0.6):
                    self.follow, self.probe_next, self.echo = (mp, list(PLANNER_OPS)), True, None
                for t in touched:
                    self.same_grid(t)
                if self.step % 5 == 4 or self.step == steps - 1:
                    for t in self.maps:
                        self.same_grid(t, "an op on another map touched ")
            except (AssertionError, self.GemError) as e:
                args = self.trace[-1] if len(self.trace) > at else {}
                raise AssertionError(f"seed {self.seed} step {self.step} op {op} on {mp.name()} {args}: {type(e).__name__}: {e}") from e
        return steps

    def close(self):
        if not self.device:
            return
        try:
            for k, v in (FULL_DEBUG_DEFAULTS if self.full else DEBUG_DEFAULTS).items():
                self.emap.debug_set(k, v)
        finally:
            self.emap.close()


def scenario(seed, backend="device", profile="base"):
    """one scenario: {"seed", "steps", "maps": [names], "trace": [one dict per call, in order]}; AssertionError on the first mismatch"""
    s = Scenario(seed, backend, profile)
    try:
        steps = s.run()
        return {"seed": seed, "steps": steps, "maps": [(m.role, m.geom) for m in s.maps], "trace": s.trace}
    finally:
        s.close()


POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1"),
                        ("covariance", "<f4"), ("intensity", "<f4"), ("travers", "<f4")])          # = gem_amd.api.POINT_DTYPE (no import without the library)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--backend", choices=["device", "reference", "host"], default="device")
    ap.add_argument("--profile", choices=["base", "full"], default="base")
    a = ap.parse_args()
    t0 = time.time(); n = 0; calls = 0
    seed = a.seed * 100000
    while time.time() - t0 < a.seconds:
        t1 = time.time()
        try:
            r = scenario(seed, a.backend, a.profile)
        except AssertionError as e:
            print(f"MISMATCH in scenario seed {seed}: {e}", flush=True)
            return 1
        n += 1; calls += len(r["trace"])
        print(f"ok seed {seed} steps {r['steps']} calls {len(r['trace'])} maps {[g for _, g in r['maps']]} {time.time() - t1:.2f} s", flush=True)
        seed += 1
    print(f"SUMMARY: {n} scenarios, {calls} calls, {time.time() - t0:.0f} s, no mismatch", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
