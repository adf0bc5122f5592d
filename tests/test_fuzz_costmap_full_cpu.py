"""What the full profile of the costmap soak (tools/fuzz_costmap.py, profile="full"; tests/test_fuzz_costmap_full_gpu.py) covers, asserted
without a GPU: the scenarios of the committed seed blocks run with backend="reference", which drives the model and the numpy references
alone, and their op traces are counted.  As in tests/test_fuzz_costmap_cpu.py these are conditions on the INPUTS of the GPU test -- the
voxel layer, the tiled MapGrid, the rollout and DWA among the op chains -- met by the generator's weights and the choice of seeds, not
measurements of the library."""
import sys
import time
from collections import Counter
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import fuzz_costmap as fz  # noqa: E402

# the blocks of consecutive seeds tests/test_fuzz_costmap_full_gpu.py runs, one parametrised case per block
FULL_SEED_BLOCKS = [range(3040, 3048), range(3112, 3120), range(3168, 3176)]
SEEDS = [s for b in FULL_SEED_BLOCKS for s in b]
NEW_ARENA_OPS = ("voxel_observe", "prepare_map_grid_tiled", "dwa_best", "rollout_best")
PLANNERS = ("dwa_best", "rollout_best")
T0 = time.time()


@pytest.fixture(scope="module")
def runs():
    return [fz.scenario(s, "reference", "full") for s in SEEDS]


@pytest.fixture(scope="module")
def calls(runs):
    return [c for r in runs for c in r["trace"]]


def share(cs, pred):
    return sum(1 for c in cs if pred(c)) / max(len(cs), 1)


def observed(calls):
    """the voxel_observe calls that ran with at least one observation"""
    return [c for c in calls if c["op"] == "voxel_observe" and not c["refused"] and c["n_obs"] >= 1]


def test_the_blocks_are_what_the_issue_sizes(runs):
    assert 16 <= len(SEEDS) <= 24 and len(set(SEEDS)) == len(SEEDS) and all(len(b) == 8 and b.step == 1 for b in FULL_SEED_BLOCKS)
    for r in runs:
        assert 20 <= r["steps"] <= 30 and 2 <= len(r["maps"]) <= 4
        assert r["maps"][0][1] == r["maps"][1][1] and (r["maps"][0][0], r["maps"][1][0]) == ("layer", "master")     # merge's pair
    assert set(fz.FULL_OPS) > set(fz.OPS) and all(fz.FULL_OPS[k] == v for k, v in fz.OPS.items())
    assert set(fz.FULL_GEOMS) > set(fz.GEOMS) and set(fz.LONG) == set(fz.FULL_GEOMS) - set(fz.GEOMS)
    for g in ("513x66", "70x520"):                                       # past 512 one way: nine tiles; a seam at 64 / 65 the other way
        x, y = fz.FULL_GEOMS[g]
        assert max(x, y) > 512 and 64 < min(x, y) <= 128 and fz.capped_fits(fz.cref.Costmap(x, y, 0.1, 0.0, 0.0))
    assert not fz.capped_fits(fz.cref.Costmap(*fz.FULL_GEOMS["1x4100"], 0.1, 0.0, 0.0))                  # the one map above the capped prepare's cap


def test_every_op_kind_occurs_at_least_five_times(calls):
    n = Counter(c["op"] for c in calls)
    print(sorted(n.items()))
    assert all(n[k] >= 5 for k in fz.FULL_OPS), {k: n[k] for k in fz.FULL_OPS if n[k] < 5}


def test_every_form_occurs(calls):
    obs = observed(calls)
    assert {c["config"][0] for c in obs} == {1, 10, 16} and {c["config"][4] for c in obs} == {0, 2}
    assert {c["config"][3] for c in obs} == {0, 15, 16} and len({c["config"][1] for c in obs}) == 2 and {c["config"][2] < 0 for c in obs} == {False, True}
    late = sum(c["late"] for c in obs)                                   # mark_threshold 2, bounds asked for, a marking cloud: the late bounds path
    assert late >= 3, late
    assert {(m, cl) for c in obs for _n, _w, _h, m, cl in c["obs"]} == {(True, True), (False, True), (True, False)}
    assert {w for c in obs for _n, w, _h, _m, _c in c["obs"]} == {"inside", "off"}
    assert {h for c in obs for _n, _w, h, _m, _c in c["obs"]} == {"inside", "above", "below"}
    assert {(c["on_device"], c["bounds"]) for c in obs} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {c["n_obs"] for c in obs} == {1, 2, 3}
    assert {c["window"] is None for c in calls if c["op"] == "write_voxels" and not c["refused"]} == {False, True}     # whole map and window
    assert sum(1 for c in calls if c["op"] == "read_voxels" and not c["refused"]) >= 3
    mixed = sum(c.get("mixed", False) for c in calls)                    # capped and tiled prepares in one map's slots, nothing stale in between
    assert mixed >= 3, mixed
    for op in ("prepare_map_grid_tiled", "prepare_map_grid_front_tiled"):
        chunks = {c["chunk"] for c in calls if c["op"] == op}
        assert 0 in chunks and any(0 < k <= 3 for k in chunks), (op, chunks)
    assert {c["which"] for c in calls if c["op"] == "prepare_map_grid_tiled"} == {1, 2, 3}
    ro = [c for c in calls if c["op"] == "rollout_best"]
    assert {(c["costs"], c["device"]) for c in ro if not c["refused"]} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {c["pose"] for c in ro if not c["refused"]} == {"on", "blocked", "off"} and len({c["state"] for c in ro}) >= 4 and {c["flags"] for c in ro} == {0, 1}
    dw = [c for c in calls if c["op"] == "dwa_best" and not c["refused"]]
    assert {(c["totals"], c["device"]) for c in dw} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {col for c in dw for kind, _g, col in c["critics"] if kind == fz.cr.EXTERNAL} == {0, 1}
    assert {g for c in dw for kind, g, _c in c["critics"] if kind == fz.cr.MAPGRID} == set(fz.SLOTS)
    assert len({c["n_traj"] for c in dw}) >= 4 and len({c["T"] for c in dw}) >= 4
    print("late", late, "mixed", mixed)


def test_every_geometry_occurs(runs, calls):
    seen = {g for r in runs for _role, g in r["maps"]} | {c["geom"] for c in calls}
    assert seen == set(fz.FULL_GEOMS), set(fz.FULL_GEOMS) - seen
    for op in NEW_ARENA_OPS:                                             # each on a long map, a strip and a 1 x N map
        on = {c["geom"] for c in calls if c["op"] == op and not c.get("refused")}
        assert on & set(fz.LONG) and {"65x3", "1x70"} <= on, (op, on)
    for op in ("nav_plan", "frontiers"):                                 # moved off the long maps mostly (HEAVY_ON_LONG), not always
        assert {c["geom"] for c in calls if c["op"] == op} & set(fz.LONG), op


def test_the_capped_prepare_above_the_cap_is_refused(calls):
    """1 x 4100 alone is above ceil(size_x / 64) * size_y <= 4096; a fresh tiled grid must survive the refusal"""
    ref = [c for c in calls if c["op"] in ("prepare_map_grid", "prepare_map_grid_front") and c.get("refused")]
    assert len(ref) >= 3 and all(c["geom"] == "1x4100" for c in ref) and any(c["kept"] for c in ref), [(c["geom"], c["kept"]) for c in ref]
    assert any(c["geom"] in ("513x66", "70x520") and not c.get("refused") for c in calls if c["op"] == "prepare_map_grid")


def test_a_smaller_call_follows_a_larger_one_in_every_new_arena(runs):
    """per handle, consecutive calls of one op kind that ran: by cells for voxel_observe and the tiled prepare, by trajectories and
    candidates for the planners"""
    pairs = Counter()
    size = {"voxel_observe": "cells", "prepare_map_grid_tiled": "cells", "dwa_best": "n_traj", "rollout_best": "n_cand"}
    for r in runs:
        last = {}
        for c in r["trace"]:
            if c["op"] in size and not c.get("refused") and c.get("n_obs", 1) >= 1:
                v = c[size[c["op"]]]
                if c["op"] in last and v < last[c["op"]]:
                    pairs[c["op"]] += 1
                last[c["op"]] = v
    print(dict(pairs))
    assert all(pairs[op] >= 3 for op in NEW_ARENA_OPS), dict(pairs)


def test_the_voxel_shares(calls):
    obs = observed(calls)
    changed, cleared, lethal = (share(obs, lambda c, k=k: c[k]) for k in ("changed", "cleared_marked", "lethal"))
    print("voxel_observe calls", len(obs), "changed a byte", changed, "cleared a marked voxel", cleared, "made a cell lethal", lethal)
    assert len(obs) >= 20 and changed >= 1 / 3 and cleared >= 1 / 3 and lethal >= 1 / 3


def test_rolls_resets_and_recreations_of_maps_with_voxels(calls):
    def partly(c):                                                       # moved, and some of the map survives
        (mx, my), (sx, sy) = c["moved"], c["size"]
        return (mx, my) != (0, 0) and abs(mx) < sx and abs(my) < sy
    rolls = sum(1 for c in calls if c["op"] == "roll" and c["vox_known"] and partly(c))
    resets = sum(1 for c in calls if c["op"] == "reset" and c["vox_known"])
    recreated = sum(c["had_voxels"] for c in calls if c["op"] == "recreate")
    print("rolls", rolls, "resets", resets, "recreated", recreated)
    assert rolls >= 3 and resets >= 3 and recreated >= 3


def test_the_planners_refusals_and_winners(calls):
    pl = [c for c in calls if c["op"] in PLANNERS]
    refused = share(pl, lambda c: c["refused"])
    causes = Counter(c["cause"] for c in pl if c["refused"])
    answered = [c for c in calls if c["op"] == "rollout_best" and not c["refused"]]
    valid = share(answered, lambda c: c["valid"])
    print("planner calls", len(pl), "refused", refused, dict(causes), "rollouts answered", len(answered), "valid winner", valid,
          "all rejected", sum(c["all_rejected"] for c in answered), "stages", sorted(Counter(c["stage"] for c in answered).items()))
    assert refused <= 1 / 2 and set(causes) >= {"observe", "voxel_observe", "roll", "recreate"}, (refused, dict(causes))
    for op in PLANNERS:
        assert any(c["refused"] for c in pl if c["op"] == op) and any(not c["refused"] for c in pl if c["op"] == op), op
    assert len(answered) >= 10 and valid >= 1 / 3 and any(c["all_rejected"] for c in answered)
    assert {c["stage"] for c in answered} == {1, 2, 3}
    dw = [c for c in calls if c["op"] == "dwa_best" and not c["refused"]]
    assert share(dw, lambda c: c["n_valid"] >= 1) >= 1 / 3 and any(c["n_valid"] == 0 for c in dw)


def test_voxel_entries_on_a_map_without_voxels(calls):
    n = Counter(c["op"] for c in calls if c["op"] in fz.VOXEL_OPS and c["refused"] and not c.get("twice"))
    twice = sum(1 for c in calls if c.get("twice"))
    print(dict(n), "attached twice", twice)
    assert sum(n.values()) >= 3 and len(n) >= 3 and twice >= 3


def test_the_host_twins_agree_along_the_chains(runs):
    """backend="host": besides the base profile's four twins, gem_voxlayer_host, gem_rollout_plan / gem_rollout_host and gem_trajgen_plan /
    gem_trajgen_generate against the model at every step that has one, on grids, columns and distance grids with a history; the draws do
    not depend on the backend"""
    for r in runs:
        assert repr(fz.scenario(r["seed"], "host", "full")["trace"]) == repr(r["trace"])


def test_a_scenario_is_deterministic_in_its_seed(runs):
    for r in runs[:4]:
        again = fz.scenario(r["seed"], "reference", "full")
        assert repr(again["trace"]) == repr(r["trace"]) and again["maps"] == r["maps"]
    assert repr(runs[0]["trace"]) != repr(runs[1]["trace"])
    base = fz.scenario(runs[0]["seed"], "reference")                     # the base profile of the same seed is another scenario, of base ops alone
    assert {c["op"] for c in base["trace"]} <= set(fz.OPS) and {g for _r, g in base["maps"]} <= set(fz.GEOMS)


def test_the_running_time_of_this_module():
    """printed for the record (the last test of the module: everything above has run)"""
    print(f"this module took {time.time() - T0:.1f} s for {len(SEEDS)} seeds")
