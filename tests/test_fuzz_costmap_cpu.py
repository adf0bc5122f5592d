"""What the costmap soak (tools/fuzz_costmap.py, tests/test_fuzz_costmap_gpu.py) covers, asserted without a GPU: the scenarios of the
committed seed blocks run with backend="reference", which drives the model and the numpy references alone, and their op traces are
counted.  A random generator's coverage cannot be taken for granted; these shares are conditions on the INPUTS of the GPU test, met by
the generator's probabilities and the choice of seeds, not measurements of the library."""
import sys
from collections import Counter, defaultdict
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import fuzz_costmap as fz  # noqa: E402

# the blocks of consecutive seeds tests/test_fuzz_costmap_gpu.py runs, one parametrised case per block
SEED_BLOCKS = [range(1000, 1008), range(1008, 1016), range(1016, 1024)]
SEEDS = [s for b in SEED_BLOCKS for s in b]
OP_KINDS = list(fz.OPS)
ARENA_OPS = fz.ARENA_OPS


@pytest.fixture(scope="module")
def runs():
    return [fz.scenario(s, "reference") for s in SEEDS]


@pytest.fixture(scope="module")
def calls(runs):
    return [c for r in runs for c in r["trace"]]


def share(cs, pred):
    return sum(1 for c in cs if pred(c)) / max(len(cs), 1)


def test_the_blocks_are_what_the_issue_sizes(runs):
    assert 20 <= len(SEEDS) <= 30 and len(set(SEEDS)) == len(SEEDS)
    for r in runs:
        assert 20 <= r["steps"] <= 30 and 2 <= len(r["maps"]) <= 4
        assert r["maps"][0][1] == r["maps"][1][1] and (r["maps"][0][0], r["maps"][1][0]) == ("layer", "master")     # merge's pair


def test_every_op_kind_occurs_at_least_five_times(calls):
    n = Counter(c["op"] for c in calls)
    print(sorted(n.items()))
    assert all(n[k] >= 5 for k in OP_KINDS), {k: n[k] for k in OP_KINDS if n[k] < 5}
    # the forms inside a kind
    assert {c["form"] for c in calls if c["op"] == "roll"} == {"update_origin", "roll_to"}
    assert {c["kind"] for c in calls if c["op"] == "roll"} == {"zero", "few", "negative", "far"}
    assert {(c["on_device"], c["bounds"]) for c in calls if c["op"] == "mark_points"} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {c["on_device"] for c in calls if c["op"] == "observe"} == {False, True}
    assert {c["n_obs"] for c in calls if c["op"] == "observe"} >= {1, 2, 3}
    assert {f for c in calls if c["op"] == "observe" for f in c["flags"]} == {(True, True), (False, True), (True, False)}
    assert {m for c in calls if c["op"] == "observe" for m in c["on_map"]} == {False, True}
    inf = float("inf")
    assert any(r == inf for c in calls if c["op"] == "observe" for r in c["ranges"]) and any(r < inf for c in calls if c["op"] == "observe" for r in c["ranges"])
    assert {(c["mode"], c["window"] is None) for c in calls if c["op"] == "merge"} == {(m, w) for m in (0, 1) for w in (False, True)}
    assert {(c["params"][3], c["window"] is None) for c in calls if c["op"] == "inflate"} == {(u, w) for u in (False, True) for w in (False, True)}
    assert {c["slot"] for c in calls if c["op"] == "read_map_grid"} == set(fz.SLOTS)
    assert any(c["refusal"] for c in calls if c["op"] == "best_trajectory") and any(not c["refusal"] for c in calls if c["op"] == "best_trajectory")
    assert any(k == fz.cr.MAPGRID for c in calls if c["op"] == "best_trajectory" and not c["refusal"] for k, _g, _f, _s in c["critics"])


def test_every_geometry_occurs(runs, calls):
    seen = {g for r in runs for _role, g in r["maps"]} | {c["geom"] for c in calls}
    assert seen == set(fz.GEOMS), set(fz.GEOMS) - seen
    cells = {g: x * y for g, (x, y) in fz.GEOMS.items()}
    assert any(v < 8192 for v in cells.values()) and any(v > 8192 for v in cells.values())          # kCostLdsCells, either side
    assert {63, 64, 65, 129} <= {v for xy in fz.GEOMS.values() for v in xy}                           # kNavTile's seams
    for op in ARENA_OPS:                                                 # each on a strip, a 1 x N map and the largest
        assert {c["geom"] for c in calls if c["op"] == op} >= {"65x3", "1x70", "130x129"}, op


def test_the_debug_keys_take_both_values(calls):
    assert {c["direct"] for c in calls if c["op"] == "observe"} == {0, 1}
    for op in ("nav_plan", "frontiers"):
        chunks = {c["chunk"] for c in calls if c["op"] == op}
        assert 0 in chunks and any(0 < k <= 3 for k in chunks), (op, chunks)


def test_the_shares(calls):
    obs = [c for c in calls if c["op"] == "observe"]
    assert share(obs, lambda c: c["changed"]) >= 1 / 3 and share(obs, lambda c: c["cleared_lethal"]) >= 1 / 3
    plans = [c for c in calls if c["op"] == "nav_plan"]
    assert share(plans, lambda c: not c["found"]) <= 1 / 3
    searches = [c for c in calls if c["op"] == "frontiers" and c["fresh"]]
    assert len(searches) >= 5 and share(searches, lambda c: c["n_kept"] == 0) <= 1 / 3
    rolls = [c for c in calls if c["op"] == "roll"]

    def partly(c):                                                       # moved, and some of the map survives
        (mx, my), (sx, sy) = c["moved"], c["size"]
        return (mx, my) != (0, 0) and abs(mx) < sx and abs(my) < sy
    assert share(rolls, partly) >= 1 / 3
    print("observe changed", share(obs, lambda c: c["changed"]), "cleared lethal", share(obs, lambda c: c["cleared_lethal"]),
          "not found", share(plans, lambda c: not c["found"]), "no frontier kept", share(searches, lambda c: c["n_kept"] == 0), "rolls partly", share(rolls, partly))


def test_inflation_keys_recur_and_change_on_one_map(calls):
    infl = [c for c in calls if c["op"] == "inflate" and c["same_key"] is not None and c["seeds"] > 0]
    assert sum(c["same_key"] for c in infl) >= 3 and sum(not c["same_key"] for c in infl) >= 3


def test_a_small_map_follows_a_larger_one_in_every_shared_arena(runs):
    """per handle, consecutive calls of one op kind: an op's scratch arenas are touched by that op alone, so `directly after` is counted
    in the sequence of that op's calls"""
    pairs = Counter()
    for r in runs:
        last = {}
        for c in r["trace"]:
            if c["op"] in ARENA_OPS and not (c["op"] == "frontiers" and not c["fresh"]) and not (c["op"] == "observe" and c["n_obs"] == 0):
                if c["op"] in last and c["cells"] < last[c["op"]]:
                    pairs[c["op"]] += 1
                last[c["op"]] = c["cells"]
    print(dict(pairs))
    assert all(pairs[op] >= 3 for op in ARENA_OPS), dict(pairs)


def test_stale_and_fresh_reads_of_everything(calls):
    n = defaultdict(Counter)
    for c in calls:
        if c["op"] in ("read_potential", "read_frontiers", "read_map_grid", "nav_plan_to", "score_map_grid"):
            n[c["op"]][c["fresh"]] += 1
    print({k: dict(v) for k, v in n.items()})
    for op in ("read_potential", "read_frontiers", "read_map_grid"):
        assert n[op][True] >= 1 and n[op][False] >= 1, (op, dict(n[op]))
    assert n["read_potential"][True] >= 3 and n["read_frontiers"][True] >= 3 and n["read_map_grid"][True] >= 3


def test_an_id_is_reused(calls):
    assert sum(c["group"] for c in calls if c["op"] == "recreate") >= 3


def test_the_host_twins_agree_along_the_chains(runs):
    """backend="host": gem_navplan_host, gem_frontiers_host, gem_obstacle_host and gem_inflation_table against the model at every step
    that has one, on grids with a history; the draws do not depend on the backend"""
    for r in runs:
        assert repr(fz.scenario(r["seed"], "host")["trace"]) == repr(r["trace"])


def test_a_scenario_is_deterministic_in_its_seed(runs):
    for r in runs[:4]:
        again = fz.scenario(r["seed"], "reference")
        assert repr(again["trace"]) == repr(r["trace"]) and again["maps"] == r["maps"]
    assert repr(runs[0]["trace"]) != repr(runs[1]["trace"])
