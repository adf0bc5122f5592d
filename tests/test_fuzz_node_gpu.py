"""A short node-cycle soak inside the GPU suite: tools/fuzz_node.py's scenarios (random map sizes -- one of them L = 1025 --, starting
capacities, trajectories, front ends and pipeline knobs, drawn inside the scenario), the device local map and submap stack in the
node's order every frame, bit for bit against the oracle and the restatements."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))


@pytest.mark.gpu
@pytest.mark.one_pipeline
@pytest.mark.parametrize("seeds,frames", [((8_100_000,), 6), ((8_100_001, 8_100_002, 8_100_003, 8_100_004, 8_100_005, 8_100_006), None)])
def test_random_node_cycles_match(oracle_mod, seeds, frames):
    import fuzz_node
    spilled = 0
    for seed in seeds:
        spilled += fuzz_node.scenario(seed, frames)["spilled"]        # raises AssertionError with the seed on a mismatch
    assert spilled > 0
