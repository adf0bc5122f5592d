"""The full profile of the costmap soak on the device: the scenarios of tools/fuzz_costmap.py with profile="full" -- the base profile's
chains with the voxel layer, the tiled MapGrid, the trajectory rollout and DWA among them, on maps up to 513 x 66, 70 x 520 and
1 x 4100 -- compared step by step and exactly (bytes, voxel columns, int32, doubles by ==, the rollout's 64 answer bytes) with the
chained numpy references.  This is the test of what those features keep BETWEEN calls ("Between calls"): the voxel scratch
all maps share left all-zero, the two column grids a roll flips between, the bounds words four entries share, the slots and the
generation both prepares write, the planners' arenas.  A failure names the seed, the step, the op and its arguments; `python -c "import
sys; sys.path.insert(0, 'tools'); import fuzz_costmap as f; f.scenario(SEED, profile='full')"` reproduces it alone.
tests/test_fuzz_costmap_full_cpu.py asserts, without a GPU, what these seeds cover."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent)); sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import fuzz_costmap as fz  # noqa: E402
from test_fuzz_costmap_full_cpu import FULL_SEED_BLOCKS  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]


@pytest.mark.parametrize("block", FULL_SEED_BLOCKS, ids=lambda b: f"seeds {b.start}-{b.stop - 1}")
def test_full_costmap_scenarios_equal_the_chained_references(block):
    calls = 0
    for seed in block:
        r = fz.scenario(seed, "device", "full")                          # AssertionError with seed, step, op and arguments on a mismatch
        calls += len(r["trace"])
    assert calls >= 20 * len(block)
