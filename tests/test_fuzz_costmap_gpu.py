"""The costmap soak on the device: the scenarios of tools/fuzz_costmap.py -- random chains of every costmap operation on two to four
costmaps of one handle, small and large ones taking turns in the shared arenas -- compared step by step and exactly (bytes, int32, doubles
by ==) with the chained numpy references.  This is the test of what the costmap family keeps BETWEEN calls ("Between calls"):
scratch left clean, the cached inflation table, the roll's two grids, the generation numbers, ids handed out again.  A failure names
the seed, the step, the op and its arguments; `python -c "import sys; sys.path.insert(0, 'tools'); import fuzz_costmap as f;
f.scenario(SEED)"` reproduces it alone.  tests/test_fuzz_costmap_cpu.py asserts, without a GPU, what these seeds cover."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent)); sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import fuzz_costmap as fz  # noqa: E402
from test_fuzz_costmap_cpu import SEED_BLOCKS  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.one_pipeline]


@pytest.mark.parametrize("block", SEED_BLOCKS, ids=lambda b: f"seeds {b.start}-{b.stop - 1}")
def test_costmap_scenarios_equal_the_chained_references(block):
    calls = 0
    for seed in block:
        r = fz.scenario(seed, "device")                                  # AssertionError with seed, step, op and arguments on a mismatch
        calls += len(r["trace"])
    assert calls >= 20 * len(block)
