"""The register budget of k_frame's lean form, read from the built gfx950 code objects (tools/code_objects.py metadata only).

The lean form (k_frame<FLAGS, true>) is declared for eight workgroups of 256 threads per CU.  The CU admits that many only if a
wave needs at most 64 VGPRs AND at most 80 SGPRs (min(8, 800 / (sgprs rounded up to 16, + 16)) blocks of four waves), and a private
segment would put memory traffic into a latency-bound kernel.  The generic form keeps its own budget of six per CU.
CPU-only: nothing is launched."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import code_objects  # noqa: E402


@pytest.fixture(scope="module")
def frame_kernels():
    from gem_amd import build
    ks = [k for k in code_objects.all_kernels(build.build(force=False)) if "k_frameILi" in k["name"]]
    assert ks, "no k_frame instantiation in the library"
    return ks


def pick(ks, flags, lean):
    m = [k for k in ks if f"k_frameILi{flags}ELb{int(lean)}E" in k["name"]]
    assert len(m) == 1, (flags, lean, [k["name"] for k in ks])
    return m[0]


@pytest.mark.parametrize("flags", [0, 4])
def test_lean_form_fits_eight_workgroups_per_cu(frame_kernels, flags):
    k = pick(frame_kernels, flags, True)
    print(k)
    assert k["vgpr"] <= 64, k
    assert k["sgpr"] <= 80, k
    assert k["vgpr_spill"] == 0, k
    assert k["scratch"] == 0, k


@pytest.mark.parametrize("flags", [0, 4])
def test_generic_form_keeps_its_budget(frame_kernels, flags):
    k = pick(frame_kernels, flags, False)
    print(k)
    assert k["vgpr"] <= 80, k
