"""frame_tile's owner phase sized by the wave, without a GPU.

1. The sorting networks of gem_amd/csrc/gem_frame_sort.hpp on the host (tests/cpp/frame_sort_check.cpp, a host-only HIP build):
   for every size 2 / 4 / 8, every count up to the largest the size is picked for and every permutation of that many distinct keys
   padded with ~0u, the sized network returns what the full 8-key network returns.
2. The code objects: the lean production kernels k_frame<0, true> / <4, true> carry no stamp code, which shows as their scalar
   spills -- 2 / 4 words (8 / 12 with the stamps; 0 was the aim: what is left is the `owned` lane mask saved across the slow path
   and, with lowest tracking, that mask and a tile base across the prologue) -- and the stamped diagnostic kernels exist beside
   them, one per FLAGS, within the same budget of eight workgroups per CU."""
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))


def test_sized_networks_equal_the_full_network(tmp_path):
    from gem_amd.build import hipcc_path
    exe = tmp_path / "frame_sort_check"
    res = subprocess.run([hipcc_path(), "--offload-host-only", "-x", "hip", "-std=c++17", "-O2", "-Wall", "-Werror",
                          str(ROOT / "tests" / "cpp" / "frame_sort_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr


@pytest.fixture(scope="module")
def kernels():
    import code_objects
    from gem_amd import build
    return code_objects.all_kernels(build.build(force=False))


def one(kernels, sub):
    m = [k for k in kernels if sub in k["name"]]
    assert len(m) == 1, (sub, [k["name"] for k in m])
    return m[0]


@pytest.mark.parametrize("flags,spill", [(0, 2), (4, 4)])
def test_lean_production_kernel_scalar_spills(kernels, flags, spill):
    k = one(kernels, f"k_frameILi{flags}ELb1E")
    print(k)
    assert k["sgpr_spill"] <= spill, k


@pytest.mark.parametrize("flags", [0, 4])
def test_stamped_kernel_fits_eight_workgroups_per_cu(kernels, flags):
    k = one(kernels, f"k_frame_stampedILi{flags}E")
    print(k)
    assert k["vgpr"] <= 64 and k["sgpr"] <= 80 and k["vgpr_spill"] == 0 and k["scratch"] == 0, k
