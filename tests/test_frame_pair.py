"""Two sweeps per k_frame launch (gem_amd/csrc/gem_frame_pair.hpp, gem_frame_pair.hip), without a GPU:
- the hold / pair / flush decision is a pure host function: tests/cpp/frame_pair_check.cpp runs every sequence of up to 8 events
  (pairable add, add that may not share a launch, flush) against a plain model -- every sweep binned once and fused once, in call
  order, nothing put off behind a flush;
- the pair kernel keeps the lean form's budget (at most 64 VGPRs, 80 SGPRs, no vector spill, no scratch: eight workgroups per CU)
  and preloads no kernel argument (it is not in the lean kernels' translation unit).
Nothing is launched."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import code_objects  # noqa: E402


def test_every_sequence_of_events(tmp_path):
    from gem_amd.build import hipcc_path
    exe = tmp_path / "frame_pair_check"
    res = subprocess.run([hipcc_path(), "--offload-host-only", "-x", "hip", "-std=c++17", "-O2", "-Wall", "-Werror",
                          str(ROOT / "tests" / "cpp" / "frame_pair_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
    m = re.search(r"sequences (\d+) pairs (\d+) held_flushed (\d+)", run.stdout)
    assert int(m.group(1)) == sum(3 ** n for n in range(1, 9)) and int(m.group(2)) > 0 and int(m.group(3)) > 0, run.stdout


@pytest.fixture(scope="module")
def pair_kernels():
    from gem_amd import build
    ks = [k for k in code_objects.all_kernels(build.build(force=False)) if "pair_k_frame" in k["name"]]
    assert len(ks) == 1, [k["name"] for k in ks]
    return ks


def test_pair_kernel_keeps_the_budget(pair_kernels):
    for k in pair_kernels:
        print(k)
        assert k["vgpr"] <= 64 and k["sgpr"] <= 80 and k["vgpr_spill"] == 0 and k["scratch"] == 0, k


def test_pair_kernel_preloads_nothing(pair_kernels):
    for k in pair_kernels:
        assert k["preload"] == 0, k
