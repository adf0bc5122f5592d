"""The overlapping pair kernel (gem_amd/csrc/gem_frame_pair.hpp, gem_frame_pair.hip), without a GPU:
- the one pure host function it introduces -- frame_pair_same_map, the per-launch check that both fused sweeps describe the same map
  through the same tile map -- against a plain statement (tests/cpp/frame_pair_overlap_check.cpp), a stand-alone program built with
  the address and undefined-behaviour sanitizers on the host;
- the kernel keeps the lean form's budget (at most 64 VGPRs, 80 SGPRs, no vector spill, no scratch, no static LDS: eight workgroups
  per CU), preloads no kernel argument, and the parent's pair kernel is still in the library beside it.
Nothing is launched."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import code_objects  # noqa: E402


def test_same_map_against_a_plain_statement(tmp_path):
    from gem_amd.build import hipcc_path
    exe = tmp_path / "frame_pair_overlap_check"
    res = subprocess.run([hipcc_path(), "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                          "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                          str(ROOT / "tests" / "cpp" / "frame_pair_overlap_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
    m = re.search(r"fields (\d+) fails 0", run.stdout)
    assert m and int(m.group(1)) == 11, run.stdout


@pytest.fixture(scope="module")
def kernels():
    from gem_amd import build
    return code_objects.all_kernels(build.build(force=False))


def test_overlapping_kernel_keeps_the_budget(kernels):
    ks = [k for k in kernels if "pairov_k_frame" in k["name"]]
    assert len(ks) == 1, [k["name"] for k in ks]
    k = ks[0]
    print(k)
    assert k["vgpr"] <= 64 and k["sgpr"] <= 80 and k["vgpr_spill"] == 0 and k["scratch"] == 0, k
    assert k["preload"] == 0 and k["lds"] == 0, k                   # (no static LDS: the launch passes kFrameLds, eight of which fit a CU)


def test_parent_pair_kernel_stays(kernels):
    assert len([k for k in kernels if "pair_k_frame" in k["name"]]) == 1
