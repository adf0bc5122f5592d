"""The head of k_frame's lean form (gem_amd/csrc/gem_frame_lean.hpp, gem_frame_lean.hip), without a GPU:
- frame_lean_head copies every word of the head from a filled argument block (tests/cpp/frame_lean_head_check.cpp, host-only build);
- the four lean kernels -- k_frame<0 / 4, true> and k_frame_stamped<0 / 4> -- are built with kernel-argument preloading and their
  kernel descriptors ask for exactly the head's dwords, 1..14 of them; every other kernel of the library asks for none (the flag
  acts on a whole translation unit: nothing else may have been compiled with it);
- the lean kernels keep their register budget with the 16 user SGPRs (tests/test_frame_lean_code_objects.py checks the production
  pair; here the stamped pair too).
Nothing is launched."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import code_objects  # noqa: E402


@pytest.fixture(scope="module")
def head_dwords(tmp_path_factory):
    from gem_amd.build import hipcc_path
    exe = tmp_path_factory.mktemp("head") / "frame_lean_head_check"
    res = subprocess.run([hipcc_path(), "--offload-host-only", "-x", "hip", "-std=c++17", "-O2", "-Wall", "-Werror",
                          str(ROOT / "tests" / "cpp" / "frame_lean_head_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
    return int(re.search(r"head dwords (\d+)", run.stdout).group(1))


@pytest.fixture(scope="module")
def kernels():
    from gem_amd import build
    ks = code_objects.all_kernels(build.build(force=False))
    assert len(ks) > 100, len(ks)
    return ks


def is_lean(name):
    return re.search(r"k_frameILi[04]ELb1EE", name) is not None or "k_frame_stampedILi" in name


def test_head_copies_every_word(head_dwords):
    assert 1 <= head_dwords <= 14, head_dwords


def test_lean_kernels_preload_the_head(kernels, head_dwords):
    lean = [k for k in kernels if is_lean(k["name"])]
    assert len(lean) == 4, [k["name"] for k in lean]
    for k in lean:
        print(k["name"], k["preload"])
        assert 1 <= k["preload"] <= 14 and k["preload"] == head_dwords, k


def test_no_other_kernel_preloads(kernels):
    others = [k for k in kernels if not is_lean(k["name"])]
    assert len(others) == len(kernels) - 4
    assert [k["name"] for k in others if k["preload"] != 0] == []


def test_lean_kernels_keep_their_budget(kernels):
    for k in kernels:
        if is_lean(k["name"]):
            assert k["vgpr"] <= 64 and k["sgpr"] <= 80 and k["vgpr_spill"] == 0 and k["scratch"] == 0, k
