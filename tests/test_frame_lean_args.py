"""The argument block of k_frame's lean form on the host alone (gem_amd/csrc/gem_frame_lean.hpp, tests/cpp/frame_lean_check.cpp):
the multiply-high division of the block -> tile map, the map itself and the fill from FuseArgs / BinArgs.  A host-only HIP build:
runs without a GPU."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_lean_argument_block_division_tile_map_and_fill(tmp_path):
    from gem_amd.build import hipcc_path
    exe = tmp_path / "frame_lean_check"
    res = subprocess.run([hipcc_path(), "--offload-host-only", "-x", "hip", "-std=c++17", "-O2", "-Wall", "-Werror",
                          str(ROOT / "tests" / "cpp" / "frame_lean_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
