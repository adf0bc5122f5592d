"""Builds libgem_hip.so (gfx950) in-tree with hipcc.

The shared library is the product: hand-written HIP kernels + the C ABI of include/gem_hip.h.
It is built into gem_amd/lib/ so that it travels with the source tree (no JIT cache).
hipcc cross-compiles for gfx950 without a GPU present.
"""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent
CSRC = ROOT / "csrc"
LIBDIR = ROOT / "lib"
LIB = LIBDIR / "libgem_hip.so"

SOURCES = [CSRC / "gem_kernels.hip", CSRC / "gem_frame_lean.hip", CSRC / "gem_frame_pair.hip", CSRC / "gem_sort.hip", CSRC / "gem_capi.cpp", CSRC / "gem_capi_core.cpp", CSRC / "gem_capi_pipeline.cpp", CSRC / "gem_capi_comm.cpp",
           CSRC / "gem_clean.hip", CSRC / "gem_capi_clean.cpp", CSRC / "gem_local.hip", CSRC / "gem_capi_local.cpp",
           CSRC / "gem_voxel.hip", CSRC / "gem_capi_voxel.cpp", CSRC / "gem_global.hip", CSRC / "gem_capi_global.cpp",
           CSRC / "gem_compose.hip", CSRC / "gem_capi_compose.cpp", CSRC / "gem_costmap.hip", CSRC / "gem_capi_costmap.cpp",
           CSRC / "gem_octree.hip", CSRC / "gem_capi_octree.cpp", CSRC / "gem_depth.hip", CSRC / "gem_capi_depth.cpp",
           CSRC / "gem_history.hip", CSRC / "gem_capi_history.cpp",
           CSRC / "gem_footprint.hip", CSRC / "gem_capi_footprint.cpp", CSRC / "gem_inflate.hip", CSRC / "gem_capi_inflate.cpp",
           CSRC / "gem_mapgrid.hip", CSRC / "gem_mapgrid_tiled.hip", CSRC / "gem_capi_mapgrid.cpp", CSRC / "gem_critics.hip", CSRC / "gem_capi_critics.cpp",
           CSRC / "gem_trajgen.hip", CSRC / "gem_capi_trajgen.cpp", CSRC / "gem_navplan.hip", CSRC / "gem_capi_navplan.cpp", CSRC / "gem_navgrad.hip", CSRC / "gem_capi_navpath.cpp", CSRC / "gem_navquad.hip",
           CSRC / "gem_frontier.hip", CSRC / "gem_capi_frontier.cpp", CSRC / "gem_obstacle.hip", CSRC / "gem_capi_obstacle.cpp",
           CSRC / "gem_voxlayer.hip", CSRC / "gem_capi_voxlayer.cpp", CSRC / "gem_rollout.hip", CSRC / "gem_capi_rollout.cpp"]
HEADERS = [CSRC / "gem_device.hpp", CSRC / "gem_kernels.hpp", CSRC / "gem_frame_lean.hpp", CSRC / "gem_frame_pair.hpp", CSRC / "gem_frame_tile.hpp", CSRC / "gem_frame_sort.hpp", CSRC / "gem_wave.hpp", CSRC / "gem_compact.hpp", CSRC / "gem_transport.hpp", CSRC / "gem_hostcopy.hpp", CSRC / "gem_capi_internal.hpp", CSRC / "gem_plan.hpp", CSRC / "gem_clean.hpp", CSRC / "gem_local.hpp", CSRC / "gem_voxel.hpp", CSRC / "gem_global.hpp", CSRC / "gem_compose.hpp", CSRC / "gem_costmap.hpp", CSRC / "gem_lsd.hpp", CSRC / "gem_octree.hpp", CSRC / "gem_depth.hpp", CSRC / "gem_history.hpp", CSRC / "gem_footprint.hpp", CSRC / "gem_inflate.hpp", CSRC / "gem_mapgrid.hpp", CSRC / "gem_mapgrid_tiled.hpp", CSRC / "gem_score_device.hpp", CSRC / "gem_critics.hpp", CSRC / "gem_trajgen.hpp", CSRC / "gem_sincos.hpp",
           CSRC / "gem_navplan.hpp", CSRC / "gem_navpath.hpp", CSRC / "gem_navgrad.hpp", CSRC / "gem_navquad.hpp", ROOT.parent / "include" / "gem_hip_navpath.h", ROOT.parent / "include" / "gem_hip_navquad.h", CSRC / "gem_frontier.hpp", CSRC / "gem_costmap_host.hpp", CSRC / "gem_cost_pass.hpp", CSRC / "gem_observe_host.hpp", CSRC / "gem_rounds.hpp", CSRC / "gem_tile_round.hpp", CSRC / "gem_obstacle.hpp", CSRC / "gem_voxlayer.hpp", CSRC / "gem_rollout.hpp", ROOT.parent / "include" / "gem_hip_rollout.h", ROOT.parent / "include" / "gem_hip_voxlayer.h", ROOT.parent / "include" / "gem_hip_frontier.h", ROOT.parent / "include" / "gem_hip_obstacle.h",
           ROOT.parent / "include" / "gem_hip_debug.h", ROOT.parent / "include" / "gem_hip.h", ROOT.parent / "include" / "gem_hip_history.h",
           ROOT.parent / "include" / "gem_hip_footprint.h", ROOT.parent / "include" / "gem_hip_inflate.h", ROOT.parent / "include" / "gem_hip_mapgrid.h", ROOT.parent / "include" / "gem_hip_mapgrid_tiled.h",
           ROOT.parent / "include" / "gem_hip_critics.h", ROOT.parent / "include" / "gem_hip_trajgen.h", ROOT.parent / "include" / "gem_hip_navplan.h"]

# -ffp-contract=off: cell indices must be bit-exact with the reference arithmetic, so no product+sum
# may be contracted into an FMA (see csrc/gem_device.hpp).  hipcc's default IEEE divide/sqrt stay on.
FLAGS = [
    "--offload-arch=gfx950", "-O3", *(["-g"] if os.environ.get("GEM_DEBUG_BUILD") else []), "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
    "-Wno-unused-value", "-Wno-unused-result",
    *os.environ.get("GEM_BUILD_DEFINES", "").split(),          # build-time experiments (A/B builds on the GPU box), e.g. -DGEM_X=1
]

# Flags of one source alone, behind FLAGS.  gem_frame_lean.hip: the leading scalar parameters of k_frame's lean form are preloaded
# into user SGPRs (14 dwords, the hardware's limit); an -mllvm option acts on every kernel of a file, hence the file of its own.
SOURCE_FLAGS = {
    "gem_frame_lean.hip": ["-mllvm", "-amdgpu-kernarg-preload-count=14"],
}


def compile_flags(src: Path, extra=()) -> list:
    """The compile line's flags for `src`: FLAGS (GEM_BUILD_DEFINES among them), `extra`, then the source's own."""
    return [f for f in FLAGS if f != "-shared"] + list(extra) + SOURCE_FLAGS.get(src.name, [])


def flag_line(extra=()) -> str:
    """What a rebuild of every object is keyed on: the common flags and every source's own."""
    own = "".join(f" [{name}: {' '.join(fl)}]" for name, fl in sorted(SOURCE_FLAGS.items()))
    return " ".join(compile_flags(Path("-"), extra)) + own


def hipcc_path() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm to build libgem_hip.so)")


def is_stale() -> bool:
    if not LIB.exists():
        return True
    t = LIB.stat().st_mtime
    return any(p.stat().st_mtime > t for p in SOURCES + HEADERS)


def _stale(target: Path, deps) -> bool:
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any(p.stat().st_mtime > t for p in deps)


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile libgem_hip.so if missing or older than its sources.  Returns its path.
    One object per source (gem_amd/lib/obj, compiled side by side; only what changed is recompiled), then one link."""
    if not force and not is_stale():
        return LIB
    LIBDIR.mkdir(exist_ok=True)
    objdir = LIBDIR / "obj"
    objdir.mkdir(exist_ok=True)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    tag = objdir / ".flags"
    line = flag_line()
    if not tag.exists() or tag.read_text() != line:                    # different flags (GEM_BUILD_DEFINES, GEM_DEBUG_BUILD, a source's own): everything again
        force = True
    jobs = []
    for src in SOURCES:
        obj = objdir / (src.stem + ".o")
        if force or _stale(obj, [src] + HEADERS):
            cmd = [hipcc_path(), *compile_flags(src), "-c", str(src), "-o", str(obj)]
            if verbose:
                print(" ".join(cmd))
            jobs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    errors = []
    for src, proc in jobs:
        out, _ = proc.communicate()
        if proc.returncode != 0:
            errors.append(f"{src.name}: hipcc failed ({proc.returncode}):\n{out}")
    if errors:
        raise RuntimeError("\n".join(errors))
    tag.write_text(line)
    cmd = [hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC", *[str(objdir / (s.stem + ".o")) for s in SOURCES], "-o", str(LIB),
           f"-L{rocm}/lib", "-lrccl", "-pthread", f"-Wl,-rpath,{rocm}/lib"]
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc (link) failed ({res.returncode}):\n{res.stdout}\n{res.stderr}")
    return LIB


def build_variant(name: str, defines: str, verbose: bool = False) -> Path:
    """An A/B build with extra -D flags into gem_amd/lib_ab/<name>/libgem_hip.so (tools only: tools/ab_run.sh copies it over the
    library of the GPU box's scratch copy of the tree, variant by variant; the product library here is not touched)."""
    out = ROOT / "lib_ab" / name
    objdir = out / "obj"
    objdir.mkdir(parents=True, exist_ok=True)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    jobs = []
    for src in SOURCES:
        obj = objdir / (src.stem + ".o")
        cmd = [hipcc_path(), *compile_flags(src, defines.split()), "-c", str(src), "-o", str(obj)]
        if verbose:
            print(" ".join(cmd))
        jobs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for src, proc in jobs:
        o, _ = proc.communicate()
        if proc.returncode != 0:
            raise RuntimeError(f"{src.name}: hipcc failed ({proc.returncode}):\n{o}")
    lib = out / "libgem_hip.so"
    res = subprocess.run([hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC", *[str(objdir / (s.stem + ".o")) for s in SOURCES], "-o", str(lib),
                          f"-L{rocm}/lib", "-lrccl", "-pthread", f"-Wl,-rpath,{rocm}/lib"], capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc (link) failed ({res.returncode}):\n{res.stdout}\n{res.stderr}")
    return lib


if __name__ == "__main__":
    import sys
    if len(sys.argv) >= 3 and sys.argv[1] == "--variant":          # python -m gem_amd.build --variant NAME "-DX=1 -DY=2"
        print(build_variant(sys.argv[2], " ".join(sys.argv[3:]), verbose=True))
    else:
        print(build(force=True, verbose=True))
