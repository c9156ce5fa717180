"""Build libmi_nerf.so, libmi_nerf_iqa.so, libmi_nerf_occ.so, libmi_nerf_scene.so, libmi_nerf_mesh.so, libmi_nerf_geo.so and libmi_nerf_pose.so with hipcc for gfx950 (cross-compiles without a GPU).

    python -m nerf_pytorch_paeng_amd.build [--force]          the shipped libraries (clean build: ~1 min 20 s on 8 cores)
    python -m nerf_pytorch_paeng_amd.build --variant TAG -DFOO -DBAR=1     an A/B variant (tools/ab_probe.py)
    python -m nerf_pytorch_paeng_amd.build --diag             the -DMN_DIAG variant (s_memtime stamps; never shipped or timed)
    python -m nerf_pytorch_paeng_amd.build --clean            remove every object and every variant

What lands where:
  nerf_pytorch_paeng_amd/libmi_nerf.so (+ .stamp)   the ONE artefact inside the package: git-ignored, NOT gpurun-ignored, so it travels
                                                    with the repository snapshot to the GPU box.  The stamp is a hash of every source,
                                                    header and flag: the library is up to date iff the stamp matches (no mtimes, no
                                                    objects needed -- the GPU box gets neither).
  nerf_pytorch_paeng_amd/libmi_nerf_iqa.so (+ .stamp)   the image-quality metrics (include/mi_nerf_iqa.h, csrc/iqa.hip): a library of its own with a stamp
                                                    of its own; libmi_nerf.so's sources and stamp inputs do not know it.
  nerf_pytorch_paeng_amd/libmi_nerf_occ.so (+ .stamp)   occupancy-grid rendering (include/mi_nerf_occ.h, csrc/occ.hip): a third library with a stamp of its
                                                    own, linked against libmi_nerf.so (rpath $ORIGIN), whose public entries it calls.
  nerf_pytorch_paeng_amd/libmi_nerf_scene.so (+ .stamp) procedural solid scenes (include/mi_nerf_scene.h, csrc/scene.hip): a fourth library with a stamp
                                                    of its own; it includes no other header and links against no other library of the project.
  nerf_pytorch_paeng_amd/libmi_nerf_mesh.so (+ .stamp)  mesh extraction (include/mi_nerf_mesh.h, csrc/mesh.hip): a fifth library with a stamp of its own,
                                                    linked against libmi_nerf.so (rpath $ORIGIN) like libmi_nerf_occ.so.
  nerf_pytorch_paeng_amd/libmi_nerf_geo.so (+ .stamp)   geometry losses (include/mi_nerf_geo.h, csrc/geo.hip): a sixth library with a stamp of its own; it
                                                    includes csrc/common.h and csrc/stage_dev.h and links against no other library of the project.
  nerf_pytorch_paeng_amd/libmi_nerf_pose.so (+ .stamp)  ray and pose gradients (include/mi_nerf_pose.h, csrc/pose.hip): a seventh library with a stamp of its
                                                    own; it includes csrc/common.h and links against no other library of the project.
  build_scratch/obj/                                objects of the shipped library (cache; tests/test_packing_cpu.py disassembles them)
  build_scratch/obj_TAG/, build_scratch/libmi_nerf_TAG.so    variants.  build_scratch/ is git-ignored AND gpurun-ignored: a variant is
                                                    built where it is used (tools/ab_probe.py builds the ones it is asked for on the box).
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(ROOT, "include")
SCRATCH = os.path.join(ROOT, "build_scratch")
LIB = os.path.join(HERE, "libmi_nerf.so")
STAMP = LIB + ".stamp"
SOURCES = ["api.hip", "stages.hip", "mlp_fp32.hip", "mlp_fp32_wide.hip", "mlp_bf16.hip", "mlp_f16.hip", "mlp_f16s.hip", "mlp_f16s_stash.hip", "dgrad_f16s.hip", "mlp_train.hip", "frames.hip", "comm.hip", "pack.cpp", "pack_half.hip"]
# libmi_nerf_iqa.so: its own sources and its own header; common.h and mi_nerf.h are not part of it
IQA_LIB = os.path.join(HERE, "libmi_nerf_iqa.so")
IQA_STAMP = IQA_LIB + ".stamp"
IQA_SOURCES = ["iqa.hip"]
# libmi_nerf_occ.so: its own source and header; it includes mi_nerf.h (types, public entries) and links against libmi_nerf.so
OCC_LIB = os.path.join(HERE, "libmi_nerf_occ.so")
OCC_STAMP = OCC_LIB + ".stamp"
OCC_SOURCES = ["occ.hip"]
# libmi_nerf_scene.so: its own source and its own header, nothing else
SCENE_LIB = os.path.join(HERE, "libmi_nerf_scene.so")
SCENE_STAMP = SCENE_LIB + ".stamp"
SCENE_SOURCES = ["scene.hip"]
# libmi_nerf_mesh.so: its own source and header; it includes mi_nerf.h (types, three public entries) and links against libmi_nerf.so
MESH_LIB = os.path.join(HERE, "libmi_nerf_mesh.so")
MESH_STAMP = MESH_LIB + ".stamp"
MESH_SOURCES = ["mesh.hip"]
# libmi_nerf_geo.so: its own source and header; it shares common.h / stage_dev.h with libmi_nerf.so at compile time and nothing at link time
GEO_LIB = os.path.join(HERE, "libmi_nerf_geo.so")
GEO_STAMP = GEO_LIB + ".stamp"
GEO_SOURCES = ["geo.hip"]
# libmi_nerf_pose.so: its own source and header; it shares common.h with libmi_nerf.so at compile time and nothing at link time
POSE_LIB = os.path.join(HERE, "libmi_nerf_pose.so")
POSE_STAMP = POSE_LIB + ".stamp"
POSE_SOURCES = ["pose.hip"]
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function",
         # the MLP kernel's register-resident design needs its k-loops FULLY unrolled (static register indices)
         "-mllvm", "-pragma-unroll-threshold=1000000"]
# mlp_bf16.hip / mlp_f16.hip manage the whole AGPR file by hand (explicit a[N] operands in asm statements): hipcc must not park spilled VGPRs there
FILE_FLAGS = {"mlp_bf16.hip": ["-mllvm", "-amdgpu-spill-vgpr-to-agpr=0"], "mlp_f16.hip": ["-mllvm", "-amdgpu-spill-vgpr-to-agpr=0"],
              "mlp_f16s.hip": ["-mllvm", "-amdgpu-spill-vgpr-to-agpr=0"],
              "mlp_f16s_stash.hip": ["-mllvm", "-amdgpu-spill-vgpr-to-agpr=0"], "dgrad_f16s.hip": ["-mllvm", "-amdgpu-spill-vgpr-to-agpr=0"]}


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the MI355X path cannot be built (there is no CPU fallback)")
    return exe


def _headers():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join(INCLUDE, "mi_nerf.h")]


def _iqa_headers():
    return [os.path.join(INCLUDE, "mi_nerf_iqa.h")]


def _occ_headers():
    return [os.path.join(INCLUDE, "mi_nerf_occ.h"), os.path.join(INCLUDE, "mi_nerf.h")]


def _scene_headers():
    return [os.path.join(INCLUDE, "mi_nerf_scene.h")]


def _mesh_headers():
    return [os.path.join(INCLUDE, "mi_nerf_mesh.h"), os.path.join(INCLUDE, "mi_nerf.h")]


def _geo_headers():
    return [os.path.join(INCLUDE, "mi_nerf_geo.h"), os.path.join(CSRC, "common.h"), os.path.join(CSRC, "stage_dev.h"), os.path.join(INCLUDE, "mi_nerf.h")]


def _digest(paths, extra=()) -> str:
    h = hashlib.sha256()
    for p in paths:
        h.update(os.path.basename(p).encode())
        with open(p, "rb") as fh:
            h.update(fh.read())
    h.update(repr(list(extra)).encode())
    return h.hexdigest()


def source_stamp(defines=()) -> str:
    """Hash of everything the library is made of: sources, headers, flags (and a variant's -D list)."""
    return _digest([os.path.join(CSRC, s) for s in SOURCES] + _headers(), [FLAGS, sorted(FILE_FLAGS.items()), list(defines)])


def object_dir(tag: str = "") -> str:
    return os.path.join(SCRATCH, "obj" + ("_" + tag if tag else ""))


def _compile(src: str, force: bool, extra=(), tag: str = "", headers=None) -> str:
    """One translation unit -> build_scratch/obj[_TAG]/SRC.o, skipped when the object's own stamp (source + headers + flags) matches."""
    bdir = object_dir(tag)
    os.makedirs(bdir, exist_ok=True)
    obj = os.path.join(bdir, src + ".o")
    spath = os.path.join(CSRC, src)
    cmd_flags = [*FLAGS, *FILE_FLAGS.get(src, []), *extra]
    want = _digest([spath] + (_headers() if headers is None else headers), cmd_flags)
    stamp = obj + ".stamp"
    if not force and os.path.exists(obj) and os.path.exists(stamp) and open(stamp).read() == want:
        return obj
    r = subprocess.run([_hipcc(), *cmd_flags, "-x", "hip", "-c", spath, "-o", obj], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
    if r.stderr.strip():
        sys.stderr.write(r.stderr)
    with open(stamp, "w") as fh:
        fh.write(want)
    return obj


def ensure_object(src: str) -> str:
    """The shipped library's object of one source (compiled on demand): what the object checks of tests/test_packing_cpu.py read."""
    return _compile(src, False)


def _link(objs, lib: str, extra=()) -> None:
    r = subprocess.run([_hipcc(), "-shared", "-fPIC", f"--offload-arch={ARCH}", *objs, *extra, "-o", lib], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")


def build_library(force: bool = False, verbose: bool = False) -> str:
    want = source_stamp()
    if not force and os.path.exists(LIB) and os.path.exists(STAMP) and open(STAMP).read() == want:
        if verbose:
            print(f"up to date: {LIB} ({os.path.getsize(LIB) / 1024:.0f} KiB, stamp {want[:16]})")
        return LIB
    with ThreadPoolExecutor(max_workers=6) as ex:
        objs = list(ex.map(lambda s: _compile(s, force), SOURCES))
    _link(objs, LIB)
    with open(STAMP, "w") as fh:
        fh.write(want)
    if verbose:
        print(f"built {LIB} ({os.path.getsize(LIB) / 1024:.0f} KiB, stamp {want[:16]})")
    return LIB


def iqa_source_stamp() -> str:
    return _digest([os.path.join(CSRC, s) for s in IQA_SOURCES] + _iqa_headers(), [FLAGS])


def build_iqa_library(force: bool = False, verbose: bool = False) -> str:
    """libmi_nerf_iqa.so, a no-op when its stamp matches (like build_library)."""
    want = iqa_source_stamp()
    if not force and os.path.exists(IQA_LIB) and os.path.exists(IQA_STAMP) and open(IQA_STAMP).read() == want:
        if verbose:
            print(f"up to date: {IQA_LIB} ({os.path.getsize(IQA_LIB) / 1024:.0f} KiB, stamp {want[:16]})")
        return IQA_LIB
    objs = [_compile(s, force, headers=_iqa_headers()) for s in IQA_SOURCES]
    _link(objs, IQA_LIB)
    with open(IQA_STAMP, "w") as fh:
        fh.write(want)
    if verbose:
        print(f"built {IQA_LIB} ({os.path.getsize(IQA_LIB) / 1024:.0f} KiB, stamp {want[:16]})")
    return IQA_LIB


OCC_LINK = ["-L" + HERE, "-lmi_nerf", "-Wl,-rpath,$ORIGIN"]


def occ_source_stamp() -> str:
    return _digest([os.path.join(CSRC, s) for s in OCC_SOURCES] + _occ_headers(), [FLAGS, OCC_LINK[1:]])


def build_occ_library(force: bool = False, verbose: bool = False) -> str:
    """libmi_nerf_occ.so, a no-op when its stamp matches (like build_library).  It links against libmi_nerf.so, which is built first."""
    build_library()
    want = occ_source_stamp()
    if not force and os.path.exists(OCC_LIB) and os.path.exists(OCC_STAMP) and open(OCC_STAMP).read() == want:
        if verbose:
            print(f"up to date: {OCC_LIB} ({os.path.getsize(OCC_LIB) / 1024:.0f} KiB, stamp {want[:16]})")
        return OCC_LIB
    objs = [_compile(s, force, headers=_occ_headers()) for s in OCC_SOURCES]
    _link(objs, OCC_LIB, OCC_LINK)
    with open(OCC_STAMP, "w") as fh:
        fh.write(want)
    if verbose:
        print(f"built {OCC_LIB} ({os.path.getsize(OCC_LIB) / 1024:.0f} KiB, stamp {want[:16]})")
    return OCC_LIB


def scene_source_stamp() -> str:
    return _digest([os.path.join(CSRC, s) for s in SCENE_SOURCES] + _scene_headers(), [FLAGS])


def build_scene_library(force: bool = False, verbose: bool = False) -> str:
    """libmi_nerf_scene.so, a no-op when its stamp matches (like build_library)."""
    want = scene_source_stamp()
    if not force and os.path.exists(SCENE_LIB) and os.path.exists(SCENE_STAMP) and open(SCENE_STAMP).read() == want:
        if verbose:
            print(f"up to date: {SCENE_LIB} ({os.path.getsize(SCENE_LIB) / 1024:.0f} KiB, stamp {want[:16]})")
        return SCENE_LIB
    objs = [_compile(s, force, headers=_scene_headers()) for s in SCENE_SOURCES]
    _link(objs, SCENE_LIB)
    with open(SCENE_STAMP, "w") as fh:
        fh.write(want)
    if verbose:
        print(f"built {SCENE_LIB} ({os.path.getsize(SCENE_LIB) / 1024:.0f} KiB, stamp {want[:16]})")
    return SCENE_LIB


def mesh_source_stamp() -> str:
    return _digest([os.path.join(CSRC, s) for s in MESH_SOURCES] + _mesh_headers(), [FLAGS, OCC_LINK[1:]])


def build_mesh_library(force: bool = False, verbose: bool = False) -> str:
    """libmi_nerf_mesh.so, a no-op when its stamp matches (like build_library).  It links against libmi_nerf.so, which is built first."""
    build_library()
    want = mesh_source_stamp()
    if not force and os.path.exists(MESH_LIB) and os.path.exists(MESH_STAMP) and open(MESH_STAMP).read() == want:
        if verbose:
            print(f"up to date: {MESH_LIB} ({os.path.getsize(MESH_LIB) / 1024:.0f} KiB, stamp {want[:16]})")
        return MESH_LIB
    objs = [_compile(s, force, headers=_mesh_headers()) for s in MESH_SOURCES]
    _link(objs, MESH_LIB, OCC_LINK)
    with open(MESH_STAMP, "w") as fh:
        fh.write(want)
    if verbose:
        print(f"built {MESH_LIB} ({os.path.getsize(MESH_LIB) / 1024:.0f} KiB, stamp {want[:16]})")
    return MESH_LIB


def geo_source_stamp() -> str:
    return _digest([os.path.join(CSRC, s) for s in GEO_SOURCES] + _geo_headers(), [FLAGS])


def build_geo_library(force: bool = False, verbose: bool = False) -> str:
    """libmi_nerf_geo.so, a no-op when its stamp matches (like build_library).  It links against no other library of the project."""
    want = geo_source_stamp()
    if not force and os.path.exists(GEO_LIB) and os.path.exists(GEO_STAMP) and open(GEO_STAMP).read() == want:
        if verbose:
            print(f"up to date: {GEO_LIB} ({os.path.getsize(GEO_LIB) / 1024:.0f} KiB, stamp {want[:16]})")
        return GEO_LIB
    objs = [_compile(s, force, headers=_geo_headers()) for s in GEO_SOURCES]
    _link(objs, GEO_LIB)
    with open(GEO_STAMP, "w") as fh:
        fh.write(want)
    if verbose:
        print(f"built {GEO_LIB} ({os.path.getsize(GEO_LIB) / 1024:.0f} KiB, stamp {want[:16]})")
    return GEO_LIB


def _pose_headers():
    return [os.path.join(INCLUDE, "mi_nerf_pose.h"), os.path.join(CSRC, "common.h"), os.path.join(INCLUDE, "mi_nerf.h")]


def pose_source_stamp() -> str:
    return _digest([os.path.join(CSRC, s) for s in POSE_SOURCES] + _pose_headers(), [FLAGS])


def build_pose_library(force: bool = False, verbose: bool = False) -> str:
    """libmi_nerf_pose.so, a no-op when its stamp matches (like build_library).  It links against no other library of the project."""
    want = pose_source_stamp()
    if not force and os.path.exists(POSE_LIB) and os.path.exists(POSE_STAMP) and open(POSE_STAMP).read() == want:
        if verbose:
            print(f"up to date: {POSE_LIB} ({os.path.getsize(POSE_LIB) / 1024:.0f} KiB, stamp {want[:16]})")
        return POSE_LIB
    objs = [_compile(s, force, headers=_pose_headers()) for s in POSE_SOURCES]
    _link(objs, POSE_LIB)
    with open(POSE_STAMP, "w") as fh:
        fh.write(want)
    if verbose:
        print(f"built {POSE_LIB} ({os.path.getsize(POSE_LIB) / 1024:.0f} KiB, stamp {want[:16]})")
    return POSE_LIB


def variant_path(tag: str) -> str:
    return os.path.join(SCRATCH, f"libmi_nerf_{tag}.so")


def build_variant(tag: str, defines) -> str:
    """A/B variant build_scratch/libmi_nerf_TAG.so built with extra -D flags (tools/ab_probe.py times it against the shipped one)."""
    lib = variant_path(tag)
    want = source_stamp(defines)
    if os.path.exists(lib) and os.path.exists(lib + ".stamp") and open(lib + ".stamp").read() == want:
        return lib
    with ThreadPoolExecutor(max_workers=6) as ex:
        objs = list(ex.map(lambda s: _compile(s, False, tuple(defines), tag), SOURCES))
    _link(objs, lib)
    with open(lib + ".stamp", "w") as fh:
        fh.write(want)
    return lib


def build_diag_library() -> str:
    """Diagnostic variant (-DMN_DIAG: s_memtime stamps per kernel segment).  Never shipped or timed."""
    return build_variant("diag", ["-DMN_DIAG"])


def clean() -> None:
    """Remove every object and variant; the shipped library stays."""
    shutil.rmtree(SCRATCH, ignore_errors=True)
    for f in os.listdir(HERE):                             # pre-round-4 layouts
        if f.startswith("libmi_nerf_") and f.endswith(".so"):
            os.remove(os.path.join(HERE, f))
    for d in os.listdir(CSRC):
        if d == "build" or d.startswith("build_"):
            shutil.rmtree(os.path.join(CSRC, d), ignore_errors=True)


if __name__ == "__main__":
    if "--clean" in sys.argv:
        clean()
    elif "--diag" in sys.argv:
        print(build_diag_library())
    elif "--variant" in sys.argv:                  # python -m ...build --variant TAG -DFOO -DBAR=1
        i = sys.argv.index("--variant")
        print(build_variant(sys.argv[i + 1], [a for a in sys.argv[i + 2:] if a.startswith("-D")]))
    else:
        print(build_library(force="--force" in sys.argv, verbose=True))
        print(build_iqa_library(force="--force" in sys.argv, verbose=True))
        print(build_occ_library(force="--force" in sys.argv, verbose=True))
        print(build_scene_library(force="--force" in sys.argv, verbose=True))
        print(build_mesh_library(force="--force" in sys.argv, verbose=True))
        print(build_geo_library(force="--force" in sys.argv, verbose=True))
        print(build_pose_library(force="--force" in sys.argv, verbose=True))
