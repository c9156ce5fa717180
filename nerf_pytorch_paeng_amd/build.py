"""Build libmi_nerf.so and the ten shared libraries beside it with hipcc for gfx950 (cross-compiles without a GPU).

    python -m nerf_pytorch_paeng_amd.build [--force]          the shipped libraries (clean build: ~1 min 20 s on 8 cores)
    python -m nerf_pytorch_paeng_amd.build --variant TAG -DFOO -DBAR=1     an A/B variant (tools/ab_probe.py)
    python -m nerf_pytorch_paeng_amd.build --diag             the -DMN_DIAG variant (s_memtime stamps; never shipped or timed)
    python -m nerf_pytorch_paeng_amd.build --clean            remove every object and every variant

LIBRARIES has one record per library: its name ("" is libmi_nerf.so itself), its sources, its extra link arguments, and whether libmi_nerf.so
is built first because the library links against it (rpath $ORIGIN).  _build() builds any record; the build_*_library names bind to it.
occ and mesh link against libmi_nerf.so; mesh is two translation units (mesh.hip: extraction, which calls the fused network entries;
mesh_view.hip: the rasteriser, which calls nothing of libmi_nerf.so); geo is two as well (geo.hip: the compositing pair; lattice_reg.hip: the grid
regularisers); the other libraries (voxgrad, the radiance grid's
backward pass, among them) link against none of the project's.

What lands where:
  nerf_pytorch_paeng_amd/libmi_nerf[_NAME].so (+ .stamp)   the shipped libraries: the only artefacts inside the package, git-ignored, copied with the tree
        to a GPU box.  A stamp hashes the library's sources, EVERY header under csrc/ and include/, the flags and the link arguments; the library is
        up to date iff the stamp matches (no mtimes, no objects needed -- the GPU box gets neither).  Every header for every library: the one rule
        that cannot miss a header reached through another (csrc/abi_error.h is in all eleven, csrc/vox_rule.h in vox and voxgrad, csrc/block_scan.h in
        mesh, occ, vox, iqa and libmi_nerf.so's frames.hip, csrc/row_slab.h in occ and mesh); a one-file library is rebuilt a few seconds too often.
  build_scratch/obj/                                objects of the shipped libraries (cache; tests/test_packing_cpu.py disassembles them)
  build_scratch/obj_TAG/, build_scratch/libmi_nerf_TAG.so    variants of libmi_nerf.so.  build_scratch/ is git-ignored and is not copied: a variant is
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
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function",
         # the MLP kernel's register-resident design needs its k-loops FULLY unrolled (static register indices)
         "-mllvm", "-pragma-unroll-threshold=1000000"]
# mlp_bf16.hip / mlp_f16.hip manage the whole AGPR file by hand (explicit a[N] operands in asm statements): hipcc must not park spilled VGPRs there
FILE_FLAGS = {"mlp_bf16.hip": ["-mllvm", "-amdgpu-spill-vgpr-to-agpr=0"], "mlp_f16.hip": ["-mllvm", "-amdgpu-spill-vgpr-to-agpr=0"],
              "mlp_f16s.hip": ["-mllvm", "-amdgpu-spill-vgpr-to-agpr=0"],
              "mlp_f16s_stash.hip": ["-mllvm", "-amdgpu-spill-vgpr-to-agpr=0"], "dgrad_f16s.hip": ["-mllvm", "-amdgpu-spill-vgpr-to-agpr=0"]}
LINK_NERF = ["-L" + HERE, "-lmi_nerf", "-Wl,-rpath,$ORIGIN"]
# name -> (sources, extra link arguments, libmi_nerf.so is built first); iqa, scene, geo, pose, optim, lpips, vox and voxgrad link against no other library of the project
LIBRARIES = {
    "": (SOURCES, [], False),
    "iqa": (["iqa.hip"], [], False),
    "occ": (["occ.hip"], LINK_NERF, True),
    "scene": (["scene.hip"], [], False),
    "mesh": (["mesh.hip", "mesh_view.hip"], LINK_NERF, True),
    "geo": (["geo.hip", "lattice_reg.hip"], [], False),
    "pose": (["pose.hip"], [], False),
    "optim": (["optim.hip"], [], False),
    "lpips": (["lpips.hip"], [], False),
    "vox": (["vox.hip"], [], False),
    "voxgrad": (["voxgrad.hip"], [], False),
}


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the MI355X path cannot be built (there is no CPU fallback)")
    return exe


def _headers():
    return [os.path.join(d, f) for d in (CSRC, INCLUDE) for f in sorted(os.listdir(d)) if f.endswith(".h")]


def _digest(paths, extra=()) -> str:
    h = hashlib.sha256()
    for p in paths:
        h.update(os.path.basename(p).encode())
        with open(p, "rb") as fh:
            h.update(fh.read())
    h.update(repr(list(extra)).encode())
    return h.hexdigest()


def source_stamp(defines=(), name: str = "") -> str:
    """Hash of everything library `name` is made of: sources, headers, flags, link arguments (and a variant's -D list)."""
    sources, link, _ = LIBRARIES[name]
    return _digest([os.path.join(CSRC, x) for x in sources] + _headers(), [FLAGS, sorted(FILE_FLAGS.items()), link[1:], list(defines)])


def object_dir(tag: str = "") -> str:
    return os.path.join(SCRATCH, "obj" + ("_" + tag if tag else ""))


def _compile(src: str, force: bool, extra=(), tag: str = "") -> str:
    """One translation unit -> build_scratch/obj[_TAG]/SRC.o, skipped when the object's own stamp (source + headers + flags) matches."""
    bdir = object_dir(tag)
    os.makedirs(bdir, exist_ok=True)
    obj = os.path.join(bdir, src + ".o")
    spath = os.path.join(CSRC, src)
    cmd_flags = [*FLAGS, *FILE_FLAGS.get(src, []), *extra]
    want = _digest([spath] + _headers(), cmd_flags)
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


def variant_path(tag: str) -> str:
    return os.path.join(SCRATCH, f"libmi_nerf_{tag}.so")


def _build(name: str, force: bool = False, verbose: bool = False, tag: str = "", defines=()) -> str:
    """Library `name` of LIBRARIES, or with a tag the variant of it built with extra -D flags; a no-op when its stamp matches."""
    sources, link, needs_nerf = LIBRARIES[name]
    if needs_nerf:
        _build("")
    lib = variant_path(tag) if tag else os.path.join(HERE, f"libmi_nerf_{name}.so") if name else LIB
    want = source_stamp(defines, name)
    done = not force and os.path.exists(lib) and os.path.exists(lib + ".stamp") and open(lib + ".stamp").read() == want
    if not done:
        with ThreadPoolExecutor(max_workers=6) as ex:
            objs = list(ex.map(lambda x: _compile(x, force, tuple(defines), tag), sources))
        _link(objs, lib, link)
        with open(lib + ".stamp", "w") as fh:
            fh.write(want)
    if verbose:
        print(f"{'up to date:' if done else 'built'} {lib} ({os.path.getsize(lib) / 1024:.0f} KiB, stamp {want[:16]})")
    return lib


def build_library(force: bool = False, verbose: bool = False) -> str: return _build("", force, verbose)
def build_iqa_library(force: bool = False, verbose: bool = False) -> str: return _build("iqa", force, verbose)
def build_occ_library(force: bool = False, verbose: bool = False) -> str: return _build("occ", force, verbose)
def build_scene_library(force: bool = False, verbose: bool = False) -> str: return _build("scene", force, verbose)
def build_mesh_library(force: bool = False, verbose: bool = False) -> str: return _build("mesh", force, verbose)
def build_geo_library(force: bool = False, verbose: bool = False) -> str: return _build("geo", force, verbose)
def build_pose_library(force: bool = False, verbose: bool = False) -> str: return _build("pose", force, verbose)
def build_optim_library(force: bool = False, verbose: bool = False) -> str: return _build("optim", force, verbose)
def build_lpips_library(force: bool = False, verbose: bool = False) -> str: return _build("lpips", force, verbose)
def build_vox_library(force: bool = False, verbose: bool = False) -> str: return _build("vox", force, verbose)
def build_voxgrad_library(force: bool = False, verbose: bool = False) -> str: return _build("voxgrad", force, verbose)


def build_variant(tag: str, defines) -> str:
    """A/B variant build_scratch/libmi_nerf_TAG.so built with extra -D flags (tools/ab_probe.py times it against the shipped one)."""
    return _build("", tag=tag, defines=defines)


def build_diag_library() -> str:
    """Diagnostic variant (-DMN_DIAG: s_memtime stamps per kernel segment).  Never shipped or timed."""
    return build_variant("diag", ["-DMN_DIAG"])


def clean() -> None:
    """Remove every object, every variant and stale files in the package; the shipped libraries stay."""
    shutil.rmtree(SCRATCH, ignore_errors=True)
    shipped = {"libmi_nerf.so"} | {f"libmi_nerf_{name}.so" for name in LIBRARIES if name}
    for f in os.listdir(HERE):                             # stale: a libmi_nerf*.so that no record of LIBRARIES names
        if f.startswith("libmi_nerf") and f.endswith((".so", ".so.stamp")) and f.removesuffix(".stamp") not in shipped:
            os.remove(os.path.join(HERE, f))
    for d in os.listdir(CSRC):                             # stale: object directories of earlier layouts
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
        for name in LIBRARIES:
            print(_build(name, force="--force" in sys.argv, verbose=True))
