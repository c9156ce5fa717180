"""libmi_nerf_vox.so / include/mi_nerf_vox.h and nerf_pytorch_paeng_amd/baked.py without a GPU: the header, the ctypes table
(nerf_pytorch_paeng_amd/_vox.py) and the library's dynamic symbols name the same entries; the library exports nothing of the others and
stands alone; a C99 program links against it; the size and step-bound formulas; every refusal answers MI_VOX_EINVAL with a message before
any HIP call; the projection matrix inverts the basis; the restatement the GPU tests compare with (tests/vox_restate.py) has the
properties of the rule."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import vox_restate as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1


@pytest.fixture(scope="module")
def vox():
    """The library is built when the tree is fresh (a no-op when it is up to date), like tests/conftest.py does for libmi_nerf.so."""
    from nerf_pytorch_paeng_amd import _vox
    from nerf_pytorch_paeng_amd.build import build_vox_library
    build_vox_library()
    _vox.lib()
    return _vox


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def test_header_table_and_symbols_agree_and_only_mi_vox_is_exported(vox):
    from nerf_pytorch_paeng_amd import _geo, _iqa, _lib, _lpips, _mesh, _occ, _optim, _pose, _scene
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_vox.h")).read()
    declared = set(re.findall(r"\b(mi_vox_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(vox.SIGNATURES), declared ^ set(vox.SIGNATURES)
    new = _exports(vox.LIB_PATH)
    assert {n for n in new if n.startswith("mi_")} == declared                              # the header's entries and no other mi_* name
    assert not [n for n in new if not n.startswith("mi_vox_") and not n.startswith("_Z")]     # beside them only the kernels' C++ launch stubs
    for other in (_lib, _geo, _iqa, _lpips, _mesh, _occ, _optim, _pose, _scene):
        assert not set(vox.SIGNATURES) & set(other.SIGNATURES)
    assert len(_lib.SIGNATURES) == 68
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "mi_nerf_vox.h":
            assert "mi_vox_" not in open(os.path.join(ROOT, "include", other)).read(), other
    # the header names entries of no other library; the lattice's header is referred to by file name
    assert set(re.findall(r"\bmi_[a-z]+_(?!h\b)", re.sub(r"mi_nerf(_[a-z]+)?\.h", "", hdr))) <= {"mi_vox_"}
    assert "include/mi_nerf_mesh.h" in hdr and '#include "mi_nerf' not in hdr
    assert len(re.findall(r"^\s*#\s*ifdef __cplusplus", hdr, re.M)) == 2
    assert vox.lib().mi_vox_abi_version() == vox.ABI_VERSION == int(re.search(r"#define MI_VOX_ABI_VERSION (\d+)", hdr).group(1))
    for name in ("MAX_RES", "BLOCK", "MAX_DIRS", "MAX_STEPS"):
        assert getattr(vox, name) == int(re.search(rf"#define MI_VOX_{name} (\d+)", hdr).group(1)), name
    assert C.sizeof(vox.Grid) == 36 and C.sizeof(vox.RenderCfg) == 32
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [n for n in sorted(declared) if n not in doc] == []


def test_the_library_stands_alone_and_is_in_the_build_table(vox):
    from nerf_pytorch_paeng_amd import build
    assert build.LIBRARIES["vox"] == (["vox.hip"], [], False)
    assert "ten shared libraries" in build.__doc__
    dyn = subprocess.run(["readelf", "-d", vox.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libmi_nerf" not in dyn.replace("libmi_nerf_vox.so", "")
    und = subprocess.run(["nm", "-D", "--undefined-only", vox.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not [ln for ln in und.splitlines() if ln.split()[-1].startswith("mi_")]


def test_the_source_holds_no_preprocessor_conditional_no_ablation_macro_and_no_atomic():
    """tests/test_packing_cpu.py allows 14 conditionals in csrc/ and counts 13; this source and the header that holds the rule add none."""
    for name in ("vox.hip", "vox_rule.h"):
        src = open(os.path.join(ROOT, "nerf_pytorch_paeng_amd", "csrc", name)).read()
        assert not re.findall(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b", src, re.M) and "MN_" not in src, name
        assert not re.findall(r"\batomic[A-Z]|__atomic_|\basm\b", src), name


def test_header_compiles_as_c99_and_the_library_links_and_answers(tmp_path, vox):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not found")
    pkg = os.path.dirname(vox.LIB_PATH)
    exe = str(tmp_path / "vox_consumer")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "vox_consumer.c"), "-L", pkg, "-lmi_nerf_vox", f"-Wl,-rpath,{pkg}", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"vox c_abi consumer ok: ABI {vox.ABI_VERSION}" in run.stdout


# ---------------------------------------------------------------------------------------------------
# sizes and the step bound
# ---------------------------------------------------------------------------------------------------
def _grid(vox, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), res=(20, 20, 20)):
    return vox.Grid((C.c_float * 3)(*lo), (C.c_float * 3)(*hi), (C.c_int32 * 3)(*res))


def test_the_sizes_and_the_step_bound_follow_their_formulas(vox):
    L = vox.lib()
    assert [L.mi_vox_record_floats(B) for B in (0, 1, 2, 3, 4, 5, 8, 9, 10, 16)] == [0, 4, 0, 0, 16, 0, 0, 32, 0, 0]
    for res in ((1, 1, 1), (8, 8, 8), (9, 8, 7), (17, 9, 33), (512, 512, 512), (5, 4, 3)):
        g = _grid(vox, res=res)
        want = math.prod(-(-r // 8) for r in res)
        assert L.mi_vox_skip_bytes(C.byref(g)) == want == math.prod(VR.skip_shape(res)), res
    for lo, hi, step in (((-1, -1, -1), (1, 1, 1), 0.05), ((-1.2, -1.2, -1.2), (1.2, 1.2, 1.2), 2.4 / 512), ((0, 0, 0), (3, 4, 12), 1.0),
                         ((0, 0, 0), (3, 4, 12), 13.0), ((0, 0, 0), (3, 4, 12), 100.0)):
        g = _grid(vox, lo, hi)
        lo32, hi32 = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
        want = math.ceil(math.sqrt(float(((hi32 - lo32) ** 2).sum())) / float(np.float32(step))) + 1
        assert L.mi_vox_max_steps(C.byref(g), step) == want == VR.max_steps(lo, hi, step), (lo, hi, step)
    assert L.mi_vox_max_steps(C.byref(_grid(vox, (0, 0, 0), (3, 4, 12))), 1.0) == 14
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert L.mi_vox_max_steps(C.byref(_grid(vox)), bad) == 0 and "step" in vox.last_error()
    assert L.mi_vox_skip_bytes(C.byref(_grid(vox, res=(0, 8, 8)))) == 0 and "res" in vox.last_error()
    assert L.mi_vox_skip_bytes(None) == 0


# ---------------------------------------------------------------------------------------------------
# refusals: made-up addresses that are never dereferenced -- every call below is refused before the first HIP call (a call that got as
# far as one would answer MI_VOX_EHIP, "HIP error ... no ROCm-capable device", on a machine without a GPU)
# ---------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
GOOD = dict(lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), res=(20, 12, 9), B=9, D=32, raw=0x10000, proj=0x20000, index=0x30000, M=1000, sigma=0x40000,
            coef=0x50000, skip=0x60000, rays=0x70000, n=257, step=0.05, near=0.0, far=6.0, T_min=0.0, bg=(1.0, 1.0, 1.0), use_skip=1, cfg=True,
            rgb=0x80000, disp=0x90000, acc=0xA0000, depth=0xB0000, visited=0xC0000, grid=True)
# case -> (overrides, the entries it applies to: p project, s build_skip, r render)
REFUSALS = {
    "NULL grid": (dict(grid=False), "psr"),
    "res 0": (dict(res=(20, 0, 9)), "psr"),
    "res 513": (dict(res=(513, 12, 9)), "psr"),
    "res negative": (dict(res=(20, 12, -1)), "psr"),
    "lo above hi": (dict(lo=(1.0, -1.0, -1.0), hi=(-1.0, 1.0, 1.0)), "psr"),
    "empty axis": (dict(lo=(-1.0, 1.0, -1.0)), "psr"),
    "NaN box": (dict(hi=(1.0, 1.0, NAN)), "psr"),
    "infinite box": (dict(hi=(INF, 1.0, 1.0)), "psr"),
    "B 2": (dict(B=2), "pr"),
    "B 0": (dict(B=0), "pr"),
    "B 16": (dict(B=16), "pr"),
    "D below B": (dict(D=8), "p"),
    "D above 256": (dict(D=257), "p"),
    "M negative": (dict(M=-1), "p"),
    "NULL raw": (dict(raw=None), "p"),
    "NULL proj": (dict(proj=None), "p"),
    "NULL index": (dict(index=None), "p"),
    "NULL coef": (dict(coef=None), "pr"),
    "raw not 16-byte aligned": (dict(raw=0x10008), "p"),
    "coef not 16-byte aligned": (dict(coef=0x50004), "pr"),
    "index not 8-byte aligned": (dict(index=0x30004), "p"),
    "sigma not 4-byte aligned": (dict(sigma=0x40002), "psr"),
    "NULL sigma": (dict(sigma=None), "sr"),
    "NULL skip": (dict(skip=None), "sr"),
    "NULL cfg": (dict(cfg=False), "r"),
    "step 0": (dict(step=0.0), "r"),
    "step negative": (dict(step=-0.05), "r"),
    "step NaN": (dict(step=NAN), "r"),
    "step infinite": (dict(step=INF), "r"),
    "too many steps": (dict(step=2.0 * math.sqrt(3.0) / 65536.0), "r"),
    "near above far": (dict(near=6.0, far=2.0), "r"),
    "near NaN": (dict(near=NAN), "r"),
    "T_min negative": (dict(T_min=-0.1), "r"),
    "T_min 1": (dict(T_min=1.0), "r"),
    "T_min NaN": (dict(T_min=NAN), "r"),
    "bg NaN": (dict(bg=(1.0, NAN, 1.0)), "r"),
    "use_skip 2": (dict(use_skip=2), "r"),
    "n negative": (dict(n=-1), "r"),
    "NULL rays": (dict(rays=None), "r"),
    "NULL rgb": (dict(rgb=None), "r"),
    "rays not 4-byte aligned": (dict(rays=0x70002), "r"),
    "acc not 4-byte aligned": (dict(acc=0xA0001), "r"),
    "visited not 4-byte aligned": (dict(visited=0xC0002), "r"),
}


def _call(mod, entry, a):
    L = mod.lib()
    g = C.byref(_grid(mod, a["lo"], a["hi"], a["res"])) if a["grid"] else None
    if entry == "p":
        rc = L.mi_vox_project(g, a["B"], a["D"], a["raw"], a["proj"], a["index"], a["M"], a["sigma"], a["coef"], None)
    elif entry == "s":
        rc = L.mi_vox_build_skip(g, a["sigma"], a["skip"], None)
    else:
        cfg = C.byref(mod.RenderCfg(a["step"], a["near"], a["far"], a["T_min"], (C.c_float * 3)(*a["bg"]), a["use_skip"])) if a["cfg"] else None
        rc = L.mi_vox_render(g, a["B"], a["sigma"], a["coef"], a["skip"], a["rays"], a["n"], cfg, a["rgb"], a["disp"], a["acc"], a["depth"], a["visited"],
                             None)
    return rc, mod.last_error()


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_answer_einval_with_a_message_before_any_hip_call(vox, case):
    over, entries = REFUSALS[case]
    for entry in entries:
        rc, msg = _call(vox, entry, dict(GOOD, **over))
        assert rc == EINVAL, (case, entry, rc, msg)
        assert msg and "HIP error" not in msg, (case, entry, msg)


def test_the_good_arguments_of_the_refusal_table_reach_the_device(vox):
    """The table's base case is refused by nothing: each entry gets as far as its launch, which fails here for want of a device
    (MI_VOX_EHIP) -- so every refusal above is owed to its one override.  Nullable arguments may be NULL; nothing is launched for no work."""
    if torch.cuda.is_available():
        pytest.skip("made-up addresses must not reach a real device")
    for entry in "psr":
        rc, msg = _call(vox, entry, dict(GOOD))
        assert rc == 2 and "HIP error" in msg, (entry, rc, msg)
    for over in (dict(disp=None, acc=None, depth=None, visited=None), dict(skip=None, use_skip=0), dict(far=INF), dict(step=1.01 * 2.0 * math.sqrt(3.0) / 65535.0)):
        rc, msg = _call(vox, "r", dict(GOOD, **over))
        assert rc == 2 and "HIP error" in msg, (over, rc, msg)
    rc, msg = _call(vox, "p", dict(GOOD, sigma=None, D=9))
    assert rc == 2 and "HIP error" in msg, (rc, msg)
    assert _call(vox, "p", dict(GOOD, M=0))[0] == 0 and _call(vox, "r", dict(GOOD, n=0))[0] == 0


# ---------------------------------------------------------------------------------------------------
# baked.py on the host
# ---------------------------------------------------------------------------------------------------
def test_the_projection_matrix_inverts_the_basis_at_the_fibonacci_directions(vox):
    from nerf_pytorch_paeng_amd import baked
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    for B in (1, 4, 9):
        for D in sorted({B, 9, 12, 32, 64, 256}):
            dirs = baked.fibonacci_directions(D)
            assert dirs.dtype == np.float64 and np.abs(np.linalg.norm(dirs, axis=1) - 1).max() <= 1e-15
            Y = baked.sh_basis(dirs, B)
            P = baked.projection_matrix(D, B)
            assert P.shape == (B, D) and P.dtype == np.float64
            assert np.abs(P @ Y - np.eye(B)).max() <= 1e-12, (B, D)
            assert np.abs(Y - VR.sh_basis(dirs, B, np.float64)).max() <= 1e-15              # one basis in the package and in the restatement
    assert 2.0 < np.linalg.cond(baked.sh_basis(baked.fibonacci_directions(9), 9)) < 2.3
    assert np.linalg.cond(baked.sh_basis(baked.fibonacci_directions(64), 9)) < 1.02
    # the basis is orthonormal on the sphere: the Gram matrix over many directions is the identity / (4 pi) up to the quadrature
    Y = baked.sh_basis(baked.fibonacci_directions(20000), 9)
    assert np.abs(4 * math.pi * (Y.T @ Y) / 20000 - np.eye(9)).max() <= 2e-4
    for bad in (dict(D=8, B=9), dict(D=257, B=1), dict(D=32, B=2)):
        with pytest.raises(MiNerfError):
            baked.projection_matrix(**bad)


def test_the_grid_object_knows_its_sizes_and_refuses_what_the_library_refuses(vox, tmp_path):
    from nerf_pytorch_paeng_amd import baked
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    g = baked.RadianceGrid(-1.0, (1.0, 2.0, 3.0), (17, 9, 33), B=4)
    assert g.points == (34, 10, 18) and g.skip_shape == (5, 2, 3) and g.record_floats == 16 and g.device is None
    assert g.nbytes == 4 * 34 * 10 * 18 * 17 + 30
    assert g.cell_edge() == float(np.float32(2.0) / np.float32(17))
    for bad in (dict(res=0), dict(res=513), dict(B=2), dict(lo=1.0, hi=1.0)):
        with pytest.raises(MiNerfError):
            baked.RadianceGrid(**dict(dict(lo=-1.0, hi=1.0, res=8, B=9), **bad))
    with pytest.raises(MiNerfError, match="holds nothing"):
        g.render(torch.zeros(1, 6))
    g.allocate("cpu")
    with pytest.raises(MiNerfError, match="HIP device"):
        g.render(torch.zeros(1, 6))
    g.sigma[3, 2, 1] = 2.5
    g.coef[3, 2, 1, :12] = torch.arange(12.0)
    g.skip[0, 0, 0] = 1
    g.save(str(tmp_path / "g.npz"))
    h = baked.RadianceGrid.load(str(tmp_path / "g.npz"))
    assert (h.lo, h.hi, h.res, h.B) == (g.lo, g.hi, g.res, g.B)
    assert torch.equal(h.sigma, g.sigma) and torch.equal(h.coef, g.coef) and torch.equal(h.skip, g.skip)


# ---------------------------------------------------------------------------------------------------
# the restatement's own properties
# ---------------------------------------------------------------------------------------------------
def _const_box(res, sigma, B=1, colour=0.5):
    P = tuple(r + 1 for r in reversed(res))
    s = np.full(P, sigma, np.float32)
    coef = np.zeros(P + (VR.record_floats(B),), np.float32)
    coef[..., 0:3] = np.float32(colour / VR.C0)
    return s, coef


RAYS = np.array([[-3.0, 0.1, 0.2, 1.0, 0.0, 0.0],           # along x through the whole box: chord 2
                 [-3.0, -2.0, 0.3, 1.5, 1.0, -0.1],          # oblique, |d| != 1
                 [0.2, 0.1, -0.3, 0.0, 0.0, 2.0],            # from inside, two zero components
                 [-3.0, 0.1, 0.2, -1.0, 0.0, 0.0],           # pointing away: a miss
                 [0.0, 5.0, 0.0, 1.0, 0.0, 0.0]], np.float32)  # a zero component outside its slab: a miss


def _chord(rays, lo, hi, near, far):
    o, d = rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64)
    with np.errstate(all="ignore"):
        ta, tb = (lo - o) / d, (hi - o) / d
        inside = (o >= lo) & (o <= hi)
        a = np.where(d != 0, np.minimum(ta, tb), np.where(inside, -np.inf, np.inf)).max(1)
        b = np.where(d != 0, np.maximum(ta, tb), np.where(inside, np.inf, -np.inf)).min(1)
    return np.maximum(np.minimum(b, far) - np.maximum(a, near), 0.0) * np.linalg.norm(d, axis=1)


def test_restatement_constant_box_is_beer_lambert_and_a_miss_is_the_background():
    lo, hi, res, sig = (-1.0,) * 3, (1.0,) * 3, (6, 5, 4), float(np.float32(1.7))
    s, coef = _const_box(res, sig)
    bg = (0.25, 0.5, 1.0)
    out = VR.render(lo, hi, res, 1, s, coef, RAYS, 0.07, 0.0, 100.0, bg=bg)
    chord = _chord(RAYS, -1.0, 1.0, 0.0, 100.0)
    assert chord[0] == 2.0 and chord[3] == 0 and chord[4] == 0 and chord[1] > 0 and abs(chord[2] - 1.3) <= 1e-7
    want = 1.0 - np.exp(-sig * chord)
    assert np.abs(out["acc"] - want).max() <= 1e-13, np.abs(out["acc"] - want).max()
    for i in (3, 4):                                                                        # a miss: the background, nothing else
        assert tuple(out["rgb"][i]) == bg and out["acc"][i] == 0 and out["depth"][i] == 0 and out["disp"][i] == 0 and out["samples"][i] == 0
    assert np.abs(out["rgb"][:3] - (0.5 * want[:3, None] + (1 - want[:3, None]) * np.asarray(bg))).max() <= 1e-7    # colour 0.5 through an fp32 coefficient
    assert (out["samples"][:3] == np.ceil(chord[:3] / np.float64(np.float32(0.07)) - 1e-9)).all()
    # a NaN ray and a zero direction are misses too
    bad = np.array([[np.nan, 0, 0, 1, 0, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, np.inf, 0, 0]], np.float32)
    out = VR.render(lo, hi, res, 1, s, coef, bad, 0.07, 0.0, 100.0, bg=bg)
    assert (out["rgb"] == np.asarray(bg)).all() and not out["acc"].any() and not out["disp"].any()


def test_restatement_halving_the_step_changes_nothing_on_a_constant_box():
    lo, hi, res = (-1.0,) * 3, (1.0,) * 3, (6, 5, 4)
    s, coef = _const_box(res, 0.9)
    a = VR.render(lo, hi, res, 1, s, coef, RAYS, 0.1, 0.0, 100.0)
    b = VR.render(lo, hi, res, 1, s, coef, RAYS, 0.05, 0.0, 100.0)
    for k in ("rgb", "acc"):
        assert np.abs(a[k] - b[k]).max() <= 1e-13, k
    assert (b["samples"][:3] >= 2 * a["samples"][:3] - 1).all()
    # depth is the alpha-weighted midpoint: it converges, it is not step-free
    assert np.abs(a["depth"] - b["depth"]).max() <= 0.05


def test_restatement_truncated_last_interval_keeps_acc_continuous_across_a_change_of_sample_count():
    """t_far slides across an interval boundary: the sample count changes by one, the outputs by no more than the slide allows."""
    lo, hi, res = (-1.0,) * 3, (1.0,) * 3, (6, 5, 4)
    rng = np.random.default_rng(5)
    s = rng.uniform(0.2, 3.0, (5, 6, 7)).astype(np.float32)
    coef = np.zeros((5, 6, 7, 4), np.float32)
    coef[..., :3] = rng.uniform(0.0, 3.0, (5, 6, 7, 3))
    ray = RAYS[:1]
    step = 0.25                                                  # t0 = 2: boundaries at 2.25, 2.5, ...
    eps = 1e-6
    below = VR.render(lo, hi, res, 1, s, coef, ray, step, 0.0, 2.75 - eps)
    above = VR.render(lo, hi, res, 1, s, coef, ray, step, 0.0, 2.75 + eps)
    assert below["samples"][0] == 3 and above["samples"][0] == 4
    for k in ("rgb", "acc", "depth"):
        assert np.abs(below[k] - above[k]).max() <= 3.0 * 2 * eps * 8, k          # sigma <= 3 over a width that moves by 2 eps, times t <= 3 for depth, with room
    # and T_min only ever removes samples
    full = VR.render(lo, hi, res, 1, s, coef, RAYS, 0.05, 0.0, 100.0)
    cut = VR.render(lo, hi, res, 1, s, coef, RAYS, 0.05, 0.0, 100.0, T_min=0.1)
    assert (cut["samples"] <= full["samples"]).all() and (cut["samples"][:3] < full["samples"][:3]).any()
    assert np.abs(cut["acc"] - full["acc"]).max() <= 0.1 and np.abs(cut["rgb"] - full["rgb"]).max() <= 0.1


def test_restatement_float32_follows_float64_and_skip_plane_has_its_margin():
    lo, hi, res = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (17, 9, 20)
    rng = np.random.default_rng(6)
    P = (21, 10, 18)
    s = np.where(rng.uniform(size=P) < 0.5, 0, rng.uniform(0, 8, P)).astype(np.float32)
    coef = rng.normal(0, 1, P + (32,)).astype(np.float32)
    a = VR.render(lo, hi, res, 9, s, coef, RAYS, 0.03, 0.0, 100.0)
    b = VR.render(lo, hi, res, 9, s, coef, RAYS, 0.03, 0.0, 100.0, dtype=np.float32)
    assert b["rgb"].dtype == np.float32
    for k in ("rgb", "acc", "depth", "disp"):
        assert 0 < np.abs(a[k] - b[k]).max() <= 2e-5, (k, np.abs(a[k] - b[k]).max())
    # one occupied point on a block face (x = 8) sets both neighbouring blocks, and through the margin nothing further
    z = np.zeros(P, np.float32)
    z[3, 4, 8] = 1.0
    sk = VR.build_skip(z, res)
    assert sk.shape == (3, 2, 3) and sk[0, 0, 0] == 1 and sk[0, 0, 1] == 1 and sk[0, 0, 2] == 0 and sk[1].sum() == 0 and sk[0, 1].sum() == 0
    z[3, 4, 8] = 0
    z[8, 8, 16] = 1.0                                          # a corner of blocks in all three axes: 2 x 2 x 2 blocks
    assert VR.build_skip(z, res).sum() == 8 and VR.build_skip(z, res)[2].sum() == 0
    z[8, 8, 16] = 0
    z[3, 4, 7] = 1.0                                           # one cell before the face: the margin sets the next block too
    assert VR.build_skip(z, res)[0, 0].tolist() == [1, 1, 0]
    z[3, 4, 7] = 0
    z[3, 4, 6] = 1.0                                           # two cells before: not any more
    assert VR.build_skip(z, res)[0, 0].tolist() == [1, 0, 0]
    # the projection restated: constant colour over all directions lands in coefficient 0 alone
    from nerf_pytorch_paeng_amd import baked
    raw = np.zeros((3, 32, 4), np.float32)
    raw[..., :3] = np.float32(0.7)
    raw[:, 0, 3] = (2.0, -1.0, np.nan)
    sig, rec = VR.project(raw, baked.projection_matrix(32, 9).astype(np.float32), 9)
    assert sig.tolist() == [2.0, 0.0, 0.0]
    assert np.abs(rec[:, 0:3] * VR.C0 - 1 / (1 + math.exp(-0.7))).max() <= 1e-6 and np.abs(rec[:, 3:27]).max() <= 1e-6 and not rec[:, 27:].any()
