"""libmi_nerf_voxgrad.so / include/mi_nerf_voxgrad.h without a GPU: the header, the ctypes table (nerf_pytorch_paeng_amd/_voxgrad.py) and
the library's dynamic symbols name the same entries; the library exports nothing of the others and stands alone; a C99 program links
against it; every refusal answers MI_VOXGRAD_EINVAL with a message before any HIP call; and the comparator the GPU tests use
(tests/voxgrad_restate.py) is held against finite differences of the forward restatement (tests/vox_restate.py) in float64."""
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
from tests import voxgrad_restate as VG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1


@pytest.fixture(scope="module")
def voxgrad():
    """The library is built when the tree is fresh (a no-op when it is up to date)."""
    from nerf_pytorch_paeng_amd import _voxgrad
    from nerf_pytorch_paeng_amd.build import build_voxgrad_library
    build_voxgrad_library()
    _voxgrad.lib()
    return _voxgrad


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


# ---------------------------------------------------------------------------------------------------
# 1. header, table, symbols
# ---------------------------------------------------------------------------------------------------
def test_header_table_and_symbols_agree_and_only_mi_voxgrad_is_exported(voxgrad):
    from nerf_pytorch_paeng_amd import _geo, _iqa, _lib, _lpips, _mesh, _occ, _optim, _pose, _scene, _vox
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_voxgrad.h")).read()
    declared = set(re.findall(r"\b(mi_voxgrad_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(voxgrad.SIGNATURES) == {"mi_voxgrad_abi_version", "mi_voxgrad_last_error", "mi_voxgrad_render_backward"}
    new = _exports(voxgrad.LIB_PATH)
    assert {n for n in new if n.startswith("mi_")} == declared                                  # the header's entries and no other mi_* name
    assert not [n for n in new if not n.startswith("mi_voxgrad_") and not n.startswith("_Z")]     # beside them only the kernels' C++ launch stubs
    for other in (_lib, _geo, _iqa, _lpips, _mesh, _occ, _optim, _pose, _scene, _vox):
        assert not set(voxgrad.SIGNATURES) & set(other.SIGNATURES)
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "mi_nerf_voxgrad.h":
            assert "mi_voxgrad_" not in open(os.path.join(ROOT, "include", other)).read(), other
    # the header names entries of no other library, includes no project header, and refers to the render rule by file name
    for prefix in ("mi_vox_", "mi_mesh_", "mi_lpips_", "mi_optim_", "mi_geo_", "mi_pose_", "mi_scene_", "mi_occ_", "mi_iqa_", "mi_nerf_render"):
        assert prefix not in hdr, prefix
    assert "THE RENDER RULE of include/mi_nerf_vox.h" in hdr and '#include "' not in hdr
    assert len(re.findall(r"^\s*#\s*ifdef __cplusplus", hdr, re.M)) == 2
    assert "atomic" in hdr and "NOT bit-identical" in hdr                                       # the exception is stated where the ABI is
    assert voxgrad.lib().mi_voxgrad_abi_version() == voxgrad.ABI_VERSION == 1 == int(re.search(r"#define MI_VOXGRAD_ABI_VERSION (\d+)", hdr).group(1))
    for name in ("MAX_RES", "BLOCK", "MAX_STEPS"):
        assert getattr(voxgrad, name) == getattr(_vox, name) == int(re.search(rf"#define MI_VOXGRAD_{name} (\d+)", hdr).group(1)), name
    assert C.sizeof(voxgrad.Grid) == C.sizeof(_vox.Grid) == 36 and C.sizeof(voxgrad.RenderCfg) == C.sizeof(_vox.RenderCfg) == 32
    assert [(n, t) for n, t in voxgrad.Grid._fields_] == [(n, t) for n, t in _vox.Grid._fields_]
    assert [(n, t) for n, t in voxgrad.RenderCfg._fields_] == [(n, t) for n, t in _vox.RenderCfg._fields_]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [n for n in sorted(declared) if n not in doc] == []


def test_the_library_stands_alone_and_is_in_the_build_table(voxgrad):
    from nerf_pytorch_paeng_amd import build
    assert build.LIBRARIES["voxgrad"] == (["voxgrad.hip"], [], False)
    assert len(build.LIBRARIES) == 11 and "libmi_nerf.so and the ten shared libraries beside it" in build.__doc__ and "all eleven" in build.__doc__
    dyn = subprocess.run(["readelf", "-d", voxgrad.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libmi_nerf" not in dyn.replace("libmi_nerf_voxgrad.so", "")
    und = subprocess.run(["nm", "-D", "--undefined-only", voxgrad.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not [ln for ln in und.splitlines() if ln.split()[-1].startswith("mi_")]


def test_the_source_holds_no_preprocessor_conditional_no_ablation_macro_and_no_inline_assembly():
    csrc = os.path.join(ROOT, "nerf_pytorch_paeng_amd", "csrc")
    src, rule = open(os.path.join(csrc, "voxgrad.hip")).read(), open(os.path.join(csrc, "vox_rule.h")).read()
    for name, text in (("voxgrad.hip", src), ("vox_rule.h", rule)):
        assert not re.findall(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b", text, re.M) and "MN_" not in text, name
        assert not re.findall(r"\basm\b", text), name
    assert '#include "../../include/mi_nerf_voxgrad.h"' in src and "mi_nerf_vox.h\"" not in src     # it includes its own header alone
    assert '#include "vox_rule.h"' in src and not re.findall(r"#\s*include\s*[\"<][^\"<>]*mi_nerf\w*\.h", rule)   # the shared rule knows no public header


def test_header_compiles_as_c99_and_the_library_links_and_answers(tmp_path, voxgrad):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not found")
    pkg = os.path.dirname(voxgrad.LIB_PATH)
    exe = str(tmp_path / "voxgrad_consumer")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "voxgrad_consumer.c"), "-L", pkg, "-lmi_nerf_voxgrad", f"-Wl,-rpath,{pkg}", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"voxgrad c_abi consumer ok: ABI {voxgrad.ABI_VERSION}" in run.stdout


# ---------------------------------------------------------------------------------------------------
# 2. refusals: made-up addresses that are never dereferenced -- every call below is refused before the first HIP call (a call that got as
# far as one would answer MI_VOXGRAD_EHIP, "HIP error ... no ROCm-capable device", on a machine without a GPU)
# ---------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
GOOD = dict(lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), res=(20, 12, 9), B=9, sigma=0x40000, coef=0x50000, skip=0x60000, rays=0x70000, n=257, step=0.05,
            near=0.0, far=6.0, T_min=0.0, bg=(1.0, 1.0, 1.0), use_skip=1, cfg=True, g_rgb=0x80000, g_acc=0x90000, g_depth=0xA0000, d_sigma=0xB0000,
            d_coef=0xC0000, rgb=0xD0000, acc=0xE0000, depth=0xF0000, grid=True)
REFUSALS = {
    "NULL grid": dict(grid=False),
    "res 0": dict(res=(20, 0, 9)),
    "res 513": dict(res=(513, 12, 9)),
    "res negative": dict(res=(20, 12, -1)),
    "lo above hi": dict(lo=(1.0, -1.0, -1.0), hi=(-1.0, 1.0, 1.0)),
    "empty axis": dict(lo=(-1.0, 1.0, -1.0)),
    "NaN box": dict(hi=(1.0, 1.0, NAN)),
    "infinite box": dict(hi=(INF, 1.0, 1.0)),
    "B 2": dict(B=2),
    "B 0": dict(B=0),
    "B 16": dict(B=16),
    "NULL cfg": dict(cfg=False),
    "step 0": dict(step=0.0),
    "step negative": dict(step=-0.05),
    "step NaN": dict(step=NAN),
    "step infinite": dict(step=INF),
    "too many steps": dict(step=2.0 * math.sqrt(3.0) / 65536.0),
    "near above far": dict(near=6.0, far=2.0),
    "near NaN": dict(near=NAN),
    "T_min negative": dict(T_min=-0.1),
    "T_min 1": dict(T_min=1.0),
    "T_min NaN": dict(T_min=NAN),
    "bg NaN": dict(bg=(1.0, NAN, 1.0)),
    "bg infinite": dict(bg=(INF, 1.0, 1.0)),
    "use_skip 2": dict(use_skip=2),
    "n negative": dict(n=-1),
    "NULL sigma": dict(sigma=None),
    "NULL coef": dict(coef=None),
    "NULL skip": dict(skip=None),
    "NULL rays": dict(rays=None),
    "NULL g_rgb": dict(g_rgb=None),
    "NULL d_sigma": dict(d_sigma=None),
    "NULL d_coef": dict(d_coef=None),
    "coef not 16-byte aligned": dict(coef=0x50004),
    "d_coef not 16-byte aligned": dict(d_coef=0xC0008),
    "sigma not 4-byte aligned": dict(sigma=0x40002),
    "rays not 4-byte aligned": dict(rays=0x70002),
    "g_rgb not 4-byte aligned": dict(g_rgb=0x80001),
    "g_acc not 4-byte aligned": dict(g_acc=0x90002),
    "g_depth not 4-byte aligned": dict(g_depth=0xA0003),
    "d_sigma not 4-byte aligned": dict(d_sigma=0xB0002),
    "rgb_check not 4-byte aligned": dict(rgb=0xD0002),
    "acc_check not 4-byte aligned": dict(acc=0xE0001),
    "depth_check not 4-byte aligned": dict(depth=0xF0002),
}


def _call(mod, a):
    g = C.byref(mod.Grid((C.c_float * 3)(*a["lo"]), (C.c_float * 3)(*a["hi"]), (C.c_int32 * 3)(*a["res"]))) if a["grid"] else None
    cfg = C.byref(mod.RenderCfg(a["step"], a["near"], a["far"], a["T_min"], (C.c_float * 3)(*a["bg"]), a["use_skip"])) if a["cfg"] else None
    rc = mod.lib().mi_voxgrad_render_backward(g, a["B"], a["sigma"], a["coef"], a["skip"], a["rays"], a["n"], cfg, a["g_rgb"], a["g_acc"], a["g_depth"],
                                              a["d_sigma"], a["d_coef"], a["rgb"], a["acc"], a["depth"], None)
    return rc, mod.last_error()


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_answer_einval_with_a_message_before_any_hip_call(voxgrad, case):
    rc, msg = _call(voxgrad, dict(GOOD, **REFUSALS[case]))
    assert rc == EINVAL, (case, rc, msg)
    assert msg and "HIP error" not in msg and msg.startswith("mi_voxgrad_render_backward"), (case, msg)


def test_the_good_arguments_of_the_refusal_table_reach_the_device(voxgrad):
    """The table's base case is refused by nothing: it gets as far as its launch, which fails here for want of a device (MI_VOXGRAD_EHIP)
    -- so every refusal above is owed to its one override.  Nullable arguments may be NULL; nothing is launched for no work, and no
    pointer is looked at then."""
    assert _call(voxgrad, dict(GOOD, n=0))[0] == 0
    assert _call(voxgrad, dict(GOOD, n=0, sigma=None, coef=0x50004, skip=None, rays=None, g_rgb=None, d_sigma=None, d_coef=None))[0] == 0
    if torch.cuda.is_available():
        pytest.skip("made-up addresses must not reach a real device")
    for over in (dict(), dict(g_acc=None, g_depth=None), dict(rgb=None, acc=None, depth=None), dict(skip=None, use_skip=0), dict(far=INF),
                 dict(step=1.01 * 2.0 * math.sqrt(3.0) / 65535.0)):
        rc, msg = _call(voxgrad, dict(GOOD, **over))
        assert rc == 2 and "HIP error" in msg, (over, rc, msg)


# ---------------------------------------------------------------------------------------------------
# 3. the comparator against itself: the analytic float64 gradient against differences of the forward restatement
# ---------------------------------------------------------------------------------------------------
def _case():
    from tests.test_gpu_vox import CFG, GRID_SPECS, grid_arrays, make_rays
    spec = GRID_SPECS["5x4x3"]
    B = 9
    sigma, coef = grid_arrays("5x4x3", B)
    rays = make_rays(spec["lo"], spec["hi"], 12, 10 + B)
    step = 0.5 * float(min((np.float32(spec["hi"][i]) - np.float32(spec["lo"][i])) / np.float32(spec["res"][i]) for i in range(3)))
    rng = np.random.default_rng(77)
    G = rng.normal(0.0, 1.0, (12, 3)).astype(np.float32)
    ga = rng.normal(0.0, 1.0, 12).astype(np.float32)
    gd = rng.normal(0.0, 1.0, 12).astype(np.float32)
    return spec, B, sigma, coef, rays, step, CFG, G, ga, gd


def test_the_analytic_gradient_meets_finite_differences_of_the_forward_restatement_in_float64():
    spec, B, sigma, coef, rays, step, CFG, G, ga, gd = _case()
    assert rays.shape == (12, 6)
    G64, ga64, gd64 = G.astype(np.float64), ga.astype(np.float64), gd.astype(np.float64)

    def per_ray_loss(s, c):
        out = VR.render(spec["lo"], spec["hi"], spec["res"], B, s, c, rays, step, CFG["near"], CFG["far"])
        return (G64 * out["rgb"]).sum(1) + ga64 * out["acc"] + gd64 * out["depth"]

    an = VG.backward(spec["lo"], spec["hi"], spec["res"], B, sigma, coef, rays, step, CFG["near"], CFG["far"], G, ga, gd)
    fwd = VR.render(spec["lo"], spec["hi"], spec["res"], B, sigma, coef, rays, step, CFG["near"], CFG["far"])
    for k in ("rgb", "acc", "depth"):                                           # the backward's own forward is the forward
        assert np.abs(an[k] - fwd[k]).max() <= 1e-14, k
    assert (an["samples"] == fwd["samples"]).all() and an["samples"].sum() >= 40

    # THE STEP.  h = 2^-16: a power of two far above the spacing of every fp32 input here (|x| < 32: spacing <= 2^-19), so x +- h are fp32
    # values and the restatement, which reads its inputs as fp32, sees exactly the step that divides the difference.
    # THE BAR, from the float64 error model of a central difference, h^2 |f'''| / 6 + eps |f| / h, term by term:
    #   f'''   an element of sigma enters through exp(-sigma_s delta) alone.  Along one ray the samples that touch a lattice point lie in the
    #          2 x 2 x 2 cells around it, so sum over them of w_e delta <= 2 |cell diagonal|; the third derivative of that ray's loss is at
    #          most (2 diag)^3 s_max, s_max = max over rays of |G|_1 + |ga| + |gd| t_far bounding every s_k and every partial sum's weight.
    #          All 12 rays may touch the point.  (coef enters linearly away from the clamp: no truncation at all.)
    #   eps|f| the loss is differenced ray by ray, so |f| is one ray's loss, <= s_max; its evaluation is a few hundred float64 operations
    #          whose errors mostly cancel in a sum of positive weights: 16 eps s_max is the allowance, and at most 12 rays add up.
    # Both terms are bounds from the inputs, fixed before any gradient is looked at; the margin over the model is not a measurement.
    h = 2.0 ** -16
    eps = 2.0 ** -53
    diag = math.sqrt(sum(((spec["hi"][i] - spec["lo"][i]) / spec["res"][i]) ** 2 for i in range(3)))
    s_max = float((np.abs(G64).sum(1) + np.abs(ga64) + np.abs(gd64) * CFG["far"]).max())
    bar = h * h / 6.0 * 12 * (2.0 * diag) ** 3 * s_max + 12 * 16 * eps * s_max / h
    assert bar <= 1e-6                                                          # gradients here are 1e-3 .. 1: the bar separates right from wrong
    # no kink within reach: a pre-clamp colour moves by at most h |w_e Y_b| <= 1.1 h under a perturbation of one coefficient
    assert an["qdist_all"] >= 10 * h, an["qdist_all"]

    rng = np.random.default_rng(78)
    # sigma: elements some sample touches that hold density themselves (the forward restatement drops the colour of a sample with
    # sigma_s <= 0, a kink at sigma_s = 0 that the points without density are differenced across below, one-sidedly)
    s_touched = np.argwhere((an["d_sigma"]["c"] > 0) & (sigma > 0))
    c_touched = np.argwhere(an["d_coef"]["c"] > 0)
    assert len(s_touched) >= 20 and len(c_touched) >= 200
    picks = [("sigma", tuple(i)) for i in s_touched[rng.choice(len(s_touched), 20, replace=False)]]
    picks += [("coef", tuple(i)) for i in c_touched[rng.choice(len(c_touched), 20, replace=False)]]
    assert len(picks) == 40
    worst, largest = 0.0, 0.0
    for which, at in picks:
        up, dn = (sigma.copy(), coef.copy()), (sigma.copy(), coef.copy())
        i = 0 if which == "sigma" else 1
        up[i][at] += np.float32(h)
        dn[i][at] -= np.float32(h)
        assert float(up[i][at]) - float(dn[i][at]) == 2 * h
        fd = float(((per_ray_loss(*up) - per_ray_loss(*dn)) / (2 * h)).sum())
        got = float(an["d_" + which]["g"][at])
        worst, largest = max(worst, abs(fd - got)), max(largest, abs(got))
        assert abs(fd - got) <= bar, (which, at, fd, got, bar)
    print(f"\n[voxgrad restatement vs central differences] worst |diff| {worst:.3e}, bar {bar:.3e}, largest gradient {largest:.3e}", end="")
    assert largest >= 1e-2

    # density where there is none: points with sigma == 0 that a sample touches.  The rendered function exists for sigma >= 0 only, so the
    # difference is one-sided, (-3 f(x) + 4 f(x + h) - f(x + 2 h)) / (2 h): truncation h^2 |f'''| / 3 and (3 + 4 + 1) / 2 = 4 times the
    # rounding term of the central form -- 4 times the bar covers both.
    z_touched = np.argwhere((an["d_sigma"]["c"] > 0) & (sigma == 0))
    assert len(z_touched) >= 8
    base = per_ray_loss(sigma, coef)
    moved = 0
    for at in (tuple(i) for i in z_touched[rng.choice(len(z_touched), 8, replace=False)]):
        one, two = sigma.copy(), sigma.copy()
        one[at] = np.float32(h)
        two[at] = np.float32(2 * h)
        fd = float(((-3.0 * base + 4.0 * per_ray_loss(one, coef) - per_ray_loss(two, coef)) / (2 * h)).sum())
        got = float(an["d_sigma"]["g"][at])
        moved += abs(got) > 1e-4
        assert abs(fd - got) <= 4 * bar, (at, fd, got, 4 * bar)
    assert moved >= 4                                                           # empty points do receive a gradient


def test_the_float32_restatement_follows_the_float64_one_and_the_skip_rule_removes_samples():
    spec, B, sigma, coef, rays, step, CFG, G, ga, gd = _case()
    args = (spec["lo"], spec["hi"], spec["res"], B, sigma, coef, rays, step, CFG["near"], CFG["far"], G, ga, gd)
    a = VG.backward(*args)
    b = VG.backward(*args, dtype=np.float32)
    assert b["d_sigma"]["g"].dtype == np.float32 and b["d_coef"]["g"].dtype == np.float32
    for k in ("d_sigma", "d_coef"):
        e = VG.error(b[k]["g"], a[k])
        print(f"\n[voxgrad restatement float32 against float64] {k}: e_ref {e:.3e}", end="")
        # No constant bounds this: the rule forms T = T (1 - alpha) and S - P_k by subtraction, so behind an opaque surface a contribution
        # can lose most of its digits in fp32 -- which is why the GPU tests measure the library against this restatement's own error.
        assert 0 < e < 1.0, (k, e)
        assert not a[k]["g"][a[k]["A"] == 0].any() and ((a[k]["c"] > 0) == (a[k]["A"] > 0)).all()
    assert not a["d_coef"]["c"][..., 3 * B:].any()                               # the padding receives nothing
    # a plane that is all ones removes nothing; all zeros removes everything; T_min only ever removes samples
    ones = np.ones(VR.skip_shape(spec["res"]), np.uint8)
    c = VG.backward(*args, skip=ones)
    assert np.array_equal(c["d_coef"]["g"], a["d_coef"]["g"]) and np.array_equal(c["d_sigma"]["g"], a["d_sigma"]["g"])
    z = VG.backward(*args, skip=0 * ones)
    assert not z["d_sigma"]["c"].any() and not z["d_coef"]["c"].any() and not z["acc"].any()
    cut = VG.backward(*args, T_min=0.2)
    assert (cut["samples"] <= a["samples"]).all() and cut["samples"].sum() < a["samples"].sum()
    # absent g_acc / g_depth are zeros; the gradient is linear in the upstream gradients
    only = VG.backward(*args[:10], G, None, None)
    zero = VG.backward(*args[:10], G, 0 * ga, 0 * gd)
    assert np.array_equal(only["d_sigma"]["g"], zero["d_sigma"]["g"]) and np.array_equal(only["d_coef"]["g"], zero["d_coef"]["g"])
    twice = VG.backward(*args[:10], 2 * G, 2 * ga, 2 * gd)
    assert np.abs(twice["d_sigma"]["g"] - 2 * a["d_sigma"]["g"]).max() <= 1e-12
