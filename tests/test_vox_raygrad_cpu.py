"""THE RAY GRADIENT RULE (mi_vox_render_backward_rays, mi_vox_render_sparse_backward_rays of include/mi_nerf_vox.h) without a GPU: the two
entries are declared, bound and exported within ABI 2 and named in INTEGRATION.md; a C99 program links against them; every refusal answers
MI_VOX_EINVAL with a message before any HIP call; and the restatement the GPU tests compare with (tests/vox_raygrad_restate.py) is the
derivative of the render rule's restatement (tests/vox_restate.py): float64 against central differences, on rays that take every branch of
the slab."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import vox_raygrad_restate as RG
from tests import vox_restate as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
f32 = np.float32
NAMES = ("mi_vox_render_backward_rays", "mi_vox_render_sparse_backward_rays")


@pytest.fixture(scope="module")
def vox():
    from nerf_pytorch_paeng_amd import _vox
    from nerf_pytorch_paeng_amd.build import build_vox_library
    build_vox_library()
    _vox.lib()
    return _vox


# ---------------------------------------------------------------------------------------------------
# header, table, symbols
# ---------------------------------------------------------------------------------------------------
def test_the_two_entries_are_declared_bound_and_exported_within_abi_2(vox):
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_vox.h")).read()
    declared = set(re.findall(r"\b(mi_vox_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", vox.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in declared and name in vox.SIGNATURES and name in exported, name
        assert name in doc, name
    assert vox.ABI_VERSION == 2 == vox.lib().mi_vox_abi_version() and "#define MI_VOX_ABI_VERSION 2" in hdr
    assert "THE RAY GRADIENT RULE" in hdr and "WRITTEN, not added" in hdr and "use_skip 0 and 1 are EQUAL" in hdr
    assert [len(vox.SIGNATURES[n][1]) for n in NAMES] == [16, 19]
    # the render entries' arguments up to cfg, then the same eight
    for new, old, k in zip(NAMES, ("mi_vox_render", "mi_vox_render_sparse"), (8, 11)):
        assert vox.SIGNATURES[new][1][:k] == vox.SIGNATURES[old][1][:k] and vox.SIGNATURES[new][1][k:] == [C.c_void_p] * 8


def test_the_kernel_lives_in_vox_hip_without_atomic_inline_assembly_or_conditional():
    src = open(os.path.join(ROOT, "nerf_pytorch_paeng_amd", "csrc", "vox.hip")).read()
    assert "void ray_grad_kernel(" in src and "fetch_record<B, ST>" in src
    assert not re.findall(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b", src, re.M) and "MN_" not in src
    assert not re.findall(r"\batomic[A-Z]|__atomic_|\basm\b", src)
    from nerf_pytorch_paeng_amd import build
    assert build.LIBRARIES["vox"] == (["vox.hip"], [], False) and len(build.LIBRARIES) == 11


def test_header_compiles_as_c99_and_the_new_entries_link_and_answer(tmp_path, vox):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not found")
    pkg = os.path.dirname(vox.LIB_PATH)
    exe = str(tmp_path / "vox_raygrad_consumer")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "vox_raygrad_consumer.c"), "-L", pkg, "-lmi_nerf_vox", f"-Wl,-rpath,{pkg}", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"vox raygrad c_abi consumer ok: ABI {vox.ABI_VERSION}" in run.stdout


# ---------------------------------------------------------------------------------------------------
# refusals: made-up addresses that are never dereferenced -- every call below is refused before the first HIP call
# ---------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
GOOD = dict(lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), res=(20, 12, 9), B=9, fmt=1, M=1000, sigma=0x1000000, coef=0x2000000, slot=0x3000000, skip=0x4000000,
            rays=0x5000000, n=257, step=0.05, near=0.0, far=6.0, T_min=0.0, bg=(1.0, 1.0, 1.0), use_skip=1, cfg=True, g_rgb=0x6000000, g_acc=0x7000000,
            g_depth=0x8000000, d_rays=0x9000000, rgb=0xA000000, acc=0xB000000, depth=0xC000000, grid=True)
# case -> (overrides, the entries it applies to: d dense, s sparse)
REFUSALS = {
    "NULL grid": (dict(grid=False), "ds"),
    "res 0": (dict(res=(20, 0, 9)), "ds"),
    "res 513": (dict(res=(513, 12, 9)), "ds"),
    "NaN box": (dict(hi=(1.0, 1.0, NAN)), "ds"),
    "B 2": (dict(B=2), "ds"),
    "fmt 2": (dict(fmt=2), "s"),
    "fmt negative": (dict(fmt=-1), "s"),
    "M negative": (dict(M=-1), "s"),
    "M above the lattice": (dict(M=21 * 13 * 10 + 1), "s"),
    "NULL cfg": (dict(cfg=False), "ds"),
    "step 0": (dict(step=0.0), "ds"),
    "step NaN": (dict(step=NAN), "ds"),
    "too many steps": (dict(step=2.0 * math.sqrt(3.0) / 65536.0), "ds"),
    "near above far": (dict(near=6.0, far=2.0), "ds"),
    "T_min 1": (dict(T_min=1.0), "ds"),
    "bg NaN": (dict(bg=(1.0, NAN, 1.0)), "ds"),
    "use_skip 2": (dict(use_skip=2), "ds"),
    "n negative": (dict(n=-1), "ds"),
    "NULL sigma": (dict(sigma=None), "ds"),
    "NULL coef": (dict(coef=None), "ds"),
    "NULL slot": (dict(slot=None), "s"),
    "NULL skip with use_skip": (dict(skip=None), "ds"),
    "NULL rays": (dict(rays=None), "ds"),
    "NULL g_rgb": (dict(g_rgb=None), "ds"),
    "NULL d_rays": (dict(d_rays=None), "ds"),
    "coef not 16-byte aligned": (dict(coef=0x2000008), "ds"),
    "slot not 4-byte aligned": (dict(slot=0x3000002), "s"),
    "sigma not 4-byte aligned": (dict(sigma=0x1000002), "ds"),
    "rays not 4-byte aligned": (dict(rays=0x5000002), "ds"),
    "g_rgb not 4-byte aligned": (dict(g_rgb=0x6000001), "ds"),
    "g_acc not 4-byte aligned": (dict(g_acc=0x7000002), "ds"),
    "g_depth not 4-byte aligned": (dict(g_depth=0x8000003), "ds"),
    "d_rays not 4-byte aligned": (dict(d_rays=0x9000002), "ds"),
    "rgb_check not 4-byte aligned": (dict(rgb=0xA000002), "ds"),
    "acc_check not 4-byte aligned": (dict(acc=0xB000001), "ds"),
    "depth_check not 4-byte aligned": (dict(depth=0xC000002), "ds"),
    "d_rays is rays": (dict(d_rays=0x5000000), "ds"),
    "d_rays ends inside rays": (dict(d_rays=0x5000000 - 257 * 24 + 4), "ds"),
}


def _call(mod, entry, a):
    L = mod.lib()
    g = C.byref(mod.Grid((C.c_float * 3)(*a["lo"]), (C.c_float * 3)(*a["hi"]), (C.c_int32 * 3)(*a["res"]))) if a["grid"] else None
    cfg = C.byref(mod.RenderCfg(a["step"], a["near"], a["far"], a["T_min"], (C.c_float * 3)(*a["bg"]), a["use_skip"])) if a["cfg"] else None
    tail = (a["g_rgb"], a["g_acc"], a["g_depth"], a["d_rays"], a["rgb"], a["acc"], a["depth"], None)
    if entry == "d":
        rc = L.mi_vox_render_backward_rays(g, a["B"], a["sigma"], a["coef"], a["skip"], a["rays"], a["n"], cfg, *tail)
    else:
        rc = L.mi_vox_render_sparse_backward_rays(g, a["B"], a["fmt"], a["sigma"], a["slot"], a["coef"], a["M"], a["skip"], a["rays"], a["n"], cfg, *tail)
    return rc, mod.last_error()


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_answer_einval_with_a_message_before_any_hip_call(vox, case):
    over, entries = REFUSALS[case]
    for entry in entries:
        rc, msg = _call(vox, entry, dict(GOOD, **over))
        assert rc == EINVAL, (case, entry, rc, msg)
        assert msg and "HIP error" not in msg, (case, entry, msg)


def test_the_good_arguments_of_the_refusal_table_reach_the_device(vox):
    """The base case is refused by nothing: each entry gets as far as its launch, which fails here for want of a device.  Nullable
    arguments may be NULL; an empty table needs no table; nothing is launched for no rays."""
    if torch.cuda.is_available():
        pytest.skip("made-up addresses must not reach a real device")
    for entry in "ds":
        for over in (dict(), dict(g_acc=None, g_depth=None, rgb=None, acc=None, depth=None), dict(skip=None, use_skip=0), dict(far=INF)):
            rc, msg = _call(vox, entry, dict(GOOD, **over))
            assert rc == 2 and "HIP error" in msg, (entry, over, rc, msg)
        assert _call(vox, entry, dict(GOOD, n=0, sigma=None, rays=None, d_rays=None, g_rgb=None))[0] == 0
    rc, msg = _call(vox, "s", dict(GOOD, M=0, coef=None))
    assert rc == 2 and "HIP error" in msg, (rc, msg)


# ---------------------------------------------------------------------------------------------------
# the restatement against central differences of the render rule's restatement, float64
# ---------------------------------------------------------------------------------------------------
LO, HI, RES, B = (-1.0, -0.7, -0.5), (0.9, 1.3, 0.8), (5, 4, 3), 9
NEAR, FAR, STEP = 0.3, 4.5, 0.13
# (what, origin, direction)
RAYS = [
    ("entry through x", (-2.5, 0.31, 0.12), (1.0, 0.05, 0.03)),
    ("entry through x, from the far side", (2.7, 0.55, 0.21), (-0.9, -0.12, -0.07)),
    ("entry through y", (0.13, -2.2, 0.22), (0.07, 1.0, -0.04)),
    ("entry through y, from the far side", (-0.33, 3.0, 0.05), (0.11, -1.1, 0.06)),
    ("entry through z", (0.21, 0.42, -2.4), (-0.05, 0.08, 1.0)),
    ("entry through z, from the far side", (-0.41, 0.17, 2.6), (0.09, 0.04, -0.95)),
    ("oblique, |d| = 2", (-2.1, -1.6, -1.2), (1.3, 1.2, 0.92)),
    ("oblique, |d| = 0.5, cut by t_far", (1.5, 1.7, 1.1), (-0.27, -0.3, -0.21)),
    ("origin inside the box: t0 = t_near", (0.1, 0.2, 0.1), (0.8, 0.45, -0.3)),
    ("origin inside, leaving through z", (-0.3, 0.6, -0.1), (0.12, -0.2, 0.9)),
    ("t_far inside the box: t1 = t_far", (-4.0, 0.4, 0.2), (1.0, 0.02, 0.01)),
    ("t_far inside the box, through y", (0.2, -4.0, 0.3), (-0.03, 1.0, 0.02)),
    ("d_y == 0", (-2.0, 0.37, -0.2), (1.0, 0.0, 0.11)),
    ("d_x == 0 and d_z == 0", (0.27, -2.0, 0.33), (0.0, 1.0, 0.0)),
    ("a miss", (-3.0, 0.1, 0.2), (-1.0, 0.1, 0.0)),
    ("a miss beside the box", (-3.0, 2.5, 0.2), (1.0, 0.0, 0.0)),
]


def _arrays():
    rng = np.random.default_rng(28)
    P = tuple(r + 1 for r in reversed(RES))
    sigma = np.where(rng.uniform(size=P) < 0.25, 0.0, rng.uniform(0.3, 5.0, P)).astype(f32)
    coef = np.zeros(P + (VR.record_floats(B),), f32)
    coef[..., :3 * B] = rng.normal(0.0, 0.5, P + (3 * B,))
    coef[..., :3] += f32(0.5 / VR.C0)
    return sigma, coef


def _rays():
    """The table's rays rounded to multiples of 2^-10: fp32 values with room for an exact step of 2^-16."""
    return (np.round(np.asarray([list(o) + list(d) for _, o, d in RAYS], np.float64) * 1024.0) / 1024.0).astype(f32)


def _loss(out, G, ga, gd):
    return (out["rgb"] * G).sum(1) + ga * out["acc"] + gd * out["depth"]


def test_the_float64_restatement_is_the_derivative_of_the_render_restatement():
    """Central differences at h and h / 2 per component.  The two estimates differ by three times the truncation error of the finer one
    (its leading term), so their spread bounds it; the rounding of a difference quotient is eps |f| / h with |f| the sum of the loss's
    absolute terms.  The analytic value is allowed FACTOR times that margin.  An element is left out when the ray's branch signature
    (slab axes, interval count, cell sequence, clamp states) differs between x - h and x + h: there the quotient straddles a kink."""
    FACTOR, h, eps = 4.0, 2.0 ** -15, 2.0 ** -52
    sigma, coef = _arrays()
    rays = _rays().astype(np.float64)
    n = len(rays)
    rng = np.random.default_rng(29)
    G, ga, gd = rng.normal(0, 1, (n, 3)).astype(f32).astype(np.float64), rng.normal(0, 1, n).astype(f32).astype(np.float64), rng.normal(0, 1, n).astype(f32).astype(np.float64)
    args = (LO, HI, RES, B, sigma, coef)
    kw = dict(T_min=0.0, bg=(0.9, 0.6, 0.3))

    # the restatements take fp32 inputs: the rays are multiples of 2^-10 below 4, so x +- h and x +- h / 2 are fp32 values too
    def render64(r):
        assert np.array_equal(r.astype(f32).astype(np.float64), r)
        return VR.render(*args, r, STEP, NEAR, FAR, **kw)

    def grad64(r):
        return RG.ray_grad(*args, r, STEP, NEAR, FAR, G, ga, gd, **kw)

    base = grad64(rays)
    out0 = render64(rays)
    for k in ("rgb", "acc", "depth"):
        assert np.array_equal(base[k], out0[k]), k                                           # one forward in both restatements
    # the rays take the branches they are named for
    sig = base["sig"]
    assert [s[0] for s in sig[:6]] == [0, 0, 1, 1, 2, 2] and all(s[1] >= 0 for s in sig[:6])
    assert sig[8][0] == -1 and sig[9][0] == -1 and sig[9][1] == 2 and sig[10][1] == -1 and sig[11][1] == -1 and sig[10][0] == 0 and sig[11][0] == 1
    assert sig[14][2] and sig[15][2] and not any(s[2] for s in sig[:14])
    assert not base["g"][14:].any() and not base["A"][14:].any()
    assert all(any(smp[3] for smp in s[3]) for s in sig[:14])                               # every hit ends in a cut interval
    assert (base["samples"][:14] >= 3).all() and float(out0["acc"][:14].min()) > 0.05
    F = np.abs(out0["rgb"] * G).sum(1) + np.abs(ga * out0["acc"]) + np.abs(gd * out0["depth"])
    left_out = tested = 0
    worst = 0.0
    for j in range(6):
        est = []
        for hh in (h, 0.5 * h):
            up, dn = rays.copy(), rays.copy()
            up[:, j] += hh
            dn[:, j] -= hh
            est.append((_loss(render64(up), G, ga, gd) - _loss(render64(dn), G, ga, gd)) / (2.0 * hh))
            if hh == h:
                s_up, s_dn = grad64(up)["sig"], grad64(dn)["sig"]
        for i in range(14):
            if s_up[i] != s_dn[i] or s_up[i] != sig[i]:
                left_out += 1
                continue
            tested += 1
            margin = abs(est[0][i] - est[1][i]) + eps * F[i] / (0.5 * h)
            err = abs(base["g"][i, j] - est[1][i])
            worst = max(worst, err / margin)
            assert err <= FACTOR * margin, (RAYS[i][0], j, base["g"][i, j], est[0][i], est[1][i], margin)
    print(f"\n[raygrad fd] {tested} elements tested, {left_out} left out at a kink, worst error / margin {worst:.3f}", end="")
    assert left_out <= 0.1 * (left_out + tested), (left_out, tested)
    assert np.abs(base["g"][:14]).min(0).max() > 1e-3 and (np.abs(base["g"][:14]) > 1e-6).mean() > 0.9


def test_the_float32_restatement_follows_the_float64_one_within_the_bar_s_scale():
    sigma, coef = _arrays()
    rays = _rays()
    rng = np.random.default_rng(29)
    n = len(rays)
    G, ga, gd = rng.normal(0, 1, (n, 3)).astype(f32), rng.normal(0, 1, n).astype(f32), rng.normal(0, 1, n).astype(f32)
    a = RG.ray_grad(LO, HI, RES, B, sigma, coef, rays, STEP, NEAR, FAR, G, ga, gd, bg=(0.9, 0.6, 0.3))
    b = RG.ray_grad(LO, HI, RES, B, sigma, coef, rays, STEP, NEAR, FAR, G, ga, gd, bg=(0.9, 0.6, 0.3), dtype=np.float32)
    assert b["g"].dtype == np.float32 and a["g"].dtype == np.float64
    e = RG.error(b["g"], a)
    assert 0 < e <= int(a["c"].max()) * 2.0 ** -24, e                                        # A is the scale of the rounding
    assert (a["A"][:14] >= np.abs(a["g"][:14])).all()
    # absent upstream gradients are zeros
    z = np.zeros(n, f32)
    c = RG.ray_grad(LO, HI, RES, B, sigma, coef, rays, STEP, NEAR, FAR, G, bg=(0.9, 0.6, 0.3))
    d = RG.ray_grad(LO, HI, RES, B, sigma, coef, rays, STEP, NEAR, FAR, G, z, z, bg=(0.9, 0.6, 0.3))
    assert np.array_equal(c["g"], d["g"])
