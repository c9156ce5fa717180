"""A SIGNED GRID (mi_vox_build_skip_signed, mi_vox_render_signed, mi_vox_render_sparse_signed of include/mi_nerf_vox.h; the Signed paragraph
of THE BACKWARD RULE of include/mi_nerf_voxgrad.h) without a GPU:
  (a) the three entries are declared, bound and exported within ABI 2 and named in INTEGRATION.md; a C99 program links against them; every
      refusal answers MI_VOX_EINVAL with a message before any HIP call;
  (b) on planes that are >= 0 the signed restatement (tests/vox_signed_restate.py) equals tests/vox_restate.py's, array-equal in fp32 and fp64;
  (c) the float64 signed backward is the derivative of the signed render: central differences on a plane of mixed signs;
  (d) a planar front is found inside a cell by the signed rule and on a lattice plane by the unsigned one;
  (e) a sphere's silhouette error at least halves under ``to_signed``'s rule;
  (f) the header's statements about the tool chain on a signed plane hold in the restatements."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import vox_refine_restate as RF
from tests import vox_restate as VR
from tests import vox_signed_restate as SR
from tests import vox_sparse_restate as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
f32 = np.float32
NAMES = ("mi_vox_build_skip_signed", "mi_vox_render_signed", "mi_vox_render_sparse_signed")
TWINS = ("mi_vox_build_skip", "mi_vox_render", "mi_vox_render_sparse")


@pytest.fixture(scope="module")
def vox():
    from nerf_pytorch_paeng_amd import _vox
    from nerf_pytorch_paeng_amd.build import build_vox_library
    build_vox_library()
    _vox.lib()
    return _vox


# ---------------------------------------------------------------------------------------------------
# (a) header, table, symbols, a C99 consumer, refusals
# ---------------------------------------------------------------------------------------------------
def test_the_three_entries_are_declared_bound_and_exported_within_abi_2(vox):
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_vox.h")).read()
    declared = set(re.findall(r"\b(mi_vox_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", vox.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, twin in zip(NAMES, TWINS):
        assert name in declared and name in vox.SIGNATURES and name in exported and name in doc, name
        assert vox.SIGNATURES[name] == vox.SIGNATURES[twin], name                  # the arguments of the unsigned counterpart
    assert vox.ABI_VERSION == 2 == vox.lib().mi_vox_abi_version() and "#define MI_VOX_ABI_VERSION 2" in hdr
    assert "A SIGNED GRID" in hdr and "sigma_s = fmaxf(the interpolation of sigma, 0)" in hdr and "0 iff sigma <= 0" in hdr
    grad = open(os.path.join(ROOT, "include", "mi_nerf_voxgrad.h")).read()
    assert "A SIGNED GRID of include/mi_nerf_vox.h" in grad and "only where the interpolation is >= 0" in grad
    assert "#define MI_VOXGRAD_ABI_VERSION 1" in grad


def test_the_signed_kernels_live_in_vox_hip_beside_the_unsigned_ones():
    src = open(os.path.join(ROOT, "nerf_pytorch_paeng_amd", "csrc", "vox.hip")).read()
    assert "void render_signed_kernel(" in src and "void skip_signed_kernel(" in src and "void render_kernel(" in src and "void skip_kernel(" in src
    assert not re.findall(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b", src, re.M) and not re.findall(r"\batomic[A-Z]|__atomic_|\basm\b|__shared__ float", src)
    signed = src[src.index("void render_signed_kernel("):src.index("mi_vox_render_backward_rays, mi_vox_render_sparse_backward_rays")]
    assert "fmaxf(group_sum(w * a.sigma[at]), 0.0f)" in signed and "__shared__" not in signed
    back = open(os.path.join(ROOT, "nerf_pytorch_paeng_amd", "csrc", "voxgrad.hip")).read()
    assert back.count("fmaxf(group_sum(w * a.sigma[at]), 0.0f)") == 1 and "fmaxf(raw_s, 0.0f)" in back and "if (raw_s >= 0.0f) ps += w * dsig;" in back


def test_header_compiles_as_c99_and_the_signed_entries_link_and_answer(tmp_path, vox):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not found")
    pkg = os.path.dirname(vox.LIB_PATH)
    exe = str(tmp_path / "vox_signed_consumer")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "vox_signed_consumer.c"), "-L", pkg, "-lmi_nerf_vox", f"-Wl,-rpath,{pkg}", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"vox signed c_abi consumer ok: ABI {vox.ABI_VERSION}" in run.stdout


# made-up addresses that are never dereferenced: every call below is refused before the first HIP call
NAN, INF = float("nan"), float("inf")
GOOD = dict(lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), res=(20, 12, 9), B=9, fmt=1, M=1000, sigma=0x1000000, coef=0x2000000, slot=0x3000000, skip=0x4000000,
            rays=0x5000000, n=257, step=0.05, near=0.0, far=6.0, T_min=0.0, bg=(1.0, 1.0, 1.0), use_skip=1, cfg=True, rgb=0xA000000, disp=0xB000000,
            acc=0xC000000, depth=0xD000000, visited=0xE000000, grid=True)
# case -> (overrides, the entries it applies to: k skip builder, d dense renderer, s sparse renderer): the refusals of the unsigned entries
REFUSALS = {
    "NULL grid": (dict(grid=False), "kds"),
    "res 0": (dict(res=(20, 0, 9)), "kds"),
    "res 513": (dict(res=(513, 12, 9)), "kds"),
    "lo above hi": (dict(lo=(1.0, -1.0, -1.0), hi=(-1.0, 1.0, 1.0)), "kds"),
    "NaN box": (dict(hi=(1.0, 1.0, NAN)), "kds"),
    "infinite box": (dict(hi=(INF, 1.0, 1.0)), "kds"),
    "B 2": (dict(B=2), "ds"),
    "B 0": (dict(B=0), "ds"),
    "fmt 2": (dict(fmt=2), "s"),
    "fmt negative": (dict(fmt=-1), "s"),
    "M negative": (dict(M=-1), "s"),
    "M above the lattice": (dict(M=21 * 13 * 10 + 1), "s"),
    "NULL cfg": (dict(cfg=False), "ds"),
    "step 0": (dict(step=0.0), "ds"),
    "step NaN": (dict(step=NAN), "ds"),
    "step infinite": (dict(step=INF), "ds"),
    "too many steps": (dict(step=2.0 * math.sqrt(3.0) / 65536.0), "ds"),
    "near above far": (dict(near=6.0, far=2.0), "ds"),
    "near NaN": (dict(near=NAN), "ds"),
    "T_min negative": (dict(T_min=-0.1), "ds"),
    "T_min 1": (dict(T_min=1.0), "ds"),
    "bg NaN": (dict(bg=(1.0, NAN, 1.0)), "ds"),
    "use_skip 2": (dict(use_skip=2), "ds"),
    "n negative": (dict(n=-1), "ds"),
    "NULL sigma": (dict(sigma=None), "kds"),
    "NULL coef": (dict(coef=None), "ds"),
    "NULL slot": (dict(slot=None), "s"),
    "NULL skip": (dict(skip=None), "kds"),
    "NULL rays": (dict(rays=None), "ds"),
    "NULL rgb": (dict(rgb=None), "ds"),
    "coef not 16-byte aligned": (dict(coef=0x2000008), "ds"),
    "slot not 4-byte aligned": (dict(slot=0x3000002), "s"),
    "sigma not 4-byte aligned": (dict(sigma=0x1000002), "kds"),
    "rays not 4-byte aligned": (dict(rays=0x5000002), "ds"),
    "rgb not 4-byte aligned": (dict(rgb=0xA000002), "ds"),
    "disp not 4-byte aligned": (dict(disp=0xB000001), "ds"),
    "acc not 4-byte aligned": (dict(acc=0xC000002), "ds"),
    "depth not 4-byte aligned": (dict(depth=0xD000003), "ds"),
    "visited not 4-byte aligned": (dict(visited=0xE000002), "ds"),
}


def _call(mod, entry, a, signed=True):
    L = mod.lib()
    g = C.byref(mod.Grid((C.c_float * 3)(*a["lo"]), (C.c_float * 3)(*a["hi"]), (C.c_int32 * 3)(*a["res"]))) if a["grid"] else None
    cfg = C.byref(mod.RenderCfg(a["step"], a["near"], a["far"], a["T_min"], (C.c_float * 3)(*a["bg"]), a["use_skip"])) if a["cfg"] else None
    tail = (a["rays"], a["n"], cfg, a["rgb"], a["disp"], a["acc"], a["depth"], a["visited"], None)
    name = {"k": "mi_vox_build_skip", "d": "mi_vox_render", "s": "mi_vox_render_sparse"}[entry] + ("_signed" if signed else "")
    if entry == "k":
        rc = getattr(L, name)(g, a["sigma"], a["skip"], None)
    elif entry == "d":
        rc = getattr(L, name)(g, a["B"], a["sigma"], a["coef"], a["skip"], *tail)
    else:
        rc = getattr(L, name)(g, a["B"], a["fmt"], a["sigma"], a["slot"], a["coef"], a["M"], a["skip"], *tail)
    return rc, mod.last_error(), name


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_answer_einval_with_a_message_before_any_hip_call(vox, case):
    over, entries = REFUSALS[case]
    for entry in entries:
        rc, msg, name = _call(vox, entry, dict(GOOD, **over))
        assert rc == EINVAL, (case, entry, rc, msg)
        assert msg and "HIP error" not in msg and msg.startswith(name), (case, entry, msg)
        rc_u, msg_u, name_u = _call(vox, entry, dict(GOOD, **over), signed=False)    # the unsigned counterpart refuses it too, in the same words
        assert rc_u == EINVAL and msg_u[len(name_u):] == msg[len(name):], (case, entry, msg, msg_u)


def test_the_good_arguments_of_the_refusal_table_reach_the_device(vox):
    """The table's base case is refused by nothing: it gets as far as its launch, which fails here for want of a device -- so every
    refusal above is owed to its one override.  Nothing is launched for no work, and no pointer is looked at then."""
    for entry in "ds":
        assert _call(vox, entry, dict(GOOD, n=0))[0] == 0
        assert _call(vox, entry, dict(GOOD, n=0, sigma=None, coef=0x2000008, slot=None, skip=None, rays=None, rgb=None))[0] == 0
    if torch.cuda.is_available():
        pytest.skip("made-up addresses must not reach a real device")
    for entry in "kds":
        for over in (dict(), dict(disp=None, acc=None, depth=None, visited=None)) + ((dict(skip=None, use_skip=0), dict(far=INF)) if entry != "k" else ()):
            rc, msg, _ = _call(vox, entry, dict(GOOD, **over))
            assert rc == 2 and "HIP error" in msg, (entry, over, rc, msg)


# ---------------------------------------------------------------------------------------------------
# (b) on a plane that is >= 0 the two rules are one
# ---------------------------------------------------------------------------------------------------
def _small_case(B=9, n=12):
    from tests.test_gpu_vox import CFG, GRID_SPECS, grid_arrays, make_rays
    spec = GRID_SPECS["5x4x3"]
    sigma, coef = grid_arrays("5x4x3", B)
    rays = make_rays(spec["lo"], spec["hi"], n, 10 + B)
    step = 0.5 * float(min((f32(spec["hi"][i]) - f32(spec["lo"][i])) / f32(spec["res"][i]) for i in range(3)))
    return spec, sigma, coef, rays, step, CFG


def mixed_signs(P, seed):
    """A plane of mixed signs, fp32: magnitudes 0.5 .. 12, about 45 % of the points negative."""
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0.5, 12.0, P)
    return (mag * np.where(rng.uniform(size=P) < 0.45, -1.0, 1.0)).astype(f32)


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
@pytest.mark.parametrize("B", (1, 4, 9))
def test_on_a_nonnegative_plane_the_signed_restatement_equals_the_unsigned_one(B, dtype):
    spec, sigma, coef, rays, step, CFG = _small_case(B, 40)
    assert (sigma >= 0).all() and (sigma == 0).any() and (sigma > 0).any()
    for T_min in (0.0, 1e-3):
        a = VR.render(spec["lo"], spec["hi"], spec["res"], B, sigma, coef, rays, step, CFG["near"], CFG["far"], T_min=T_min, dtype=dtype)
        b = SR.render(spec["lo"], spec["hi"], spec["res"], B, sigma, coef, rays, step, CFG["near"], CFG["far"], T_min=T_min, dtype=dtype)
        for k in ("rgb", "disp", "acc", "depth", "samples"):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), (k, T_min)
    assert a["acc"].max() > 0.05
    for res in ((5, 4, 3), (17, 9, 20), (24, 24, 24)):
        P = tuple(r + 1 for r in reversed(res))
        rng = np.random.default_rng(sum(res))
        for s in (np.zeros(P, f32), np.where(rng.uniform(size=P) < 0.004, 1.0, 0.0).astype(f32)):
            assert np.array_equal(SR.build_skip(s, res), VR.build_skip(s, res))
        # and on a signed plane the byte says "no point > 0", which negatives do not set
        neg = np.where(rng.uniform(size=P) < 0.004, 1.0, -3.0).astype(f32)
        assert np.array_equal(SR.build_skip(neg, res), VR.build_skip(np.maximum(neg, 0), res)) and VR.build_skip(neg, res).all()


# ---------------------------------------------------------------------------------------------------
# (c) the float64 signed backward against central differences of the signed render
# ---------------------------------------------------------------------------------------------------
def test_the_signed_backward_meets_central_differences_of_the_signed_render_in_float64():
    """The setting of tests/test_voxgrad_cpu.py -- the 5x4x3 grid, B = 9, its 12 rays, h = 2^-16 and its bar, formula and reasoning -- on a
    plane of mixed signs.  The ReLU adds one kink, at interpolation = 0; the seed is one for which every sample's |interpolation| is at
    least 2^-10, 64 times the step, and the test asserts that itself: no sample and no element is excluded."""
    spec, _, coef, rays, step, CFG = _small_case(9, 12)
    B = 9
    sigma = mixed_signs(coef.shape[:3], 200)
    assert (sigma < 0).sum() >= 40 and (sigma > 0).sum() >= 40 and rays.shape == (12, 6)
    rng = np.random.default_rng(77)
    G = rng.normal(0.0, 1.0, (12, 3)).astype(f32)
    ga = rng.normal(0.0, 1.0, 12).astype(f32)
    gd = rng.normal(0.0, 1.0, 12).astype(f32)
    G64, ga64, gd64 = G.astype(np.float64), ga.astype(np.float64), gd.astype(np.float64)
    args = (spec["lo"], spec["hi"], spec["res"], B)

    def per_ray_loss(s, c):
        out = SR.render(*args, s, c, rays, step, CFG["near"], CFG["far"])
        return (G64 * out["rgb"]).sum(1) + ga64 * out["acc"] + gd64 * out["depth"]

    an = SR.backward(*args, sigma, coef, rays, step, CFG["near"], CFG["far"], G, ga, gd)
    fwd = SR.render(*args, sigma, coef, rays, step, CFG["near"], CFG["far"])
    for k in ("rgb", "acc", "depth"):
        assert np.abs(an[k] - fwd[k]).max() <= 1e-14, k
    assert (an["samples"] == fwd["samples"]).all() and an["samples"].sum() >= 40
    h = 2.0 ** -16
    # THE CONDITION: a perturbation of one element by h moves an interpolation by at most h (weights <= 1), so no sample changes sides
    assert an["min_abs"] >= 2.0 ** -10 and fwd["min_abs"] == an["min_abs"], an["min_abs"]
    assert an["qdist_all"] >= 10 * h, an["qdist_all"]
    eps = 2.0 ** -53
    diag = math.sqrt(sum(((spec["hi"][i] - spec["lo"][i]) / spec["res"][i]) ** 2 for i in range(3)))
    s_max = float((np.abs(G64).sum(1) + np.abs(ga64) + np.abs(gd64) * CFG["far"]).max())
    bar = h * h / 6.0 * 12 * (2.0 * diag) ** 3 * s_max + 12 * 16 * eps * s_max / h
    assert bar <= 1e-6
    # every element of sigma that a sample touches -- those that only samples below 0 touch included: they must get exactly nothing --
    # and twenty coefficients
    touched = np.argwhere((an["d_sigma"]["c"] > 0) | an["neg_only"])
    assert len(touched) >= 30 and an["neg_only"].any() and not an["d_sigma"]["g"][an["neg_only"]].any()
    c_touched = np.argwhere(an["d_coef"]["c"] > 0)
    picks = [("sigma", tuple(i)) for i in touched] + [("coef", tuple(i)) for i in c_touched[np.random.default_rng(78).choice(len(c_touched), 20, replace=False)]]
    worst = largest = 0.0
    for which, at in picks:
        up, dn = (sigma.copy(), coef.copy()), (sigma.copy(), coef.copy())
        i = 0 if which == "sigma" else 1
        up[i][at] += f32(h)
        dn[i][at] -= f32(h)
        assert float(up[i][at]) - float(dn[i][at]) == 2 * h
        fd = float(((per_ray_loss(*up) - per_ray_loss(*dn)) / (2 * h)).sum())
        got = float(an["d_" + which]["g"][at])
        worst, largest = max(worst, abs(fd - got)), max(largest, abs(got))
        assert abs(fd - got) <= bar, (which, at, fd, got, bar)
    print(f"\n[signed backward vs central differences] {len(picks)} elements, worst |diff| {worst:.3e}, bar {bar:.3e}, largest gradient {largest:.3e}", end="")
    assert largest >= 1e-2
    # the unsigned rule's gradient is another one on this plane: the widening is not a no-op
    from tests import voxgrad_restate as VG
    old = VG.backward(*args, np.maximum(sigma, 0), coef, rays, step, CFG["near"], CFG["far"], G, ga, gd)
    assert np.abs(old["d_sigma"]["g"] - an["d_sigma"]["g"]).max() > 1e-3


def test_on_a_nonnegative_plane_the_signed_backward_is_the_backward_rule():
    from tests import voxgrad_restate as VG
    spec, sigma, coef, rays, step, CFG = _small_case(9, 12)
    rng = np.random.default_rng(77)
    G, ga, gd = rng.normal(0.0, 1.0, (12, 3)).astype(f32), rng.normal(0.0, 1.0, 12).astype(f32), rng.normal(0.0, 1.0, 12).astype(f32)
    args = (spec["lo"], spec["hi"], spec["res"], 9, sigma, coef, rays, step, CFG["near"], CFG["far"], G, ga, gd)
    for dtype in (np.float32, np.float64):
        a, b = VG.backward(*args, dtype=dtype), SR.backward(*args, dtype=dtype)
        for k in ("d_sigma", "d_coef"):
            assert np.array_equal(a[k]["g"], b[k]["g"]) and np.array_equal(a[k]["c"], b[k]["c"]) and np.array_equal(a[k]["A"], b[k]["A"]), (k, dtype)
        for k in ("rgb", "acc", "depth"):
            assert np.array_equal(a[k], b[k]), (k, dtype)
    assert not b["neg_only"].any()


# ---------------------------------------------------------------------------------------------------
# (d) a planar front: the signed rule finds it inside a cell
# ---------------------------------------------------------------------------------------------------
def test_a_planar_front_is_found_inside_its_cell_by_the_signed_rule_alone():
    """8^3 cells of edge 0.25 in [-1, 1]^3, a front x >= x0 of density 4096, rays along +x, intervals of a cell / 8.  The unsigned plane
    knows inside and outside (4096 where x_j > x0, else 0): the same plane for every x0 in [0, 0.25), so the same depth.  The signed
    plane is the field 4096 (x - x0) / cell clipped to +-4096: linear across the front's cell, with its zero at x0."""
    res, lo, hi, cell, dense = (8, 8, 8), (-1.0,) * 3, (1.0,) * 3, 0.25, 4096.0
    step = cell / 8
    xs = -1.0 + cell * np.arange(9)
    rng = np.random.default_rng(5)
    rays = np.zeros((16, 6), f32)
    rays[:, 0], rays[:, 1:3], rays[:, 3] = -2.0, rng.uniform(-0.9, 0.9, (16, 2)), 1.0
    coef = np.zeros((9, 9, 9, 4), f32)
    depths_u, depths_s = [], []
    for x0 in (0.0, 0.05, 0.1, 0.2):
        inside = np.broadcast_to(np.where(xs > x0, dense, 0.0), (9, 9, 9)).astype(f32)
        smooth = np.broadcast_to(np.clip(dense * (xs - x0) / cell, -dense, dense), (9, 9, 9)).astype(f32)
        u = VR.render(lo, hi, res, 1, inside, coef, rays, step, 0.0, 10.0)
        s = SR.render(lo, hi, res, 1, smooth, coef, rays, step, 0.0, 10.0)
        assert np.abs(u["acc"] - 1).max() < 1e-6 and np.abs(s["acc"] - 1).max() < 1e-6
        hit = x0 + 2.0                                                           # the ray parameter at the front: o_x = -2, |d| = 1
        assert np.abs(s["depth"] - hit).max() <= step, (x0, s["depth"] - 2.0)
        depths_u.append(u["depth"])
        depths_s.append(s["depth"])
        print(f"\n[planar front x0={x0}] depth - o_x: signed {float(s['depth'].mean()) - 2.0:.3f}, unsigned {float(u['depth'].mean()) - 2.0:.3f}", end="")
    for dpt in depths_u[1:]:
        assert np.array_equal(dpt, depths_u[0])                                  # the unsigned rule answers the same for all four
    assert float(depths_s[3].mean() - depths_s[0].mean()) > 0.15                 # the signed rule's answers follow the front


# ---------------------------------------------------------------------------------------------------
# (e) a sphere's silhouette
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", (16, 32))
def test_a_spheres_silhouette_error_halves_under_to_signed(res):
    """A sphere of radius 0.6 in [-1, 1]^3, binary density 4096 / 0 at the lattice points, 96 x 96 orthographic rays along +z, step of half
    a cell; truth: acc = 1 inside the disc of radius 0.6.  Observed ratios signed / unsigned of mean |acc - truth|: 0.33 and 0.15."""
    n, radius, dense = 96, 0.6, 4096.0
    x = np.linspace(-1.0, 1.0, res + 1)
    Z, Y, X = np.meshgrid(x, x, x, indexing="ij")
    inside = np.where(X * X + Y * Y + Z * Z < radius * radius, dense, 0.0).astype(f32)
    px = (np.arange(n) + 0.5) / n * 2.0 - 1.0
    U, V = np.meshgrid(px, px, indexing="xy")
    rays = np.zeros((n * n, 6), f32)
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 5] = U.reshape(-1), V.reshape(-1), -2.0, 1.0
    truth = (rays[:, 0].astype(np.float64) ** 2 + rays[:, 1].astype(np.float64) ** 2 < radius * radius).astype(np.float64)
    coef = np.zeros(inside.shape + (4,), f32)
    step = 0.5 * (2.0 / res)
    signed = SR.to_signed(inside)
    assert signed.min() == -dense and (signed == 0).any() and np.array_equal(signed > 0, inside > 0)
    e_u = float(np.abs(VR.render((-1.0,) * 3, (1.0,) * 3, (res,) * 3, 1, inside, coef, rays, step, 0.0, 10.0)["acc"] - truth).mean())
    s = SR.render((-1.0,) * 3, (1.0,) * 3, (res,) * 3, 1, signed, coef, rays, step, 0.0, 10.0)
    e_s = float(np.abs(s["acc"] - truth).mean())
    area_u = float(VR.render((-1.0,) * 3, (1.0,) * 3, (res,) * 3, 1, inside, coef, rays, step, 0.0, 10.0)["acc"].mean() / truth.mean())
    print(f"\n[sphere {res}^3] mean |acc - truth|: unsigned {e_u:.4f}, signed {e_s:.4f}, ratio {e_s / e_u:.2f}; covered / true area: unsigned {area_u:.3f}, "
          f"signed {float(s['acc'].mean() / truth.mean()):.3f}", end="")
    assert e_u > 0.02 and e_s <= 0.5 * e_u, (e_u, e_s)


# ---------------------------------------------------------------------------------------------------
# (f) the tool chain on a signed plane
# ---------------------------------------------------------------------------------------------------
def _blob_plane(P, seed):
    """A signed plane with blobs of density, a negative halo around them that reaches further than one point, and zeros far away."""
    from tests.test_gpu_vox import _blobs
    rng = np.random.default_rng(seed)
    mask = _blobs(P, rng, 0.75)
    near = SP.active_set(SP.active_set(mask.astype(f32)).astype(f32))             # two points around the density
    sigma = np.where(mask, rng.uniform(0.5, 12.0, P), np.where(near, -rng.uniform(0.5, 12.0, P), 0.0)).astype(f32)
    return sigma


def test_the_tool_chain_reads_a_signed_plane_as_the_header_says():
    res, lo, hi, B = (9, 8, 7), (-1.0, -0.9, -0.8), (1.0, 0.9, 0.8), 4
    P = tuple(r + 1 for r in reversed(res))
    sigma = _blob_plane(P, 11)
    assert (sigma > 0).sum() > 30 and (sigma < 0).sum() > 30 and (sigma == 0).sum() > 30
    rng = np.random.default_rng(12)
    coef = np.zeros(P + (16,), f32)
    coef[..., :12] = rng.normal(0.0, 0.8, P + (12,))
    coef[..., :3] += f32(0.5 / VR.C0)
    rays = RF.rays_into_box(lo, hi, 48, 13)
    step = 0.5 * float(min((f32(hi[i]) - f32(lo[i])) / f32(res[i]) for i in range(3)))
    keys = ("rgb", "disp", "acc", "depth")

    def render(s, c, dtype=np.float32, skip=None):
        return SR.render(lo, hi, res, B, s, c, rays, step, 0.0, 10.0, dtype=dtype, skip=skip)

    base = render(sigma, coef)
    assert base["acc"].max() > 0.3
    # skipping: a sample in a block whose signed byte is 0 adds exactly nothing
    plane = SR.build_skip(sigma, res)
    skipped = render(sigma, coef, skip=plane)
    for k in keys:
        assert np.array_equal(base[k], skipped[k], equal_nan=True), k
    # 1. activity and compact storage: wherever the rule reads a record, the record is in the table
    slot, M = SP.slots(sigma)
    assert np.array_equal(slot >= 0, SP.active_set(np.maximum(sigma, 0))) and 0 < M < sigma.size
    for fmt in (0, 1):
        table = SP.table_of(coef, slot, M, fmt)
        through = SP.to_dense(slot, table, M)                                    # zero records at inactive points
        want = render(sigma, SP.pack(coef.reshape(-1, 16), fmt).astype(f32).reshape(coef.shape))      # the dense records, rounded as the table's
        got = render(sigma, through)
        for k in keys:
            assert np.array_equal(got[k], want[k], equal_nan=True), (fmt, k)
    # 2. mi_vox_prune at tau = 0 changes no output bit, though it does change the plane
    s2, c2 = RF.prune(sigma, coef, 0.0)
    assert (s2 != sigma).any() and (s2[sigma > 0] == sigma[sigma > 0]).all()
    pruned = render(s2, c2)
    for k in keys:
        assert np.array_equal(base[k], pruned[k], equal_nan=True), k
    assert np.array_equal(SR.build_skip(s2, res), plane)
    # 3. invisible negatives: a point <= 0 whose 26 neighbours are <= 0 may hold any negative number
    hidden = ~SP.active_set(np.maximum(sigma, 0))
    assert hidden.sum() > 30
    wild = sigma.copy()
    wild[hidden] = -rng.uniform(0.0, 1e6, int(hidden.sum())).astype(f32)
    other = render(wild, coef)
    for k in keys:
        assert np.array_equal(base[k], other[k], equal_nan=True), k
    # 4. mi_vox_resample: an integer refinement represents the identical field -- float64 renders at the coarse grid's step agree to the
    # rounding of the resampled values (fp32 values of a float64 interpolation: relative 2^-24 of sigma, times an optical depth <= 12 * 4)
    fine = tuple(2 * r for r in res)
    s_f, c_f = RF.resample(lo, hi, res, lo, hi, fine, B, sigma, coef, dtype=np.float64)
    a = render(sigma, coef, np.float64)
    b = SR.render(lo, hi, fine, B, s_f.astype(f32), c_f.astype(f32), rays, step, 0.0, 10.0)
    for k in ("rgb", "acc", "depth"):
        assert np.abs(a[k] - b[k]).max() <= 2.0 ** -24 * 48 * 16, (k, float(np.abs(a[k] - b[k]).max()))
    assert (s_f < 0).any() and (s_f > 0).any()
