"""Pruning by visibility (mi_vox_view, mi_vox_shadow_bytes, mi_vox_shadow, mi_vox_seen, mi_vox_prune_seen of include/mi_nerf_vox.h) without
a GPU: the struct and the four entries are declared, bound and exported within ABI 2; a C99 program links against them; every refusal
answers MI_VOX_EINVAL with a message before any HIP call; and the restatement the GPU tests compare with (tests/vox_seen_restate.py) has
the properties the header states -- Beer-Lambert's optical depth in a uniform box, nothing in front of a wall and the wall's depth behind
it, the pruning rule itself under od_max = +inf."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import vox_refine_restate as RR
from tests import vox_seen_restate as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
f32 = np.float32
NAMES = ("mi_vox_shadow_bytes", "mi_vox_shadow", "mi_vox_seen", "mi_vox_prune_seen")


@pytest.fixture(scope="module")
def vox():
    from nerf_pytorch_paeng_amd import _vox
    from nerf_pytorch_paeng_amd.build import build_vox_library
    build_vox_library()
    _vox.lib()
    return _vox


def _grid(vox, lo, hi, res):
    return vox.Grid((C.c_float * 3)(*lo), (C.c_float * 3)(*hi), (C.c_int32 * 3)(*res))


# ---------------------------------------------------------------------------------------------------
# header, table, symbols
# ---------------------------------------------------------------------------------------------------
def test_the_view_and_the_four_entries_are_declared_bound_and_exported_within_abi_2(vox):
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_vox.h")).read()
    declared = set(re.findall(r"\b(mi_vox_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", vox.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in declared and name in vox.SIGNATURES and name in exported, name
        assert name in doc, name
    assert "mi_vox_view" in doc and "typedef struct mi_vox_view" in hdr
    assert vox.ABI_VERSION == 2 == vox.lib().mi_vox_abi_version() and "#define MI_VOX_ABI_VERSION 2" in hdr
    for rule in ("THE SHADOW RULE", "THE VISIBILITY RULE", "THE SEEN PRUNING RULE"):
        assert rule in hdr, rule
    assert C.sizeof(vox.View) == 84
    assert [n for n, _ in vox.View._fields_] == ["H", "W", "fx", "fy", "cx", "cy", "c2w", "depth_near", "depth_step", "slices"]
    assert [len(vox.SIGNATURES[n][1]) for n in NAMES] == [1, 6, 6, 9]
    assert vox.SIGNATURES["mi_vox_seen"][1][3] is C.c_int32 and vox.SIGNATURES["mi_vox_prune_seen"][1][2:4] == [C.c_float, C.c_float]
    assert vox.SIGNATURES["mi_vox_shadow_bytes"][0] is C.c_size_t


def test_the_new_source_text_holds_no_atomic_no_inline_assembly_and_no_conditional():
    """The expression of tests/test_vox_cpu.py, on the text as it stands with the new kernels in it."""
    for name in ("vox.hip", "vox_rule.h"):
        src = open(os.path.join(ROOT, "nerf_pytorch_paeng_amd", "csrc", name)).read()
        assert not re.findall(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b", src, re.M) and "MN_" not in src, name
        assert not re.findall(r"\batomic[A-Z]|__atomic_|\basm\b", src), name
    src = open(os.path.join(ROOT, "nerf_pytorch_paeng_amd", "csrc", "vox.hip")).read()
    for kernel in ("shadow_kernel", "seen_kernel", "prune_seen_kernel"):
        assert f"void {kernel}(" in src, kernel


def test_header_compiles_as_c99_and_the_new_entries_link_and_answer(tmp_path, vox):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not found")
    pkg = os.path.dirname(vox.LIB_PATH)
    exe = str(tmp_path / "vox_seen_consumer")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "vox_seen_consumer.c"), "-L", pkg, "-lmi_nerf_vox", f"-Wl,-rpath,{pkg}", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"vox seen c_abi consumer ok: ABI {vox.ABI_VERSION}" in run.stdout


def test_the_size_of_a_shadow_volume_follows_its_formula(vox):
    L = vox.lib()
    eye = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 4.0)
    for H, W, K in ((1, 1, 8), (19, 23, 64), (800, 800, 528), (8192, 8192, 65536)):
        v = vox.View(H, W, 30.0, 30.0, 11.0, 9.0, (C.c_float * 12)(*eye), 2.0, 0.05, K)
        assert L.mi_vox_shadow_bytes(C.byref(v)) == H * W * K * 4, (H, W, K)
    assert L.mi_vox_shadow_bytes(None) == 0 and "view" in vox.last_error()


# ---------------------------------------------------------------------------------------------------
# refusals: made-up addresses that are never dereferenced -- every call below is refused before the first HIP call.  The addresses lie
# 16 MiB apart: the largest array of the base case (a 21 x 13 x 10 lattice of 128-byte records; a 19 x 23 x 64 volume) stays below that.
# ---------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
POSE = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 4.0)
GOOD = dict(lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), res=(20, 12, 9), B=9, tau=0.5, od_max=6.9, bias=2, H=19, W=23, fx=30.0, fy=30.0, cx=11.0, cy=9.0,
            pose=POSE, near=2.0, dstep=0.05, K=64, sigma=0x1000000, coef=0x2000000, sigma_out=0x3000000, tvol=0x4000000, od=0x5000000, skip=0x6000000,
            grid=True, view=True)
# case -> (overrides, the entries it applies to: b shadow_bytes, h shadow, s seen, p prune_seen)
REFUSALS = {
    "NULL grid": (dict(grid=False), "hsp"),
    "res 0": (dict(res=(20, 0, 9)), "hsp"),
    "res 513": (dict(res=(513, 12, 9)), "hsp"),
    "NaN box": (dict(hi=(1.0, 1.0, NAN)), "hsp"),
    "lo above hi": (dict(lo=(1.0, -1.0, -1.0), hi=(-1.0, 1.0, 1.0)), "hsp"),
    "NULL view": (dict(view=False), "bhs"),
    "K not a multiple of 8": (dict(K=60), "bhs"),
    "K 0": (dict(K=0), "bhs"),
    "K negative": (dict(K=-8), "bhs"),
    "K over the maximum": (dict(K=65536 + 8), "bhs"),
    "H 0": (dict(H=0), "bhs"),
    "W 8193": (dict(W=8193), "bhs"),
    "fx 0": (dict(fx=0.0), "bhs"),
    "fy 0": (dict(fy=0.0), "bhs"),
    "fx NaN": (dict(fx=NAN), "bhs"),
    "cx infinite": (dict(cx=INF), "bhs"),
    "NaN pose": (dict(pose=POSE[:5] + (NAN,) + POSE[6:]), "bhs"),
    "infinite translation": (dict(pose=POSE[:11] + (INF,)), "bhs"),
    "negative depth_near": (dict(near=-0.5), "bhs"),
    "depth_near NaN": (dict(near=NAN), "bhs"),
    "depth_step 0": (dict(dstep=0.0), "bhs"),
    "depth_step negative": (dict(dstep=-0.05), "bhs"),
    "depth_step infinite": (dict(dstep=INF), "bhs"),
    "negative bias": (dict(bias=-1), "s"),
    "NaN od_max": (dict(od_max=NAN), "p"),
    "negative od_max": (dict(od_max=-1.0), "p"),
    "minus infinite od_max": (dict(od_max=-INF), "p"),
    "tau negative": (dict(tau=-0.5), "p"),
    "tau NaN": (dict(tau=NAN), "p"),
    "tau infinite": (dict(tau=INF), "p"),
    "B 2": (dict(B=2), "p"),
    "NULL sigma": (dict(sigma=None), "hp"),
    "NULL tvol": (dict(tvol=None), "hs"),
    "NULL od": (dict(od=None), "sp"),
    "NULL sigma_out": (dict(sigma_out=None), "p"),
    "NULL coef": (dict(coef=None), "p"),
    "misaligned tvol (16 bytes)": (dict(tvol=0x4000010), "hs"),
    "misaligned tvol (4 bytes)": (dict(tvol=0x4000004), "hs"),
    "sigma not 4-byte aligned": (dict(sigma=0x1000002), "hp"),
    "od not 4-byte aligned": (dict(od=0x5000002), "sp"),
    "coef not 16-byte aligned": (dict(coef=0x2000008), "p"),
    "tvol is sigma": (dict(tvol=0x1000000), "h"),
    "tvol ends inside sigma": (dict(tvol=0x1000000 - 19 * 23 * 64 * 4 + 32), "h"),
    "od is tvol": (dict(od=0x4000000), "s"),
    "od inside tvol": (dict(od=0x4000000 + 4 * 1000), "s"),
    "sigma_out is sigma_in": (dict(sigma_out=0x1000000), "p"),
    "sigma_out inside sigma_in": (dict(sigma_out=0x1000000 + 4 * 1000), "p"),
    "od is sigma_out": (dict(od=0x3000000), "p"),
    "od inside coef": (dict(od=0x2000000 + 4096), "p"),
}


def _call(mod, entry, a):
    L = mod.lib()
    g = C.byref(_grid(mod, a["lo"], a["hi"], a["res"])) if a["grid"] else None
    v = C.byref(mod.View(a["H"], a["W"], a["fx"], a["fy"], a["cx"], a["cy"], (C.c_float * 12)(*a["pose"]), a["near"], a["dstep"], a["K"])) if a["view"] else None
    if entry == "b":
        rc = EINVAL if L.mi_vox_shadow_bytes(v) == 0 else 0
    elif entry == "h":
        rc = L.mi_vox_shadow(g, a["sigma"], a["skip"], v, a["tvol"], None)
    elif entry == "s":
        rc = L.mi_vox_seen(g, v, a["tvol"], a["bias"], a["od"], None)
    else:
        rc = L.mi_vox_prune_seen(g, a["B"], a["tau"], a["od_max"], a["sigma"], a["od"], a["sigma_out"], a["coef"], None)
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
    (MI_VOX_EHIP) -- so every refusal above is owed to its one override.  The skip plane may be NULL, od_max infinite, bias and tau 0."""
    if torch.cuda.is_available():
        pytest.skip("made-up addresses must not reach a real device")
    assert _call(vox, "b", dict(GOOD))[0] == 0
    for entry in "hsp":
        for over in (dict(), dict(skip=None), dict(od_max=INF, tau=0.0), dict(bias=0), dict(B=1), dict(K=8, near=0.0), dict(K=65536, H=1, W=1)):
            rc, msg = _call(vox, entry, dict(GOOD, **over))
            assert rc == 2 and "HIP error" in msg, (entry, over, rc, msg)


# ---------------------------------------------------------------------------------------------------
# baked.py on the host
# ---------------------------------------------------------------------------------------------------
def test_views_read_their_poses_once_and_the_slices_cover_the_box(vox):
    from nerf_pytorch_paeng_amd import baked
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    K = [[30.0, 0.0, 11.0], [0.0, 25.0, 9.0], [0.0, 0.0, 1.0]]
    p34 = np.stack([SR.look_at((-4.0, 0.0, 0.0), (0.0, 0.0, 0.0)), SR.look_at((0.0, 0.5, 5.0), (0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)),
                    SR.look_at((-4.0, 0.0, 0.0), (-8.0, 0.0, 0.0))])
    p44 = np.concatenate([p34, np.broadcast_to(np.array([0, 0, 0, 1], f32), (3, 1, 4))], 1)
    a, b = baked.Views(19, 23, K, p34), baked.Views(19, 23, torch.tensor(K), torch.from_numpy(p44))
    assert len(a) == len(b) == 3 and a.poses.shape == (3, 3, 4) and a.poses.dtype == np.float32 and np.array_equal(a.poses, b.poses)
    assert (a.H, a.W, a.fx, a.fy, a.cx, a.cy) == (19, 23, 30.0, 25.0, 11.0, 9.0) == (b.H, b.W, b.fx, b.fy, b.cx, b.cy)
    for bad in (p34[0], np.zeros((2, 4, 3), f32)):
        with pytest.raises(MiNerfError, match="poses"):
            baked.Views(19, 23, K, bad)
    g = baked.RadianceGrid(-1.0, 1.0, 16, B=1)
    step = 0.5 * g.cell_edge()
    vs = g.view_slices(a)
    assert [C.sizeof(v) for v in vs] == [84] * 3 and all(v.slices % 8 == 0 and 8 <= v.slices for v in vs)
    assert all(v.depth_step == f32(step) for v in vs)
    assert vs[0].depth_near == 3.0 and (vs[0].slices - 8) * step <= 2.0 < vs[0].slices * step            # depths 3 .. 5 along the axis
    assert vs[2].depth_near == 0.0 and vs[2].slices == 8                                                    # the box lies behind that camera
    corners = np.array([[(-1.0, 1.0)[(e >> i) & 1] for i in range(3)] for e in range(8)])
    for v, pose in zip(vs[:2], p34[:2].astype(np.float64)):
        z = -((corners - pose[:, 3]) @ pose[:, :3])[:, 2]
        assert v.depth_near <= z.min() + 1e-6 and v.depth_near + v.slices * step > z.max()
    assert g.view_slices(a, step=0.25)[0].slices == 16                                                     # floor(2 / 0.25) + 1 = 9 slices, rounded up
    with pytest.raises(MiNerfError, match="slices"):
        g.view_slices(a, step=1e-6)
    with pytest.raises(MiNerfError, match="step"):
        g.view_slices(a, step=0.0)
    with pytest.raises(MiNerfError, match="holds nothing"):
        g.seen(a)
    g.allocate("cpu")
    with pytest.raises(MiNerfError, match="Views"):
        g.seen(p34)
    with pytest.raises(MiNerfError, match="HIP device"):
        g.seen(a)
    with pytest.raises(MiNerfError, match="od plane"):
        g.prune(0.0, seen=torch.zeros(3, 3, 3))
    with pytest.raises(MiNerfError, match="T_vis"):
        g.prune(0.0, seen=torch.zeros(g.points), T_vis=2.0)


# ---------------------------------------------------------------------------------------------------
# the restatement's own properties, in float64
# ---------------------------------------------------------------------------------------------------
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def _view(c2w, near, step, K, H=19, W=23, f=30.0):
    return SR.View(H, W, f, f, 0.5 * (W - 1), 0.5 * (H - 1), c2w, near, step, K)


def _length_before(view, t_end):
    """Per pixel (float64): the length of the ray's piece inside the box [-1, 1]^3 with parameter in [0, t_end]."""
    o, d, L = SR.pixel_rays(view, np.float64)
    d = np.stack(d, 1)
    with np.errstate(all="ignore"):
        ta, tb = (-1.0 - o) / d, (1.0 - o) / d
        inside = (o >= -1.0) & (o <= 1.0)
        a = np.where(d != 0, np.minimum(ta, tb), np.where(inside, -np.inf, np.inf)).max(1)
        b = np.where(d != 0, np.maximum(ta, tb), np.where(inside, np.inf, -np.inf)).min(1)
    return np.maximum(np.minimum(b, t_end) - np.maximum(a, 0.0), 0.0) * L, L


def test_restatement_uniform_box_is_density_times_length_to_within_one_slice():
    """sigma = s everywhere: od_k = s * (length of the ray inside the box before slice k).  The rule takes a slice whole or not at all by
    its midpoint, so the entry and the exit are each placed to within half a slice: one slice length together, times s."""
    s, res = float(f32(1.7)), (6, 5, 4)
    sigma = np.full((5, 6, 7), s, f32)
    for c2w, near, step, K in ((SR.look_at((-4.0, 0.3, 0.2), (0.0, 0.0, 0.0)), 2.5, 0.07, 56), (SR.look_at((2.0, 3.0, 2.5), (0.1, 0.0, -0.2)), 1.0, 0.11, 56),
                               (SR.look_at((0.2, 0.1, -0.3), (1.0, 0.5, 0.0)), 0.0, 0.05, 48)):          # the last one from inside the box
        view = _view(c2w, near, step, K)
        tvol = SR.shadow(LO, HI, res, sigma, view, np.float64).reshape(-1, K)
        assert not tvol[:, 0].any() and (np.diff(tvol, axis=1) >= 0).all() and tvol.max() > s
        worst = 0.0
        for k in range(K):
            want, L = _length_before(view, float(f32(near)) + k * float(f32(step)))
            worst = max(worst, float((np.abs(tvol[:, k] - s * want) / (s * float(f32(step)) * L)).max()))
        assert worst <= 1.0 + 1e-9, worst
        # float32 follows float64
        t32 = SR.shadow(LO, HI, res, sigma, view, np.float32)
        assert t32.dtype == np.float32 and 0 < np.abs(t32.reshape(-1, K) - tvol).max() <= 1e-5


def test_restatement_opaque_wall_hides_what_lies_behind_it_and_nothing_in_front():
    """A wall of lattice points (x index 4 of 9: the plane x = 0) of density s in an 8^3 grid, the camera on the -x axis looking along +x: a
    sample at ray parameter m lies at x = -4 + m, so the slices before a lattice point's own hold only samples in front of it.  od is
    exactly 0 at every point on the camera's side that the view looks at; behind the wall it is the integral of the tent through the
    wall, s * cell_edge / cos(angle) in full, at least half of that once the point's slice front has passed the wall's middle."""
    s, res, edge = 50.0, (8, 8, 8), 0.25
    sigma = np.zeros((9, 9, 9), f32)
    sigma[:, :, 4] = s
    view = _view(SR.look_at((-4.0, 0.0, 0.0), (0.0, 0.0, 0.0)), 3.0, 0.125, 24, H=33, W=33, f=45.0)
    tvol = SR.shadow(LO, HI, res, sigma, view, np.float64)
    assert tvol.max() >= s * edge * 0.99
    for bias, first_behind in ((0, 5), (2, 6)):
        od = SR.seen(LO, HI, res, view, tvol, bias, np.full((9, 9, 9), np.inf), np.float64)
        look = SR.looked_at(LO, HI, res, view, np.float64)[0]
        assert look.all() and np.isfinite(od).all()                                       # f = 45 at depth 3: the near face spans +-15 of the +-16 pixels
        assert not od[:, :, :4].any()                                                     # in front of the wall: exactly 0
        assert (od[:, :, first_behind:] >= s * edge / 2).all(), od[:, :, first_behind:].min()
    # a camera that looks away sees nothing, and a point outside the frustum stays +inf
    away = _view(SR.look_at((-4.0, 0.0, 0.0), (-8.0, 0.0, 0.0)), 0.0, 0.125, 8)
    od = SR.seen(LO, HI, res, away, SR.shadow(LO, HI, res, sigma, away, np.float64), 2, np.full((9, 9, 9), np.inf), np.float64)
    assert np.isinf(od).all()
    narrow = _view(SR.look_at((-4.0, 0.0, 0.0), (0.0, 0.0, 0.0)), 3.0, 0.125, 24, H=9, W=9, f=50.0)      # +-4 pixels of 50 at depth >= 3: |y| <= 0.27 at most
    od = SR.seen(LO, HI, res, narrow, SR.shadow(LO, HI, res, sigma, narrow, np.float64), 0, np.full((9, 9, 9), np.inf), np.float64)
    assert np.isinf(od[0, 0]).all() and np.isinf(od[:, 8]).all() and np.isfinite(od[4, 4]).all()
    # the minimum over views does not depend on their order, and a second view from behind uncovers the far side
    back = _view(SR.look_at((4.0, 0.0, 0.0), (0.0, 0.0, 0.0)), 3.0, 0.125, 24, H=33, W=33, f=45.0)
    ab, ba = SR.seen_all(LO, HI, res, sigma, [view, back], 0, np.float64), SR.seen_all(LO, HI, res, sigma, [back, view], 0, np.float64)
    assert np.array_equal(ab, ba) and not ab[:, :, :4].any() and not ab[:, :, 5:].any() and (ab[:, :, 4] <= s * edge).all()


def test_restatement_bias_shifts_the_slice_and_clamps_at_the_first():
    sigma = np.zeros((9, 9, 9), f32)
    sigma[:, :, 2:] = 3.0
    view = _view(SR.look_at((-4.0, 0.0, 0.0), (0.0, 0.0, 0.0)), 3.0, 0.125, 24, H=33, W=33, f=45.0)
    tvol = SR.shadow(LO, HI, (8, 8, 8), sigma, view, np.float32)
    look, fi, fj, k0 = SR.looked_at(LO, HI, (8, 8, 8), view, np.float32)
    start = np.full((9, 9, 9), np.inf, f32)
    prev = None
    for bias in (0, 2, 5, 100):
        od = SR.seen(LO, HI, (8, 8, 8), view, tvol, bias, start, np.float32)
        assert od.dtype == np.float32 and np.array_equal(od[k0 - bias < 0], np.zeros((k0 - bias < 0).sum(), f32))
        inner = look & (k0 - bias >= 0) & (k0 - bias < view.K)
        assert np.array_equal(od[inner], tvol[fj[inner], fi[inner], (k0 - bias)[inner]])
        assert prev is None or (od <= prev).all()                                         # a larger bias only ever uncovers
        prev = od
    assert not prev.any()                                                                  # bias 100: every slice clamps to the first
    # k >= K leaves the point alone
    short = _view(SR.look_at((-4.0, 0.0, 0.0), (0.0, 0.0, 0.0)), 3.0, 0.125, 8, H=33, W=33, f=45.0)
    od = SR.seen(LO, HI, (8, 8, 8), short, SR.shadow(LO, HI, (8, 8, 8), sigma, short, np.float32), 0, start, np.float32)
    assert np.isfinite(od[:, :, :4]).all() and np.isinf(od[:, :, 4:]).all()                # depth 3 + 8 * 0.125 = 4: x < 0


def test_restatement_prune_seen_with_an_infinite_od_max_is_prune():
    rng = np.random.default_rng(29)
    for P in ((4, 5, 6), (10, 13, 21), (3, 2, 66)):
        sigma = np.where(rng.uniform(size=P) < 0.05, rng.uniform(0.1, 3.0, P), 0.0).astype(f32)
        coef = rng.normal(0, 1, P + (16,)).astype(f32)
        od = np.where(rng.uniform(size=P) < 0.3, np.inf, rng.uniform(0.0, 12.0, P)).astype(f32)
        for tau in (0.0, 1.0):
            a, b = SR.prune_seen(sigma, coef, tau, math.inf, od), RR.prune(sigma, coef, tau)
            assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
            keep, full = SR.kept_seen_set(sigma, tau, 6.9, od), RR.kept_set(sigma, tau)
            assert not (keep & ~full).any() and 0 < keep.sum() < full.sum()
            seeds = (sigma > f32(tau)) & (od <= f32(6.9))
            assert np.array_equal(keep, RR.kept_set(seeds.astype(f32), 0.5))
            s, c = SR.prune_seen(sigma, coef, tau, 6.9, od)
            assert np.array_equal(s, np.where(keep, sigma, 0)) and not c[~keep].any() and np.array_equal(c[keep].view(np.uint32), coef[keep].view(np.uint32))
        bad = od.copy()
        bad[sigma > 0] = np.nan                                                           # a NaN od is no seed, whatever od_max
        assert not SR.kept_seen_set(sigma, 0.0, math.inf, bad).any()
        assert not SR.prune_seen(sigma, coef, 0.0, 0.0, np.full(P, 1e-30, f32))[0].any()   # od_max = 0 keeps only what is seen through nothing
