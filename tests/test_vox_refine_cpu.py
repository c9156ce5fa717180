"""mi_vox_resample and mi_vox_prune of include/mi_nerf_vox.h (THE RESAMPLING RULE, THE PRUNING RULE) without a GPU: the two entries are
declared, bound and exported within ABI 2; a C99 program links against them; every refusal answers MI_VOX_EINVAL with a message before
any HIP call; and the restatement the GPU tests compare with (tests/vox_refine_restate.py) has the properties the header states -- exact on
an exactly representable case, the identical field after an integer refinement (the renders agree), pruning by the active stencil."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import vox_refine_restate as RR
from tests import vox_restate as VR
from tests import vox_sparse_restate as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
f32 = np.float32


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
def test_the_two_entries_are_declared_bound_and_exported_within_abi_2(vox):
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_vox.h")).read()
    declared = set(re.findall(r"\b(mi_vox_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", vox.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in ("mi_vox_resample", "mi_vox_prune"):
        assert name in declared and name in vox.SIGNATURES and name in exported, name
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read(), name
    assert vox.ABI_VERSION == 2 == vox.lib().mi_vox_abi_version() and "#define MI_VOX_ABI_VERSION 2" in hdr
    assert "THE RESAMPLING RULE" in hdr and "THE PRUNING RULE" in hdr and "edge extension" in hdr
    assert len(vox.SIGNATURES["mi_vox_resample"][1]) == 8 and len(vox.SIGNATURES["mi_vox_prune"][1]) == 7
    assert vox.SIGNATURES["mi_vox_prune"][1][2] is C.c_float


def test_header_compiles_as_c99_and_the_new_entries_link_and_answer(tmp_path, vox):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not found")
    pkg = os.path.dirname(vox.LIB_PATH)
    exe = str(tmp_path / "vox_refine_consumer")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "vox_refine_consumer.c"), "-L", pkg, "-lmi_nerf_vox", f"-Wl,-rpath,{pkg}", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"vox refine c_abi consumer ok: ABI {vox.ABI_VERSION}" in run.stdout


# ---------------------------------------------------------------------------------------------------
# refusals: made-up addresses that are never dereferenced -- every call below is refused before the first HIP call.  The addresses lie
# 16 MiB apart: the largest array of the base case (a 21 x 13 x 10 lattice of 128-byte records, and the 41 x 25 x 19 one) stays below that.
# ---------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
GOOD = dict(lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), res=(20, 12, 9), lo_d=(-1.0, -1.0, -1.0), hi_d=(1.0, 1.0, 1.0), res_d=(40, 24, 18), B=9, tau=0.5,
            sigma=0x1000000, coef=0x2000000, sigma_d=0x3000000, coef_d=0x4000000, grid=True, grid_d=True)
# case -> (overrides, the entries it applies to: s resample, p prune).  For prune, sigma_d is sigma_out.
REFUSALS = {
    "NULL grid": (dict(grid=False), "sp"),
    "NULL destination grid": (dict(grid_d=False), "s"),
    "res 0": (dict(res=(20, 0, 9)), "sp"),
    "res 513": (dict(res=(513, 12, 9)), "sp"),
    "res negative": (dict(res=(20, 12, -1)), "sp"),
    "lo above hi": (dict(lo=(1.0, -1.0, -1.0), hi=(-1.0, 1.0, 1.0)), "sp"),
    "empty axis": (dict(lo=(-1.0, 1.0, -1.0)), "sp"),
    "NaN box": (dict(hi=(1.0, 1.0, NAN)), "sp"),
    "infinite box": (dict(hi=(INF, 1.0, 1.0)), "sp"),
    "destination res 0": (dict(res_d=(0, 24, 18)), "s"),
    "destination res 513": (dict(res_d=(40, 24, 513)), "s"),
    "destination lo above hi": (dict(lo_d=(-1.0, 2.0, -1.0)), "s"),
    "destination NaN box": (dict(lo_d=(NAN, -1.0, -1.0)), "s"),
    "destination infinite box": (dict(hi_d=(1.0, INF, 1.0)), "s"),
    "B 2": (dict(B=2), "sp"),
    "B 0": (dict(B=0), "sp"),
    "B 16": (dict(B=16), "sp"),
    "NULL sigma": (dict(sigma=None), "sp"),
    "NULL coef": (dict(coef=None), "sp"),
    "NULL destination sigma": (dict(sigma_d=None), "sp"),
    "NULL destination coef": (dict(coef_d=None), "s"),
    "sigma not 4-byte aligned": (dict(sigma=0x1000002), "sp"),
    "coef not 16-byte aligned": (dict(coef=0x2000008), "sp"),
    "destination sigma not 4-byte aligned": (dict(sigma_d=0x3000001), "sp"),
    "destination coef not 16-byte aligned": (dict(coef_d=0x4000004), "s"),
    "destination sigma is the source sigma": (dict(sigma_d=0x1000000), "sp"),
    "destination coef is the source coef": (dict(coef_d=0x2000000), "s"),
    "destination sigma is the source coef": (dict(sigma_d=0x2000000), "s"),
    "destination coef is the source sigma": (dict(coef_d=0x1000000), "s"),
    "destination sigma inside the source sigma": (dict(sigma_d=0x1000000 + 4 * 1000), "sp"),
    "tau negative": (dict(tau=-0.5), "p"),
    "tau NaN": (dict(tau=NAN), "p"),
    "tau infinite": (dict(tau=INF), "p"),
    "tau minus infinity": (dict(tau=-INF), "p"),
}


def _call(mod, entry, a):
    L = mod.lib()
    g = C.byref(_grid(mod, a["lo"], a["hi"], a["res"])) if a["grid"] else None
    if entry == "s":
        gd = C.byref(_grid(mod, a["lo_d"], a["hi_d"], a["res_d"])) if a["grid_d"] else None
        rc = L.mi_vox_resample(g, gd, a["B"], a["sigma"], a["coef"], a["sigma_d"], a["coef_d"], None)
    else:
        rc = L.mi_vox_prune(g, a["B"], a["tau"], a["sigma"], a["sigma_d"], a["coef"], None)
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
    (MI_VOX_EHIP) -- so every refusal above is owed to its one override."""
    if torch.cuda.is_available():
        pytest.skip("made-up addresses must not reach a real device")
    for entry in "sp":
        for over in (dict(), dict(B=1), dict(B=4), dict(tau=0.0), dict(res_d=(7, 512, 1), lo_d=(-3.0, 0.0, 0.5), hi_d=(-2.0, 0.5, 7.0))):
            rc, msg = _call(vox, entry, dict(GOOD, **over))
            assert rc == 2 and "HIP error" in msg, (entry, over, rc, msg)


# ---------------------------------------------------------------------------------------------------
# the restatement's own properties
# ---------------------------------------------------------------------------------------------------
def test_restatement_exact_case_nodes_midpoints_and_padding():
    """Box [0, 8]^3, res 4 -> 8, small integers: steps 2 and 1, inv 0.5, fractions 0 and 0.5, weights in eighths -- all exact in fp32."""
    rng = np.random.default_rng(25)
    for B in (1, 4, 9):
        R = VR.record_floats(B)
        sigma = rng.integers(0, 16, (5, 5, 5)).astype(f32)
        coef = np.full((5, 5, 5, R), np.nan, f32)                                          # poisoned padding
        coef[..., :3 * B] = rng.integers(-8, 9, (5, 5, 5, 3 * B)).astype(f32)
        for dtype in (np.float32, np.float64):
            s, c = RR.resample((0, 0, 0), (8, 8, 8), (4, 4, 4), (0, 0, 0), (8, 8, 8), (8, 8, 8), B, sigma, coef, dtype)
            assert s.dtype == dtype and c.dtype == dtype and s.shape == (9, 9, 9) and c.shape == (9, 9, 9, R)
            # fine points on coarse nodes: the source bit for bit, the last plane included
            assert np.array_equal(s[::2, ::2, ::2].astype(f32).view(np.uint32), sigma.view(np.uint32))
            assert np.array_equal(c[::2, ::2, ::2, :3 * B].astype(f32).view(np.uint32), coef[..., :3 * B].view(np.uint32))
            assert np.array_equal(s[8, 8, 8], sigma[4, 4, 4]) and np.array_equal(s[8, ::2, 8], sigma[4, :, 4])
            # midpoints: exact means of 2, 4 and 8 nodes
            assert np.array_equal(s[::2, ::2, 1::2], (sigma[:, :, :-1] + sigma[:, :, 1:]) / 2)
            assert np.array_equal(s[1::2, ::2, ::2], (sigma[:-1] + sigma[1:]) / 2)
            assert np.array_equal(s[1::2, 1::2, ::2], (sigma[:-1, :-1] + sigma[1:, :-1] + sigma[:-1, 1:] + sigma[1:, 1:]) / 4)
            cube = sum(sigma[dz:4 + dz, dy:4 + dy, dx:4 + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)) / 8
            assert np.array_equal(s[1::2, 1::2, 1::2], cube)
            kc = coef[..., :3 * B]
            assert np.array_equal(c[::2, 1::2, ::2, :3 * B], (kc[:, :-1] + kc[:, 1:]) / 2)
            # padding zero though the source's is poisoned, and nothing of it leaked
            assert not c[..., 3 * B:].any() and np.isfinite(c).all()
    # float32 and float64 agree exactly here
    a, b = (RR.resample((0, 0, 0), (8, 8, 8), (4, 4, 4), (0, 0, 0), (8, 8, 8), (8, 8, 8), 9, sigma, coef, d) for d in (np.float32, np.float64))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_restatement_edge_extension_and_crop():
    """A destination point outside the source box takes the value at the nearest face; a destination box inside the source crops."""
    rng = np.random.default_rng(26)
    sigma = rng.integers(0, 9, (4, 5, 6)).astype(f32)                                      # res (5, 4, 3), box [0, 5] x [0, 4] x [0, 3]: unit cells
    coef = rng.integers(-4, 5, (4, 5, 6, 4)).astype(f32)
    s, c = RR.resample((0, 0, 0), (5, 4, 3), (5, 4, 3), (-2, -1, 1), (7, 6, 2), (9, 7, 1), 1, sigma, coef, np.float32)
    assert s.shape == (2, 8, 10)
    xs, ys, zs = np.clip(np.arange(-2, 8), 0, 5), np.clip(np.arange(-1, 7), 0, 4), np.array([1, 2])
    assert np.array_equal(s, sigma[np.ix_(zs, ys, xs)]) and np.array_equal(c[..., :3], coef[np.ix_(zs, ys, xs)][..., :3])
    s, c = RR.resample((0, 0, 0), (5, 4, 3), (5, 4, 3), (1, 1, 1), (3, 2, 2), (2, 1, 1), 1, sigma, coef, np.float32)
    assert np.array_equal(s, sigma[1:3, 1:3, 1:4]) and np.array_equal(c[..., :3], coef[1:3, 1:3, 1:4, :3])


def test_restatement_refining_does_not_change_the_picture():
    """Trilinear interpolation reproduces every function of span{1, x, y, z, xy, xz, yz, xyz}, so on the same box an integer refinement
    represents the identical field: vox_restate.render in float64 gives the same picture from a 6^3 grid and from its float64 resample to
    12^3 and 18^3 -- at the SAME explicit step (the default follows the cell edge and would differ).

    vox_restate.render takes its arrays as fp32 values.  The data are therefore multiples of 27 / 2^k: halves and thirds of them, and
    products of three such weights, are short dyadic numbers, so the refined grids are fp32 values themselves and passing them on loses
    nothing beyond 1e-13 (the float64 resample, whose thirds are rounded, lies that close to those values).  What is left is float64 rounding in a
    few hundred samples per ray of order 1: far below 1e-9, which in turn is far below any change of the field."""
    rng = np.random.default_rng(27)
    B, lo, hi = 9, (-1.0, -0.8, -1.1), (1.0, 0.9, 1.0)
    sigma = (27.0 / 32.0 * rng.integers(0, 13, (7, 7, 7))).astype(f32)                     # densities 0 .. 10.1
    sigma[rng.uniform(size=sigma.shape) < 0.3] = 0.0
    coef = np.zeros((7, 7, 7, 32), f32)
    coef[..., :27] = 27.0 / 1024.0 * rng.integers(-24, 25, (7, 7, 7, 27))                  # +- 0.63
    coef[..., :3] += f32(27.0 / 1024.0 * 67)                                               # colours around 0.5 (0.5 / Y_0 = 1.77)
    rays = RR.rays_into_box(lo, hi, 96, 5)
    step = 0.11
    base = VR.render(lo, hi, (6, 6, 6), B, sigma, coef, rays, step, 0.3, 3.2, dtype=np.float64)
    assert (base["acc"] > 0.05).sum() > 40 and (base["acc"] < 0.999).sum() > 20
    for k in (2, 3):
        s, c = RR.resample(lo, hi, (6, 6, 6), lo, hi, (6 * k,) * 3, B, sigma, coef, np.float64)
        assert np.abs(s.astype(f32) - s).max() <= 1e-13 and np.abs(c.astype(f32) - c).max() <= 1e-13      # fp32 values, as said above
        assert np.abs(s[::k, ::k, ::k] - sigma).max() <= 1e-13                                                # a fine point on a coarse node
        fine = VR.render(lo, hi, (6 * k,) * 3, B, s, c, rays, step, 0.3, 3.2, dtype=np.float64)
        for name in ("rgb", "acc", "depth", "disp"):
            d = float(np.abs(fine[name] - base[name]).max())
            assert d <= 1e-9, (k, name, d)
        assert np.array_equal(fine["samples"], base["samples"])


def test_restatement_pruning_is_the_active_stencil_with_a_threshold():
    rng = np.random.default_rng(28)
    for P in ((4, 5, 6), (10, 13, 21), (3, 2, 66)):
        sigma = np.where(rng.uniform(size=P) < 0.02, rng.uniform(0.1, 3.0, P), 0.0).astype(f32)
        sigma[-1, -1, -1] = 1e-30                                                          # one dense point in the last corner: clipping
        coef = rng.normal(0, 1, P + (16,)).astype(f32)                                     # padding included: a kept record keeps every bit
        s, c = RR.prune(sigma, coef, 0.0)
        act = SR.active_set(sigma)
        assert np.array_equal(RR.kept_set(sigma, 0.0), act) and 0 < act.sum() < act.size
        assert np.array_equal(s.view(np.uint32), sigma.view(np.uint32))                    # tau = 0 keeps sigma: a point with sigma > 0 is active
        assert not c[~act].any() and np.array_equal(c[act].view(np.uint32), coef[act].view(np.uint32)) and coef[~act].any()
        mid = 1.0
        s, c = RR.prune(sigma, coef, mid)
        keep = RR.kept_set(sigma, mid)
        assert keep.sum() < act.sum() and not (keep & ~act).any()
        assert np.array_equal(s, np.where(keep, sigma, 0)) and (s[(sigma > mid)] == sigma[sigma > mid]).all() and not c[~keep].any()
        for tau in (float(sigma.max()), 2.0 * float(sigma.max())):
            s, c = RR.prune(sigma, coef, tau)
            assert not s.any() and not c.any()
    # the invariant the backward pass relies on: afterwards the records of inactive points (under the new sigma) are zero
    s, c = RR.prune(sigma, coef, 1.0)
    assert not c[~SR.active_set(s)].any()
