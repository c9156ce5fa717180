"""THE LATTICE REGULARISERS of include/mi_nerf_geo.h (libmi_nerf_geo.so, csrc/lattice_reg.hip) without a GPU: the comparator the GPU tests use
(tests/lattice_reg_restate.py) is held against central differences of its own value in float64; the library answers ABI 2; a C99 program
links against the new entries; every refusal answers MI_GEO_EINVAL with a message before any HIP call; the scratch size is 0 for a bad
shape and non-zero otherwise; and the Python surface refuses what it must."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import lattice_reg_restate as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def geo():
    """The library is built when the tree is fresh (a no-op when it is up to date)."""
    from nerf_pytorch_paeng_amd import _geo
    from nerf_pytorch_paeng_amd.build import build_geo_library
    build_geo_library()
    _geo.lib()
    return _geo


# ---------------------------------------------------------------------------------------------------
# 1. the comparator against itself: the analytic float64 gradient against central differences of the float64 value
# ---------------------------------------------------------------------------------------------------
# THE STEP.  h = 2^-16, a power of two far above the spacing of every input here (|x| < 32), so x +- h are exact.
# THE BAR, from the float64 error model of a central difference, h^2 |f'''| / 6 + eps64 |f| / h, term by term:
#   f'''   TV: one element enters four terms t = |(sqrt(eps), d)|, Euclidean norms of a vector that moves along u = (-1, -1, -1) in its own
#          term and along a unit vector in each of the three backward ones.  The third directional derivative of a Euclidean norm is
#          -3 (u.n)(|u|^2 - (u.n)^2) / |x|^2 with n = x / |x|: at most 3 |u|^3 / |x|^2 in size.  So |f'''| <= 3 (3 sqrt(3) + 3) / t_lo^2, t_lo
#          the smallest t of the input less the sqrt(3) 2 h by which a t can move under the step -- and t >= sqrt(eps) whatever the input.
#          SP: f''' = (32 s^3 - 48 s) / (1 + 2 s^2)^3; with s / (1 + 2 s^2)^3 <= 0.19 and s / (1 + 2 s^2) <= 2^-3/2 that is at most 11.
#   eps|f| the value is a sum of non-negative terms, each a handful of float64 operations (4 eps64 relative is the allowance for one), added
#          by math.fsum, which rounds the exact sum once: 5 eps64 sum|t| bounds the error of one evaluation, and a difference holds two.
# Both terms are bounds from eps and the inputs, fixed before any gradient is looked at.
H = 2.0 ** -16
EPS64 = 2.0 ** -53
TV_EPS = 1e-2              # t >= 0.1: the curvature term stays a bound one can meet at this h (the rule is the same for every eps > 0)


def _value_tv(v, C, mask):
    r = LR.tv(v, C, TV_EPS, mask=mask, dtype=np.float64)
    return r["value"]


def _pattern_mask(P):
    m = np.ones(LR.mask_shape(P), np.uint8)
    m[-1, 0, 0] = 0                                                  # one empty block beside full ones
    m[0, 0, -1] = 7                                                  # any non-zero byte counts
    return m


@pytest.mark.parametrize("P,C,masked", [((3, 4, 5), 1, False), ((3, 4, 5), 3, False), ((10, 3, 17), 1, True), ((10, 3, 17), 3, True)])
def test_tv_restatement_meets_central_differences_of_its_own_value_in_float64(P, C, masked):
    rng = np.random.default_rng(100 + 10 * P[0] + C)
    v = rng.normal(0.0, 1.0, P + (C,)).astype(np.float32).astype(np.float64)
    assert np.abs(v).max() < 32
    mask = _pattern_mask(P) if masked else None
    if masked:
        assert mask.shape == (2, 1, 2) and (mask == 0).sum() == 1
    an = LR.tv(v, C, TV_EPS, mask=mask, dtype=np.float64)
    n, total = an["count"], float(np.abs(an["terms"]).sum())
    t_lo = math.sqrt(TV_EPS) - 2.0 * math.sqrt(3.0) * H
    bar = H * H / 6.0 * 3.0 * (3.0 * math.sqrt(3.0) + 3.0) / t_lo ** 2 + 2.0 * 5.0 * EPS64 * total / (2.0 * H)
    assert bar <= 1e-6                                               # gradients here are up to ~3: the bar separates right from wrong
    cnt = LR.counted(P, mask)
    assert n == int(cnt.sum()) * C and (masked == (not cnt.all()))
    picks = [tuple(i) for i in np.argwhere(np.ones(P + (C,), bool))]
    if masked:
        picks = [picks[i] for i in rng.choice(len(picks), 120, replace=False)]
        # ... and every point around the empty block's faces, where own or a backward term is absent
        picks += [(8, y, x, c) for y in range(3) for x in (7, 8) for c in range(C)] + [(7, 1, 3, 0), (9, 2, 0, C - 1), (9, 2, 8, 0)]
    worst = largest = 0.0
    for at in picks:
        up, dn = v.copy(), v.copy()
        up[at] += H
        dn[at] -= H
        fd = (_value_tv(up, C, mask) - _value_tv(dn, C, mask)) / (2.0 * H)
        got = float(an["g"][at])
        worst, largest = max(worst, abs(fd - got)), max(largest, abs(got))
        assert abs(fd - got) <= bar, (at, fd, got, bar)
        if not an["written"][at[:3]]:
            assert got == 0.0 and fd == 0.0
    print(f"\n[lattice TV restatement vs central differences {P} C={C} mask={masked}] worst |diff| {worst:.3e}, bar {bar:.3e}, largest gradient {largest:.3e}", end="")
    assert largest >= 0.5
    if masked:
        assert not an["written"][9, 0, 0] and an["written"][8, 0, 0] and not cnt[8, 0, 0]      # written through the backward term alone
        assert not an["terms"][8:, :, :8].any()


@pytest.mark.parametrize("P,masked", [((3, 4, 5), False), ((10, 3, 17), True)])
def test_sparsity_restatement_meets_central_differences_of_its_own_value_in_float64(P, masked):
    rng = np.random.default_rng(7 + P[0])
    s = np.abs(rng.normal(0.0, 1.0, P)).astype(np.float32).astype(np.float64)
    s.ravel()[::7] = 0.0
    mask = _pattern_mask(P) if masked else None
    an = LR.sparsity(s, mask=mask, dtype=np.float64)
    total = float(np.abs(an["terms"]).sum())
    bar = H * H / 6.0 * 11.0 + 2.0 * 5.0 * EPS64 * total / (2.0 * H)
    assert bar <= 1e-6
    cnt = LR.counted(P, mask)
    for at in (tuple(i) for i in np.argwhere(np.ones(P, bool))):
        up, dn = s.copy(), s.copy()
        up[at] += H
        dn[at] -= H
        fd = (LR.sparsity(up, mask=mask, dtype=np.float64)["value"] - LR.sparsity(dn, mask=mask, dtype=np.float64)["value"]) / (2.0 * H)
        got = float(an["g"][at]) if cnt[at] else 0.0
        assert abs(fd - got) <= bar, (at, fd, got, bar)
    # the point of the prior (the header's figures): it peaks near sigma = 0.7 and has died off at a solid's density
    g = LR.sparsity(np.array([[[0.70710678, 4096.0], [0.0, 0.0]], [[0.0, 0.0], [0.0, 0.0]]], np.float32))["g"]
    assert abs(float(g[0, 0, 0]) - math.sqrt(2.0)) < 1e-6 and 4.8e-4 < float(g[0, 0, 1]) < 5.0e-4


def test_the_float32_restatement_follows_the_float64_one():
    rng = np.random.default_rng(5)
    v = rng.normal(0.0, 1.0, (10, 3, 17, 4)).astype(np.float32)
    d0 = rng.normal(0.0, 1.0, v.shape).astype(np.float32)
    mask = _pattern_mask((10, 3, 17))
    a = LR.tv(v, 3, 1e-8, mask=mask, scale=0.25, d_v=d0, dtype=np.float64)
    b = LR.tv(v, 3, 1e-8, mask=mask, scale=0.25, d_v=d0, dtype=np.float32)
    assert b["g"].dtype == np.float32 and b["d"].dtype == np.float32 and b["terms"].dtype == np.float32
    assert np.abs(b["g"] - a["g"]).max() < 1e-5 and np.abs(b["d"] - a["d"]).max() < 1e-5
    assert np.array_equal(b["d"][..., 3], d0[..., 3])                                       # the padding is not touched
    assert np.array_equal(b["d"][~b["written"]], d0[~b["written"]]) and (~b["written"]).any()
    zeros = LR.tv(v, 3, 1e-8, mask=0 * mask, scale=0.25, d_v=d0)
    assert np.array_equal(zeros["d"], d0) and zeros["value"] == 0.0 and zeros["count"] == 0
    ones = LR.tv(v, 3, 1e-8, mask=1 + 0 * mask, scale=0.25, d_v=d0)
    none = LR.tv(v, 3, 1e-8, scale=0.25, d_v=d0)
    assert np.array_equal(ones["d"], none["d"]) and ones["value"] == none["value"]


# ---------------------------------------------------------------------------------------------------
# 2, 3. ABI, C99 consumer
# ---------------------------------------------------------------------------------------------------
def test_the_library_answers_abi_2_and_the_new_source_is_in_the_geo_record(geo):
    from nerf_pytorch_paeng_amd import build
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_geo.h")).read()
    assert geo.lib().mi_geo_abi_version() == geo.ABI_VERSION == 2 == int(re.search(r"#define MI_GEO_ABI_VERSION (\d+)", hdr).group(1))
    assert geo.LATTICE_MAX_POINTS == 513 == int(re.search(r"#define MI_GEO_LATTICE_MAX_POINTS (\d+)", hdr).group(1))
    assert "THE LATTICE REGULARISERS" in hdr and "include/mi_nerf_vox.h" in hdr
    new = {"mi_geo_lattice_scratch_bytes", "mi_geo_lattice_tv", "mi_geo_lattice_sparsity"}
    assert new <= set(geo.SIGNATURES) and {n for n in geo.SIGNATURES if "lattice" in n} == new
    assert build.LIBRARIES["geo"] == (["geo.hip", "lattice_reg.hip"], [], False)
    assert "-ffp-contract=off" in build.FLAGS and "lattice_reg.hip" not in build.FILE_FLAGS
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [n for n in sorted(new) if n not in doc] == []


def test_the_new_source_holds_no_preprocessor_conditional_no_ablation_macro_and_no_inline_assembly():
    src = open(os.path.join(ROOT, "nerf_pytorch_paeng_amd", "csrc", "lattice_reg.hip")).read()
    assert not re.findall(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b", src, re.M) and "MN_" not in src
    assert not re.findall(r"\basm\b", src) and not re.findall(r"atomic\w*\s*\(", src)
    assert '#include "../../include/mi_nerf_geo.h"' in src and len(re.findall(r"#\s*include\s*\"[^\"]*mi_nerf", src)) == 1


def test_header_compiles_as_c99_and_the_new_entries_link_and_answer(tmp_path, geo):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not found")
    pkg = os.path.dirname(geo.LIB_PATH)
    exe = str(tmp_path / "lattice_reg_consumer")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "lattice_reg_consumer.c"), "-L", pkg, "-lmi_nerf_geo", f"-Wl,-rpath,{pkg}", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "lattice_reg c_abi consumer ok: ABI 2" in run.stdout


# ---------------------------------------------------------------------------------------------------
# 4. refusals: made-up addresses that are never dereferenced -- every call below is refused before the first HIP call (a call that got as
# far as one would answer MI_GEO_EHIP, "HIP error ... no ROCm-capable device", on a machine without a GPU)
# ---------------------------------------------------------------------------------------------------
GOOD = dict(P=(10, 17, 9), R=4, C=3, v=0x100000, mask=0x200000, eps=1e-8, scale=0.5, d_v=0x300000, value=0x400000, scratch=0x500000, bytes=None)
REFUSALS = {
    "NULL P": dict(P=None),
    "P_z 1": dict(P=(1, 17, 9)),
    "P_y 0": dict(P=(10, 0, 9)),
    "P_x 514": dict(P=(10, 17, 514)),
    "P negative": dict(P=(10, -3, 9)),
    "R 2": dict(R=2),
    "R 8": dict(R=8),
    "R 0": dict(R=0),
    "R 64": dict(R=64),
    "C 0": dict(C=0),
    "C above R": dict(C=5),
    "eps 0": dict(eps=0.0),
    "eps negative": dict(eps=-1e-8),
    "eps NaN": dict(eps=NAN),
    "eps infinite": dict(eps=INF),
    "scale NaN": dict(scale=NAN),
    "scale infinite": dict(scale=-INF),
    "NULL v": dict(v=None),
    "v not 16-byte aligned": dict(v=0x100004),
    "d_v not 16-byte aligned": dict(d_v=0x300008),
    "plane not 4-byte aligned": dict(R=1, C=1, v=0x100002),
    "plane gradient not 4-byte aligned": dict(R=1, C=1, d_v=0x300001),
    "value not 8-byte aligned": dict(value=0x400004),
    "scratch not 8-byte aligned": dict(scratch=0x500004),
    "scratch too small": dict(bytes=-8),
    "NULL scratch with a value": dict(scratch=None),
    "d_v is v": dict(d_v=0x100000),
    "d_v overlaps the end of v": dict(d_v=0x100000 + 4 * (10 * 17 * 9 * 4 - 4)),
    "v overlaps the end of d_v": dict(v=0x300000 + 4 * (10 * 17 * 9 * 4 - 4)),
}
ONLY_TV = ("R ", "C ", "eps ", "v not 16", "d_v not 16")


def _p3(P):
    return None if P is None else (C.c_int32 * 3)(*P)


def _calls(L, a):
    """(name, rc, message) of the TV entry and, where the case applies to a plane, of the sparsity entry."""
    out = []
    nbytes = a["bytes"]                                             # None: what the shape needs; negative: that many bytes short of it
    if nbytes is None or nbytes < 0:
        nbytes = int(L.mi_geo_lattice_scratch_bytes(_p3(a["P"]), a["R"], a["C"])) + (nbytes or 0)
    rc = L.mi_geo_lattice_tv(_p3(a["P"]), a["R"], a["C"], a["v"], a["mask"], a["eps"], a["scale"], a["d_v"], a["value"], a["scratch"], nbytes, None)
    out.append(("mi_geo_lattice_tv", rc, L.mi_geo_last_error().decode()))
    if a["R"] == 1:
        rc = L.mi_geo_lattice_sparsity(_p3(a["P"]), a["v"], a["mask"], a["scale"], a["d_v"], a["value"], a["scratch"], nbytes, None)
        out.append(("mi_geo_lattice_sparsity", rc, L.mi_geo_last_error().decode()))
    return out


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_answer_einval_with_a_message_before_any_hip_call(geo, case):
    over = REFUSALS[case]
    runs = [dict(GOOD, **over)]
    if not case.startswith(ONLY_TV):                                  # the same refusal on the plane, through both entries
        plane = dict(dict(GOOD, R=1, C=1), **over)
        if "overlaps" in case:
            n = 4 * (10 * 17 * 9 - 1)
            plane.update({k: (0x100000 if k == "d_v" else 0x300000) + n for k in over})
        runs.append(plane)
    seen = 0
    for a in runs:
        for name, rc, msg in _calls(geo.lib(), a):
            assert rc == EINVAL, (case, name, rc, msg)
            assert msg.startswith(name) and "HIP error" not in msg, (case, name, msg)
            seen += 1
    assert seen >= (1 if case.startswith(ONLY_TV) else 3)


def test_the_good_arguments_of_the_refusal_table_are_refused_by_nothing(geo):
    """The table's base case gets as far as its launch, which fails here for want of a device (MI_GEO_EHIP) -- so every refusal above is
    owed to its one override.  With no output asked for nothing is launched, and the arguments are still checked."""
    L = geo.lib()
    quiet = dict(GOOD, d_v=None, value=None, scratch=None, bytes=0)
    for a in (quiet, dict(quiet, mask=None), dict(quiet, R=1, C=1), dict(quiet, R=32, C=27), dict(quiet, R=16, C=12), dict(quiet, P=(2, 2, 2)),
              dict(quiet, P=(513, 513, 513))):
        for name, rc, msg in _calls(L, a):
            assert rc == 0, (a, name, rc, msg)
    for name, rc, msg in _calls(L, dict(quiet, eps=0.0)) + _calls(L, dict(quiet, R=1, C=1, v=None)):
        assert rc == EINVAL and msg.startswith(name), (name, rc, msg)
    if torch.cuda.is_available():
        pytest.skip("made-up addresses must not reach a real device")
    for over in (dict(), dict(mask=None), dict(value=None, scratch=None, bytes=0), dict(d_v=None), dict(R=1, C=1), dict(scale=0.0)):
        for name, rc, msg in _calls(L, dict(GOOD, **over)):
            assert rc == 2 and "HIP error" in msg, (over, name, rc, msg)


# ---------------------------------------------------------------------------------------------------
# 5. scratch bytes
# ---------------------------------------------------------------------------------------------------
def test_scratch_bytes_is_zero_for_bad_arguments_and_not_otherwise(geo):
    f = geo.lib().mi_geo_lattice_scratch_bytes
    for P in ((2, 2, 2), (3, 2, 9), (10, 17, 9), (25, 25, 25), (257, 257, 257), (513, 513, 513)):
        for R, Cn in ((1, 1), (4, 3), (16, 12), (32, 27), (32, 1), (4, 4)):
            n = int(f(_p3(P), R, Cn))
            blocks = math.prod(LR.mask_shape(P))
            assert n > 0 and n % 8 == 0 and n <= 8 * blocks, (P, R, Cn, n)
            assert n == int(f(_p3(P), R, 1))                          # the counted channels do not change the launch
    assert int(f(_p3((257, 257, 257)), 32, 27)) == 8 * 32 ** 3        # one workgroup per block of the mask at R = 32
    for P, R, Cn in ((None, 4, 3), ((1, 2, 2), 4, 3), ((2, 2, 514), 4, 3), ((2, 0, 2), 1, 1), ((2, -2, 2), 1, 1), ((9, 9, 9), 2, 1), ((9, 9, 9), 8, 3),
                     ((9, 9, 9), 0, 0), ((9, 9, 9), 4, 0), ((9, 9, 9), 4, 5), ((9, 9, 9), 1, 2), ((9, 9, 9), 32, 33), ((9, 9, 9), -4, 1)):
        assert int(f(_p3(P), R, Cn)) == 0, (P, R, Cn)


# ---------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------
def test_wrappers_refuse_sparse_grids_host_tensors_and_bad_weights():
    from nerf_pytorch_paeng_amd import baked, baked_train
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    host = baked.RadianceGrid(-1.0, 1.0, (5, 4, 3), B=4).allocate("cpu")
    for call in (lambda: baked_train.lattice_tv(host), lambda: baked_train.lattice_tv(host, "coef", scale=1.0),
                 lambda: baked_train.lattice_sparsity(host, mask=True)):
        with pytest.raises(MiNerfError, match="HIP device"):          # no GPU: loudly, no fallback
            call()
    with pytest.raises(MiNerfError, match="compact"):
        baked_train.lattice_tv(baked.SparseRadianceGrid(-1.0, 1.0, (5, 4, 3), B=4).allocate("cpu"))
    with pytest.raises(MiNerfError, match="RadianceGrid expected"):
        baked_train.lattice_sparsity(torch.zeros(4, 4, 4))
    with pytest.raises(MiNerfError, match="holds nothing"):
        baked_train.lattice_tv(baked.RadianceGrid(-1.0, 1.0, (5, 4, 3), B=4))
    rays, target = torch.zeros(8, 6), torch.zeros(8, 3)
    for kw in (dict(tv_sigma=-1.0), dict(tv_coef=NAN), dict(sparsity=INF), dict(tv_sigma="1")):
        with pytest.raises(MiNerfError, match="tv_sigma="):
            baked_train.finetune(host, rays, target, steps=1, **kw)
