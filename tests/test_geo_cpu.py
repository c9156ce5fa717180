"""libmi_nerf_geo.so / include/mi_nerf_geo.h without a GPU: the header is C99 on its own and a C program links against the library; the header,
the ctypes table (nerf_pytorch_paeng_amd/_geo.py) and the library's dynamic symbols name the same entries; the library exports nothing of the
others and libmi_nerf.so is what it was (exactly the names of _lib.SIGNATURES); every refusal answers MI_GEO_EINVAL with a message before any
HIP call; ``opts.geometry`` refuses what it must.

``restate`` (torch, written from THE DISTORTION RULE of the header as its O(S^2) definition on oracle.restate.post_process, not from the kernel)
is what the GPU tests compare with, through autograd; ``scan_forms`` states the header's closed forms, and the two agree to 1e-12 in float64."""
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import pytest
import torch

from oracle import restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------
# restatement (from include/mi_nerf_geo.h)
# ---------------------------------------------------------------------------------------------------
def intervals(z, near, far):
    """t, delta, m of THE DISTORTION RULE for depths z [n,S] (any dtype)."""
    t = (z - near) / (far - near)
    delta = torch.cat([t[:, 1:] - t[:, :-1], torch.zeros_like(t[:, :1])], -1)
    return t, delta, t + delta / 2


def distortion_definition(w, z, near, far):
    """sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 delta_i, per ray: the O(S^2) definition."""
    _, delta, m = intervals(z, near, far)
    pair = (w[:, :, None] * w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum((1, 2))
    return pair + (w * w * delta).sum(-1) / 3.0


def scan_forms(w, z, near, far):
    """(qd [n,S], distortion [n]) by the header's closed forms: exclusive prefix / suffix sums of w and w m."""
    _, delta, m = intervals(z, near, far)
    wm = w * m
    W_lt, M_lt = torch.cumsum(w, -1) - w, torch.cumsum(wm, -1) - wm
    W_gt, M_gt = w.sum(-1, keepdim=True) - W_lt - w, wm.sum(-1, keepdim=True) - M_lt - wm
    pt = m * (W_lt - W_gt) - (M_lt - M_gt)
    return 2.0 * pt + (2.0 / 3.0) * w * delta, (w * pt).sum(-1) + (w * w * delta).sum(-1) / 3.0


def restate(raw, z, d, near, far):
    """(rgb, acc, weights, depth, distortion) in the dtype of the inputs: oracle.restate.post_process plus the definition."""
    rgb, _, acc, w, depth = R.post_process(raw, z, d)
    if z.shape[1] == 1:                                             # the reference's slice of an empty distance tensor leaves no sample: w is [n,0]
        w = raw[..., 3] * 0.0
    return rgb, acc, w, depth, distortion_definition(w, z, near, far)


def composite_case(n, S, seed, hard=False):
    """raw, z (ascending), rays: the inputs of tests/test_gpu_train.py's compositing cases."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(n, S, 4, generator=g)
    raw[..., 3] = raw[..., 3] * (30.0 if hard else 3.0)             # hard: saturated alphas (u_i -> 1e-10) and many relu-dead samples
    z = torch.sort(2.0 + 4.0 * torch.rand(n, S, generator=g), -1).values
    d = torch.randn(n, 3, generator=g)
    o = torch.randn(n, 3, generator=g)
    return raw, z, torch.cat([o, d], -1)


def test_scan_forms_equal_autograd_of_the_definition_in_float64():
    for n, S, hard in ((9, 70, False), (5, 7, False), (4, 130, True)):
        raw, z, rays = composite_case(n, S, 7 + S, hard)
        raw, z, d = raw.double(), z.double(), rays[:, 3:].double()
        w = R.post_process(raw, z, d)[3].clone().requires_grad_(True)
        loss = distortion_definition(w, z, 2.0, 6.0)
        loss.sum().backward()
        qd, value = scan_forms(w.detach(), z, 2.0, 6.0)
        e_q = float((qd - w.grad).abs().max() / w.grad.abs().max())
        e_v = float((value - loss.detach()).abs().max())
        assert e_q < 1e-12 and e_v < 1e-12, (n, S, hard, e_q, e_v)
    # one sample: no interval, no pair
    w1, z1 = torch.tensor([[0.7]], dtype=torch.float64), torch.tensor([[3.0]], dtype=torch.float64)
    assert float(distortion_definition(w1, z1, 2.0, 6.0)) == 0.0 and float(scan_forms(w1, z1, 2.0, 6.0)[1]) == 0.0


# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def geo():
    """The library is built when the tree is fresh (a no-op when it is up to date), like tests/conftest.py does for libmi_nerf.so."""
    from nerf_pytorch_paeng_amd import _geo
    from nerf_pytorch_paeng_amd.build import build_geo_library
    build_geo_library()
    _geo.lib()
    return _geo


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def test_header_table_and_symbols_agree_and_the_libraries_do_not_mix(geo):
    from nerf_pytorch_paeng_amd import _lib
    from nerf_pytorch_paeng_amd.build import build_library
    build_library()
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_geo.h")).read()
    declared = set(re.findall(r"\b(mi_geo_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(geo.SIGNATURES), declared ^ set(geo.SIGNATURES)
    new = _exports(geo.LIB_PATH)
    assert {n for n in new if n.startswith("mi_")} == declared                             # the header's entries, and no mi_nerf_* name
    assert not [n for n in new if n.startswith("mi_nerf_")]
    old = _exports(_lib.LIB_PATH)
    assert {n for n in old if n.startswith("mi_")} == set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 68       # libmi_nerf.so: its entries and nothing of this
    assert not set(geo.SIGNATURES) & set(_lib.SIGNATURES)
    for other in ("mi_nerf.h", "mi_nerf_occ.h", "mi_nerf_iqa.h", "mi_nerf_scene.h", "mi_nerf_mesh.h"):
        assert "mi_geo_" not in open(os.path.join(ROOT, "include", other)).read()
    assert '#include "mi_nerf' not in hdr                                                  # the header stands alone
    assert geo.lib().mi_geo_abi_version() == geo.ABI_VERSION == int(re.search(r"#define MI_GEO_ABI_VERSION (\d+)", hdr).group(1))
    assert geo.MAX_SAMPLES == int(re.search(r"#define MI_GEO_MAX_SAMPLES (\d+)", hdr).group(1))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [n for n in sorted(declared) if n not in doc] == []


def test_the_library_stands_alone(geo):
    dyn = subprocess.run(["readelf", "-d", geo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libmi_nerf" not in dyn
    und = subprocess.run(["nm", "-D", "--undefined-only", geo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not [ln for ln in und.splitlines() if ln.split()[-1].startswith("mi_")]


def test_header_compiles_as_c99_and_the_library_links_and_answers(tmp_path, geo):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not found")
    pkg = os.path.dirname(geo.LIB_PATH)
    exe = str(tmp_path / "geo_consumer")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "geo_consumer.c"), "-L", pkg, "-lmi_nerf_geo", f"-Wl,-rpath,{pkg}", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"geo c_abi consumer ok: ABI {geo.ABI_VERSION}" in run.stdout


# made-up addresses that are never dereferenced: every call below is refused before the first HIP call (a call that got as far as one would
# answer MI_GEO_EHIP, "HIP error ... no ROCm-capable device", on a machine without a GPU)
GOOD = dict(raw=0x1000, z=0x2000, rays=0x3000, stride=6, n=8, S=64, near=2.0, far=6.0, d_raw=0x4000)
REFUSALS = {
    "S 0": dict(S=0),
    "S 1025": dict(S=1025),
    "ray_stride 4": dict(stride=4),
    "far == near": dict(far=2.0),
    "far < near": dict(far=1.0),
    "near NaN": dict(near=NAN),
    "far inf": dict(far=INF),
    "near -inf": dict(near=-INF),
    "negative n": dict(n=-1),
    "NULL raw": dict(raw=None),
    "NULL z": dict(z=None),
    "NULL rays": dict(rays=None),
    "unaligned raw": dict(raw=0x1004),
}


def _call_both(L, a):
    fwd = L.mi_geo_composite(a["raw"], a["z"], a["rays"], a["stride"], a["n"], a["S"], a["near"], a["far"], 0x5000, None, None, None, None, 0x6000, None)
    msg_f = L.mi_geo_last_error()
    bwd = L.mi_geo_composite_backward(a["raw"], a["z"], a["rays"], a["stride"], a["n"], a["S"], a["near"], a["far"], 0x5000, None, None, 0x6000, None,
                                      a["d_raw"], None)
    return (fwd, msg_f.decode()), (bwd, L.mi_geo_last_error().decode())


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_answer_einval_with_a_message_before_any_hip_call(geo, case):
    for rc, msg in _call_both(geo.lib(), dict(GOOD, **REFUSALS[case])):
        assert rc == EINVAL, (case, rc, msg)
        assert msg and "HIP error" not in msg, (case, msg)


def test_a_null_or_unaligned_d_raw_is_refused_and_no_rays_are_a_no_op(geo):
    L = geo.lib()
    for bad in (None, 0x4004):
        (_, _), (rc, msg) = _call_both(L, dict(GOOD, d_raw=bad))
        assert rc == EINVAL and "d_raw" in msg and "HIP error" not in msg, (bad, rc, msg)
    # n == 0: nothing is launched, and the device pointers may be NULL, as those of empty buffers are
    assert L.mi_geo_composite(None, None, None, 6, 0, 64, 2.0, 6.0, None, None, None, None, None, None, None) == 0, geo.last_error()
    assert L.mi_geo_composite_backward(None, None, None, 3, 0, 64, 2.0, 6.0, None, None, None, None, None, None, None) == 0, geo.last_error()
    assert L.mi_geo_composite_backward(None, None, None, 3, 0, 0, 2.0, 6.0, None, None, None, None, None, None, None) == EINVAL       # the rest is still checked


# ---------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------
def test_geometry_options_refuse_what_they_must():
    from nerf_pytorch_paeng_amd import geometry, harness
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    assert geometry.parse_options(None, 2.0, 6.0) is None
    g = geometry.parse_options({"distortion_weight": 0.01}, 2.0, 6.0)
    assert (g["acc_weight"], g["depth_weight"], g["distortion_weight"], g["targets"]) == (0.0, 0.0, 0.01, None)
    fn = lambda r: (r[:, 0], r[:, 1])                               # noqa: E731
    assert geometry.parse_options({"acc_weight": 0.1, "targets": fn}, 2.0, 6.0)["targets"] is fn
    for bad, what in (({"acc_weight": 0.1}, "targets"), ({"depth_weight": 1.0}, "targets"), ({"acc_wieght": 0.1}, "unknown key"),
                      ({"distortion_weight": 0.01, "lambda": 1}, "unknown key"), ({"acc_weight": -1.0, "targets": fn}, ">= 0"),
                      ({"distortion_weight": "0.01"}, ">= 0"), ({"acc_weight": 0.1, "targets": 3}, "callable"), ([0.1, 0.0, 0.01], "mapping")):
        with pytest.raises(MiNerfError, match=what):
            geometry.parse_options(bad, 2.0, 6.0)
    # harness.train refuses before it touches the model, the data or a device
    opts = SimpleNamespace(near=2.0, far=6.0, geometry={"acc_weight": 0.1})
    with pytest.raises(MiNerfError, match="targets"):
        harness.train(1, [0], None, (None, None), (4, 4), None, None, None, None, None, None, opts)
    opts.geometry = {"acc_weight": 0.1, "targets": fn, "depth": 1.0}
    with pytest.raises(MiNerfError, match="unknown key"):
        harness.train(1, [0], None, (None, None), (4, 4), None, None, None, None, None, None, opts)


def test_wrappers_refuse_host_tensors_and_bad_shapes():
    from nerf_pytorch_paeng_amd import geometry
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    raw, z, rays = torch.zeros(4, 8, 4), torch.zeros(4, 8), torch.zeros(4, 6)
    with pytest.raises(MiNerfError, match="HIP device"):            # no GPU: loudly, no fallback
        geometry.composite_geo(raw, z, rays, 2.0, 6.0)
    with pytest.raises(MiNerfError, match="HIP device"):
        geometry.composite_geo_backward(raw, z, rays, 2.0, 6.0, g_acc=torch.zeros(4))
    with pytest.raises(MiNerfError, match="raw must be"):
        geometry.composite_geo(torch.zeros(4, 7, 4), z, rays, 2.0, 6.0)
    with pytest.raises(MiNerfError, match="rays must be"):
        geometry.composite_geo(raw, z, torch.zeros(4, 4), 2.0, 6.0)
    for kw, name in ((dict(g_rgb=torch.zeros(4, 4)), "g_rgb"), (dict(g_acc=torch.zeros(5)), "g_acc"), (dict(g_depth=torch.zeros(4, 1)), "g_depth"),
                     (dict(g_distortion=torch.zeros(3)), "g_distortion"), (dict(g_weights=torch.zeros(4, 9)), "g_weights")):
        with pytest.raises(MiNerfError, match=name):
            geometry.composite_geo_backward(raw, z, rays, 2.0, 6.0, **kw)
