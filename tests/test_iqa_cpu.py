"""libmi_nerf_iqa.so / include/mi_nerf_iqa.h without a GPU: the header is C99 and a C program links against the library; the header, the ctypes
table (nerf_pytorch_paeng_amd/_iqa.py) and the library's dynamic symbols name the same entries; libmi_nerf.so is what it was (exactly the
names of _lib.SIGNATURES) and the new library exports nothing of it; every refusal answers MI_IQA_EINVAL with a message before any HIP call;
the window is the one of the definition.  The float64 oracle the GPU tests compare with (``ssim_oracle``, torch on the CPU, written from the
definition in the header, not from the kernel) is defined here and checks itself on the closed forms."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
C1, C2 = 0.01 ** 2, 0.03 ** 2


# ---------------------------------------------------------------------------------------------------
# the oracle: SSIM as include/mi_nerf_iqa.h defines it, torch on the CPU
# ---------------------------------------------------------------------------------------------------
def window_1d(dtype=torch.float64) -> torch.Tensor:
    i = torch.arange(11, dtype=dtype)
    g = torch.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2))
    return g / g.sum()


def matlab_factor(H: int, W: int) -> int:
    return max(1, int(math.floor(min(H, W) / 256 + 0.5)))


def ssim_oracle(pred: torch.Tensor, target: torch.Tensor, *, downsample: int = 1, clamp_cs: bool = False, dtype=torch.float64):
    """(value, map [H'-10, W'-10, 3]) of one [H, W, 3] pair, everything in ``dtype`` (float64: the oracle; float32: the comparator)."""
    H, W, _ = pred.shape
    f = matlab_factor(H, W) if downsample == 0 else downsample
    x = pred.to(dtype).permute(2, 0, 1)[None]                     # [1, 3, H, W]
    y = target.to(dtype).permute(2, 0, 1)[None]
    if f > 1:
        x, y = F.avg_pool2d(x, f), F.avg_pool2d(y, f)             # floor mode: the remainder rows and columns are dropped
    g = window_1d(dtype)
    w2 = torch.outer(g, g)[None, None].repeat(3, 1, 1, 1)         # the 2-D window of the same formula, one per channel

    def blur(t):
        return F.conv2d(t, w2, groups=3)                          # 'valid'

    mx, my = blur(x), blur(y)
    vx, vy, cov = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    if clamp_cs:
        cs = (2 * cov + C2) / (vx + vy + C2)
        cs = torch.where(cs < 0, torch.zeros_like(cs), cs)        # keeps a NaN
        smap = (2 * mx * my + C1) / (mx * mx + my * my + C1) * cs
    else:
        smap = ((2 * mx * my + C1) * (2 * cov + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return smap.mean(), smap[0].permute(1, 2, 0)


# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def iqa():
    """The library is built when the tree is fresh (a no-op when it is up to date), like tests/conftest.py does for libmi_nerf.so."""
    from nerf_pytorch_paeng_amd import _iqa
    from nerf_pytorch_paeng_amd.build import build_iqa_library
    build_iqa_library()
    _iqa.lib()
    return _iqa


def test_oracle_closed_forms():
    g = torch.Generator().manual_seed(0)
    img = torch.rand(23, 31, 3, generator=g)
    for kw in ({}, {"clamp_cs": True}, {"downsample": 2}):
        v, m = ssim_oracle(img, img, **kw)
        assert abs(float(v) - 1.0) < 1e-12 and float((m - 1).abs().max()) < 1e-12
    for a, b in ((0.2, 0.9), (0.5, 0.5), (0.0, 1.0), (0.03, 0.04)):
        v, _ = ssim_oracle(torch.full((15, 17, 3), a), torch.full((15, 17, 3), b))
        xa, xb = float(torch.tensor(a, dtype=torch.float32)), float(torch.tensor(b, dtype=torch.float32))
        assert abs(float(v) - (2 * xa * xb + C1) / (xa * xa + xb * xb + C1)) < 1e-12
    assert ssim_oracle(torch.rand(11, 11, 3, generator=g), torch.rand(11, 11, 3, generator=g))[1].shape == (1, 1, 3)
    assert ssim_oracle(torch.rand(50, 47, 3, generator=g), torch.rand(50, 47, 3, generator=g), downsample=3)[1].shape == (6, 5, 3)
    assert [matlab_factor(*hw) for hw in ((800, 800), (378, 504), (48, 48), (384, 384), (383, 900))] == [3, 1, 1, 2, 1]
    bad = img.clone()
    bad[4, 5, 1] = float("nan")
    assert torch.isnan(ssim_oracle(bad, img)[0]) and torch.isnan(ssim_oracle(bad, img, clamp_cs=True)[0])


def test_header_compiles_as_c99_and_the_library_links_and_answers(tmp_path, iqa):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not found")
    pkg = os.path.dirname(iqa.LIB_PATH)
    exe = str(tmp_path / "iqa_consumer")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "iqa_consumer.c"), "-L", pkg, "-lmi_nerf_iqa", f"-Wl,-rpath,{pkg}", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"iqa c_abi consumer ok: ABI {iqa.ABI_VERSION}" in run.stdout


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def test_header_table_and_symbols_agree_and_the_two_libraries_do_not_mix(iqa):
    from nerf_pytorch_paeng_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_iqa.h")).read()
    declared = set(re.findall(r"\b(mi_iqa_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(iqa.SIGNATURES), declared ^ set(iqa.SIGNATURES)
    new = _exports(iqa.LIB_PATH)
    assert {n for n in new if n.startswith("mi_iqa_")} == declared
    assert not [n for n in new if n.startswith("mi_nerf_")]
    old = _exports(_lib.LIB_PATH)
    assert {n for n in old if n.startswith("mi_")} == set(_lib.SIGNATURES)            # libmi_nerf.so: its 68 entries and nothing of this
    assert not set(iqa.SIGNATURES) & set(_lib.SIGNATURES)
    assert "mi_iqa_" not in open(os.path.join(ROOT, "include", "mi_nerf.h")).read()
    assert iqa.lib().mi_iqa_abi_version() == iqa.ABI_VERSION == int(re.search(r"#define MI_IQA_ABI_VERSION (\d+)", hdr).group(1))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [n for n in sorted(declared) if n not in doc] == []


GOOD = dict(pred=0x1000, target=0x2000, n_frames=2, H=64, W=48, downsample=1, flags=0, out=0x3000, map=None, scratch=0x4000,
            scratch_bytes=1 << 20, stream=None)
REFUSALS = {
    "NULL pred": dict(pred=None),
    "NULL target": dict(target=None),
    "NULL out": dict(out=None),
    "NULL scratch": dict(scratch=None),
    "n_frames 0": dict(n_frames=0),
    "n_frames negative": dict(n_frames=-3),
    "H below the window": dict(H=10),
    "W below the window": dict(W=10),
    "pooled H below the window": dict(H=21, downsample=2),
    "pooled W below the window": dict(W=32, downsample=3),
    "negative downsample": dict(downsample=-1),
    "unknown flag bit": dict(flags=2),
    "unknown high flag bit": dict(flags=0x80000001),
    "scratch too small": dict(scratch_bytes=8),
    "H of zero": dict(H=0),
    "W too large": dict(W=(1 << 18) + 1),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_answer_einval_with_a_message_before_any_hip_call(iqa, case):
    """The pointers are made-up addresses that are never dereferenced: every call here is refused before the first HIP call (a call that
    got as far as a launch would answer MI_IQA_EHIP, "HIP error ... no ROCm-capable device", on a machine without a GPU)."""
    a = dict(GOOD, **REFUSALS[case])
    L = iqa.lib()
    rc = L.mi_iqa_ssim(a["pred"], a["target"], a["n_frames"], a["H"], a["W"], a["downsample"], a["flags"], a["out"], a["map"], a["scratch"],
                       a["scratch_bytes"], a["stream"])
    msg = L.mi_iqa_last_error().decode()
    assert rc == EINVAL, (case, rc, msg)
    assert msg and "HIP error" not in msg, (case, msg)


def test_size_queries_refuse_and_answer(iqa):
    L = iqa.lib()
    assert L.mi_iqa_ssim_scratch_bytes(2, 64, 48, 1) >= 2 * 8 and L.mi_iqa_ssim_scratch_bytes(1, 11, 11, 1) == 8
    assert L.mi_iqa_ssim_scratch_bytes(40, 800, 800, 1) == 40 * L.mi_iqa_ssim_scratch_bytes(1, 800, 800, 1)
    for bad in ((0, 64, 48, 1), (1, 10, 48, 1), (1, 64, 48, -1), (1, 64, 48, 5)):
        assert L.mi_iqa_ssim_scratch_bytes(*bad) == 0 and L.mi_iqa_last_error()
    assert [L.mi_iqa_ssim_downsample_factor(h, w, 0) for h, w in ((800, 800), (378, 504), (48, 48), (384, 384), (383, 900))] == [3, 1, 1, 2, 1]
    assert L.mi_iqa_ssim_downsample_factor(64, 48, 4) == 4 and L.mi_iqa_ssim_downsample_factor(64, 48, 5) == 0
    assert L.mi_iqa_ssim_window(None) == EINVAL


def test_window_is_the_one_of_the_definition(iqa):
    taps = iqa.ssim_window()
    assert len(taps) == 11 == iqa.SSIM_TAPS
    assert abs(math.fsum(taps) - 1.0) <= 1e-15
    assert all(taps[i] == taps[10 - i] for i in range(11))
    raw = [math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)]
    assert abs(taps[5] - raw[5] / math.fsum(raw)) <= 1e-16
    assert max(abs(t - float(w)) for t, w in zip(taps, window_1d())) <= 1e-16


def test_ops_ssim_refuses_host_tensors_and_bad_shapes(iqa):
    from nerf_pytorch_paeng_amd import ops
    a = torch.rand(16, 16, 3)
    with pytest.raises(ops.MiNerfError):
        ops.ssim(a, a)                                               # host tensors: no CPU fallback
    with pytest.raises(ops.MiNerfError):
        ops.ssim(a, torch.rand(16, 17, 3))
    with pytest.raises(ops.MiNerfError):
        ops.ssim(torch.rand(256, 3), torch.rand(256, 3))             # flat frame without hw
    with pytest.raises(ops.MiNerfError):
        ops.ssim(torch.rand(256, 3), torch.rand(256, 3), hw=(16, 15))
    with pytest.raises(ops.MiNerfError):
        ops.ssim(torch.rand(16, 16, 4), torch.rand(16, 16, 4))
