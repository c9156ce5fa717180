"""The f16 render modes (MI_NERF_MODE_F16 = 8: both networks on the f16 MFMA kernel; MI_NERF_MODE_F16_BF16 = 9: coarse network in f16, fine
network in bf16), checked without a GPU: the mode values and their Python surface, the argument refusals in front of the first HIP call, the
layout assumption the kernel's weight addressing rests on (csrc/mlp_half_core.h: the split-precision blob's hi quads, 2 KiB apart, ARE the
bf16 stream), the object checks of mlp_f16.hip, and the f16 rounding-point oracle the GPU tests hold the kernel to."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import _lib, harness, ops, synthetic
from nerf_pytorch_paeng_amd._lib import MiNerfError
from oracle import restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
QUAD = 1024                     # bytes of one A-fragment quad (64 lanes x 16 B)
SLOT_QUADS, TAIL_BF16, TAIL_F16S, TAIL_USED = 32, 224, 208, 204

# mfma_hazard_check.py --strict per kernel of mlp_f16.hip (see STRICT_RELIANCE in test_packing_cpu.py): pairs inside their window only at the
# matrix pipe's issue interval, as of hipcc 7.2.  Pinned so that the number cannot grow silently.
STRICT_RELIANCE_F16 = {
    "mlp_f16_kernelILi256ELi10ELi4ELi4ELi0ELi4E": 4,
    "mlp_f16_kernelILi256ELi10ELi4ELi2ELi0ELi4E": 192,
    "mlp_f16_kernelILi256ELi10ELi4ELi4ELi2ELi4E": 196,
}


# ---------------------------------------------------------------------------------------------------
# the oracle: R.mlp_forward_bf16's rounding points with f16 for bf16
# ---------------------------------------------------------------------------------------------------
def f16_round(t: torch.Tensor) -> torch.Tensor:
    """Round to float16 (nearest even; through fp32, as the kernel converts its fp32 values) and return in the input's dtype."""
    return t.to(torch.float32).to(torch.float16).to(t.dtype)


def mlp_forward_f16(sd, prefix: str, x: torch.Tensor, D: int, in_x: int, in_d: int, skips=(4,), dtype=torch.float32) -> torch.Tensor:
    """``R.mlp_forward`` with the ROUNDING POINTS of the f16 MFMA variant (csrc/mlp_f16.hip), which are R.mlp_forward_bf16's with f16 for
    bf16: the weights of every Linear rounded (except the view-direction columns of linear_d, which the kernel folds into a per-ray fp32
    bias), gamma(x) rounded, every activation rounded where it becomes the next layer's input (after ReLU; linear_feat's output without
    ReLU), products accumulated in ``dtype``, biases in full precision."""
    def wq(name, cols=None):
        w = torch.as_tensor(sd[f"{prefix}{name}.weight"]).float()
        if cols is None:
            return f16_round(w).to(dtype)
        w = w.clone()
        w[:, cols] = f16_round(w[:, cols])
        return w.to(dtype)

    def b(name):
        return torch.as_tensor(sd[f"{prefix}{name}.bias"]).to(dtype)
    x = x.to(dtype)
    gx, gd = f16_round(x[:, :in_x]), x[:, in_x:in_x + in_d]
    h = gx
    for i in range(D):
        h = f16_round(torch.relu(h @ wq(f"linear_x.{i}").T + b(f"linear_x.{i}")))
        if i in skips:
            h = torch.cat([gx, h], -1)
    W = torch.as_tensor(sd[f"{prefix}linear_feat.weight"]).shape[0]
    sigma = h @ wq("linear_density").T + b("linear_density")
    feat = f16_round(h @ wq("linear_feat").T + b("linear_feat"))
    g = f16_round(torch.relu(torch.cat([feat, gd], -1) @ wq("linear_d", slice(0, W)).T + b("linear_d")))
    rgb = g @ wq("linear_color").T + b("linear_color")
    return torch.cat([rgb, sigma], -1)


def test_f16_oracle_is_the_split_precision_oracle_without_its_lo_terms(monkeypatch):
    """The oracle above, in fp64, is R.mlp_forward_f16split with every lo half zeroed: the same rounding points, hi = f16(value)."""
    D, W = 8, 256
    sd = synthetic.make_state_dict(3, D, W)
    rs = np.random.RandomState(5)
    ray = torch.from_numpy(rs.normal(size=(40, 6)).astype(np.float32))
    z = torch.sort(torch.from_numpy(rs.uniform(2, 6, (40, 24)).astype(np.float32)), -1)[0]
    x = R.embed(ray, z, 10, 4)
    ours = mlp_forward_f16(sd, "model_fine.", x, D, 63, 27, dtype=torch.float64)
    monkeypatch.setattr(R, "f16_split", lambda t: (t.to(torch.float32).to(torch.float16).to(torch.float32), torch.zeros_like(t, dtype=torch.float32)))
    ref = R.mlp_forward_f16split(sd, "model_fine.", x, D, 63, 27, dtype=torch.float64)
    # mlp_forward_f16split hands every layer's output on in fp32; ours keeps fp64 up to the next rounding point (which goes through fp32)
    err = float((ours.to(torch.float32).double() - ref.double()).abs().max())
    print(f"f16 oracle vs split-precision oracle without lo terms: max |diff| {err:.1e}")
    assert err <= 1e-12, err
    assert float((ours - R.mlp_forward(sd, "model_fine.", x, D, 63, 27, dtype=torch.float64)).abs().max()) > 1e-4      # it does round


# ---------------------------------------------------------------------------------------------------
# mode values and the Python surface
# ---------------------------------------------------------------------------------------------------
def _header_defines():
    text = open(os.path.join(ROOT, "include", "mi_nerf.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(MI_NERF_\w+)\s+(\d+)", text)}


def test_mode_values():
    d = _header_defines()
    assert d["MI_NERF_MODE_F16"] == 8 and d["MI_NERF_MODE_F16_BF16"] == 9
    assert (ops.MODE_F16, ops.MODE_F16_BF16) == (8, 9)
    assert d["MI_NERF_ABI_VERSION"] == 4                                                   # a compatible extension of ABI 4
    assert not any(k.startswith("MI_NERF_MODE_") and v in (4, 7) for k, v in d.items())      # 4 retired, 7 reserved


FLAGS = ("bf16", "f16s", "coarse_f16s", "f16", "coarse_f16")
# the flags that name a mode (in FLAGS order) -> MI_NERF_MODE_* at points_per_wave 0 / 32 / 64 (None: refused), as render_cfg has
# resolved them since the f16 modes were added; every other combination is refused at every launch shape
SWEEP = {(0, 0, 0, 0, 0): (0, 0, 0), (1, 0, 0, 0, 0): (1, 3, 2), (0, 1, 0, 0, 0): (5, 5, 5), (1, 0, 1, 0, 0): (6, None, None),
         (0, 0, 0, 1, 0): (8, None, None), (1, 0, 0, 0, 1): (9, None, None)}


def test_render_cfg_and_precision_strings_resolve_to_modes():
    cfg = lambda **kw: ops.render_cfg(2.0, 6.0, 64, 128, False, **kw)
    assert cfg(f16=True).mode == 8
    assert cfg(bf16=True, coarse_f16=True).mode == 9
    assert cfg(bf16=True, coarse_f16s=True).mode == 6 and cfg(f16s=True).mode == 5 and cfg().mode == 0 and cfg(bf16=True).mode == 1
    bad = [dict(f16=True, bf16=True), dict(f16=True, f16s=True), dict(f16=True, coarse_f16=True), dict(f16=True, coarse_f16s=True),
           dict(f16=True, points_per_wave=64), dict(coarse_f16=True), dict(coarse_f16=True, f16s=True), dict(bf16=True, coarse_f16=True, coarse_f16s=True),
           dict(bf16=True, coarse_f16=True, points_per_wave=32), dict(bf16=True, f16s=True, coarse_f16=True)]
    for kw in bad:
        with pytest.raises(MiNerfError):
            cfg(**kw)
    with pytest.raises(MiNerfError):
        ops.time_mlp_rays(ops.make_net(8, 256, 4), None, None, torch.zeros(1, 1), None, 1, bf16=True, f16=True)
    P = lambda s: harness._precision(type("O", (), {"precision": s})())
    want = {"fp32": ((), "fp32", "fp32", 0), "bf16": (("bf16",), "bf16", "bf16", 1), "f16s": (("f16s",), "f16s", "f16s", 5),
            "f16s+bf16": (("bf16", "coarse_f16s"), "f16s", "bf16", 6), "f16": (("f16",), "f16", "f16", 8),
            "f16+bf16": (("bf16", "coarse_f16"), "f16", "bf16", 9)}
    for s, (on, coarse, fine, mode) in want.items():
        assert P(s) == {k: k in on for k in FLAGS}, s
        prec = ops.precision(**P(s))
        assert (prec.coarse, prec.fine, prec.mode) == (coarse, fine, mode), s
        assert prec.reads_f16s == (coarse in ("f16s", "f16")), s
    for s in ("fp16", "f16+f16s", "bf16+f16"):
        with pytest.raises(ValueError):
            P(s)


def test_every_flag_combination_resolves_to_its_mode_or_is_refused():
    for bits in itertools.product((0, 1), repeat=len(FLAGS)):
        kw = dict(zip(FLAGS, map(bool, bits)))
        for ppw, mode in zip((0, 32, 64), SWEEP.get(bits, (None, None, None))):
            if mode is None:
                with pytest.raises(MiNerfError):
                    ops.precision(**kw, points_per_wave=ppw)
                with pytest.raises(MiNerfError):
                    ops.render_cfg(2.0, 6.0, 64, 128, False, points_per_wave=ppw, **kw)
            else:
                assert ops.precision(**kw, points_per_wave=ppw).mode == mode, (kw, ppw)
                assert ops.render_cfg(2.0, 6.0, 64, 128, False, points_per_wave=ppw, **kw).mode == mode, (kw, ppw)
    with pytest.raises(MiNerfError):                # the retired 8-wave shape: refused before the library sees mode 4 (which it refuses too)
        ops.render_cfg(2.0, 6.0, 64, 128, False, True, points_per_wave=832)
    with pytest.raises(MiNerfError):
        ops.time_mlp_rays(ops.make_net(8, 256, 4), None, None, torch.zeros(1, 1), None, 1, True, 832)


def _render_call(lib, net, mode):
    """mi_nerf_render_rays with host stubs for every pointer: an argument error must be answered before any of them is looked at."""
    cfg = ops.render_cfg(2.0, 6.0, 1, 0, False)
    cfg.mode = mode
    rays = (C.c_float * 6)(0, 0, 0, 0, 0, -1)
    out = (C.c_float * 8)()
    blob, ws = (C.c_char * 16)(), (C.c_char * 16)()
    rc = lib.mi_nerf_render_rays(C.byref(net), C.cast(blob, C.c_void_p), None, C.byref(cfg), C.cast(rays, C.c_void_p), 1, None, None,
                                 C.cast(ws, C.c_void_p), 1 << 20, C.cast(out, C.c_void_p), C.cast(C.byref(out, 12), C.c_void_p), None, None, None)
    return rc, lib.mi_nerf_last_error().decode()


def test_argument_refusals_without_a_gpu():
    lib = _lib.lib()
    narrow = ops.make_net(8, 128, 4)
    for mode in (8, 9):
        rc, msg = _render_call(lib, narrow, mode)
        assert rc == EINVAL and "f16 variant" in msg and "HIP error" not in msg, (mode, rc, msg)
    rc = lib.mi_nerf_time_mlp_rays(C.byref(narrow), None, None, None, 1, 1, None, 1, 8, C.byref(C.c_float()), None)
    msg = lib.mi_nerf_last_error().decode()
    assert rc == EINVAL and "f16 variant" in msg, (rc, msg)
    for mode in (7, 4):                                            # reserved / retired: still refused
        rc, msg = _render_call(lib, ops.make_net(8, 256, 4), mode)
        assert rc == EINVAL and "HIP error" not in msg, (mode, rc, msg)
    assert "MI_NERF_MODE_" in _render_call(lib, ops.make_net(8, 256, 4), 7)[1]
    rc = lib.mi_nerf_time_mlp_rays(C.byref(ops.make_net(8, 256, 4)), None, None, None, 1, 1, None, 1, 9, C.byref(C.c_float()), None)
    assert rc == EINVAL and "MI_NERF_MODE_" in lib.mi_nerf_last_error().decode()      # mode 9 is two networks: render_rays only


def test_depth_refusals_without_a_gpu():
    """The depth limits (csrc/half_layout.h; ops.F16S_FWD_MAX_D, HALF_64PT_MAX_D, F16S_DGRAD_MAX_D) and netDepth 2..16 itself are argument
    checks: answered with an error that names the depth or the limit, before the first HIP call (on a machine without a GPU any HIP call
    would put "HIP error" into the message) and before any of the host stubs handed over as device pointers is looked at."""
    lib = _lib.lib()
    stub = C.cast((C.c_char * 64)(), C.c_void_p)

    def refused(rc, *needles):
        msg = lib.mi_nerf_last_error().decode()
        assert rc == EINVAL and all(s in msg for s in needles) and "HIP error" not in msg, (rc, msg)

    for D in (15, 16):                                             # the split-precision forward: alone, as the training forward, in a render mode
        net = ops.make_net(D, 256, D - 2)
        refused(lib.mi_nerf_mlp_rays_f16s(C.byref(net), stub, stub, stub, 4, 8, stub, None), f"D = {D} does not fit (D <= {ops.F16S_FWD_MAX_D})")
        refused(lib.mi_nerf_mlp_rays_train_f16s(C.byref(net), stub, stub, stub, 4, 8, stub, stub, 1 << 40, None), f"(D <= {ops.F16S_FWD_MAX_D})")
        for mode in (5, 6):
            rc, msg = _render_call(lib, net, mode)
            assert rc == EINVAL and f"(D <= {ops.F16S_FWD_MAX_D})" in msg and "HIP error" not in msg, (mode, rc, msg)
        refused(lib.mi_nerf_time_mlp_rays(C.byref(net), stub, stub, stub, 1, 1, stub, 1, 5, C.byref(C.c_float()), None), f"(D <= {ops.F16S_FWD_MAX_D})")
    for D in (13, 16):                                             # bf16 at 64 points per wave (the plan itself picks 32 for such a network)
        refused(lib.mi_nerf_mlp_rays_bf16_shape(C.byref(ops.make_net(D, 256, 4)), stub, stub, stub, 4, 8, stub, 64, None),
                f"D = {D} does not fit (D <= {ops.HALF_64PT_MAX_D})")
    net16 = ops.make_net(16, 256, 4)
    for mode in (2, 3):                                            # the split-precision backward-data chain, with or without the split-precision products
        refused(lib.mi_nerf_mlp_backward_mode(C.byref(net16), stub, stub, stub, stub, 4, 8, stub, stub, stub, 1 << 40, stub, 0, mode, None),
                f"D = 16 does not fit (D <= {ops.F16S_DGRAD_MAX_D})")
    for D in (17, 1):                                              # netDepth 2..16: every forward family, the training forward and backward
        for W in (128, 256, 512):
            refused(lib.mi_nerf_mlp_rays(C.byref(ops.make_net(D, W, -1)), stub, stub, stub, 4, 8, stub, None), f"D={D}")
        net = ops.make_net(D, 256, -1)
        refused(lib.mi_nerf_mlp_rays_bf16_shape(C.byref(net), stub, stub, stub, 4, 8, stub, 0, None), f"D={D}")
        refused(lib.mi_nerf_mlp_rays_f16s(C.byref(net), stub, stub, stub, 4, 8, stub, None), f"D={D}")
        refused(lib.mi_nerf_time_mlp_rays(C.byref(net), stub, stub, stub, 1, 1, stub, 1, 8, C.byref(C.c_float()), None), f"D={D}")
        for fn in (lib.mi_nerf_mlp_rays_train, lib.mi_nerf_mlp_rays_train_f16s):
            refused(fn(C.byref(net), stub, stub, stub, 4, 8, stub, stub, 1 << 40, None), f"D={D}")
        for mode in (0, 1, 3):
            refused(lib.mi_nerf_mlp_backward_mode(C.byref(net), stub, stub, stub, stub, 4, 8, stub, stub, stub, 1 << 40, stub, 0, mode, None), f"D={D}")
        for size_fn in (lib.mi_nerf_packed_bytes, lib.mi_nerf_packed_bytes_bf16, lib.mi_nerf_packed_bytes_f16s, lib.mi_nerf_packed_bytes_bwd_f16s):
            assert size_fn(C.byref(net)) == 0 and f"D={D}" in lib.mi_nerf_last_error().decode()


# ---------------------------------------------------------------------------------------------------
# the kernel's addressing assumption: the f16s blob's hi quads, read as the ring reads them, are the bf16 stream
# ---------------------------------------------------------------------------------------------------
def _exact_state_dict(D, skip):
    """Weights k * 2^-8 with |k| < 128: exactly representable in bf16 and in f16, so both packers carry them unrounded."""
    sd = synthetic.make_state_dict(9, D, 256, skips=(skip,) if skip >= 0 else ())
    rs = np.random.RandomState(D)
    out = {}
    for k, v in sd.items():
        v = np.asarray(v)
        out[k] = (rs.randint(-127, 128, size=v.shape) / 256.0).astype(np.float32) if k.endswith("weight") else v
    return out


def _ring_reads(walk_bytes, real_bytes):
    """Blob offsets the f16 kernel's weight ring reads for every stream position, in the order wstream_ring.h issues them: slot s (32
    positions), wave w (8 positions each), DMA i: fetch_off + 16 KiB w + 2 KiB i, the last slot's shares past the blob moved 32 KiB back.
    A restatement of hring_dma<.., true> / hring_next_fetch<true> / the src_lim set-up in hring_start<.., true> (wstream_ring.h, whose comments point here):
    it checks that this arithmetic fits the blobs, not that the kernel still does this arithmetic -- the GPU parity tests do that."""
    n_slots = walk_bytes // (2 * SLOT_QUADS * QUAD)
    pos = {}
    for s in range(n_slots):
        fetch_off = s * 2 * SLOT_QUADS * QUAD
        for w in range(4):
            src_lim = walk_bytes - SLOT_QUADS * QUAD - (w + 1) * 8 * 2 * QUAD
            src = fetch_off - SLOT_QUADS * QUAD if fetch_off > src_lim else fetch_off
            for i in range(8):
                g = src + w * 8 * 2 * QUAD + (i & 3) * QUAD + (8192 if i >= 4 else 0) + (i & 3) * QUAD      # per-lane address + instruction offset
                assert 0 <= g and g + QUAD <= real_bytes, (s, w, i, g, real_bytes)                         # never past the blob's stream
                pos[s * SLOT_QUADS + w * 8 + i] = g
    return pos


@pytest.mark.parametrize("D,skip", [(8, 4), (3, -1), (5, 0)])
def test_f16s_hi_quads_are_the_bf16_stream(D, skip):
    sd = _exact_state_dict(D, skip)
    net = ops.make_net(D, 256, skip)
    b16 = ops.pack_module(sd, "model_fine.", net, bf16=True).numpy()
    f16s = ops.pack_module(sd, "model_fine.", net, f16s=True).numpy()
    hb, hs = (np.frombuffer(b[:64].tobytes(), dtype=np.uint32) for b in (b16, f16s))
    so_b, sb_b, sdo_b, sf_b = (int(hb[i]) for i in (7, 8, 10, 11))
    so_s, sb_s, sdo_s, sf_s = (int(hs[i]) for i in (7, 8, 10, 11))
    n_quads = sb_b // QUAD
    body = n_quads - TAIL_BF16
    assert sb_s // (2 * QUAD) == body + TAIL_F16S and body % SLOT_QUADS == 0
    bstream = b16[so_b:so_b + sb_b].view(np.uint16).reshape(n_quads, 512)
    sstream = f16s[so_s:so_s + sb_s]
    as_f32_bf16 = (bstream.astype(np.uint32) << 16).view(np.float32)
    walk = (body + TAIL_BF16) * 2 * QUAD                                 # what mlp_rays_f16 hands the kernel as its stream length
    reads = _ring_reads(walk, sb_s)
    used = list(range(body)) + [body + q for q in range(TAIL_USED)]
    for q in used:
        hi = sstream[reads[q]:reads[q] + QUAD].view(np.float16).astype(np.float32)
        assert np.array_equal(hi, as_f32_bf16[q]), q
    pairs = sstream.reshape(-1, 2, QUAD)
    assert not pairs[:, 1].any()                                         # every lo quad is zero: the weights are exact in f16
    assert [reads[q] // (2 * QUAD) for q in used] == used               # position q is pair q of the blob (the hi half: offset 0 of the pair)
    assert float(np.abs(as_f32_bf16[body + TAIL_USED:]).max()) == 0.0   # the bf16 padding is zero too
    assert sf_b == sf_s and np.array_equal(b16[sdo_b:sdo_b + 4 * sf_b], f16s[sdo_s:sdo_s + 4 * sf_s])      # the side tables


# ---------------------------------------------------------------------------------------------------
# object checks of mlp_f16.hip (the check functions of test_packing_cpu.py)
# ---------------------------------------------------------------------------------------------------
def test_f16_object_owns_m0_and_the_agpr_file():
    from tests import test_packing_cpu as P
    P.test_fragment_file_kernels_own_m0_and_the_agpr_file("mlp_f16.hip", "v_mfma_f32_16x16x32_f16", 4000)


def test_f16_object_mfma_hazards():
    from tests import test_packing_cpu as P
    P.test_mfma_destinations_and_c_operands_are_left_alone_for_their_wait_states("mlp_f16.hip", 4000)


def test_f16_object_reliance_on_the_mfma_issue_interval(capsys):
    from nerf_pytorch_paeng_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mfma_hazard_check as H
    if not os.path.exists(H.OBJDUMP):
        pytest.skip("llvm-objdump not found")
    seen = set()
    for name, ins in H.kernels_of(H.device_asm(build.ensure_object("mlp_f16.hip"))).items():
        n, bad = H.check(ins, strict=True)
        if n == 0:
            continue
        keys = [k for k in STRICT_RELIANCE_F16 if k in name]
        limit = STRICT_RELIANCE_F16[keys[0]] if keys else 0
        seen.update(keys)
        with capsys.disabled():
            print(f"\n  strict  mlp_f16.hip  {name[:84]}: {n} MFMAs, {len(bad)} pairs rely on the issue interval (pinned: {limit})")
        assert len(bad) <= limit, f"{name}: {len(bad)} pairs rely on the MFMA issue interval, pinned {limit}; worst: {bad[:3]}"
    assert seen == set(STRICT_RELIANCE_F16), seen                  # the three launch shapes of the f16 kernel, and no other kernel
