"""THE LATTICE REGULARISERS on the GPU (include/mi_nerf_geo.h, csrc/lattice_reg.hip, nerf_pytorch_paeng_amd/baked_train.py) against the numpy
restatement of the header's rule (tests/lattice_reg_restate.py).

The gradient equals the fp32 restatement BIT FOR BIT (d_v pre-filled, so the add is tested); padding channels and unwritten elements keep
their bits; two runs give the same bits, the value included.  The TV value is held against the exactly rounded float64 sum of the
restatement's fp32 terms with the any-order summation bound (n - 1) 2^-53 sum|t|; the SP value against the float64 restatement with that
bound plus 4 * 2^-52 per term for the device's double log1p (a supposition: twice the 2 ulp such libraries commonly document; the measured
figure is in docs/design/24_lattice_regularisers.md).  References are computed once per case and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import _geo, baked, baked_train, ops, scenes, synthetic
from nerf_pytorch_paeng_amd._lib import stream_ptr
from tests import lattice_reg_restate as LR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32
LATTICES = ((2, 2, 2), (3, 2, 9), (10, 17, 9), (25, 25, 25))
CHANNELS = ((1, 1), (4, 3), (16, 12), (32, 27))
MASKS = ("none", "ones", "pattern", "zeros")
INPUTS = ("normal", "constant region", "jump", "negative")
EPS, SCALE = 1e-8, 0.37


def make_mask(P, kind, seed):
    if kind == "none":
        return None
    shape = LR.mask_shape(P)
    if kind == "ones":
        return np.ones(shape, np.uint8)
    if kind == "zeros":
        return np.zeros(shape, np.uint8)
    rng = np.random.default_rng(seed)
    m = (rng.random(shape) < 0.5).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)      # empty blocks beside full ones
    if m.size > 1:
        m.ravel()[0], m.ravel()[-1] = 0, 200
    return m


def make_input(P, R, Cn, kind, seed):
    """v [P, R] (or [P] for the plane): the counted channels by ``kind``, the padding NaN -- it must enter no result."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0.0, 1.0, P + (R,)).astype(f32)
    if kind == "constant region":
        v[: max(1, P[0] // 2), :, : max(2, P[2] // 2)] = f32(0.75)              # d = 0 exactly, t = sqrtf(eps)
    elif kind == "jump":
        v[...] = 0.0
        v[P[0] // 2:, P[1] // 2:] = f32(4096.0)                                 # the solids of SolidScene next to empty space
    elif kind == "negative":
        v = -np.abs(v) * f32(3.0)
    v[..., Cn:] = np.nan
    return v[..., 0].copy() if R == 1 else v


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def run_tv(P, R, Cn, v, mask, scale, d_v, value=True):
    """One direct call; returns (d_v after the call or None, value as a Python float or None)."""
    L = _geo.lib()
    P3 = (C.c_int32 * 3)(*P)
    out = None if d_v is None else d_v.clone()
    val = scratch = None
    n = 0
    if value:
        n = int(L.mi_geo_lattice_scratch_bytes(P3, R, Cn))
        assert n > 0
        val = torch.full((), float("nan"), dtype=torch.float64, device=DEV)
        scratch = torch.full((n // 8,), float("nan"), dtype=torch.float64, device=DEV)
    with ops._guard(DEV):
        _geo.check(L.mi_geo_lattice_tv(P3, R, Cn, ptr(v), ptr(mask), EPS, 0.0 if scale is None else scale, ptr(out), ptr(val), ptr(scratch), n,
                                       stream_ptr(DEV)), "mi_geo_lattice_tv")
    return out, val


def run_sp(P, s, mask, scale, d_s, value=True):
    L = _geo.lib()
    P3 = (C.c_int32 * 3)(*P)
    out = None if d_s is None else d_s.clone()
    val = scratch = None
    n = 0
    if value:
        n = int(L.mi_geo_lattice_scratch_bytes(P3, 1, 1))
        val = torch.full((), float("nan"), dtype=torch.float64, device=DEV)
        scratch = torch.full((n // 8,), float("nan"), dtype=torch.float64, device=DEV)
    with ops._guard(DEV):
        _geo.check(L.mi_geo_lattice_sparsity(P3, ptr(s), ptr(mask), 0.0 if scale is None else scale, ptr(out), ptr(val), ptr(scratch), n,
                                             stream_ptr(DEV)), "mi_geo_lattice_sparsity")
    return out, val


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def bits_np(t):
    return t.cpu().numpy().view(np.int32)


# ---------------------------------------------------------------------------------------------------
# total variation
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Cn", CHANNELS)
@pytest.mark.parametrize("P", LATTICES)
def test_tv_gradient_equals_the_fp32_restatement_bit_for_bit_and_the_value_meets_the_summation_bound(P, R, Cn):
    seed = 1000 * P[0] + 10 * P[2] + R
    worst = 0.0
    for k, kind in enumerate(INPUTS):
        v = make_input(P, R, Cn, kind, seed + k)
        d0 = np.random.default_rng(seed + 50 + k).normal(0.0, 1.0, v.shape).astype(f32)      # the add is tested; the padding holds values too
        v_d, d0_d = dev(v), dev(d0)
        for m, mkind in enumerate(MASKS):
            mask = make_mask(P, mkind, seed + 100 + m)
            ref = LR.tv(v, Cn, EPS, mask=mask, scale=SCALE, d_v=d0, dtype=np.float32)
            mask_d = dev(mask)
            got, val = run_tv(P, R, Cn, v_d, mask_d, SCALE, d0_d)
            what = (P, R, Cn, kind, mkind)
            assert np.array_equal(bits_np(got), ref["d"].view(np.int32)), what                # gradient, padding and unwritten elements: the same bits
            if R > 1:
                assert np.array_equal(bits_np(got[..., Cn:]), d0[..., Cn:].view(np.int32)), what
            unwritten = ~ref["written"]
            assert np.array_equal(bits_np(got)[unwritten], d0.view(np.int32)[unwritten]), what
            if mkind == "zeros":
                assert same_bits(got, d0_d) and float(val) == 0.0, what
            # the value: any-order summation bound against the exactly rounded sum of the fp32 terms
            n, total = ref["count"], float(ref["terms"].astype(np.float64).sum())
            bound = max(n - 1, 0) * 2.0 ** -53 * total
            err = abs(float(val) - ref["value"])
            assert err <= bound, (what, float(val), ref["value"], err, bound)
            worst = max(worst, err / bound if bound > 0 else 0.0)
            # two runs: identical bits, the value included; value-only and gradient-only agree with the combined call
            again, val2 = run_tv(P, R, Cn, v_d, mask_d, SCALE, d0_d)
            assert same_bits(again, got) and torch.equal(val.view(torch.int64), val2.view(torch.int64)), what
            _, only_v = run_tv(P, R, Cn, v_d, mask_d, None, None)
            only_g, none = run_tv(P, R, Cn, v_d, mask_d, SCALE, d0_d, value=False)
            assert torch.equal(only_v.view(torch.int64), val.view(torch.int64)) and same_bits(only_g, got) and none is None, what
            if kind == "constant region" and mkind == "none" and P[0] >= 10:
                assert (ref["terms"] == np.sqrt(f32(EPS))).any()                             # d = 0 exactly does occur: t = sqrtf(eps)
    print(f"\n[lattice TV {P} R={R} C={Cn}] worst value error / bound {worst:.3f}", end="")


def test_tv_with_no_output_is_a_no_op_and_masked_out_workgroups_write_nothing():
    P, R, Cn = (25, 25, 25), 32, 27
    v = make_input(P, R, Cn, "normal", 3)
    d0 = dev(np.random.default_rng(4).normal(0.0, 1.0, v.shape).astype(f32))
    out, val = run_tv(P, R, Cn, dev(v), None, None, None, value=False)
    assert out is None and val is None
    # one block set: its points and their forward neighbours move, every other workgroup leaves its elements alone
    mask = np.zeros(LR.mask_shape(P), np.uint8)
    mask[1, 1, 1] = 1
    got, val = run_tv(P, R, Cn, dev(v), dev(mask), SCALE, d0)
    ref = LR.tv(v, Cn, EPS, mask=mask, scale=SCALE, d_v=d0.cpu().numpy())
    assert np.array_equal(bits_np(got), ref["d"].view(np.int32)) and float(val) > 0
    changed = (bits_np(got) != bits_np(d0)).any(-1)
    assert changed[8:16, 8:16, 8:16].all() and not changed[~ref["written"]].any() and ref["written"].sum() == 8 ** 3 + 3 * 8 ** 2


# ---------------------------------------------------------------------------------------------------
# sparsity
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", LATTICES)
def test_sparsity_gradient_equals_the_fp32_restatement_bit_for_bit_and_the_value_meets_its_bound(P):
    seed = 77 * P[0] + P[2]
    worst = 0.0
    for k, kind in enumerate(INPUTS):
        s = make_input(P, 1, 1, kind, seed + k)
        d0 = np.random.default_rng(seed + 50 + k).normal(0.0, 1.0, s.shape).astype(f32)
        s_d, d0_d = dev(s), dev(d0)
        for m, mkind in enumerate(MASKS):
            mask = make_mask(P, mkind, seed + 100 + m)
            ref = LR.sparsity(s, mask=mask, scale=SCALE, d_sigma=d0, dtype=np.float32)
            mask_d = dev(mask)
            got, val = run_sp(P, s_d, mask_d, SCALE, d0_d)
            what = (P, kind, mkind)
            assert np.array_equal(bits_np(got), ref["d"].view(np.int32)), what
            if mkind == "zeros":
                assert same_bits(got, d0_d) and float(val) == 0.0, what
            n, total = ref["count"], float(np.abs(ref["terms"]).sum())
            bound = max(n - 1, 0) * 2.0 ** -53 * total + 4.0 * 2.0 ** -52 * total
            err = abs(float(val) - ref["value"])
            print(f"\n[lattice SP {what}] value {float(val):.17g}, float64 restatement {ref['value']:.17g}, error {err:.3e}, bound {bound:.3e}", end="")
            assert err <= bound, (what, float(val), ref["value"], err, bound)
            worst = max(worst, err / bound if bound > 0 else 0.0)
            again, val2 = run_sp(P, s_d, mask_d, SCALE, d0_d)
            assert same_bits(again, got) and torch.equal(val.view(torch.int64), val2.view(torch.int64)), what
            _, only_v = run_sp(P, s_d, mask_d, None, None)
            only_g, none = run_sp(P, s_d, mask_d, SCALE, d0_d, value=False)
            assert torch.equal(only_v.view(torch.int64), val.view(torch.int64)) and same_bits(only_g, got) and none is None, what
    print(f"\n[lattice SP {P}] worst value error / bound {worst:.3f}", end="")


# ---------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------
def _grid():
    from tests.test_gpu_vox import make_grid
    g, _, _ = make_grid("5x4x3", 4)
    h = baked.RadianceGrid(g.lo, g.hi, g.res, 4).allocate(DEV)
    h.sigma.copy_(g.sigma)
    h.coef.copy_(g.coef)
    return h.build_skip()


def test_wrappers_give_the_bits_of_the_direct_calls():
    h = _grid()
    P = h.points
    assert h.record_floats == 16 and sorted(P) == [4, 5, 6]
    mask = torch.ones_like(h.skip)
    for which, R, Cn in (("sigma", 1, 1), ("coef", 16, 12)):
        v = getattr(h, which)
        d0 = torch.from_numpy(np.random.default_rng(9).normal(0.0, 1.0, tuple(v.shape)).astype(f32)).to(DEV)
        for m, m_d in ((None, None), (True, h.skip), (mask, mask)):
            want_d, want_v = run_tv(P, R, Cn, v, m_d, 0.25, d0)
            out = d0.clone()
            val = baked_train.lattice_tv(h, which, mask=m, scale=0.25, out=out)
            assert val.dtype == torch.float64 and val.dim() == 0 and val.is_cuda
            assert same_bits(out, want_d) and torch.equal(val.view(torch.int64), want_v.view(torch.int64)), (which, m is None)
            assert torch.equal(baked_train.lattice_tv(h, which, mask=m).view(torch.int64), want_v.view(torch.int64))     # value alone
        # the default target is .grad, created as zeros when absent
        v.grad = None
        baked_train.lattice_tv(h, which, scale=0.25)
        assert same_bits(v.grad, run_tv(P, R, Cn, v, None, 0.25, torch.zeros_like(v))[0])
        v.grad = None
    d0 = torch.from_numpy(np.random.default_rng(10).normal(0.0, 1.0, P).astype(f32)).to(DEV)
    want_d, want_v = run_sp(P, h.sigma, h.skip, -1.5, d0)
    out = d0.clone()
    val = baked_train.lattice_sparsity(h, mask=True, scale=-1.5, out=out)
    assert same_bits(out, want_d) and torch.equal(val.view(torch.int64), want_v.view(torch.int64)) and float(val) > 0
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    for bad in (lambda: baked_train.lattice_tv(h, "rgb"), lambda: baked_train.lattice_tv(h, mask=torch.ones(2, 2, 2, dtype=torch.uint8, device=DEV)),
                lambda: baked_train.lattice_tv(h, mask=mask.cpu()), lambda: baked_train.lattice_tv(h, "coef", scale=1.0, out=torch.zeros_like(h.sigma)),
                lambda: baked_train.lattice_tv(h, out=torch.zeros_like(h.sigma)), lambda: baked_train.lattice_tv(h, eps=0.0),
                lambda: baked_train.lattice_tv(h.compact("fp32"))):
        with pytest.raises(MiNerfError):
            bad()


def _views():
    """The 6 views of 32 x 32 of tests/test_gpu_voxgrad.py."""
    scene = scenes.SolidScene.default()
    H = W = 32
    K = scenes.scaled_camera((H, W))
    rays = []
    for i in range(6):
        pose = torch.from_numpy(synthetic.pose_spherical(60.0 * i, -30.0, 4.0)).to(DEV)
        o, d = ops.make_o_d(W, H, K, pose, DEV)
        rays.append(torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1))
    rays = torch.cat(rays).contiguous()
    return rays, scene.render(rays, 2.0, 6.0)[0]


class _Counting:
    """Stands in for the loaded library: counts the calls of every entry it hands out."""

    def __init__(self, lib):
        self.lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def test_finetune_with_zero_weights_makes_no_geo_call_and_with_weights_makes_one_per_term_and_step(monkeypatch):
    rays, target = _views()
    proxy = _Counting(_geo.lib())
    monkeypatch.setattr(_geo, "lib", lambda: proxy)
    grid = baked.RadianceGrid(-1.2, 1.2, 24, B=4).allocate(DEV)
    baked_train.finetune(grid, rays, target, steps=3, skip=False, lr_sigma=LR_SIGMA)
    baked_train.finetune(grid, rays, target, steps=3, skip=False, lr_sigma=LR_SIGMA, tv_sigma=0.0, tv_coef=0.0, sparsity=0.0)
    assert proxy.calls == {}
    baked_train.finetune(grid, rays, target, steps=3, skip=False, lr_sigma=LR_SIGMA, tv_sigma=1.0, sparsity=1.0)
    assert proxy.calls == {"mi_geo_lattice_tv": 3, "mi_geo_lattice_sparsity": 3}
    baked_train.finetune(grid, rays, target, steps=2, lr_sigma=LR_SIGMA, tv_coef=1.0)
    assert proxy.calls == {"mi_geo_lattice_tv": 5, "mi_geo_lattice_sparsity": 3}


# ---------------------------------------------------------------------------------------------------
# the training effect.  The weights were chosen on the device (docs/design/24_lattice_regularisers.md has the sweep)
# ---------------------------------------------------------------------------------------------------
LR_SIGMA, STEPS, TV_SIGMA, SPARSITY = 0.5, 60, 0.01, 0.01


def test_regularised_training_from_nothing_lowers_tv_and_sparsity_and_still_learns():
    """24^3, B = 4, allocate(), skip=False, the 6 views of 32 x 32, 60 steps, seed 0, lr_sigma 0.5; tv_sigma = sparsity = 0.01.  Signs only.
    Measured when the weights were chosen: plain TV(sigma) 7 536, SP 3 064, data loss 0.1302 -> 0.0243 (first -> last tenth); regularised
    TV(sigma) 3 552, SP 2 304, data loss 0.1279 -> 0.0255.  (w = 1: 1 007 / 284, 0.0922 -> 0.0576; w = 100 no longer learns.)"""
    rays, target = _views()
    out = {}
    for name, kw in (("plain", {}), ("regularised", dict(tv_sigma=TV_SIGMA, sparsity=SPARSITY))):
        grid = baked.RadianceGrid(-1.2, 1.2, 24, B=4).allocate(DEV)
        losses = baked_train.finetune(grid, rays, target, steps=STEPS, skip=False, lr_sigma=LR_SIGMA, seed=0, **kw)
        tenth = STEPS // 10
        out[name] = dict(tv=float(baked_train.lattice_tv(grid, "sigma")), sp=float(baked_train.lattice_sparsity(grid)),
                         first=float(losses[:tenth].mean()), last=float(losses[-tenth:].mean()))
        print(f"\n[lattice training effect, 24^3 B=4 from nothing, {STEPS} steps, {name}] TV(sigma) {out[name]['tv']:.1f}, SP {out[name]['sp']:.1f}, "
              f"data loss first / last tenth {out[name]['first']:.5f} / {out[name]['last']:.5f}", end="")
        assert bool(torch.isfinite(losses).all()) and bool((grid.sigma >= 0).all())
    assert out["regularised"]["tv"] < out["plain"]["tv"] and out["regularised"]["sp"] < out["plain"]["sp"], out
    assert out["regularised"]["last"] < out["regularised"]["first"], out
    assert out["plain"]["tv"] > 0 and out["plain"]["sp"] > 0
