"""mi_vox_resample and mi_vox_prune on the GPU (THE RESAMPLING RULE and THE PRUNING RULE of include/mi_nerf_vox.h) against their numpy
restatement (tests/vox_refine_restate.py).  Both are gathers of fp32 products and sums in a stated order, with no transcendental: the
library must equal the fp32 restatement BIT FOR BIT, padding and sigma included, and twice over.  Then: refining keeps the picture on the
device, the grid objects' plumbing, and coarse-to-fine training from an empty grid."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import _vox, baked, baked_train, ops, scenes, synthetic
from nerf_pytorch_paeng_amd._lib import MiNerfError, dev_ptr, stream_ptr
from tests import vox_refine_restate as RR
from tests import vox_restate as VR
from tests import vox_sparse_restate as SR
from tests.test_gpu_vox import make_rays

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def c_grid(lo, hi, res):
    return _vox.Grid((C.c_float * 3)(*lo), (C.c_float * 3)(*hi), (C.c_int32 * 3)(*res))


def points(res):
    return tuple(int(r) + 1 for r in reversed(res))


def source(res, B, seed, poison=True):
    """(sigma, coef) numpy fp32: random density with zeros, random records; the padding poisoned with NaN -- it must never be read."""
    rng = np.random.default_rng(seed)
    P = points(res)
    sigma = np.where(rng.uniform(size=P) < 0.3, 0.0, rng.uniform(0.0, 12.0, P)).astype(f32)
    coef = np.full(P + (VR.record_floats(B),), np.nan if poison else 0.0, f32)
    coef[..., :3 * B] = rng.normal(0.0, 0.8, P + (3 * B,))
    return sigma, coef


def hip_resample(src, dst, B, sigma, coef):
    """One call of mi_vox_resample into arrays prefilled with NaN: an element that is not written shows."""
    s, c = torch.from_numpy(sigma).to(DEV), torch.from_numpy(coef).to(DEV)
    Pd = points(dst[2])
    sd = torch.full(Pd, math.nan, dtype=torch.float32, device=DEV)
    cd = torch.full(Pd + (VR.record_floats(B),), math.nan, dtype=torch.float32, device=DEV)
    gs, gd = c_grid(*src), c_grid(*dst)
    _vox.check(_vox.lib().mi_vox_resample(C.byref(gs), C.byref(gd), B, dev_ptr(s, "sigma"), dev_ptr(c, "coef", torch.float32, 16), dev_ptr(sd, "sigma_d"),
                                          dev_ptr(cd, "coef_d", torch.float32, 16), stream_ptr(DEV)), "mi_vox_resample")
    assert np.array_equal(bits(s.cpu().numpy()), bits(sigma)) and np.array_equal(bits(c.cpu().numpy()), bits(coef))      # the source is not modified
    return sd.cpu().numpy(), cd.cpu().numpy()


BOX = ((-1.0, -0.7, -0.5), (0.9, 1.3, 0.8))
# name -> ((lo_s, hi_s, res_s), (lo_d, hi_d, res_d))
RESAMPLE_CASES = {
    "1^3 -> 3^3": ((*BOX, (1, 1, 1)), (*BOX, (3, 3, 3))),
    "6^3 -> 12^3": ((*BOX, (6, 6, 6)), (*BOX, (12, 12, 12))),
    "(5,6,7) -> (9,4,20), up and down": ((*BOX, (5, 6, 7)), (*BOX, (9, 4, 20))),
    # 804 points x 8 threads at B = 9: 6432 threads, 25.1 workgroups; a row of 68 points is longer than a wave
    "(66,2,3) -> (67,3,4), a partial last workgroup": ((*BOX, (66, 2, 3)), (*BOX, (67, 3, 4))),
    "crop: the destination strictly inside": ((*BOX, (5, 6, 7)), ((-0.6, -0.1, -0.3), (0.55, 0.9, 0.45), (7, 3, 5))),
    "edge extension: the destination reaches outside on two faces": ((*BOX, (5, 6, 7)), ((-1.6, -0.7, -0.5), (0.9, 1.3, 1.4), (8, 5, 9))),
}


@pytest.mark.parametrize("B", (1, 4, 9))
@pytest.mark.parametrize("name", sorted(RESAMPLE_CASES))
def test_resample_equals_the_fp32_restatement_bit_for_bit(name, B):
    src, dst = RESAMPLE_CASES[name]
    sigma, coef = source(src[2], B, 30 + B)
    want_s, want_c = RR.resample(*src, *dst, B, sigma, coef, np.float32)
    got_s, got_c = hip_resample(src, dst, B, sigma, coef)
    assert got_s.shape == want_s.shape and got_c.shape == want_c.shape
    assert np.isfinite(got_s).all() and np.isfinite(got_c).all()                          # every element written, no padding leaked
    assert np.array_equal(bits(got_s), bits(want_s)), (name, B, int((bits(got_s) != bits(want_s)).sum()))
    assert np.array_equal(bits(got_c), bits(want_c)), (name, B, int((bits(got_c) != bits(want_c)).sum()))
    assert not got_c[..., 3 * B:].any()
    if name.startswith("edge"):
        # points beyond the faces x = lo and z = hi repeat the value on the face
        x_out = [j for j in range(dst[2][0] + 1) if f32(dst[0][0]) + f32(j) * ((f32(dst[1][0]) - f32(dst[0][0])) / f32(dst[2][0])) < f32(src[0][0])]
        assert len(x_out) >= 2 and all(np.array_equal(got_s[:, :, j], got_s[:, :, x_out[0]]) for j in x_out)
        assert np.array_equal(got_s[-1], got_s[-2]) and np.array_equal(got_c[-1], got_c[-2])
    again_s, again_c = hip_resample(src, dst, B, sigma, coef)
    assert np.array_equal(bits(again_s), bits(got_s)) and np.array_equal(bits(again_c), bits(got_c))      # deterministic


# ---------------------------------------------------------------------------------------------------
# prune
# ---------------------------------------------------------------------------------------------------
def hip_prune(res, B, tau, sigma, coef):
    s, c = torch.from_numpy(sigma).to(DEV), torch.from_numpy(coef).to(DEV)
    out = torch.full_like(s, math.nan)
    g = c_grid((-1.0,) * 3, (1.0,) * 3, res)
    _vox.check(_vox.lib().mi_vox_prune(C.byref(g), B, float(tau), dev_ptr(s, "sigma"), dev_ptr(out, "sigma_out"), dev_ptr(c, "coef", torch.float32, 16),
                                       stream_ptr(DEV)), "mi_vox_prune")
    assert np.array_equal(bits(s.cpu().numpy()), bits(sigma))                             # sigma_in is unchanged
    return out.cpu().numpy(), c.cpu().numpy()


def prune_fields(res, seed):
    """name -> (sigma, taus): one dense point at a corner, on an edge and in the interior (the clipped stencil); a random sparse field."""
    rng = np.random.default_rng(seed)
    P = points(res)
    out = {}
    for name, at in (("corner", (P[0] - 1, P[1] - 1, P[2] - 1)), ("edge", (0, P[1] - 1, P[2] // 2)), ("interior", (P[0] // 2, P[1] // 2, P[2] // 2))):
        s = np.zeros(P, f32)
        s[at] = 2.0
        out[name] = (s, (0.0, 1.0))
    s = np.where(rng.uniform(size=P) < 0.03, rng.uniform(0.05, 2.0, P), 0.0).astype(f32)
    out["sparse"] = (s, (0.0, 0.5, float(s.max())))
    return out


@pytest.mark.parametrize("B", (1, 4, 9))
@pytest.mark.parametrize("res", ((9, 12, 20), (66, 2, 3), (2, 2, 2)))
def test_prune_equals_its_restatement_byte_for_byte(res, B):
    rng = np.random.default_rng(40 + B)
    for name, (sigma, taus) in prune_fields(res, 41).items():
        coef = rng.normal(0.0, 1.0, sigma.shape + (VR.record_floats(B),)).astype(f32)       # the padding too: a kept record keeps every bit
        for tau in taus:
            want_s, want_c = RR.prune(sigma, coef, tau)
            got_s, got_c = hip_prune(res, B, tau, sigma, coef)
            assert np.array_equal(bits(got_s), bits(want_s)), (res, B, name, tau)
            assert np.array_equal(bits(got_c), bits(want_c)), (res, B, name, tau, int((bits(got_c) != bits(want_c)).sum()))
            keep = RR.kept_set(sigma, tau)
            assert np.array_equal(bits(got_c[keep]), bits(coef[keep])) and not got_c[~keep].any()
            if tau == 0.0:
                assert np.array_equal(keep, SR.active_set(sigma)) and np.array_equal(bits(got_s), bits(sigma))
            if name == "sparse" and tau == taus[-1]:
                assert not got_s.any() and not got_c.any()                                # tau >= max sigma clears everything
            if name != "sparse" and tau == 0.0:
                assert keep.sum() == {"corner": 8, "edge": 12, "interior": 27}[name]           # the stencil clipped to the lattice
            again_s, again_c = hip_prune(res, B, tau, sigma, coef)
            assert np.array_equal(bits(again_s), bits(got_s)) and np.array_equal(bits(again_c), bits(got_c))      # deterministic


# ---------------------------------------------------------------------------------------------------
# refining keeps the picture
# ---------------------------------------------------------------------------------------------------
def test_refining_keeps_the_picture_on_the_device():
    """A smooth random field on 6^3 (densities up to about 10, a third of the rays see through), its resample to 12^3, 257 rays at one
    explicit step: max |render(fine) - render(coarse)| over rgb, acc and depth.  The two grids hold the same trilinear field up to the
    rounding of the resample, so the difference is fp32 rounding alone.  The bar: the same difference formed by the fp32 restatements on
    the CPU (resample, then render, against render), times 4 for the device's expf and its different but legal evaluation of nothing
    else.  Measured: the fp32 restatements differ by 9.54e-07 (depth; rgb 3.3e-07, acc 3.6e-07), so the bar is 3.81e-06; the MI355X gives
    9.54e-07 (docs/design/25_coarse_to_fine.md, 25.5)."""
    B, lo, hi = 9, (-1.0, -0.8, -1.1), (1.0, 0.9, 1.0)
    rng = np.random.default_rng(50)
    z, y, x = np.meshgrid(*(np.linspace(0.0, 1.0, 7),) * 3, indexing="ij")
    ph = rng.uniform(0.0, 2.0 * np.pi, 6)
    smooth = np.cos(2.1 * x + ph[0]) * np.cos(1.7 * y + ph[1]) + np.cos(2.6 * z + ph[2]) * np.cos(1.3 * x + 2.2 * y + ph[3])
    sigma = (5.0 * np.clip(smooth, 0.0, None)).astype(f32)
    coef = np.zeros((7, 7, 7, 32), f32)
    for t in range(27):
        a = rng.uniform(0.5, 2.5, 3)
        coef[..., t] = 0.5 * np.cos(a[0] * x + a[1] * y + a[2] * z + rng.uniform(0.0, 6.0))
    coef[..., :3] += f32(0.5 / VR.C0)
    rays = make_rays(lo, hi, 257, 51)
    step, near, far = 0.07, 0.3, 3.2
    fine_s, fine_c = RR.resample(lo, hi, (6,) * 3, lo, hi, (12,) * 3, B, sigma, coef, np.float32)
    ref_c = VR.render(lo, hi, (6,) * 3, B, sigma, coef, rays, step, near, far, dtype=np.float32)
    ref_f = VR.render(lo, hi, (12,) * 3, B, fine_s, fine_c, rays, step, near, far, dtype=np.float32)
    d_ref = max(float(np.abs(ref_f[k].astype(np.float64) - ref_c[k]).max()) for k in ("rgb", "acc", "depth"))
    assert 0.2 < (ref_c["acc"] > 0.05).mean() and (ref_c["acc"] < 0.99).mean() > 0.2 and float(sigma.max()) > 5.0      # density of order 10, not saturated
    g = baked.RadianceGrid(lo, hi, 6, B).allocate(DEV)
    g.sigma.copy_(torch.from_numpy(sigma))
    g.coef.copy_(torch.from_numpy(coef))
    g.build_skip()
    h = g.resample(12)
    assert np.array_equal(bits(h.sigma.cpu().numpy()), bits(fine_s)) and np.array_equal(bits(h.coef.cpu().numpy()), bits(fine_c))
    r = torch.from_numpy(rays).to(DEV)
    out_c, out_f = g.render(r, step=step, near=near, far=far), h.render(r, step=step, near=near, far=far)
    d_hip = max(float((out_f[i].double() - out_c[i].double()).abs().max()) for i in (0, 2, 3))
    print(f"\n[vox refine 6^3 -> 12^3 B=9, 257 rays, step {step}] max |fine - coarse| over rgb, acc, depth: device {d_hip:.3e}, fp32 restatement {d_ref:.3e}, "
          f"allowed {4.0 * d_ref:.3e}", end="")
    assert d_ref > 0.0 and d_hip <= 4.0 * d_ref, (d_hip, d_ref)


# ---------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------
def test_the_grid_objects_resample_prune_refuse_and_compact():
    sigma, coef = source((9, 12, 20), 4, 60, poison=False)
    sigma[:, :, 4:] = 0.0                                                                # the far part of the box empty: the skip plane has zeros
    sigma[(sigma > 0) & (sigma < 11.0)] *= 0.01                                          # fog below 0.11 around a few dense points
    g = baked.RadianceGrid(-1.0, (1.0, 0.6, 1.4), (9, 12, 20), 4).allocate(DEV)
    g.sigma.copy_(torch.from_numpy(sigma))
    g.coef.copy_(torch.from_numpy(coef))
    g.build_skip()
    keep = (g.sigma.clone(), g.coef.clone(), g.skip.clone())
    h = g.resample((18, 7, 40))
    assert type(h) is baked.RadianceGrid and h is not g and h.res == (18, 7, 40) and (h.lo, h.hi, h.B) == (g.lo, g.hi, 4) and h.sigma.device == g.sigma.device
    assert h.sigma.shape == (41, 8, 19) and h.coef.shape == (41, 8, 19, 16) and h.skip.dtype == torch.uint8
    assert np.array_equal(h.skip.cpu().numpy(), VR.build_skip(h.sigma.cpu().numpy(), h.res)) and 0 < int(h.skip.sum()) < h.skip.numel()
    assert all(torch.equal(a, b) for a, b in zip(keep, (g.sigma, g.coef, g.skip)))        # the original is untouched
    want_s, want_c = RR.resample(g.lo, g.hi, g.res, h.lo, h.hi, h.res, 4, sigma, coef, np.float32)
    assert np.array_equal(bits(h.sigma.cpu().numpy()), bits(want_s)) and np.array_equal(bits(h.coef.cpu().numpy()), bits(want_c))
    crop = g.resample(5, lo=(-0.5, -0.5, -0.5), hi=0.5)
    assert crop.res == (5, 5, 5) and crop.lo == (-0.5,) * 3 and crop.hi == (0.5,) * 3
    before = g.compact().count
    assert g.prune(0.5) is g
    want_s, want_c = RR.prune(sigma, coef, 0.5)
    assert np.array_equal(bits(g.sigma.cpu().numpy()), bits(want_s)) and np.array_equal(bits(g.coef.cpu().numpy()), bits(want_c))
    assert np.array_equal(g.skip.cpu().numpy(), VR.build_skip(want_s, g.res))
    after = g.compact().count
    print(f"\n[vox refine plumbing] records of the compact grid: {before} before prune(0.5), {after} after", end="")
    assert 0 < after < before
    for storage in ("fp32", "f16"):
        small = g.compact(storage)
        with pytest.raises(MiNerfError, match="refine the dense grid, then compact"):
            small.resample(8)
        with pytest.raises(MiNerfError, match="refine the dense grid, then compact"):
            small.prune(0.5)
    with pytest.raises(MiNerfError, match="tau"):
        g.prune(-1.0)
    with pytest.raises(MiNerfError):
        g.resample(513)
    with pytest.raises(MiNerfError, match="holds nothing"):
        baked.RadianceGrid(-1.0, 1.0, 4, 1).resample(8)


# ---------------------------------------------------------------------------------------------------
# it learns
# ---------------------------------------------------------------------------------------------------
def test_coarse_to_fine_from_an_empty_grid_learns():
    """SolidScene.default(), B = 4, 6 views of 32 x 32, an empty 12^3 grid, 40 steps at 12^3 and 40 at 24^3: the batch loss falls, and the
    grid that comes back is the fine one, in order.  Beside it the same 80 steps at 24^3 alone: reported, not asserted
    (docs/design/25_coarse_to_fine.md)."""
    scene = scenes.SolidScene.default()
    H = W = 32
    K = scenes.scaled_camera((H, W))
    rays = []
    for i in range(6):
        pose = torch.from_numpy(synthetic.pose_spherical(60.0 * i, -30.0, 4.0)).to(DEV)
        o, d = ops.make_o_d(W, H, K, pose, DEV)
        rays.append(torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1))
    rays = torch.cat(rays).contiguous()
    target = scene.render(rays, 2.0, 6.0)[0]
    start = baked.RadianceGrid(-1.2, 1.2, 12, B=4).allocate(DEV)
    grid, losses = baked_train.coarse_to_fine(start, rays, target, [(12, 40), (24, 40)], lr_sigma=0.5, skip=(False, True), seed=0)
    assert losses.shape == (80,) and losses.is_cuda and bool(torch.isfinite(losses).all())
    first, last = float(losses[:8].mean()), float(losses[-8:].mean())
    assert last < first, (first, last)
    assert grid is not start and grid.res == (24, 24, 24) and start.res == (12, 12, 12) and grid.sigma.shape == (25, 25, 25)
    assert bool((grid.sigma >= 0).all()) and bool(torch.isfinite(grid.sigma).all()) and bool(torch.isfinite(grid.coef).all())
    assert not grid.sigma.requires_grad and grid.sigma.grad is None and grid.coef.grad is None and start.sigma.grad is None
    assert np.array_equal(grid.skip.cpu().numpy(), VR.build_skip(grid.sigma.cpu().numpy(), grid.res))    # the plane describes the sigma left behind
    mse = float(torch.mean((grid.render(rays)[0] - target) ** 2))
    alone = baked.RadianceGrid(-1.2, 1.2, 24, B=4).allocate(DEV)
    l_alone = baked_train.finetune(alone, rays, target, steps=80, lr_sigma=0.5, skip=False, seed=0)
    mse_alone = float(torch.mean((alone.render(rays)[0] - target) ** 2))
    print(f"\n[vox refine coarse to fine 12^3 -> 24^3 B=4, 6 x 32 x 32, 40 + 40 steps] batch loss, mean of the first / last tenth {first:.5f} / {last:.5f}; "
          f"MSE on the training rays {mse:.5f} ({-10 * math.log10(mse):.2f} dB), {int(grid.skip.sum())} of {grid.skip.numel()} blocks occupied; "
          f"80 steps at 24^3 alone: last tenth {float(l_alone[-8:].mean()):.5f}, MSE {mse_alone:.5f} ({-10 * math.log10(mse_alone):.2f} dB), "
          f"{int(alone.skip.sum())} of {alone.skip.numel()} blocks occupied", end="")
    # per-level values and their refusals
    with pytest.raises(MiNerfError, match="per level"):
        baked_train.coarse_to_fine(start, rays, target, [(12, 1), (24, 1)], skip=(False, True, True))
    with pytest.raises(MiNerfError, match="levels"):
        baked_train.coarse_to_fine(start, rays, target, [12, 24])
    with pytest.raises(MiNerfError, match="tau"):
        baked_train.coarse_to_fine(start, rays, target, [(12, 1)], prune=-1.0)
    with pytest.raises(MiNerfError, match="compact"):
        baked_train.coarse_to_fine(start.compact(), rays, target, [(12, 1)])
    pruned, l2 = baked_train.coarse_to_fine(grid, rays, target, [(24, 2)], prune=(1.0,), batch=(512,), lr_coef=0.005)
    assert pruned is grid and l2.shape == (2,) and np.array_equal(grid.skip.cpu().numpy(), VR.build_skip(grid.sigma.cpu().numpy(), grid.res))
    assert not grid.coef[~torch.from_numpy(RR.kept_set(grid.sigma.cpu().numpy(), 0.0)).to(DEV)].any()    # records of inactive points are zero again
