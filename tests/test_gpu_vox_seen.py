"""Pruning by visibility on the GPU (mi_vox_shadow, mi_vox_seen, mi_vox_prune_seen: THE SHADOW RULE, THE VISIBILITY RULE and THE SEEN
PRUNING RULE of include/mi_nerf_vox.h) against their numpy restatement (tests/vox_seen_restate.py).  The three are gathers of fp32 products
and sums in a stated order with no transcendental: the library must equal the fp32 restatement BIT FOR BIT, and twice over.  Views are
23 x 19 pixels (437 rays: no multiple of 8 or of a workgroup's 32), the lattices the siblings' 17 x 9 x 33 (6120 points: no multiple of
256) and 5 x 4 x 3; then a 24^3 ball whose hidden interior goes while its picture stays, and the grid objects' plumbing."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import _vox, baked, baked_train
from nerf_pytorch_paeng_amd._lib import MiNerfError, dev_ptr, stream_ptr
from tests import vox_refine_restate as RR
from tests import vox_restate as VR
from tests import vox_seen_restate as SR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32
H, W = 19, 23
KMAT = [[70.0, 0.0, 11.0], [0.0, 70.0, 9.0], [0.0, 0.0, 1.0]]
BOX = ((-1.0, -0.7, -0.5), (0.9, 1.3, 0.8))
GRIDS = {"17x9x33": (17, 9, 33), "5x4x3": (5, 4, 3)}
CENTRE = (-0.05, 0.3, 0.15)
# five cameras around the box (one along an axis: direction components that are exactly 0; one close enough for the near face to leave
# the frustum) and one that looks away from it
EYES = [((-4.0, 0.3, 0.15), CENTRE, (0.0, 0.0, 1.0)), ((2.5, 3.0, 2.0), CENTRE, (0.0, 0.0, 1.0)), ((0.5, -3.5, -1.0), (0.0, 0.2, 0.1), (0.0, 0.0, 1.0)),
        ((-0.05, 0.3, 4.0), CENTRE, (0.0, 1.0, 0.0)), ((1.6, 1.9, 1.2), (0.2, 0.5, 0.3), (0.0, 0.0, 1.0))]
AWAY = ((-4.0, 0.3, 0.15), (-8.0, 0.3, 0.15), (0.0, 0.0, 1.0))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def poses(eyes):
    return np.stack([SR.look_at(*e) for e in eyes])


def points(res):
    return tuple(int(r) + 1 for r in reversed(res))


def field(res, seed):
    """sigma numpy fp32: random density with zeros, and an empty far part so that the skip plane has zeros."""
    rng = np.random.default_rng(seed)
    P = points(res)
    sigma = np.where(rng.uniform(size=P) < 0.3, 0.0, rng.uniform(0.0, 12.0, P)).astype(f32)
    sigma[:, :, (2 * P[2]) // 3:] = 0.0
    return sigma


def grid_of(res, sigma, B=1, coef=None):
    g = baked.RadianceGrid(*BOX, res, B).allocate(DEV)
    g.sigma.copy_(torch.from_numpy(sigma))
    if coef is not None:
        g.coef.copy_(torch.from_numpy(coef))
    return g.build_skip()


def hip_shadow(g, view, skip):
    """One call of mi_vox_shadow into a volume prefilled with NaN: an element that is not written shows."""
    tvol = torch.full((view.H, view.W, view.slices), math.nan, dtype=torch.float32, device=DEV)
    c = g.c_grid()
    _vox.check(_vox.lib().mi_vox_shadow(C.byref(c), dev_ptr(g.sigma, "sigma"), dev_ptr(g.skip, "skip", torch.uint8, 1) if skip else None, C.byref(view),
                                        dev_ptr(tvol, "tvol", torch.float32, 32), stream_ptr(DEV)), "mi_vox_shadow")
    return tvol


def hip_seen(g, view, tvol, bias, od):
    c = g.c_grid()
    _vox.check(_vox.lib().mi_vox_seen(C.byref(c), C.byref(view), dev_ptr(tvol, "tvol", torch.float32, 32), bias, dev_ptr(od, "od"), stream_ptr(DEV)),
               "mi_vox_seen")
    return od


@pytest.fixture(scope="module")
def cases():
    """name -> (grid on the device, sigma, the ctypes views of the five cameras and the one that looks away, their fp32 restated tvol):
    computed once, shared, left unchanged."""
    out = {}
    for name, res in GRIDS.items():
        sigma = field(res, 70 + res[0])
        g = grid_of(res, sigma)
        views = g.view_slices(baked.Views(H, W, KMAT, poses(EYES + [AWAY])))
        want = [SR.shadow(*BOX, res, sigma, SR.View.from_c(v), np.float32) for v in views]
        out[name] = (g, sigma, views, want)
    return out


# ---------------------------------------------------------------------------------------------------
# 1. the shadow volume
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_shadow_equals_the_fp32_restatement_bit_for_bit_with_and_without_the_skip_plane(cases, name):
    g, sigma, views, want = cases[name]
    assert 0 < int(g.skip.sum()) < g.skip.numel() or name == "5x4x3"
    for n, (v, ref) in enumerate(zip(views, want)):
        assert v.slices % 8 == 0 and ref.shape == (H, W, v.slices)
        on, off = hip_shadow(g, v, True).cpu().numpy(), hip_shadow(g, v, False).cpu().numpy()
        assert np.isfinite(on).all() and np.isfinite(off).all(), (name, n)                 # every element written
        assert np.array_equal(bits(on), bits(off)), (name, n)
        assert np.array_equal(bits(on), bits(ref)), (name, n, int((bits(on) != bits(ref)).sum()), float(np.abs(on - ref).max()))
        assert not on[:, :, 0].any() and (np.diff(on, axis=2) >= 0).all()
        if n < len(EYES):
            assert on.max() > 1.0, (name, n)                                               # the camera does look through density
        else:
            assert not on.any()                                                            # the one that looks away
    # a view of 1 x 1 pixels and 8 slices: one group, one store
    tiny = _vox.View(1, 1, 70.0, 70.0, 0.0, 0.0, views[0].c2w, views[0].depth_near, views[0].depth_step, 8)
    got = hip_shadow(g, tiny, True).cpu().numpy()
    assert np.array_equal(bits(got), bits(SR.shadow(*BOX, GRIDS[name], sigma, SR.View.from_c(tiny), np.float32)))


# ---------------------------------------------------------------------------------------------------
# 2., 3. the od plane
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_the_od_plane_equals_the_restatement_in_any_order_of_the_views_and_twice(cases, name):
    g, sigma, views, tv = cases[name]
    res = GRIDS[name]
    cams = baked.Views(H, W, KMAT, poses(EYES + [AWAY]))
    want = np.full(points(res), np.inf, f32)
    for v, t in zip(views, tv):
        want = SR.seen(*BOX, res, SR.View.from_c(v), t, 2, want, np.float32)
    got = g.seen(cams)
    assert got.shape == g.sigma.shape and got.dtype == torch.float32
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)), int((bits(got.cpu().numpy()) != bits(want)).sum())
    assert torch.equal(g.seen(cams), got) and torch.equal(g.seen(cams, skip=False), got)                      # twice; without the plane
    order = [3, 5, 0, 4, 2, 1]
    assert torch.equal(g.seen(baked.Views(H, W, KMAT, poses(EYES + [AWAY])[order])), got)                     # a minimum knows no order
    unseen = np.isinf(want)
    if name == "17x9x33":
        assert 0 < unseen.sum() < unseen.size                                              # points outside every frustum stay +inf
    assert (want[~unseen] >= 0).all() and (want == 0).any()
    away = g.seen(baked.Views(H, W, KMAT, poses([AWAY])))
    assert bool(torch.isinf(away).all()) and bool((away > 0).all())                        # the camera that looks away sees nothing
    # out= is filled afresh and returned
    buf = torch.zeros_like(got)
    assert g.seen(cams, out=buf) is buf and torch.equal(buf, got)


@pytest.mark.parametrize("bias", (0, 2, 5))
def test_the_bias_shifts_the_slice_and_clamps_at_the_first(cases, bias):
    g, sigma, views, tv = cases["17x9x33"]
    res = GRIDS["17x9x33"]
    for n in (0, 1, 4):
        view = SR.View.from_c(views[n])
        od = torch.full(points(res), math.inf, dtype=torch.float32, device=DEV)
        got = hip_seen(g, views[n], torch.from_numpy(tv[n]).to(DEV), bias, od).cpu().numpy()
        want = SR.seen(*BOX, res, view, tv[n], bias, np.full(points(res), np.inf, f32), np.float32)
        assert np.array_equal(bits(got), bits(want)), (bias, n)
        look, fi, fj, k0 = SR.looked_at(*BOX, res, view, np.float32)
        early = look & (k0 - bias < 0)
        assert not got[early].any() and np.isinf(got[~look]).all()                         # k - bias < 0 gives 0
        if bias == 5:
            assert early.any()
        # a plane that holds values already keeps its smaller ones
        half = np.where(np.arange(got.size).reshape(got.shape) % 2 == 0, f32(0.125), f32(np.inf))
        again = hip_seen(g, views[n], torch.from_numpy(tv[n]).to(DEV), bias, torch.from_numpy(half).to(DEV)).cpu().numpy()
        assert np.array_equal(bits(again), bits(np.fmin(half, want)))


# ---------------------------------------------------------------------------------------------------
# 4. prune_seen
# ---------------------------------------------------------------------------------------------------
def hip_prune(res, B, tau, od_max, sigma, coef, od):
    """mi_vox_prune_seen, or mi_vox_prune with od None."""
    s, c = torch.from_numpy(sigma).to(DEV), torch.from_numpy(coef).to(DEV)
    out = torch.full_like(s, math.nan)
    g = _vox.Grid((C.c_float * 3)(*BOX[0]), (C.c_float * 3)(*BOX[1]), (C.c_int32 * 3)(*res))
    if od is None:
        _vox.check(_vox.lib().mi_vox_prune(C.byref(g), B, float(tau), dev_ptr(s, "sigma"), dev_ptr(out, "sigma_out"), dev_ptr(c, "coef", torch.float32, 16),
                                           stream_ptr(DEV)), "mi_vox_prune")
    else:
        o = torch.from_numpy(od).to(DEV)
        _vox.check(_vox.lib().mi_vox_prune_seen(C.byref(g), B, float(tau), float(od_max), dev_ptr(s, "sigma"), dev_ptr(o, "od"), dev_ptr(out, "sigma_out"),
                                                dev_ptr(c, "coef", torch.float32, 16), stream_ptr(DEV)), "mi_vox_prune_seen")
        assert np.array_equal(bits(o.cpu().numpy()), bits(od))                             # od is read only
    assert np.array_equal(bits(s.cpu().numpy()), bits(sigma))                              # sigma_in is unchanged
    return out.cpu().numpy(), c.cpu().numpy()


@pytest.mark.parametrize("B", (1, 4, 9))
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_prune_seen_is_prune_under_an_infinite_od_max_and_its_restatement_under_a_finite_one(cases, name, B):
    g, _, views, tv = cases[name]
    res = GRIDS[name]
    rng = np.random.default_rng(80 + B)
    P = points(res)
    sigma = np.where(rng.uniform(size=P) < 0.06, rng.uniform(0.05, 2.0, P), 0.0).astype(f32)
    coef = rng.normal(0.0, 1.0, P + (VR.record_floats(B),)).astype(f32)                    # the canary: padding too, a kept record keeps every bit
    od = np.where(rng.uniform(size=P) < 0.3, np.inf, rng.uniform(0.0, 12.0, P)).astype(f32)
    for tau in (0.0, 0.5):
        plain_s, plain_c = hip_prune(res, B, tau, None, sigma, coef, None)
        got_s, got_c = hip_prune(res, B, tau, math.inf, sigma, coef, od)
        assert np.array_equal(bits(got_s), bits(plain_s)) and np.array_equal(bits(got_c), bits(plain_c)), (name, B, tau)
        for od_max in (6.9, 0.0):
            want_s, want_c = SR.prune_seen(sigma, coef, tau, od_max, od)
            keep = SR.kept_seen_set(sigma, tau, od_max, od)
            got_s, got_c = hip_prune(res, B, tau, od_max, sigma, coef, od)
            assert np.array_equal(got_s != 0, keep & (sigma != 0)) and np.array_equal(bits(got_s), bits(want_s)), (name, B, tau, od_max)
            assert np.array_equal(bits(got_c), bits(want_c)), (name, B, tau, od_max, int((bits(got_c) != bits(want_c)).sum()))
            assert np.array_equal(bits(got_c[keep]), bits(coef[keep])) and not got_c[~keep].any()
            if od_max == 6.9:
                assert 0 < keep.sum() < RR.kept_set(sigma, tau).sum()
            again_s, again_c = hip_prune(res, B, tau, od_max, sigma, coef, od)
            assert np.array_equal(bits(again_s), bits(got_s)) and np.array_equal(bits(again_c), bits(got_c))      # deterministic
    nan_od = np.where(sigma > 0, f32(np.nan), od)                                          # a NaN od is no seed
    got_s, got_c = hip_prune(res, B, 0.0, math.inf, sigma, coef, nan_od)
    assert not got_s.any() and not got_c.any()


# ---------------------------------------------------------------------------------------------------
# 5. the ball
# ---------------------------------------------------------------------------------------------------
BALL_RES, BALL_B, BALL_SIGMA, BALL_RADIUS, BALL_F = 24, 4, 64.0, 0.6, 50.0
BALL_K = [[BALL_F, 0.0, 11.0], [0.0, BALL_F, 9.0], [0.0, 0.0, 1.0]]
BALL_EYES = [((4.0 * s if a == 0 else 0.0, 4.0 * s if a == 1 else 0.0, 4.0 * s if a == 2 else 0.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0) if a == 2 else (0.0, 0.0, 1.0))
             for a in range(3) for s in (-1.0, 1.0)]


def ball():
    """(sigma, coef) numpy fp32 of the 24^3 grid on [-1, 1]^3: density 64 at the lattice points within 0.6 of the centre, a smooth colour
    with a first-degree part everywhere."""
    x = np.linspace(-1.0, 1.0, BALL_RES + 1)
    z, y, xx = np.meshgrid(x, x, x, indexing="ij")
    sigma = np.where(np.sqrt(xx * xx + y * y + z * z) < BALL_RADIUS, BALL_SIGMA, 0.0).astype(f32)
    coef = np.zeros(sigma.shape + (16,), f32)
    coef[..., 0], coef[..., 1], coef[..., 2] = (0.5 + 0.3 * xx) / VR.C0, (0.5 + 0.3 * y) / VR.C0, (0.5 - 0.3 * z) / VR.C0
    coef[..., 3:12] = 0.2 * np.cos(2.0 * xx + 1.0 * y + 3.0 * z)[..., None] * np.linspace(-1.0, 1.0, 9)
    return sigma, coef


def ball_rays(views):
    """rays [6 * 437, 6] fp32: the views' own pixel rays, by the restatement of THE SHADOW RULE."""
    out = []
    for v in views:
        o, d, _ = SR.pixel_rays(v, np.float32)
        out.append(np.concatenate([np.broadcast_to(o[None, :], (d[0].size, 3)), np.stack(d, 1)], 1))
    return np.concatenate(out).astype(f32)


def ball_reference(views, step, T_vis=1e-3, bias=2):
    """The restatement's side of the ball: (sigma, coef, pruned sigma, pruned coef, d_ref) with d_ref the largest change of rgb and acc
    over the six views in float64 (vox_restate.render on the grid and on the restated pruned grid)."""
    sigma, coef = ball()
    lo, hi, res = (-1.0,) * 3, (1.0,) * 3, (BALL_RES,) * 3
    od = SR.seen_all(lo, hi, res, sigma, views, bias, np.float32)
    ps, pc = SR.prune_seen(sigma, coef, 0.0, f32(-math.log(T_vis)), od)
    rays = ball_rays(views)
    a = VR.render(lo, hi, res, BALL_B, sigma, coef, rays, step, 0.0, math.inf, dtype=np.float64)
    b = VR.render(lo, hi, res, BALL_B, ps, pc, rays, step, 0.0, math.inf, dtype=np.float64)
    d_ref = max(float(np.abs(a[k] - b[k]).max()) for k in ("rgb", "acc"))
    return sigma, coef, ps, pc, od, rays, d_ref


def test_the_ball_loses_its_hidden_interior_and_keeps_its_picture():
    """24^3, sigma = 64 inside radius 0.6 of a +-1 box, B = 4, six axis views of 23 x 19 pixels from distance 4, T_vis = 1e-3, bias = 2.
    The restatement on the CPU (float64 renders of the grid and of the restated pruned grid) gives d_ref = 3.10e-07: 1345 of the 1551
    points with density keep it and 2663 of 2705 active points stay active (the stencil keeps one lattice step around every seed, so
    only the core goes).  What goes lies behind an optical depth of 6.9 and two slices of bias; at sigma * step = 64 / 24 = 2.7 per
    sample its weight in a picture is of that order (docs/design/27_grid_visibility.md, 27.5).  The device renders before and after
    may differ by 2 d_ref + 1e-5."""
    g = baked.RadianceGrid(-1.0, 1.0, BALL_RES, BALL_B).allocate(DEV)
    cams = baked.Views(H, W, BALL_K, poses(BALL_EYES))
    step = 0.5 * g.cell_edge()
    views = [SR.View.from_c(v) for v in g.view_slices(cams)]
    sigma, coef, ps, pc, od, rays, d_ref = ball_reference(views, step)
    print(f"\n[vox seen ball 24^3 B=4, 6 x 23 x 19] d_ref {d_ref:.3e}", end="")
    assert d_ref < 1e-2, d_ref                                                             # a restatement that prunes visible matter cannot pass
    g.sigma.copy_(torch.from_numpy(sigma))
    g.coef.copy_(torch.from_numpy(coef))
    g.build_skip()
    r = torch.from_numpy(rays).to(DEV)
    before = g.render(r, step=step)
    n_before = g.compact().count
    seen = g.seen(cams)
    assert np.array_equal(bits(seen.cpu().numpy()), bits(od))
    assert g.prune(0.0, seen=seen) is g
    n_after = g.compact().count
    after = g.render(r, step=step)
    want_before, want_after = int(RR.kept_set(sigma, 0.0).sum()), int(RR.kept_set(ps, 0.0).sum())
    print(f", active points {n_before} -> {n_after} (restated {want_before} -> {want_after})", end="")
    assert n_before == want_before and n_after == want_after and n_after < n_before
    assert np.array_equal(bits(g.sigma.cpu().numpy()), bits(ps)) and np.array_equal(bits(g.coef.cpu().numpy()), bits(pc))
    assert np.array_equal(g.skip.cpu().numpy(), VR.build_skip(ps, g.res))
    d_hip = max(float((after[i].double() - before[i].double()).abs().max()) for i in (0, 2))
    print(f", device max |after - before| over rgb, acc {d_hip:.3e}, allowed {2 * d_ref + 1e-5:.3e}", end="")
    assert float(before[2].max()) > 0.99 and d_hip <= 2.0 * d_ref + 1e-5, (d_hip, d_ref)


# ---------------------------------------------------------------------------------------------------
# 6. plumbing
# ---------------------------------------------------------------------------------------------------
def test_the_python_surface_views_out_coarse_to_fine_and_the_compact_grids_refusal():
    p34 = poses(BALL_EYES)
    p44 = np.concatenate([p34, np.broadcast_to(np.array([0, 0, 0, 1], f32), (6, 1, 4))], 1)
    a, b = baked.Views(H, W, BALL_K, torch.from_numpy(p44).to(DEV)), baked.Views(H, W, torch.tensor(BALL_K), p34)
    assert len(a) == len(b) == 6 and np.array_equal(a.poses, b.poses)
    sigma, coef = ball()
    g = baked.RadianceGrid(-1.0, 1.0, BALL_RES, BALL_B).allocate(DEV)
    g.sigma.copy_(torch.from_numpy(sigma))
    g.coef.copy_(torch.from_numpy(coef))
    g.build_skip()
    od = g.seen(a)
    buf = torch.empty_like(od)
    assert g.seen(b, out=buf) is buf and torch.equal(buf, od)
    assert torch.equal(g.seen(a, bias=0, out=buf), buf) and bool((buf >= od).all()) and not torch.equal(buf, od)    # less bias hides more
    with pytest.raises(MiNerfError, match="out must be"):
        g.seen(a, out=torch.empty(3, 3, 3, device=DEV))
    with pytest.raises(MiNerfError, match="bias"):
        g.seen(a, bias=-1)
    for storage in ("fp32", "f16"):
        with pytest.raises(MiNerfError, match="refine the dense grid, then compact"):
            g.compact(storage).prune(0.0, seen=od)
    with pytest.raises(MiNerfError, match="T_vis"):
        g.prune(0.0, seen=od, T_vis=-0.5)
    # T_vis = 0 asks nothing of the view: the plain rule
    h = baked.RadianceGrid(-1.0, 1.0, BALL_RES, BALL_B).allocate(DEV)
    h.sigma.copy_(g.sigma), h.coef.copy_(g.coef)
    h.prune(0.5, seen=od.fill_(0.0), T_vis=0.0)
    g.prune(0.5)
    assert torch.equal(h.sigma, g.sigma) and torch.equal(h.coef, g.coef) and torch.equal(h.skip, g.skip)
    # coarse to fine with the training views: a few steps on 12^3 -> 24^3; afterwards no record at a point that is not active
    rays = torch.from_numpy(ball_rays([SR.View.from_c(v) for v in g.view_slices(a)])).to(DEV)
    target = g.render(rays)[0].contiguous()
    start = baked.RadianceGrid(-1.0, 1.0, 12, BALL_B).allocate(DEV)
    grid, losses = baked_train.coarse_to_fine(start, rays, target, [(12, 6), (24, 6)], lr_sigma=0.5, skip=(False, True), seed=0, prune_views=a, prune_T=1e-3)
    assert grid.res == (24, 24, 24) and losses.shape == (12,) and bool(torch.isfinite(losses).all())
    active = torch.from_numpy(RR.kept_set(grid.sigma.cpu().numpy(), 0.0)).to(DEV)
    assert not grid.coef[~active].any() and np.array_equal(grid.skip.cpu().numpy(), VR.build_skip(grid.sigma.cpu().numpy(), grid.res))
    with pytest.raises(MiNerfError, match="Views"):
        baked_train.coarse_to_fine(start, rays, target, [(12, 1)], prune_views=p34)
