"""The backward pass of the radiance-grid renderer on the GPU (include/mi_nerf_voxgrad.h, nerf_pytorch_paeng_amd/baked_train.py) against the
numpy restatement of the header's rule (tests/voxgrad_restate.py), on the grids, seeded arrays and ray mix of tests/test_gpu_vox.py.

The forward the backward recomputes equals RadianceGrid.render bit for bit.  The bar for a gradient array: with
e(x) = max over the elements with A > 0 of |x - g64| / A (A the sum of the absolute contributions to the element),
    e_hip <= 4 e_ref + c_max * 2^-24,
e_ref the float32 restatement's (summing in ray, then sample order), and c_max * 2^-24 the bound for summing c fp32 terms in ANY order --
the library's sums are atomic adds, whose order is not fixed.  Elements with A = 0 are exactly 0 and the padding is never written.  No ray
is excluded.  Measured e_hip / e_ref pairs: docs/design/23_radiance_grid_training.md."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import baked, baked_train, scenes, synthetic, ops
from nerf_pytorch_paeng_amd._lib import MiNerfError
from tests import vox_restate as VR
from tests import voxgrad_restate as VG
from tests.test_gpu_vox import CFG, GRID_SPECS, make_grid, make_rays

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32
N_RAYS = (1, 7, 64, 257)
GRIDS = ("17x9x33", "5x4x3")
EPS = 2.0 ** -24
_cases = {}


def upstream(n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, (n, 3)).astype(f32), rng.normal(0.0, 1.0, n).astype(f32), rng.normal(0.0, 1.0, n).astype(f32)


def case(name, B, skip=False):
    """Everything one (grid, B, use_skip) case needs, computed once and left unchanged: the 257 rays of tests/test_gpu_vox.py, seeded
    upstream gradients, and the float64 / float32 restatements of the gradients of every prefix of the rays in N_RAYS."""
    key = (name, B, skip)
    if key not in _cases:
        g, sigma, coef = make_grid(name, B)
        rays = make_rays(g.lo, g.hi, max(N_RAYS), 10 + B)
        step = 0.5 * g.cell_edge()
        G, ga, gd = upstream(len(rays), 100 + B)
        plane = VR.build_skip(sigma, g.res) if skip else None
        args = (g.lo, g.hi, g.res, B, sigma, coef, rays, step, CFG["near"], CFG["far"], G, ga, gd)
        ref64 = VG.backward(*args, skip=plane, dtype=np.float64, prefixes=N_RAYS)
        ref32 = VG.backward(*args, skip=plane, dtype=np.float32, prefixes=N_RAYS)
        _cases[key] = SimpleNamespace(grid=g, rays=rays, step=step, G=G, ga=ga, gd=gd, ref64=ref64, ref32=ref32, plane=plane)
    return _cases[key]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(c, n, skip, G=None, ga="case", gd="case", T_min=0.0, into=None, check=False, rays=None):
    rays = c.rays[:n] if rays is None else rays
    G = c.G[:n] if G is None else G
    ga = c.ga[:n] if isinstance(ga, str) else ga
    gd = c.gd[:n] if isinstance(gd, str) else gd
    into = (None, None) if into is None else into
    out = baked_train.backward(c.grid, dev(rays), dev(G), dev(ga), dev(gd), into[0], into[1], step=c.step, near=CFG["near"], far=CFG["far"],
                               T_min=T_min, skip=skip, check=check)
    return out


def bars(what, got_sigma, got_coef, r64, r32, scale=1.0, adders=1):
    """Assert the bar for both gradient arrays: ``got`` against ``scale`` times the float64 gradient, whose elements each received
    ``adders`` times the restatement's contributions (A and c grow by the same factors).  Returns the (e_hip, e_ref) pairs."""
    pairs = {}
    for k, got in (("d_sigma", got_sigma), ("d_coef", got_coef)):
        got = got.cpu().numpy().astype(np.float64)
        ref = r64[k]
        m = ref["A"] > 0
        e_ref = VG.error(r32[k]["g"], ref)
        e_hip = float((np.abs(got[m] - scale * ref["g"][m]) / (abs(scale) * ref["A"][m])).max()) if m.any() else 0.0
        allowed = 4.0 * e_ref + adders * int(ref["c"].max()) * EPS
        print(f"\n[voxgrad {what}] {k}: e_hip {e_hip:.3e}, e_ref {e_ref:.3e}, c_max {adders * int(ref['c'].max())}, allowed {allowed:.3e}", end="")
        assert e_hip <= allowed, (what, k, e_hip, e_ref, allowed)
        assert not got[~m].any(), (what, k)                                       # untouched elements: exactly 0 in a zeroed array
        pairs[k] = (e_hip, e_ref)
    return pairs


# ---------------------------------------------------------------------------------------------------
# 4. the forward the backward recomputes is the renderer's, bit for bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 4, 9))
@pytest.mark.parametrize("name", GRIDS)
def test_the_recomputed_forward_equals_the_renderer_bit_for_bit(name, B):
    g, _, _ = make_grid(name, B)
    rays_all = make_rays(g.lo, g.hi, max(N_RAYS), 10 + B)
    step = 0.5 * g.cell_edge()
    G, ga, gd = upstream(len(rays_all), 100 + B)
    c = SimpleNamespace(grid=g, rays=rays_all, step=step, G=G, ga=ga, gd=gd)
    for n in N_RAYS:
        for skip in (False, True):
            for T_min in (0.0, 1e-3):
                want = g.render(dev(rays_all[:n]), step=step, near=CFG["near"], far=CFG["far"], T_min=T_min, skip=skip)
                _, _, rgb, acc, depth = run(c, n, skip, T_min=T_min, check=True)
                for k, x, y in (("rgb", rgb, want[0]), ("acc", acc, want[2]), ("depth", depth, want[3])):
                    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (name, B, n, skip, T_min, k)
    assert float(want[2].max()) > 0.05                                                   # the rays do meet density


# ---------------------------------------------------------------------------------------------------
# 5, 6. the gradient against the comparator, without and with the skip rule
# ---------------------------------------------------------------------------------------------------
# the skip rule is also run on the octant grid of tests/test_gpu_vox.py: the two small grids hold density in every block
GRADIENT_CASES = [(name, B, False) for name in GRIDS for B in (1, 4, 9)] + [(name, B, True) for name in GRIDS + ("24^3 octant",) for B in (1, 4, 9)]


@pytest.mark.parametrize("name,B,skip", GRADIENT_CASES)
def test_gradient_meets_the_float64_restatement(name, B, skip):
    c = case(name, B, skip)
    # the condition on the inputs: where a sample carries weight, no pre-clamp colour sits within 1e-5 of a clamp end -- there the
    # derivative's indicator could differ between fp32 and float64
    assert c.ref64["qdist_w"] >= 1e-5, c.ref64["qdist_w"]
    assert (c.ref64["samples"] > 0).sum() >= 0.3 * len(c.rays)
    if skip:
        assert np.array_equal(c.grid.skip.cpu().numpy(), c.plane)
    R3 = 3 * B
    for n in N_RAYS:
        d_sigma, d_coef = run(c, n, skip)
        bars(f"{name} B={B} n={n} skip={int(skip)}", d_sigma, d_coef, c.ref64["prefix"][n], c.ref32["prefix"][n])
        assert not d_coef[..., R3:].any()                                                # the padding floats stay exactly 0
    assert c.ref64["prefix"][257]["d_sigma"]["c"].max() > 1 and np.abs(c.ref64["prefix"][257]["d_coef"]["g"]).max() > 1e-3
    if name == "24^3 octant":
        # the rule removes samples: the plane has empty blocks, and the march without it reaches elements of d_sigma that this one leaves alone
        full = VG.backward(c.grid.lo, c.grid.hi, c.grid.res, B, *make_grid(name, B)[1:], c.rays, c.step, CFG["near"], CFG["far"], c.G, c.ga, c.gd)
        assert (c.plane == 0).any() and (c.ref64["d_sigma"]["c"] <= full["d_sigma"]["c"]).all()
        assert ((c.ref64["d_sigma"]["c"] == 0) & (full["d_sigma"]["c"] > 0)).sum() > 100


# ---------------------------------------------------------------------------------------------------
# 7. accumulation, contention, absent upstream gradients
# ---------------------------------------------------------------------------------------------------
def test_two_calls_into_one_array_add_up():
    c = case("17x9x33", 4)
    n = 257
    d_sigma, d_coef = run(c, n, False)
    d_sigma, d_coef = run(c, n, False, into=(d_sigma, d_coef))
    bars("two calls into one array", d_sigma, d_coef, c.ref64["prefix"][n], c.ref32["prefix"][n], scale=2.0, adders=2)


@pytest.mark.parametrize("B", (1, 9))
def test_64_copies_of_one_ray_give_64_times_its_gradient(B):
    """Every add of a wave meets the same addresses."""
    c = case("17x9x33", B)
    assert c.ref64["prefix"][1]["d_sigma"]["c"].sum() > 10                             # ray 0 meets density
    rays = np.repeat(c.rays[:1], 64, 0)
    d_sigma, d_coef = run(c, 64, False, G=np.repeat(c.G[:1], 64, 0), ga=np.repeat(c.ga[:1], 64), gd=np.repeat(c.gd[:1], 64), rays=rays)
    bars(f"64 copies of one ray B={B}", d_sigma, d_coef, c.ref64["prefix"][1], c.ref32["prefix"][1], scale=64.0, adders=64)


def test_absent_upstream_gradients_are_zeros():
    g, sigma, coef = make_grid("5x4x3", 4)
    rays = make_rays(g.lo, g.hi, 64, 14)
    step = 0.5 * g.cell_edge()
    G, _, _ = upstream(64, 104)
    args = (g.lo, g.hi, g.res, 4, sigma, coef, rays, step, CFG["near"], CFG["far"], G)
    r64, r32 = VG.backward(*args, dtype=np.float64), VG.backward(*args, dtype=np.float32)
    c = SimpleNamespace(grid=g, rays=rays, step=step, G=G)
    zeros = np.zeros(64, f32)
    for what, ga, gd in (("NULL", None, None), ("zeros", zeros, zeros), ("NULL g_acc", None, zeros), ("NULL g_depth", zeros, None)):
        d_sigma, d_coef = run(c, 64, False, ga=ga, gd=gd)
        bars(f"g_acc / g_depth {what}", d_sigma, d_coef, r64, r32)


# ---------------------------------------------------------------------------------------------------
# 8. autograd and plumbing
# ---------------------------------------------------------------------------------------------------
def _own_grid(name, B):
    g, sigma, coef = make_grid(name, B)
    h = baked.RadianceGrid(g.lo, g.hi, g.res, B).allocate(DEV)
    h.sigma.copy_(g.sigma)
    h.coef.copy_(g.coef)
    return h.build_skip(), sigma, coef


def test_autograd_fills_grad_as_a_direct_call_does_and_the_plumbing_holds():
    h, sigma, coef = _own_grid("5x4x3", 4)
    rays_np = make_rays(h.lo, h.hi, 64, 14)
    rays = dev(rays_np)
    step = 0.5 * h.cell_edge()
    kw = dict(step=step, near=CFG["near"], far=CFG["far"])
    ones = np.ones((64, 3), f32)
    args = (h.lo, h.hi, h.res, 4, sigma, coef, rays_np, step, CFG["near"], CFG["far"], ones)
    r64, r32 = VG.backward(*args, dtype=np.float64), VG.backward(*args, dtype=np.float32)
    # without requires_grad, and under no_grad, it is grid.render
    plain = h.render(rays, **kw)
    for x, y in zip(baked_train.render(h, rays, **kw), plain):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and not x.requires_grad
    h.sigma.requires_grad_(True)
    h.coef.requires_grad_(True)
    with torch.no_grad():
        assert not baked_train.render(h, rays, **kw)[0].requires_grad
    out = baked_train.render(h, rays, **kw)
    for x, y in zip(out, plain):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert out[0].requires_grad and out[2].requires_grad and out[3].requires_grad and not out[1].requires_grad       # disp is detached
    out[0].sum().backward()
    bars("autograd rgb.sum()", h.sigma.grad, h.coef.grad, r64, r32)
    direct = baked_train.backward(h, rays, dev(ones), **kw)
    bars("direct call", direct[0], direct[1], r64, r32)
    # a second differentiation is refused
    out = baked_train.render(h, rays, **kw)
    (gs,) = torch.autograd.grad(out[0].sum(), h.sigma, create_graph=True)
    with pytest.raises(RuntimeError):
        gs.sum().backward()
    # acc and depth carry gradients too: a loss on all three, a non-default stream
    h.sigma.grad = h.coef.grad = None
    G, ga, gd = upstream(64, 104)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        o = baked_train.render(h, rays, **kw)
        gs, gc = torch.autograd.grad((o[0] * dev(G)).sum() + (o[2] * dev(ga)).sum() + (o[3] * dev(gd)).sum(), (h.sigma, h.coef))
    side.synchronize()
    a64, a32 = VG.backward(*args[:10], G, ga, gd, dtype=np.float64), VG.backward(*args[:10], G, ga, gd, dtype=np.float32)
    bars("autograd on a side stream, rgb + acc + depth", gs, gc, a64, a32)
    # n = 0
    h.sigma.grad = h.coef.grad = None
    e = baked_train.render(h, torch.empty(0, 6, device=DEV), **kw)
    assert [tuple(t.shape) for t in e] == [(0, 3), (0,), (0,), (0,)]
    e[0].sum().backward()
    assert not h.sigma.grad.any() and not h.coef.grad.any()
    empty = baked_train.backward(h, torch.empty(0, 6, device=DEV), torch.empty(0, 3, device=DEV), **kw)
    assert not empty[0].any() and not empty[1].any()
    # refusals
    with pytest.raises(MiNerfError, match="compact"):
        baked_train.render(h.compact("fp32"), rays, **kw)
    with pytest.raises(MiNerfError):
        baked_train.render(h, rays.cpu(), **kw)
    with pytest.raises(MiNerfError):
        baked_train.render(baked.RadianceGrid(h.lo, h.hi, h.res, 4).allocate("cpu"), rays.cpu(), **kw)
    with pytest.raises(MiNerfError, match="step"):
        baked_train.backward(h, rays, dev(ones), step=0.0)


# ---------------------------------------------------------------------------------------------------
# 9. it learns
# ---------------------------------------------------------------------------------------------------
def test_finetuning_a_baked_grid_lowers_its_error_on_the_training_views():
    """A 24^3 bake of SolidScene.default(), 6 views of 32 x 32, 40 steps: the MSE on the training rays falls.  The size of the drop is
    reported, not asserted (docs/design/23_radiance_grid_training.md)."""
    scene = scenes.SolidScene.default()
    grid = baked.bake_field(scene.field, -1.2, 1.2, 24, B=4, device=DEV, shell="neighbours")
    H = W = 32
    K = scenes.scaled_camera((H, W))
    rays = []
    for i in range(6):
        pose = torch.from_numpy(synthetic.pose_spherical(60.0 * i, -30.0, 4.0)).to(DEV)
        o, d = ops.make_o_d(W, H, K, pose, DEV)
        rays.append(torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1))
    rays = torch.cat(rays).contiguous()
    target = scene.render(rays, 2.0, 6.0)[0]
    before = float(torch.mean((grid.render(rays)[0] - target) ** 2))
    losses = baked_train.finetune(grid, rays, target, steps=40)
    after = float(torch.mean((grid.render(rays)[0] - target) ** 2))
    print(f"\n[voxgrad finetune 24^3 B=4, 6 x 32 x 32, 40 steps] MSE on the training rays {before:.5f} -> {after:.5f} "
          f"(PSNR {-10 * math.log10(before):.2f} -> {-10 * math.log10(after):.2f} dB); first / last step loss {float(losses[0]):.5f} / {float(losses[-1]):.5f}", end="")
    assert losses.shape == (40,) and losses.is_cuda and bool(torch.isfinite(losses).all())
    assert after < before, (before, after)
    assert bool((grid.sigma >= 0).all()) and bool(torch.isfinite(grid.sigma).all()) and bool(torch.isfinite(grid.coef).all())
    assert not grid.sigma.requires_grad and grid.sigma.grad is None
    assert np.array_equal(grid.skip.cpu().numpy(), VR.build_skip(grid.sigma.cpu().numpy(), grid.res))    # the plane describes the sigma left behind
