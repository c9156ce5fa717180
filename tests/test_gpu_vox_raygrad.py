"""THE RAY GRADIENT RULE on the GPU (mi_vox_render_backward_rays / mi_vox_render_sparse_backward_rays of include/mi_nerf_vox.h,
RadianceGrid.render_backward_rays, nerf_pytorch_paeng_amd/baked_pose.py) against the numpy restatement of the header's rule
(tests/vox_raygrad_restate.py, itself held to central differences in tests/test_vox_raygrad_cpu.py), on the grids, seeded arrays and ray
mix of tests/test_gpu_vox.py.

The bar is the one of tests/test_gpu_voxgrad.py: with e(x) = max over the components with A > 0 of |x - g64| / A,
    e_hip <= 4 e_ref + c_max * 2^-24,
e_ref the float32 restatement's.  The library's cells, clamp states and slab axes are those of the float32 restatement (the same fp32
operations; expf touches none of them), so a sample that float32 and float64 put on different sides of a kink moves e_ref as it moves
e_hip.  Measured e_hip / e_ref pairs: docs/design/28_grid_ray_gradients.md."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import baked, baked_pose, scenes, synthetic
from tests import vox_raygrad_restate as RG
from tests.test_gpu_vox import CFG, make_grid, make_rays
from tests.test_gpu_voxgrad import upstream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32
N_RAYS = (1, 7, 33, 257)
GRIDS = ("5x4x3", "17x9x33", "24^3 octant")
EPS = 2.0 ** -24
_cases = {}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def case(name, B):
    """Everything one (grid, B) case needs, computed once and left unchanged: the 257 rays of tests/test_gpu_vox.py (the smaller ray sets
    are its prefixes: a ray's gradient depends on no other ray), seeded upstream gradients, the float64 and float32 restatements."""
    if (name, B) not in _cases:
        g, sigma, coef = make_grid(name, B)
        rays = make_rays(g.lo, g.hi, max(N_RAYS), 10 + B)
        step = 0.5 * g.cell_edge()
        G, ga, gd = upstream(len(rays), 100 + B)
        args = (g.lo, g.hi, g.res, B, sigma, coef, rays, step, CFG["near"], CFG["far"], G, ga, gd)
        ref64 = RG.ray_grad(*args, dtype=np.float64, want_sig=False)
        ref32 = RG.ray_grad(*args, dtype=np.float32, want_sig=False)
        _cases[(name, B)] = SimpleNamespace(grid=g, sigma=sigma, coef=coef, rays=rays, step=step, G=G, ga=ga, gd=gd, ref64=ref64, ref32=ref32)
    return _cases[(name, B)]


def run(c, n, skip=True, grid=None, T_min=0.0, check=False, rays=None, G=None, ga="case", gd="case"):
    rays = c.rays[:n] if rays is None else rays
    G = c.G[:n] if G is None else G
    ga = c.ga[:n] if isinstance(ga, str) else ga
    gd = c.gd[:n] if isinstance(gd, str) else gd
    return (c.grid if grid is None else grid).render_backward_rays(dev(rays), dev(G), dev(ga), dev(gd), step=c.step, near=CFG["near"], far=CFG["far"],
                                                                   T_min=T_min, skip=skip, check=check)


def bar(what, got, r64, r32, n):
    """Assert the bar on the first n rays; returns (e_hip, e_ref)."""
    got = got.cpu().numpy().astype(np.float64)
    ref = {k: r64[k][:n] for k in ("g", "A", "c")}
    m = ref["A"] > 0
    e_ref = RG.error(r32["g"][:n], ref)
    e_hip = RG.error(got, ref)
    allowed = 4.0 * e_ref + int(ref["c"].max()) * EPS
    print(f"\n[raygrad {what}] e_hip {e_hip:.3e}, e_ref {e_ref:.3e}, ratio {e_hip / e_ref if e_ref else float('nan'):.2f}, c_max {int(ref['c'].max())}, "
          f"allowed {allowed:.3e}", end="")
    assert np.isfinite(got).all(), what
    assert e_hip <= allowed, (what, e_hip, e_ref, allowed)
    assert not got[~m].any(), what                                                         # components nothing contributes to: exactly 0
    return e_hip, e_ref


# ---------------------------------------------------------------------------------------------------
# 1. accuracy against the float64 restatement; the check outputs; determinism; skipping
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 4, 9))
@pytest.mark.parametrize("name", GRIDS)
def test_gradient_meets_the_float64_restatement_and_the_forward_is_the_renderer_s(name, B):
    c = case(name, B)
    assert (c.ref64["samples"] > 0).sum() >= 0.3 * len(c.rays) and float(c.ref64["acc"].max()) > 0.05      # the rays do meet density
    assert np.abs(c.ref64["g"]).max() > 1e-3
    miss = ~(c.ref64["A"] > 0).any(1)
    assert miss[[3, 5, 8, 9]].all()                                   # a zero component outside its slab, a clean miss, a NaN ray, a zero direction
    for n in N_RAYS:
        got = {}
        for skip in (False, True):
            d_rays, rgb, acc, depth = run(c, n, skip, check=True)
            assert tuple(d_rays.shape) == (n, 6)
            bar(f"{name} B={B} n={n} skip={int(skip)}", d_rays, c.ref64, c.ref32, n)
            assert not d_rays[dev(miss[:n])].any()                                         # misses and non-finite rays: six zeros
            want = c.grid.render(dev(c.rays[:n]), step=c.step, near=CFG["near"], far=CFG["far"], skip=skip)
            for k, x, y in (("rgb", rgb, want[0]), ("acc", acc, want[2]), ("depth", depth, want[3])):
                assert torch.equal(bits(x), bits(y)), (name, B, n, skip, k)
            assert torch.equal(bits(run(c, n, skip)), bits(d_rays)), (name, B, n, skip)     # two runs, without the check outputs: the same bits
            got[skip] = d_rays
        assert torch.equal(got[False], got[True]), (name, B, n)                            # use_skip 0 equals 1
    if name == "24^3 octant":
        assert bool((c.grid.skip == 0).any())                                              # the plane has empty blocks: the march did jump


def test_the_forward_with_a_transmittance_stop_is_the_renderer_s_and_the_gradient_stays_finite():
    c = case("17x9x33", 4)
    for skip in (False, True):
        d_rays, rgb, acc, depth = run(c, 257, skip, T_min=1e-3, check=True)
        want = c.grid.render(dev(c.rays), step=c.step, near=CFG["near"], far=CFG["far"], T_min=1e-3, skip=skip)
        for k, x, y in (("rgb", rgb, want[0]), ("acc", acc, want[2]), ("depth", depth, want[3])):
            assert torch.equal(bits(x), bits(y)), (skip, k)
        assert bool(torch.isfinite(d_rays).all())


# ---------------------------------------------------------------------------------------------------
# 2. the three storages
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 4, 9))
@pytest.mark.parametrize("name", ("17x9x33", "24^3 octant"))
def test_compact_fp32_equals_dense_and_compact_f16_equals_dense_on_the_rounded_records(name, B):
    c = case(name, B)
    dense = run(c, 257, check=True)
    s32 = c.grid.compact("fp32")
    for x, y in zip(run(c, 257, grid=s32, check=True), dense):
        assert torch.equal(bits(x), bits(y)), (name, B)
    s16 = c.grid.compact("f16")
    rounded = s16.to_dense()
    assert not torch.equal(rounded.coef, c.grid.coef)                                      # binary16 did round
    for skip in (False, True):
        for x, y in zip(run(c, 257, skip, grid=s16, check=True), run(c, 257, skip, grid=rounded, check=True)):
            assert torch.equal(bits(x), bits(y)), (name, B, skip)
    want = s16.render(dev(c.rays), step=c.step, near=CFG["near"], far=CFG["far"])
    assert torch.equal(bits(run(c, 257, grid=s16, check=True)[1]), bits(want[0]))
    # an empty compact grid (no record, no table) gives zeros
    empty = baked.SparseRadianceGrid(c.grid.lo, c.grid.hi, c.grid.res, B, "f16").allocate(DEV)
    assert not run(c, 33, grid=empty).any()


def test_64_copies_of_one_ray_give_64_equal_rows_and_absent_upstream_gradients_are_zeros():
    c = case("17x9x33", 9)
    assert c.ref64["A"][0].min() > 0                                                       # ray 0 meets density
    rays = np.repeat(c.rays[:1], 64, 0)
    d = run(c, 64, rays=rays, G=np.repeat(c.G[:1], 64, 0), ga=np.repeat(c.ga[:1], 64), gd=np.repeat(c.gd[:1], 64))
    assert torch.equal(bits(d), bits(d[:1].expand(64, 6))) and torch.equal(bits(d[:1]), bits(run(c, 1)))
    zeros = np.zeros(33, f32)
    a = run(c, 33, ga=None, gd=None)
    for ga, gd in ((zeros, zeros), (None, zeros), (zeros, None)):
        assert torch.equal(bits(run(c, 33, ga=ga, gd=gd)), bits(a))
    assert not torch.equal(a, run(c, 33))
    assert tuple(c.grid.render_backward_rays(torch.empty(0, 6, device=DEV), torch.empty(0, 3, device=DEV)).shape) == (0, 6)


# ---------------------------------------------------------------------------------------------------
# 3. the autograd node
# ---------------------------------------------------------------------------------------------------
def test_the_autograd_node_renders_the_same_bits_and_hands_the_entry_s_gradient_to_the_rays():
    c = case("5x4x3", 4)
    n = 33
    kw = dict(step=c.step, near=CFG["near"], far=CFG["far"])
    rays = dev(c.rays[:n])
    plain = c.grid.render(rays, **kw)
    out = baked_pose.render(c.grid, rays, **kw)                                            # no requires_grad: grid.render, no node
    for x, y in zip(out, plain):
        assert torch.equal(bits(x), bits(y)) and not x.requires_grad and x.grad_fn is None
    rays.requires_grad_(True)
    with torch.no_grad():
        assert baked_pose.render(c.grid, rays, **kw)[0].grad_fn is None
    out = baked_pose.render(c.grid, rays, **kw)
    for x, y in zip(out, plain):
        assert torch.equal(bits(x.detach()), bits(y))
    assert out[0].requires_grad and out[2].requires_grad and out[3].requires_grad and not out[1].requires_grad       # disp is detached
    G, ga, gd = dev(c.G[:n]), dev(c.ga[:n]), dev(c.gd[:n])
    ((out[0] * G).sum() + (out[2] * ga).sum() + (out[3] * gd).sum()).backward()
    assert torch.equal(bits(rays.grad), bits(run(c, n)))
    bar("autograd rgb + acc + depth", rays.grad, c.ref64, c.ref32, n)
    # rgb alone: acc and depth receive no gradient
    rays.grad = None
    baked_pose.render(c.grid, rays, **kw)[0].mul(G).sum().backward()
    assert torch.equal(bits(rays.grad), bits(run(c, n, ga=None, gd=None)))
    # a second differentiation is refused
    (g1,) = torch.autograd.grad(baked_pose.render(c.grid, rays, **kw)[0].sum(), rays, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()
    # a compact grid is accepted, in both storages
    for storage in ("fp32", "f16"):
        sp = c.grid.compact(storage)
        r2 = dev(c.rays[:n]).requires_grad_(True)
        o = baked_pose.render(sp, r2, **kw)
        assert torch.equal(bits(o[0].detach()), bits(sp.render(r2.detach(), **kw)[0]))
        ((o[0] * G).sum() + (o[2] * ga).sum() + (o[3] * gd).sum()).backward()
        assert torch.equal(bits(r2.grad), bits(run(c, n, grid=sp)))
    # a dense grid that trains: the rays' gradient and the grid's, from one node
    h = baked.RadianceGrid(c.grid.lo, c.grid.hi, c.grid.res, 4).allocate(DEV)
    h.sigma.copy_(c.grid.sigma)
    h.coef.copy_(c.grid.coef)
    h.build_skip()
    h.sigma.requires_grad_(True)
    h.coef.requires_grad_(True)
    r3 = dev(c.rays[:n]).requires_grad_(True)
    (baked_pose.render(h, r3, **kw)[0] * G).sum().backward()
    assert torch.equal(bits(r3.grad), bits(run(c, n, ga=None, gd=None)))
    assert h.sigma.grad is not None and bool(h.sigma.grad.abs().sum() > 0) and bool(h.coef.grad.abs().sum() > 0)
    o = baked_pose.render(h, dev(c.rays[:n]), **kw)                                        # rays without a gradient: the grid's alone
    assert o[0].requires_grad


# ---------------------------------------------------------------------------------------------------
# 4. it localises
# ---------------------------------------------------------------------------------------------------
def smooth_grid(res=24, B=4):
    """A grid filled directly with smooth content, so that nothing saturates: three Gaussian density blobs of peak about 30 and colour
    records that vary smoothly with position (a constant part within [0.2, 0.8], small degree-1 parts)."""
    g = baked.RadianceGrid(-1.0, 1.0, res, B).allocate(DEV)
    ax = torch.linspace(-1.0, 1.0, res + 1, device=DEV)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    sigma = torch.zeros_like(x)
    for (cx, cy, cz), width, peak in (((-0.35, 0.1, 0.2), 0.28, 30.0), ((0.4, -0.3, -0.1), 0.22, 28.0), ((0.05, 0.45, -0.4), 0.25, 32.0)):
        sigma += peak * torch.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (2.0 * width ** 2))
    g.sigma.copy_(torch.where(sigma > 0.05, sigma, torch.zeros_like(sigma)))
    base = torch.stack([0.5 + 0.3 * torch.sin(2.0 * x + 1.0), 0.5 + 0.3 * torch.sin(2.5 * y - 0.5), 0.5 + 0.3 * torch.cos(2.0 * z + x)], -1)
    g.coef[..., 0:3] = base / 0.28209479
    g.coef[..., 3:6] = 0.1 * torch.stack([x, y, z], -1)
    g.coef[..., 6:9] = 0.1 * torch.stack([y, z, x], -1)
    g.coef[..., 9:12] = 0.1 * torch.stack([z, x, y], -1)
    return g.build_skip()


def pose_errors(a, b):
    """(rotation angle between two poses in degrees, distance of their origins)."""
    a, b = a.double().cpu(), b.double().cpu()
    cos = float(((a[:3, :3].T @ b[:3, :3]).trace() - 1.0) / 2.0)
    return math.degrees(math.acos(max(-1.0, min(1.0, cos)))), float((a[:3, 3] - b[:3, 3]).norm())


def test_a_perturbed_camera_is_recovered_against_the_grid():
    """A 48 x 48 target rendered from a known pose; ``locate`` starts from that pose turned by 2 degrees and moved by 0.05.  The fall of the
    loss and of both pose errors is asserted, its size is printed (docs/design/28_grid_ray_gradients.md)."""
    grid = smooth_grid()
    H = W = 48
    K = scenes.scaled_camera((H, W))
    true = torch.from_numpy(synthetic.pose_spherical(35.0, -25.0, 3.0)).to(DEV)[:3, :4].contiguous()

    def picture(p):
        with torch.no_grad():
            from nerf_pytorch_paeng_amd import ops
            o, d = ops.make_o_d(W, H, K, p, DEV)
            return grid.render(torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1).contiguous())[0]

    target = picture(true)
    assert 0.15 < float((target < 0.99).any(1).float().mean()) and float(target.std()) > 0.05          # the picture shows the blobs
    axis = torch.tensor([0.5, -0.7, 0.5], dtype=torch.float64)
    axis = axis / axis.norm() * math.radians(2.0)
    Kx = torch.tensor([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]], dtype=torch.float64)
    start = true.clone()
    start[:, :3] = (torch.matrix_exp(Kx) @ true[:, :3].double().cpu()).float().to(DEV)
    start[:, 3] += torch.tensor([0.03, -0.03, 0.0265], device=DEV)                                       # |.| = 0.05
    rot0, tr0 = pose_errors(start, true)
    assert abs(rot0 - 2.0) < 1e-3 and abs(tr0 - 0.05) < 1e-4
    loss0 = float(torch.mean((picture(start) - target) ** 2))
    found, losses = baked_pose.locate(grid, H, W, K, start, target.reshape(H, W, 3), steps=200, batch=1024)
    rot1, tr1 = pose_errors(found, true)
    loss1 = float(torch.mean((picture(found) - target) ** 2))
    print(f"\n[raygrad locate 24^3 B=4, 48 x 48, 200 steps of 1024 pixels] image MSE {loss0:.3e} -> {loss1:.3e}; rotation error {rot0:.3f} -> {rot1:.3f} deg; "
          f"translation error {tr0:.4f} -> {tr1:.4f}; first / last step loss {float(losses[0]):.3e} / {float(losses[-1]):.3e}", end="")
    assert tuple(found.shape) == (3, 4) and losses.shape == (200,) and losses.is_cuda and bool(torch.isfinite(losses).all())
    assert loss1 < loss0, (loss0, loss1)
    assert rot1 < rot0, (rot0, rot1)
    assert tr1 < tr0, (tr0, tr1)
    assert not grid.sigma.requires_grad and grid.sigma.grad is None
