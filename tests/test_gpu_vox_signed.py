"""A SIGNED GRID on the GPU (mi_vox_build_skip_signed, mi_vox_render_signed, mi_vox_render_sparse_signed of include/mi_nerf_vox.h, the Signed
paragraph of THE BACKWARD RULE of include/mi_nerf_voxgrad.h, ``signed=`` in baked.py and baked_train.py) against the numpy restatement
(tests/vox_signed_restate.py), on the grids, seeded records and ray mix of tests/test_gpu_vox.py.  No tolerance is invented: on planes that
are >= 0 the signed entries equal the unsigned ones bit for bit; on signed planes the renderer meets tests/test_gpu_vox.py's bar,
e_hip <= max(4 e_ref, one ulp), and the backward tests/test_gpu_voxgrad.py's, e_hip <= 4 e_ref + c_max 2^-24; skipping, compact storage,
``prune(0)`` and invisible negatives change no bit.  No ray is excluded."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import baked, baked_pose, baked_train, ops, optim, scenes, synthetic
from nerf_pytorch_paeng_amd._lib import MiNerfError
from tests import vox_restate as VR
from tests import vox_signed_restate as SR
from tests import vox_sparse_restate as SP
from tests.test_gpu_vox import CFG, GRID_SPECS, OUTPUTS, bar, grid_arrays, make_grid, make_rays

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32
EPS = 2.0 ** -24
N = 257
_planes, _grids, _cases, _backs = {}, {}, {}, {}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def signed_plane(name, B):
    """The named grid's plane with its zeros replaced: about 70 % of them by a negative number of the density's size, the rest left 0.
    The points with density are those of tests/test_gpu_vox.py, so the octant grid keeps its empty blocks."""
    if (name, B) not in _planes:
        sigma, coef = grid_arrays(name, B)
        rng = np.random.default_rng(1000 + GRID_SPECS[name]["seed"])
        neg = np.where(rng.uniform(size=sigma.shape) < 0.7, -rng.uniform(0.5, 12.0, sigma.shape), 0.0)
        _planes[(name, B)] = (np.where(sigma > 0, sigma, neg).astype(f32), coef)
    return _planes[(name, B)]


def grid_of(name, B, sigma, coef, signed):
    spec = GRID_SPECS[name]
    g = baked.RadianceGrid(spec["lo"], spec["hi"], spec["res"], B, signed=signed).allocate(DEV)
    g.sigma.copy_(dev(sigma))
    g.coef.copy_(dev(coef))
    return g.build_skip()


def signed_grid(name, B):
    if (name, B) not in _grids:
        sigma, coef = signed_plane(name, B)
        _grids[(name, B)] = grid_of(name, B, sigma, coef, True)
    return _grids[(name, B)]


def case(name, B):
    """One (grid, B) case, computed once and left unchanged: the signed grid, the 257 rays of tests/test_gpu_vox.py, both restatements."""
    if (name, B) not in _cases:
        g = signed_grid(name, B)
        sigma, coef = signed_plane(name, B)
        rays = make_rays(g.lo, g.hi, N, 10 + B)
        step = 0.5 * g.cell_edge()
        args = (g.lo, g.hi, g.res, B, sigma, coef, rays, step, CFG["near"], CFG["far"])
        _cases[(name, B)] = SimpleNamespace(grid=g, sigma=sigma, coef=coef, rays=rays, step=step, ref64=SR.render(*args, dtype=np.float64),
                                            ref32=SR.render(*args, dtype=np.float32))
    return _cases[(name, B)]


def run(g, rays, step, skip, T_min=0.0):
    return g.render(rays if isinstance(rays, torch.Tensor) else dev(rays), step=step, near=CFG["near"], far=CFG["far"], T_min=T_min, skip=skip, visited=True)


# ---------------------------------------------------------------------------------------------------
# 1. on a plane that is >= 0 the three entries are the unsigned ones, bit for bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 4, 9))
@pytest.mark.parametrize("name", sorted(GRID_SPECS))
def test_on_a_nonnegative_plane_the_signed_entries_equal_the_unsigned_ones_bit_for_bit(name, B):
    u, sigma, coef = make_grid(name, B)
    s = grid_of(name, B, sigma, coef, True)
    assert s.signed and not u.signed and torch.equal(s.skip, u.skip)                       # mi_vox_build_skip_signed
    rays = dev(np.concatenate([make_rays(u.lo, u.hi, N, 10 + B), np.repeat(make_rays(u.lo, u.hi, 1, 10 + B), 64, 0)]))     # ... and 64 copies of one ray
    step = 0.5 * u.cell_edge()
    pairs = [(u, s)] + [(u.compact(st), s.compact(st)) for st in ("fp32", "f16")]
    assert all(b.signed and not a.signed and b.count == a.count for a, b in pairs[1:])
    for a, b in pairs:
        for skip in (False, True):
            for T_min in (0.0, 1e-3):
                assert same(run(a, rays, step, skip, T_min), run(b, rays, step, skip, T_min)), (name, B, type(a).__name__, skip, T_min)
    assert float(run(s, rays, step, True)[2].max()) > 0.05


# ---------------------------------------------------------------------------------------------------
# 2, 3. signed planes against the float64 restatement; skip on = skip off; the skip plane
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 4, 9))
@pytest.mark.parametrize("name", sorted(GRID_SPECS))
def test_signed_render_meets_the_float64_restatement_and_skipping_changes_no_bit(name, B):
    c = case(name, B)
    assert (c.sigma < 0).mean() > 0.3 and (c.sigma > 0).mean() > 0.05
    assert np.isfinite(c.ref64["rgb"]).all() and (c.ref64["samples"] > 0).sum() >= 0.7 * N and (c.ref64["acc"] > 0.05).sum() >= 0.1 * N
    # the rule is another one on this plane: the unsigned rule applied to the ReLU of the plane fogs the cells around the density
    fog = VR.render(c.grid.lo, c.grid.hi, c.grid.res, B, np.maximum(c.sigma, 0), c.coef, c.rays, c.step, CFG["near"], CFG["far"])
    assert np.abs(fog["acc"] - c.ref64["acc"]).max() > 0.05
    assert np.array_equal(c.grid.skip.cpu().numpy(), SR.build_skip(c.sigma, c.grid.res))
    off, on = run(c.grid, c.rays, c.step, False), run(c.grid, c.rays, c.step, True)
    for k, got in zip(OUTPUTS, off):
        e_hip, e_ref, allowed = bar(got.cpu().numpy(), c.ref64[k], c.ref32[k])
        print(f"\n[vox signed {name} B={B}] {k}: e_hip {e_hip:.3e}, e_ref {e_ref:.3e}, allowed {allowed:.3e}", end="")
        assert e_hip <= allowed, (name, B, k, e_hip, e_ref, allowed)
    assert same(off[:4], on[:4])
    for T_min in (1e-3,):
        assert same(run(c.grid, c.rays, c.step, False, T_min)[:4], run(c.grid, c.rays, c.step, True, T_min)[:4])
    v_off, v_on = off[4].cpu().numpy().astype(np.int64), on[4].cpu().numpy().astype(np.int64)
    assert (v_on <= v_off).all() and np.abs(v_off - c.ref64["samples"]).max() <= 1
    if name == "24^3 octant":
        assert (c.grid.skip == 0).any() and v_on.sum() < v_off.sum()
        print(f"\n[vox signed {name} B={B}] visited: {int(v_on.sum())} with skipping, {int(v_off.sum())} without", end="")
    # 64 copies of one ray: 64 times the same answer
    many = run(c.grid, np.repeat(c.rays[:1], 64, 0), c.step, True)
    assert all(torch.equal(bits(x), bits(x[:1]).expand_as(x)) for x in many) and same([t[:1] for t in many], [t[:1] for t in on])


@pytest.mark.parametrize("res", ((17, 9, 20), (8, 8, 8), (5, 4, 3), (33, 16, 7)))
def test_build_skip_signed_equals_the_restatement(res):
    rng = np.random.default_rng(sum(res))
    P = tuple(r + 1 for r in reversed(res))
    fields = [np.full(P, -2.0, f32), np.where(rng.uniform(size=P) < 0.004, 1.0, -1.0).astype(f32), np.where(rng.uniform(size=P) < 0.004, 1e-30, 0.0).astype(f32),
              -np.where(rng.uniform(size=P) < 0.5, 1e-30, 0.0).astype(f32)]
    g = baked.RadianceGrid(-1.0, 1.0, res, 1, signed=True).allocate(DEV)
    for i, s in enumerate(fields):
        g.skip.fill_(9)
        g.sigma.copy_(dev(s))
        got, want = g.build_skip().skip.cpu().numpy(), SR.build_skip(s, res)
        assert got.shape == want.shape and np.array_equal(got, want), (res, i)
    assert not want.any()                                                                  # negatives and -0 set no byte


# ---------------------------------------------------------------------------------------------------
# 4. compact storage
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 4, 9))
@pytest.mark.parametrize("name", sorted(GRID_SPECS))
def test_compact_signed_equals_dense_signed_bit_for_bit(name, B):
    c = case(name, B)
    want = run(c.grid, c.rays, c.step, True)
    small = c.grid.compact("fp32")
    assert small.signed and 0 < small.count < c.sigma.size and small.count == SP.slots(c.sigma)[1]
    assert same(want, run(small, c.rays, c.step, True)) and same(run(c.grid, c.rays, c.step, False, 1e-3), run(small, c.rays, c.step, False, 1e-3))
    half = c.grid.compact("f16")
    rounded = grid_of(name, B, c.sigma, c.coef.astype(np.float16).astype(f32), True)
    assert half.signed and half.table.dtype == torch.float16 and same(run(rounded, c.rays, c.step, True), run(half, c.rays, c.step, True))
    assert half.to_dense().signed and same(run(half.to_dense(), c.rays, c.step, True), run(half, c.rays, c.step, True))


# ---------------------------------------------------------------------------------------------------
# 5. invisible negatives, prune(0), resample, files
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("17x9x33", "24^3 octant"))
def test_invisible_negatives_and_prune_0_change_no_bit(name, tmp_path):
    B = 4
    c = case(name, B)
    want = run(c.grid, c.rays, c.step, True)
    hidden = ~SP.active_set(np.maximum(c.sigma, 0))
    assert hidden.sum() > 100
    wild = c.sigma.copy()
    wild[hidden] = -np.random.default_rng(3).uniform(0.0, 1e6, int(hidden.sum())).astype(f32)
    g = grid_of(name, B, wild, c.coef, True)
    assert same(want[:4], run(g, c.rays, c.step, True)[:4]) and same(want[:4], run(g, c.rays, c.step, False)[:4]) and torch.equal(g.skip, c.grid.skip)
    g.prune(0.0)
    assert g.signed and bool((g.sigma[dev(hidden)] == 0).all()) and bool((g.sigma[dev(~hidden)] == dev(c.sigma)[dev(~hidden)]).all())
    assert same(want, run(g, c.rays, c.step, True)) and torch.equal(g.skip, c.grid.skip)
    # the flag travels: a refinement, a file, a file of the time before the flag
    fine = c.grid.resample(tuple(2 * r for r in c.grid.res))
    assert fine.signed and bool((fine.sigma < 0).any())
    a, b = run(c.grid, c.rays, c.step, True), run(fine, c.rays, c.step, True)
    assert float((a[2] - b[2]).abs().max()) <= 1e-3                                         # the identical field, up to rounding
    path = str(tmp_path / "signed.npz")
    c.grid.save(path)
    back = baked.RadianceGrid.load(path, DEV)
    assert back.signed and same(want, run(back, c.rays, c.step, True))
    u = make_grid(name, B)[0]
    u.save(path)
    with np.load(path) as f:
        assert "signed" not in f.files
    assert not baked.RadianceGrid.load(path).signed
    small = c.grid.compact("f16")
    small.save(path)
    assert baked.SparseRadianceGrid.load(path, DEV).signed and same(run(small, c.rays, c.step, True), run(baked.SparseRadianceGrid.load(path, DEV), c.rays, c.step, True))


def test_to_signed_follows_its_rule_and_keeps_the_skip_blocks():
    u, sigma, coef = make_grid("24^3 octant", 4)
    s = u.to_signed()
    assert s.signed and not u.signed and np.array_equal(s.sigma.cpu().numpy(), SR.to_signed(sigma)) and bool((s.sigma < 0).any())
    assert torch.equal(s.skip, u.skip) and torch.equal(s.coef, u.coef) and s.coef.data_ptr() != u.coef.data_ptr()
    assert np.array_equal(u.sigma.cpu().numpy(), sigma)                                    # the grid handed in is left as it is
    with pytest.raises(MiNerfError, match="signed already"):
        s.to_signed()


# ---------------------------------------------------------------------------------------------------
# 6. the backward
# ---------------------------------------------------------------------------------------------------
def back_case(name, B, skip):
    key = (name, B, skip)
    if key not in _backs:
        c = case(name, B)
        rng = np.random.default_rng(100 + B)
        G, ga, gd = rng.normal(0.0, 1.0, (N, 3)).astype(f32), rng.normal(0.0, 1.0, N).astype(f32), rng.normal(0.0, 1.0, N).astype(f32)
        plane = SR.build_skip(c.sigma, c.grid.res) if skip else None
        args = (c.grid.lo, c.grid.hi, c.grid.res, B, c.sigma, c.coef, c.rays, c.step, CFG["near"], CFG["far"], G, ga, gd)
        _backs[key] = SimpleNamespace(G=G, ga=ga, gd=gd, ref64=SR.backward(*args, skip=plane, dtype=np.float64), ref32=SR.backward(*args, skip=plane, dtype=np.float32))
    return _backs[key]


def bars(what, got_sigma, got_coef, r64, r32, scale=1.0, adders=1):
    """tests/test_gpu_voxgrad.py's bar for both gradient arrays."""
    for k, got in (("d_sigma", got_sigma), ("d_coef", got_coef)):
        got = got.cpu().numpy().astype(np.float64)
        ref = r64[k]
        m = ref["A"] > 0
        e_ref = SR.error(r32[k]["g"], ref)
        e_hip = float((np.abs(got[m] - scale * ref["g"][m]) / (abs(scale) * ref["A"][m])).max()) if m.any() else 0.0
        allowed = 4.0 * e_ref + adders * int(ref["c"].max()) * EPS
        print(f"\n[voxgrad signed {what}] {k}: e_hip {e_hip:.3e}, e_ref {e_ref:.3e}, c_max {adders * int(ref['c'].max())}, allowed {allowed:.3e}", end="")
        assert e_hip <= allowed, (what, k, e_hip, e_ref, allowed)
        assert not got[~m].any(), (what, k)


BACK_CASES = [(name, B, False) for name in ("17x9x33", "5x4x3") for B in (1, 4, 9)] + [("24^3 octant", 4, True), ("17x9x33", 9, True)]


@pytest.mark.parametrize("name,B,skip", BACK_CASES)
def test_signed_backward_meets_the_float64_restatement(name, B, skip):
    c, b = case(name, B), back_case(name, B, skip)
    assert b.ref64["qdist_w"] >= 1e-5, b.ref64["qdist_w"]
    # The ReLU's kink needs no condition of its own here: the interpolation is the same fp32 operations in the library and in the float32
    # restatement, so both take the same side at every sample, and a sample at which float64 takes the other side is part of e_ref.
    print(f"\n[voxgrad signed {name} B={B} skip={int(skip)}] smallest nonzero |interpolation| {b.ref64['min_abs_nz']:.3e}", end="")
    kw = dict(step=c.step, near=CFG["near"], far=CFG["far"], skip=skip)
    for T_min in (0.0, 1e-3):                                       # the check outputs are mi_vox_render_signed's bits
        want = c.grid.render(dev(c.rays), T_min=T_min, **kw)
        out = baked_train.backward(c.grid, dev(c.rays), dev(b.G), dev(b.ga), dev(b.gd), T_min=T_min, check=True, **kw)
        assert same(out[2:], (want[0], want[2], want[3])), (name, B, skip, T_min)
    d_sigma, d_coef = baked_train.backward(c.grid, dev(c.rays), dev(b.G), dev(b.ga), dev(b.gd), **kw)
    bars(f"{name} B={B} skip={int(skip)}", d_sigma, d_coef, b.ref64, b.ref32)
    assert not d_coef[..., 3 * B:].any()
    # an element all of whose samples interpolate below 0 receives exactly 0
    closed = b.ref64["neg_only"]
    assert closed.sum() >= 3 and not d_sigma.cpu().numpy()[closed].any() and np.abs(b.ref64["d_sigma"]["g"]).max() > 1e-3
    if not skip and B == 4:
        # 64 copies of one ray: every add of a wave meets the same addresses
        one = SR.backward(c.grid.lo, c.grid.hi, c.grid.res, B, c.sigma, c.coef, c.rays[:1], c.step, CFG["near"], CFG["far"], b.G[:1], b.ga[:1], b.gd[:1])
        one32 = SR.backward(c.grid.lo, c.grid.hi, c.grid.res, B, c.sigma, c.coef, c.rays[:1], c.step, CFG["near"], CFG["far"], b.G[:1], b.ga[:1], b.gd[:1],
                            dtype=np.float32)
        rep = lambda a: dev(np.repeat(a[:1], 64, 0))                # noqa: E731
        d_sigma, d_coef = baked_train.backward(c.grid, rep(c.rays), rep(b.G), rep(b.ga), rep(b.gd), **kw)
        bars(f"{name} B={B} 64 copies of one ray", d_sigma, d_coef, one, one32, scale=64.0, adders=64)


def test_on_a_nonnegative_plane_the_backwards_check_outputs_stay_the_unsigned_renderers():
    u, sigma, coef = make_grid("17x9x33", 9)
    rays = dev(make_rays(u.lo, u.hi, N, 19))
    G = dev(np.random.default_rng(109).normal(0.0, 1.0, (N, 3)).astype(f32))
    kw = dict(step=0.5 * u.cell_edge(), near=CFG["near"], far=CFG["far"])
    for skip in (False, True):
        want = u.render(rays, skip=skip, **kw)
        out = baked_train.backward(u, rays, G, skip=skip, check=True, **kw)
        assert same(out[2:], (want[0], want[2], want[3]))


# ---------------------------------------------------------------------------------------------------
# 7. it learns
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer", ("Adam", "LazyAdam"))
def test_finetuning_a_signed_grid_lowers_its_error_and_keeps_its_negatives(optimizer):
    """A 24^3, B = 4 bake of SolidScene.default(), to_signed(), 6 views of 32 x 32, 40 steps: the MSE on the training rays falls (its size
    is reported, not asserted) and the plane still holds negatives: nothing clamped it at 0."""
    scene = scenes.SolidScene.default()
    grid = baked.bake_field(scene.field, -1.2, 1.2, 24, B=4, device=DEV, shell="neighbours").to_signed()
    assert grid.signed and bool((grid.sigma < 0).any())
    H = W = 32
    K = scenes.scaled_camera((H, W))
    rays = []
    for i in range(6):
        pose = torch.from_numpy(synthetic.pose_spherical(60.0 * i, -30.0, 4.0)).to(DEV)
        o, d = ops.make_o_d(W, H, K, pose, DEV)
        rays.append(torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1))
    rays = torch.cat(rays).contiguous()
    target = scene.render(rays, 2.0, 6.0)[0]
    start = grid.sigma.clone()
    before = float(torch.mean((grid.render(rays)[0] - target) ** 2))
    losses = baked_train.finetune(grid, rays, target, steps=40, optimizer=torch.optim.Adam if optimizer == "Adam" else optim.LazyAdam)
    after = float(torch.mean((grid.render(rays)[0] - target) ** 2))
    moved = (grid.sigma != start)
    print(f"\n[signed finetune {optimizer} 24^3 B=4, 6 x 32 x 32, 40 steps] MSE {before:.5f} -> {after:.5f} (PSNR {-10 * math.log10(before):.2f} -> "
          f"{-10 * math.log10(after):.2f} dB); {int(moved.sum())} sigma elements moved, {int((moved & (start < 0)).sum())} of them negative at the start", end="")
    assert losses.shape == (40,) and losses.is_cuda and bool(torch.isfinite(losses).all())
    assert after < before, (before, after)
    assert bool((grid.sigma < 0).any()) and bool(torch.isfinite(grid.sigma).all()) and bool(torch.isfinite(grid.coef).all())
    assert bool((moved & (grid.sigma < 0)).any())                                          # a negative value was stepped and stayed negative
    assert grid.signed and not grid.sigma.requires_grad and grid.sigma.grad is None
    assert np.array_equal(grid.skip.cpu().numpy(), SR.build_skip(grid.sigma.cpu().numpy(), grid.res))     # rebuilt by the signed builder


def test_sigma_floor_bounds_a_signed_grid_from_below_and_coarse_to_fine_keeps_the_flag():
    c = case("5x4x3", 4)
    g = grid_of("5x4x3", 4, c.sigma, c.coef, True)
    rays = dev(c.rays)
    target = torch.rand(N, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    for opt in (torch.optim.Adam, optim.LazyAdam):
        baked_train.finetune(g, rays, target, steps=3, batch=N, lr_sigma=0.5, optimizer=opt, sigma_floor=-6.0, near=CFG["near"], far=CFG["far"])
    assert float(g.sigma.min()) >= -6.0 and bool((g.sigma < 0).any())
    fine, losses = baked_train.coarse_to_fine(g, rays, target, [((5, 4, 3), 2), ((10, 8, 6), 2)], prune=0.0, near=CFG["near"], far=CFG["far"])
    assert fine.signed and tuple(fine.res) == (10, 8, 6) and losses.shape == (4,) and bool((fine.sigma < 0).any())
    with pytest.raises(MiNerfError, match="sigma_floor"):
        baked_train.finetune(g, rays, target, steps=1, sigma_floor=1.0)
    with pytest.raises(MiNerfError, match="sigma_floor"):
        baked_train.finetune(make_grid("5x4x3", 4)[0], rays, target, steps=1, sigma_floor=-1.0)


# ---------------------------------------------------------------------------------------------------
# 8. what a signed grid refuses, and a signed bake
# ---------------------------------------------------------------------------------------------------
def test_what_reads_sigma_without_the_relu_refuses_a_signed_grid():
    g = grid_of("5x4x3", 4, *signed_plane("5x4x3", 4), True)
    rays = dev(make_rays(g.lo, g.hi, 8, 14))
    K = scenes.scaled_camera((8, 8))
    pose = torch.from_numpy(synthetic.pose_spherical(30.0, -30.0, 4.0)).to(DEV)
    views = baked.Views(8, 8, K, pose[None, :3, :4])
    for call in (lambda: g.seen(views),
                 lambda: g.prune(0.0, seen=torch.zeros_like(g.sigma)),
                 lambda: g.render_backward_rays(rays, torch.ones(8, 3, device=DEV)),
                 lambda: g.compact("f16").render_backward_rays(rays, torch.ones(8, 3, device=DEV)),
                 lambda: baked_pose.render(g, rays),
                 lambda: baked_pose.locate(g, 8, 8, K, pose, torch.zeros(8, 8, 3, device=DEV), steps=1)):
        with pytest.raises(MiNerfError, match="signed grid"):
            call()
    assert g.prune(0.0).signed                                                             # prune(tau) without seen= is defined on a signed grid


def test_a_signed_bake_keeps_the_fields_negative_side():
    scene = scenes.SolidScene.default()
    def field(rays, z):
        out = scene.field(rays, z).clone()
        out[..., 3] = torch.where(out[..., 3] > 0, out[..., 3], torch.full_like(out[..., 3], -7.5))       # a field that is negative outside its solids
        return out

    u = baked.bake_field(field, -1.2, 1.2, 16, B=1, device=DEV)
    s = baked.bake_field(field, -1.2, 1.2, 16, B=1, device=DEV, signed=True)
    k = baked.bake_field(field, -1.2, 1.2, 16, B=1, device=DEV, signed=True, clip=2.0)
    assert not u.signed and s.signed and k.signed and bool((u.sigma >= 0).all())
    assert torch.equal(s.sigma.clamp_min(0.0), u.sigma) and bool((s.sigma[u.sigma == 0] == -7.5).all())
    assert torch.equal(k.sigma, s.sigma.clamp(-2.0, 2.0)) and torch.equal(s.coef, u.coef) and torch.equal(s.skip, u.skip)
    sp = baked.bake_field(field, -1.2, 1.2, 16, B=1, device=DEV, signed=True, storage="sparse16")
    rays = dev(make_rays(s.lo, s.hi, 64, 3))
    assert sp.signed and same(sp.render(rays), s.compact("f16").render(rays))
    with pytest.raises(MiNerfError, match="clip"):
        baked.bake_field(field, -1.2, 1.2, 16, B=1, device=DEV, clip=2.0)
