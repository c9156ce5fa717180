"""Geometry losses on the device (docs/design/18_geometry_losses.md): mi_geo_composite / mi_geo_composite_backward against the float64
restatement of tests/test_geo_cpu.py (oracle.restate.post_process plus the O(S^2) definition of the distortion loss, through autograd), the
drop-in post_process, the two training nodes with ``geometry=True``, inference, and a training run in which the fog goes down.

Bars: the project's own for the compositing backward (tests/test_gpu_train.py::test_composite_backward_vs_autograd), relative to the tensor's
largest entry -- colour channels of d_raw 1e-5, density channel 1e-4 -- and 2e-5 absolute for a forward value.  Where the distortion scans enter,
the same restatement evaluated in fp32 on the CPU measures what fp32 can do on these inputs (e32), and the kernel is held to max(3 e32, bar)."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import geometry as G
from nerf_pytorch_paeng_amd import harness, ops, scenes, synthetic, train_path, weights
from nerf_pytorch_paeng_amd import nerf_process as NP
from nerf_pytorch_paeng_amd import occupancy as OC
from nerf_pytorch_paeng_amd import occupancy_train as OT
from nerf_pytorch_paeng_amd.model import NeRF, get_positional_encoder
from oracle import restate as R
from tests.test_geo_cpu import composite_case, restate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NEAR, FAR = 2.0, 6.0
COLOUR_BAR, DENSITY_BAR, FORWARD_BAR = 1e-5, 1e-4, 2e-5
# C = 1, the step to C = 2, a partly filled last lane, the largest C; and saturated alphas
CASES = [(3, 1, False), (9, 7, False), (37, 64, False), (5, 65, False), (5, 192, False), (4, 300, False), (2, 1024, False), (33, 64, True)]
GRADS = ("rgb", "acc", "depth", "distortion", "weights")
# g_rgb alone through mi_geo_composite_backward against mi_nerf_composite_backward: the same expression in both kernels, so equality is
# asserted.  A build found otherwise is held to the bars of the backward instead and recorded in docs/design/18_geometry_losses.md.
COLOUR_ONLY_BIT_EXACT = True


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = float(b.abs().max())
    return float((a - b).abs().max()) / (scale if scale > 0 else 1.0)


class Case:
    """One (n, S) case: inputs on the host and the device, one random gradient per output, and the restatement's answers, each computed once."""

    def __init__(self, n, S, hard):
        self.n, self.S, self.hard = n, S, hard
        self.raw, self.z, self.rays = composite_case(n, S, 100 + S, hard)
        g = torch.Generator().manual_seed(1000 + S)
        self.g = {"rgb": torch.randn(n, 3, generator=g), "acc": torch.randn(n, generator=g), "depth": torch.randn(n, generator=g),
                  "distortion": torch.randn(n, generator=g), "weights": torch.randn(n, S, generator=g)}
        self.dev = SimpleNamespace(raw=self.raw.to(DEV), z=self.z.to(DEV), rays=self.rays.to(DEV), g={k: v.to(DEV) for k, v in self.g.items()})
        self._ref = {}

    def forward(self, dtype):
        key = ("fwd", dtype)
        if key not in self._ref:
            with torch.no_grad():
                self._ref[key] = restate(self.raw.to(dtype), self.z.to(dtype), self.rays[:, 3:].to(dtype), NEAR, FAR)
        return self._ref[key]

    def d_raw(self, which, dtype=torch.float64):
        """autograd of sum_k <g_k, output_k> over the outputs named in ``which`` through the restatement, in ``dtype`` on the CPU."""
        key = (tuple(which), dtype)
        if key not in self._ref:
            raw = self.raw.to(dtype).requires_grad_(True)
            outs = dict(zip(GRADS, (lambda r: (r[0], r[1], r[3], r[4], r[2]))(restate(raw, self.z.to(dtype), self.rays[:, 3:].to(dtype), NEAR, FAR))))
            loss = sum((outs[k] * self.g[k].to(dtype)).sum() for k in which)
            self._ref[key] = torch.autograd.grad(loss, raw)[0]
        return self._ref[key]

    def hip(self, which, **kw):
        d = self.dev
        return G.composite_geo_backward(d.raw, d.z, d.rays, NEAR, FAR, **{"g_" + k: d.g[k] for k in which}, **kw)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}x{c[1]}{'-hard' if c[2] else ''}")
def case(request):
    return Case(*request.param)


# ---------------------------------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------------------------------
def test_forward_equals_composite_bit_for_bit_and_distortion_the_restatement(case):
    d = case.dev
    got = G.composite_geo(d.raw, d.z, d.rays, NEAR, FAR)
    want = ops.composite(d.raw, d.z, d.rays, want_all=True)
    for name, a, b in zip(("rgb", "disp", "acc", "weights", "depth"), got, want):
        assert torch.equal(a, b), (name, int((a != b).sum()))
    got3 = G.composite_geo(d.raw, d.z, d.rays[:, 3:].contiguous(), NEAR, FAR)                 # the bare direction tensor
    assert all(torch.equal(a, b) for a, b in zip(got3, got))
    ref64, ref32 = case.forward(torch.float64)[4], case.forward(torch.float32)[4]
    e32 = float((ref32.double() - ref64).abs().max())
    e_hip = float((got[5].cpu().double() - ref64).abs().max())
    print(f"\n[forward {case.n}x{case.S}{' hard' if case.hard else ''}] distortion: largest value {float(ref64.abs().max()):.3e}, e32 {e32:.2e}, e_hip {e_hip:.2e}")
    assert e_hip <= max(3.0 * e32, FORWARD_BAR), (e_hip, e32)
    assert float(got[5].min()) >= -FORWARD_BAR                                                # a sum of non-negative terms
    if case.S == 1:
        assert float(got[5].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0


def test_forward_outputs_are_optional():
    """Any output may be NULL: each one asked for alone is the number the full call writes."""
    from nerf_pytorch_paeng_amd import _geo
    from nerf_pytorch_paeng_amd._lib import dev_ptr, stream_ptr
    c = Case(5, 65, False).dev
    full = G.composite_geo(c.raw, c.z, c.rays, NEAR, FAR)
    for i, ref in enumerate(full):
        out = torch.full_like(ref, float("nan"))
        ptrs = [None] * 6
        ptrs[i] = dev_ptr(out)
        _geo.check(_geo.lib().mi_geo_composite(dev_ptr(c.raw, "raw", align=16), dev_ptr(c.z), dev_ptr(c.rays), 6, 5, 65, NEAR, FAR, *ptrs, stream_ptr(DEV)),
                   "mi_geo_composite")
        assert torch.equal(out, ref), i


# ---------------------------------------------------------------------------------------------------
# 2. / 3. backward against float64 autograd
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [("rgb",), ("acc",), ("depth",), ("weights",), GRADS], ids=lambda w: "+".join(w))
def test_backward_vs_autograd(case, which):
    got, want = case.hip(which), case.d_raw(which)
    e_col, e_den = rel_err(got[..., :3], want[..., :3]), rel_err(got[..., 3], want[..., 3])
    print(f"\n[backward {case.n}x{case.S}{' hard' if case.hard else ''} {'+'.join(which)}] colour {e_col:.2e}, density {e_den:.2e}")
    assert e_col < COLOUR_BAR and e_den < DENSITY_BAR, (e_col, e_den)


def test_backward_distortion_term_vs_autograd(case):
    """g_distortion alone: new scans with a cancelling difference.  e32: the restatement's own fp32 autograd on the CPU against float64."""
    which = ("distortion",)
    got, want = case.hip(which), case.d_raw(which)
    e32 = rel_err(case.d_raw(which, torch.float32)[..., 3], want[..., 3])
    e_hip = rel_err(got[..., 3], want[..., 3])
    print(f"\n[backward {case.n}x{case.S}{' hard' if case.hard else ''} distortion] density channel: e32 {e32:.2e}, e_hip {e_hip:.2e}")
    assert float(got[..., :3].abs().max()) == 0.0                    # the colours do not reach the distortion loss
    assert e_hip <= max(3.0 * e32, DENSITY_BAR), (e_hip, e32)


# ---------------------------------------------------------------------------------------------------
# 4. colour only
# ---------------------------------------------------------------------------------------------------
def test_colour_only_is_the_existing_backward(case):
    d = case.dev
    got = case.hip(("rgb",))
    old = ops.composite_backward(d.raw, d.z, d.rays, d.g["rgb"])
    diff = int((got != old).sum())
    print(f"\n[colour only {case.n}x{case.S}{' hard' if case.hard else ''}] {diff} of {got.numel()} values differ, max |diff| {float((got - old).abs().max()):.3e}")
    if COLOUR_ONLY_BIT_EXACT:
        assert torch.equal(got, old)
    else:
        want = case.d_raw(("rgb",))
        assert rel_err(got[..., :3], want[..., :3]) < COLOUR_BAR and rel_err(got[..., 3], want[..., 3]) < DENSITY_BAR


# ---------------------------------------------------------------------------------------------------
# 5. further properties
# ---------------------------------------------------------------------------------------------------
def test_no_gradient_gives_zeros_scaling_is_exact_and_calls_repeat(case):
    d = case.dev
    poisoned = torch.full((case.n, case.S, 4), float("nan"), device=DEV)
    zero = G.composite_geo_backward(d.raw, d.z, d.rays, NEAR, FAR, out=poisoned)
    assert zero.data_ptr() == poisoned.data_ptr() and float(poisoned.abs().max()) == 0.0      # every element written, none left NaN
    for which in (("acc", "depth"), GRADS):
        poisoned = torch.full((case.n, case.S, 4), float("nan"), device=DEV)
        once = case.hip(which, out=poisoned)
        assert not bool(torch.isnan(once).any())
        again = case.hip(which)
        assert torch.equal(once, again)                              # two calls give identical bytes
        doubled = G.composite_geo_backward(d.raw, d.z, d.rays, NEAR, FAR, **{"g_" + k: 2.0 * d.g[k] for k in which})
        # linear in the gradients, and a factor 2 is exact in fp32 -- where nothing underflows: a product that lands among the subnormal
        # numbers is rounded there, and twice the rounded number is not the rounded double (saturated alphas take T down to 1e-40 and below).
        # Exact wherever the result is at least 2^-100, 26 binary orders above the subnormals; below that, small on both sides.
        normal = once.abs() >= 2.0 ** -100
        assert torch.equal(doubled[normal], 2.0 * once[normal]), which
        assert float(doubled[~normal].abs().max() if bool((~normal).any()) else 0.0) <= 2.0 ** -98, which
        assert int(normal.sum()) > 0 or case.S == 1


def test_empty_batch_and_errors():
    e = G.composite_geo_backward(torch.empty(0, 8, 4, device=DEV), torch.empty(0, 8, device=DEV), torch.empty(0, 6, device=DEV), NEAR, FAR,
                                 g_acc=torch.empty(0, device=DEV))
    assert e.shape == (0, 8, 4)
    assert G.composite_geo(torch.empty(0, 8, 4, device=DEV), torch.empty(0, 8, device=DEV), torch.empty(0, 6, device=DEV), NEAR, FAR)[5].shape == (0,)
    with pytest.raises(ops.MiNerfError, match="near"):
        G.composite_geo(torch.zeros(2, 8, 4, device=DEV), torch.zeros(2, 8, device=DEV), torch.zeros(2, 6, device=DEV), 6.0, 2.0)
    with pytest.raises(ops.MiNerfError, match="g_acc"):
        G.composite_geo_backward(torch.zeros(2, 8, 4, device=DEV), torch.zeros(2, 8, device=DEV), torch.zeros(2, 6, device=DEV), NEAR, FAR,
                                 g_acc=torch.zeros(3, device=DEV))


# ---------------------------------------------------------------------------------------------------
# 6. post_process
# ---------------------------------------------------------------------------------------------------
def test_post_process_is_differentiable_in_acc_depth_and_weights(case):
    d = case.dev
    raw = d.raw.clone().requires_grad_(True)
    plain = NP.post_process(d.raw.clone().requires_grad_(True), d.z, d.rays[:, 3:].contiguous())
    assert plain[0].requires_grad and plain[2].requires_grad and plain[4].requires_grad and not plain[1].requires_grad and not plain[3].requires_grad
    rgb, disp, acc, wts, depth = NP.post_process(raw, d.z, d.rays[:, 3:].contiguous(), weights_grad=True)
    assert not disp.requires_grad and acc.requires_grad and wts.requires_grad and depth.requires_grad
    assert all(torch.equal(a, b) for a, b in zip(plain, (rgb, disp, acc, wts, depth)))
    ((acc * d.g["acc"]).sum() + (depth * d.g["depth"]).sum() + (wts * d.g["weights"]).sum()).backward()
    want = case.d_raw(("acc", "depth", "weights"))
    assert float(raw.grad[..., :3].abs().max()) == 0.0
    e_den = rel_err(raw.grad[..., 3], want[..., 3])
    print(f"\n[post_process {case.n}x{case.S}{' hard' if case.hard else ''}] density {e_den:.2e}")
    assert e_den < DENSITY_BAR
    # the colours alone: today's gradient, bit for bit
    raw2 = d.raw.clone().requires_grad_(True)
    (NP.post_process(raw2, d.z, d.rays[:, 3:].contiguous())[0] * d.g["rgb"]).sum().backward()
    assert torch.equal(raw2.grad, ops.composite_backward(d.raw, d.z, d.rays, d.g["rgb"]))


# ---------------------------------------------------------------------------------------------------
# the training nodes
# ---------------------------------------------------------------------------------------------------
NETS = {"fp32": (4, 128), "f16s": (8, 256)}


def lego_rays(n, seed=0):
    K, H, W = synthetic.lego_camera()
    pose = synthetic.pose_spherical(0.0, -30.0, 4.0)
    pix = torch.from_numpy(synthetic.pixel_batch(H, W, n, seed)).to(DEV)
    o, d = ops.make_o_d_pixels(W, H, K, pose, pix)
    return torch.cat([o, d], -1).contiguous()


def random_grid(seed=0, p=0.5):
    g = OC.OccupancyGrid(-2.5, 2.5, (32, 32, 32), outside_occupied=True)
    cells = np.random.RandomState(seed).rand(g.words * 32) < p
    cells[g.cells:] = False
    return g.set_bits(np.packbits(cells, bitorder="little").view(np.uint32)).to(DEV)


def make_model(D, W, seed=0):
    sd = synthetic.make_state_dict(seed, D, W)
    model = NeRF(D, W, 63, 27).to(DEV)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return sd, model


def make_opts(Sc, Nf):
    return SimpleNamespace(near=NEAR, far=FAR, N_samples_c=Sc, N_samples_f=Nf, perturb=1.0, chunk_rays=4096, chunk_pts=524288, data_type="blender",
                           gpu_ids=[0], rank=0)


def grads_of(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


# 7. geometry on but unused
@pytest.mark.parametrize("with_grid", [False, True], ids=["full", "train_occupancy"])
@pytest.mark.parametrize("family", sorted(NETS))
def test_geometry_on_but_unused_leaves_every_gradient_as_it_was(family, with_grid):
    n, Sc, Nf = 96, 64, 64
    _, model = make_model(*NETS[family])
    opts = make_opts(Sc, Nf)
    rays = lego_rays(n, 2)
    g = torch.Generator().manual_seed(21)
    t_rand, u, tgt = torch.rand(n, Sc, generator=g).to(DEV), torch.rand(n, Nf, generator=g).to(DEV), torch.rand(n, 3, generator=g).to(DEV)
    kw = dict(t_rand=t_rand, u=u, f16s=family == "f16s")
    if with_grid:
        kw["train_occupancy"] = random_grid(seed=5)
    results = []
    for extra in ({}, {"geometry": True}):
        model.zero_grad(set_to_none=True)
        out = NP.render_rays(rays, model, None, opts, **kw, **extra)
        (torch.mean((out["rgb_c"] - tgt) ** 2) + torch.mean((out["rgb_f"] - tgt) ** 2)).backward()
        results.append((out, grads_of(model)))
    (plain, g_plain), (geo, g_geo) = results
    assert sorted(plain) == ["disp_c", "disp_f", "rgb_c", "rgb_f"]
    assert sorted(set(geo) - set(plain)) == ["acc_c", "acc_f", "depth_c", "depth_f", "distortion_c", "distortion_f"]
    assert all(geo[k].shape == (n,) and geo[k].requires_grad for k in set(geo) - set(plain))
    assert all(torch.equal(geo[k], plain[k]) for k in plain)
    assert sorted(g_geo) == sorted(g_plain) and len(g_plain) == 2 * (2 * NETS[family][0] + 8)
    assert [k for k in g_plain if not torch.equal(g_geo[k], g_plain[k])] == []


# 8. geometry used
def _staged_path(model, rays, z, mask, module):
    """The code from before this change, driven stage by stage: ops.mlp_rays_train -> (raw zeroed where the mask says so) -> compositing;
    d_raw formed by hand from composite_geo_backward (zeroed likewise) -> ops.mlp_backward."""
    st = train_path._state_for(model, False)
    net = st.net
    flat = st.flat(st.params(module))
    blob = ops.pack_apply(st.map_fwd, flat)
    raw, stash = ops.mlp_rays_train(net, blob, rays, z)
    if mask is not None:
        m = mask.bool()[..., None]
        raw = torch.where(m, raw, torch.zeros_like(raw))
    rgb, _, acc, _, depth, dist = G.composite_geo(raw, z, rays, NEAR, FAR)

    def backward(g_rgb, g_acc, g_depth, g_dist):
        d_raw = G.composite_geo_backward(raw, z, rays, NEAR, FAR, g_rgb.contiguous(), g_acc.contiguous(), g_depth.contiguous(), g_dist.contiguous())
        if mask is not None:
            d_raw = torch.where(m, d_raw, torch.zeros_like(d_raw))
        grads, _ = ops.mlp_backward(net, blob, ops.pack_apply(st.map_bwd, flat), rays, z, d_raw, stash)
        return dict(zip(st.names, st.split_grads(grads)))
    return SimpleNamespace(rgb=rgb, acc=acc, depth=depth, distortion=dist, backward=backward)


def _geo_loss(out, tgt, a_t, d_t):
    """mse(rgb) + 0.1 mse(acc, a*) + 0.1 mean((depth - d*)^2) + 0.01 mean(distortion), for both networks."""
    loss = 0.0
    for k in ("c", "f"):
        loss = loss + torch.mean((out["rgb_" + k] - tgt) ** 2) + 0.1 * torch.mean((out["acc_" + k] - a_t) ** 2) \
            + 0.1 * torch.mean((out["depth_" + k] - d_t) ** 2) + 0.01 * torch.mean(out["distortion_" + k])
    return loss


@pytest.mark.parametrize("with_grid", [False, True], ids=["full", "train_occupancy"])
def test_geometry_losses_reach_the_parameters(with_grid):
    """(a) oracle/restate.py networks in float64 plus the restatement of the rule, autograd; (b) the staged code from before this change with d_raw
    formed by hand from composite_geo_backward; (c) the training node.  Depths pinned on all sides; per parameter tensor, relative to the
    tensor's largest entry: e_c <= max(3 e_b, 2e-5)."""
    D, W = NETS["fp32"]
    n, Sc, Nf = 96, 64, 64
    sd, model = make_model(D, W)
    opts = make_opts(Sc, Nf)
    rays = lego_rays(n, 2)
    g = torch.Generator().manual_seed(31)
    t_rand, u, tgt = torch.rand(n, Sc, generator=g).to(DEV), torch.rand(n, Nf, generator=g).to(DEV), torch.rand(n, 3, generator=g).to(DEV)
    a_t, d_t = torch.rand(n, generator=g).to(DEV), (NEAR + (FAR - NEAR) * torch.rand(n, generator=g)).to(DEV)
    grid = random_grid(seed=5) if with_grid else None
    z_c = ops.stratified_z(NEAR, FAR, t_rand)
    mask_c = grid.mark(rays, z_c) if with_grid else None
    w_c = ops.composite(_staged_raw(model, rays, z_c, mask_c, model.model_coarse), z_c, rays, want_all=True)[3]
    z_f = ops.fine_z(z_c, w_c, Nf, False, u)
    mask_f = grid.mark(rays, z_f) if with_grid else None
    # (b)
    bc, bf = _staged_path(model, rays, z_c, mask_c, model.model_coarse), _staged_path(model, rays, z_f, mask_f, model.model_fine)
    leaves = {k + "_" + s: getattr(b, k).clone().requires_grad_(True) for s, b in (("c", bc), ("f", bf)) for k in ("rgb", "acc", "depth", "distortion")}
    _geo_loss(leaves, tgt, a_t, d_t).backward()
    grads_b = {"model_coarse." + k: v for k, v in bc.backward(*(leaves[k + "_c"].grad for k in ("rgb", "acc", "depth", "distortion"))).items()}
    grads_b.update({"model_fine." + k: v for k, v in bf.backward(*(leaves[k + "_f"].grad for k in ("rgb", "acc", "depth", "distortion"))).items()})
    # (c)
    model.zero_grad(set_to_none=True)
    if with_grid:
        out = OT.render_train(rays, model, opts, grid, t_rand=t_rand, u=u, z_override=(z_c, z_f), geometry=True)
    else:
        out = train_path.render_train(rays, model, opts, t_rand=t_rand, u=u, z_override=(z_c, z_f), geometry=True)
    for k in leaves:                                                 # the node's forward is the staged forward
        assert torch.equal(out[k], leaves[k].detach()), k
    _geo_loss(out, tgt, a_t, d_t).backward()
    grads_c = grads_of(model)
    # (a)
    psd = {k: torch.as_tensor(v).clone().float().requires_grad_(True) for k, v in sd.items()}
    r_cpu = rays.cpu()

    def oracle(prefix, z, mask):
        z = z.cpu()
        raw = R.mlp_forward(psd, prefix, R.embed(r_cpu, z, 10, 4), D, 63, 27, dtype=torch.float64).reshape(n, z.shape[1], 4)
        if mask is not None:
            raw = raw * mask.cpu().double()[..., None]
        rgb, acc, _, depth, dist = restate(raw, z.double(), r_cpu[:, 3:].double(), NEAR, FAR)
        return rgb, acc, depth, dist
    oc, of = oracle("model_coarse.", z_c, mask_c), oracle("model_fine.", z_f, mask_f)
    ref = {k + "_" + s: v for s, o in (("c", oc), ("f", of)) for k, v in zip(("rgb", "acc", "depth", "distortion"), o)}
    _geo_loss(ref, tgt.cpu().double(), a_t.cpu().double(), d_t.cpu().double()).backward()
    print()
    bad, worst_b, worst_c = [], 0.0, 0.0
    for k, _ in model.named_parameters():
        want = psd[k].grad.double()
        scale = float(want.abs().max())
        assert scale > 0.0, k
        e_b = float((grads_b[k].cpu().double() - want).abs().max()) / scale
        e_c = float((grads_c[k].cpu().double() - want).abs().max()) / scale
        worst_b, worst_c = max(worst_b, e_b), max(worst_c, e_c)
        print(f"[{'grid' if with_grid else 'full'}] {k}: staged path {e_b:.2e}, training node {e_c:.2e}")
        if not e_c <= max(3.0 * e_b, 2e-5):
            bad.append((k, e_c, e_b))
    print(f"[{'grid' if with_grid else 'full'}] worst per-tensor gradient error vs float64: staged path {worst_b:.2e}, training node {worst_c:.2e}")
    assert len(grads_c) == 2 * (2 * D + 8) and bad == []
    # the geometry terms alone reach the parameters: no colour term, a gradient that is not zero
    model.zero_grad(set_to_none=True)
    out = train_path.render_train(rays, model, opts, t_rand=t_rand, u=u, z_override=(z_c, z_f), geometry=True)
    (torch.mean((out["acc_f"] - a_t) ** 2)).backward()
    got = grads_of(model)
    assert all(k.startswith("model_fine.") for k in got) and any(float(v.abs().max()) > 0 for v in got.values())     # nothing goes to the coarse network


def _staged_raw(model, rays, z, mask, module):
    st = train_path._state_for(model, False)
    raw, _ = ops.mlp_rays_train(st.net, ops.pack_apply(st.map_fwd, st.flat(st.params(module))), rays, z)
    return raw if mask is None else torch.where(mask.bool()[..., None], raw, torch.zeros_like(raw))


# ---------------------------------------------------------------------------------------------------
# 9. inference
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [{}, {"f16s": True}, {"bf16": True}], ids=["fp32", "f16s", "bf16"])
def test_inference_outputs_equal_composite_on_the_intermediates(flags):
    sd, model = make_model(8, 256)
    packed = weights.PackedNeRF.from_state_dict(sd, DEV)
    opts = make_opts(64, 128)
    rays = lego_rays(200, 1)
    with torch.no_grad():
        out = NP.render_rays(rays, packed, None, opts, seed=5, geometry=True, return_intermediates=True, **flags)
        plain = NP.render_rays(rays, packed, None, opts, seed=5, **flags)
        assert sorted(plain) == ["disp_c", "disp_f", "rgb_c", "rgb_f"] and all(torch.equal(out[k], plain[k]) for k in plain)
        for key in ("c", "f"):
            _, _, acc, _, depth = ops.composite(out["_raw_" + key], out["_z_" + key], rays, want_all=True)
            assert torch.equal(out["acc_" + key], acc) and torch.equal(out["depth_" + key], depth)
            assert torch.equal(out["distortion_" + key], G.composite_geo(out["_raw_" + key], out["_z_" + key], rays, NEAR, FAR)[5])
        if not flags:                                                # with a grid
            grid = random_grid(seed=3)
            occ = NP.render_rays(rays, packed, None, opts, seed=5, geometry=True, return_intermediates=True, occupancy=grid)
            _, _, acc, _, depth = ops.composite(occ["_raw_f"], occ["_z_f"], rays, want_all=True)
            assert torch.equal(occ["acc_f"], acc) and torch.equal(occ["depth_f"], depth) and occ["distortion_c"].shape == (200,)


def test_batchify_over_two_slabs_equals_one_slab(monkeypatch):
    sd, model = make_model(4, 128)
    packed = weights.PackedNeRF.from_state_dict(sd, DEV)
    opts = make_opts(64, 64)
    rays = lego_rays(200, 4)
    o, d = rays[:, :3].contiguous(), rays[:, 3:].contiguous()
    with torch.no_grad():
        one = NP.batchify_rays_and_render_by_chunk(o, d, packed, None, 800, 800, None, opts, seed=8, geometry=True)
        assert len(NP.batchify_rays_and_render_by_chunk(o, d, packed, None, 800, 800, None, opts, seed=8)) == 4
        monkeypatch.setattr(NP, "MAX_RAYS_PER_LAUNCH", 128)
        two = NP.batchify_rays_and_render_by_chunk(o, d, packed, None, 800, 800, None, opts, seed=8, geometry=True)
    assert len(one) == len(two) == 5 and sorted(one[4]) == ["acc_c", "acc_f", "depth_c", "depth_f", "distortion_c", "distortion_f"]
    assert all(torch.equal(a, b) for a, b in zip(one[:4], two[:4]))
    assert all(one[4][k].shape == (200,) and torch.equal(one[4][k], two[4][k]) for k in one[4])
    # the training path: a fifth element with a graph
    _, m = make_model(4, 128)
    monkeypatch.setattr(train_path, "MAX_TRAIN_RAYS", 128)
    res = NP.batchify_rays_and_render_by_chunk(o, d, m, None, 800, 800, None, opts, seed=8, geometry=True)
    assert len(res) == 5 and all(v.shape == (200,) and v.requires_grad for v in res[4].values())
    torch.mean(res[4]["distortion_f"]).backward()
    assert any(p.grad is not None and float(p.grad.abs().max()) > 0 for p in m.model_fine.parameters())


# ---------------------------------------------------------------------------------------------------
# 10. the fog goes down
# ---------------------------------------------------------------------------------------------------
def test_the_fog_goes_down():
    """scenes.SolidScene.default(), 12 views 48 x 48, a 4 x 128 network, 300 plain steps; then 300 more from that checkpoint twice, on the same
    ray batches: arm A plain, arm B with opts.geometry = {acc_weight 0.1, distortion_weight 0.01 (mip-NeRF 360's), targets: the scene}.  A grid
    baked from each arm (box +-1.5, 64^3, sub 2, sigma_min 0, no dilation) has fewer occupied cells in B, and over the held-out rays that meet
    nothing the mean rendered acc_f is smaller in B: both are what the added terms minimise.  Held-out PSNR is printed, not asserted."""
    warm, more, views, H = 300, 300, 12, 48
    W = H
    torch.manual_seed(0)
    opts = SimpleNamespace(near=NEAR, far=FAR, N_samples_c=64, N_samples_f=128, perturb=1.0, chunk_rays=4096, chunk_pts=524288, data_type="blender",
                           gpu_ids=[0], rank=0, exp_name="geo", N_rays=1024, global_batch=True, idx_save=1 << 30, idx_print=1 << 30, precision="fp32")
    scene = scenes.SolidScene.default()
    K = scenes.scaled_camera((H, W))
    posenc = get_positional_encoder(10), get_positional_encoder(4)
    poses = harness.get_render_pose(n_angle=views + 2, phi=-30.0, nf=4.0)
    images = scene.render_views(poses, K, (H, W), NEAR, FAR, 1024, DEV)
    i_train, i_test = list(range(views)), [views]
    model = NeRF(4, 128, 63, 27, skips=[4]).to(DEV)
    optimizer = torch.optim.Adam(model.parameters(), lr=5e-4, betas=(0.9, 0.999))
    criterion = torch.nn.MSELoss()
    getter = harness.global_batch(images, K, poses, i_train, (H, W), DEV)
    cam = (K, poses.numpy())
    NP.manual_seed(7)
    for i in range(1, warm + 1):
        harness.train(i, i_train, images, cam, (H, W), model, criterion, posenc, optimizer, getter, None, opts)
    ckpt = (copy.deepcopy(model.state_dict()), copy.deepcopy(optimizer.state_dict()))
    rng = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)      # the getter reshuffles on the device at every epoch
    o, d = ops.make_o_d(W, H, K, poses[views][:3, :4], DEV)
    held = torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1).contiguous()
    empty = scene.render(held, NEAR, FAR)[2] == 0.0
    assert 50 < int(empty.sum()) < held.shape[0] - 50

    def arm(geometry):
        m = NeRF(4, 128, 63, 27, skips=[4]).to(DEV)
        m.load_state_dict(ckpt[0])
        opt = torch.optim.Adam(m.parameters(), lr=5e-4, betas=(0.9, 0.999))
        opt.load_state_dict(copy.deepcopy(ckpt[1]))
        get = copy.deepcopy(getter)                                  # the same ray batches in both arms
        torch.set_rng_state(rng[0])
        torch.cuda.set_rng_state(rng[1], DEV)
        NP.manual_seed(1001)
        a = SimpleNamespace(**vars(opts), geometry=geometry)
        last = None
        for i in range(warm + 1, warm + more + 1):
            last = harness.train(i, i_train, images, cam, (H, W), m, criterion, posenc, opt, get, None, a)
        m.eval()
        with torch.no_grad():
            fraction = OC.OccupancyGrid(-1.5, 1.5, 64).bake(m, sub=2, sigma_min=0.0, dilate=0).fraction()
            NP.manual_seed(123)                                      # the same jitter for every held-out render
            packed = weights.packed_for(m)
            acc = NP.render_rays(held, packed, None, opts, seed=3, geometry=True)["acc_f"]
            psnr = harness.test(warm + more, i_test, posenc, packed, images[i_test], K, poses[i_test].to(DEV), (H, W), opts)["psnr"][0]
        return SimpleNamespace(fraction=float(fraction), fog=float(acc[empty].mean()), psnr=psnr, last=last)

    A = arm(None)
    B = arm({"acc_weight": 0.1, "distortion_weight": 0.01, "targets": scene})
    assert "loss_acc" not in A.last and {"loss_acc", "loss_distortion"} <= set(B.last) and "loss_depth" not in B.last
    print(f"\n[fog] occupied fraction of the 64^3 grid: plain {A.fraction:.4f}, geometry {B.fraction:.4f}; mean acc_f over {int(empty.sum())} held-out "
          f"rays that meet nothing: plain {A.fog:.5f}, geometry {B.fog:.5f}; held-out PSNR plain {A.psnr:.3f} dB, geometry {B.psnr:.3f} dB; "
          f"last step of B: loss_acc {float(B.last['loss_acc']):.3e}, loss_distortion {float(B.last['loss_distortion']):.3e}")
    assert B.fraction < A.fraction, (A.fraction, B.fraction)
    assert B.fog < A.fog, (A.fog, B.fog)
