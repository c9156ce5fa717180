"""GPU parity of the training path: gradients from the HIP backward kernels,
called through the C ABI, against torch autograd run on the CPU oracle (oracle/restate.py) with the same inputs.
Tolerances are stated per test; gradients are compared relative to the largest entry of the same tensor."""
import pytest
import torch

from nerf_pytorch_paeng_amd import ops, synthetic
from oracle import restate as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def rel_err(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = float(b.abs().max())
    return float((a - b).abs().max()) / (scale if scale > 0 else 1.0)


def _composite_case(n, S, seed, hard=False):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(n, S, 4, generator=g)
    raw[..., 3] = raw[..., 3] * (30.0 if hard else 3.0)         # hard: saturated alphas (u_i -> 1e-10) and many relu-dead samples
    z = torch.sort(2.0 + 4.0 * torch.rand(n, S, generator=g), -1).values
    d = torch.randn(n, 3, generator=g)
    o = torch.randn(n, 3, generator=g)
    G = torch.randn(n, 3, generator=g)
    return raw, z, torch.cat([o, d], -1), G


@pytest.mark.parametrize("n,S,hard", [(37, 64, False), (5, 192, False), (3, 1, False), (9, 7, False), (4, 300, False), (33, 64, True)])
def test_composite_backward_vs_autograd(n, S, hard):
    raw, z, rays, G = _composite_case(n, S, 100 + S, hard)
    raw_a = raw.clone().requires_grad_(True)
    rgb = R.post_process(raw_a, z, rays[:, 3:])[0]
    (rgb * G).sum().backward()
    want = raw_a.grad
    got = ops.composite_backward(raw.to(DEV), z.to(DEV), rays.to(DEV), G.to(DEV))
    # colour channels: products of fp32 forward quantities -> 1e-5 relative; density channel passes through a division
    # by (1 - alpha + 1e-10) and a suffix sum -> 1e-4 relative to the largest entry
    assert rel_err(got[..., :3], want[..., :3]) < 1e-5
    assert rel_err(got[..., 3], want[..., 3]) < 1e-4
    # bare direction tensor ([n,3]) form of the same call
    got3 = ops.composite_backward(raw.to(DEV), z.to(DEV), rays[:, 3:].contiguous().to(DEV), G.to(DEV))
    assert torch.equal(got3, got)


def test_composite_backward_empty_and_errors():
    e = ops.composite_backward(torch.empty(0, 8, 4, device=DEV), torch.empty(0, 8, device=DEV), torch.empty(0, 6, device=DEV),
                               torch.empty(0, 3, device=DEV))
    assert e.shape == (0, 8, 4)
    with pytest.raises(ops.MiNerfError):
        ops.composite_backward(torch.zeros(2, 8, 4, device=DEV), torch.zeros(2, 8, device=DEV), torch.zeros(2, 6, device=DEV),
                               torch.zeros(2, 4, device=DEV))


# ---------------------------------------------------------------------------------------------------
# MLP: stash forward, backward data, backward weights
# ---------------------------------------------------------------------------------------------------
def _mlp_case(D, W, skip, n, S, seed):
    net = ops.make_net(D, W, skip)
    sd = synthetic.make_state_dict(seed, D, W, skips=(skip,) if skip >= 0 else ())
    g = torch.Generator().manual_seed(seed + 7)
    o = torch.tensor([0.0, 0.0, 4.0]) + 0.2 * torch.randn(n, 3, generator=g)
    d = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, -1.0]) + 0.3 * torch.randn(n, 3, generator=g), dim=-1) * 1.1
    rays = torch.cat([o, d], -1).contiguous()
    z = torch.sort(2.0 + 4.0 * torch.rand(n, S, generator=g), -1).values
    d_raw = torch.randn(n, S, 4, generator=g)
    return net, sd, rays, z, d_raw


def _oracle_backward(net, sd, prefix, rays, z, d_raw):
    """autograd on the CPU oracle: parameter gradients (state_dict keys) + per-layer taps"""
    names = ops.param_names(net)
    psd = {prefix + k: torch.as_tensor(sd[prefix + k]).clone().float().requires_grad_(True) for k in names}
    x = R.embed(rays, z, net.L_x, net.L_d)
    taps = {}
    skips = (net.skip,) if net.skip >= 0 else ()
    out = R.mlp_forward(psd, prefix, x, net.D, 3 + 6 * net.L_x, 3 + 6 * net.L_d, skips, taps=taps)
    (out * d_raw.reshape(-1, 4)).sum().backward()
    return out.detach(), {k: psd[prefix + k].grad for k in names}, taps


# The deep cases (docs/design/10_training_path.md, "Depths 11-16").  A network has D + 1 wide weight-gradient products and a launch takes
# WG_MAXB = 12: D = 11 is one batch of exactly 12 (skip at D - 2, the last position at which one fires); D = 12 flushes behind linear_feat
# and runs linear_d as a batch of one (at 3072 points and more -- the 32 x 96 case -- on every CU, the partial buffer exactly full); D = 13
# flushes inside the trunk loop with the concatenated layer (12) last in the first batch; D = 16 has it (13) first in the second; D = 15 is
# dgrad_f16s_kernel's largest LDS footprint and D = 14 the split-precision forward's; (16, 128) the W = 128 kernels at the maximum depth,
# skip at the last position.
DEEP_BACKWARD_CASES = [(11, 256, 9, 24, 40, False), (12, 256, 4, 24, 40, False), (12, 256, 4, 24, 40, True), (12, 256, 4, 32, 96, False),
                       (13, 256, 11, 24, 40, False), (13, 256, 11, 24, 40, True), (14, 256, 12, 24, 40, True), (15, 256, 13, 24, 40, True),
                       (16, 256, 12, 24, 40, False), (16, 256, 12, 24, 40, True), (16, 128, 14, 10, 33, False)]


@pytest.mark.parametrize("D,W,skip,n,S,f16s", [(8, 256, 4, 24, 40, False), (4, 128, 1, 10, 33, False), (3, 256, -1, 7, 64, False),
                                                (8, 256, 4, 24, 40, True), (3, 256, -1, 7, 64, True), (2, 256, 0, 5, 33, True)] + DEEP_BACKWARD_CASES)
def test_mlp_backward_vs_autograd(D, W, skip, n, S, f16s):
    """Stash, per-layer gradients and parameter gradients of one network against autograd on the CPU oracle, stage by stage.
    ``f16s``: the three MFMA kernels in split precision (mlp_f16s_kernel<STASH>, dgrad_f16s_kernel, wgrad_f16s_kernel) -- same bars.
    Each of the three runs in split precision at the depths it has LDS for (ops.F16S_FWD_MAX_D = 14, ops.F16S_DGRAD_MAX_D = 15: the rule the
    training path applies); past its limit a kernel's refusal is asserted -- by name, before any launch -- and the fp32 kernel takes its place
    over the same stash layout: D = 15 is fp32 forward + split-precision backward, D = 16 fp32 forward and backward data + split-precision
    weight gradients."""
    net, sd, rays, z, d_raw = _mlp_case(D, W, skip, n, S, 11 + D)
    prefix = "model_coarse."
    _, _, taps0 = _oracle_backward(net, sd, prefix, rays, z, d_raw)               # forward taps (pre-activations) of the oracle
    packed = ops.pack_module(sd, prefix, net).to(DEV)
    raysd, zd, d_rawd = rays.to(DEV), z.to(DEV), d_raw.to(DEV)
    fwd_f16s = f16s and D <= ops.F16S_FWD_MAX_D
    packed_fwd = ops.pack_module(sd, prefix, net, f16s=True).to(DEV) if f16s else packed
    if f16s and not fwd_f16s:                                  # the blob packs at any depth up to 16 (the f16 kernel reads it); the forward launches refuse it
        for entry in (ops.mlp_rays_train, ops.mlp_rays):
            with pytest.raises(ops.MiNerfError, match=r"D = %d does not fit \(D <= 14\)" % D):
                entry(net, packed_fwd, raysd, zd, f16s=True)
        packed_fwd = packed
    bw = dict(f16s_wgrad=f16s, f16s_dgrad=f16s and ops.f16s_dgrad_fits(net))
    packed_bwd = ops.pack_module(sd, prefix, net, backward=True, f16s=bw["f16s_dgrad"]).to(DEV)      # the blob the chosen backward-data kernel reads
    P = n * S

    # 1. training forward == inference forward, and the stash holds the post-activation rows
    raw, stash = ops.mlp_rays_train(net, packed_fwd, raysd, zd, f16s=fwd_f16s)
    assert torch.equal(raw, ops.mlp_rays(net, packed_fwd, raysd, zd, f16s=fwd_f16s))
    if D > ops.F16S_DGRAD_MAX_D:                               # argument checking, before any launch: whatever blob and stage are passed
        with pytest.raises(ops.MiNerfError, match=r"D <= 15"):
            ops.mlp_backward(net, packed, packed_bwd, raysd, zd, d_rawd, stash, stage=1, f16s_wgrad=f16s, f16s_dgrad=True)
    # A unit whose pre-activation is within rounding of zero has an ambiguous ReLU derivative: the kernel and the oracle may take different
    # sides, and one such unit changes its point's contribution to every gradient below it.  Points where the two forwards disagree on a
    # sign (a few in a thousand for the split-precision forward, rarer for the fp32 one) get a zero output gradient on both sides.
    v0 = ops.train_views(net, n, S, stash=stash)
    knife = ((v0["stash_g"].cpu() > 0) != (taps0["ad"].detach() > 0)).any(dim=1)
    for l in range(D):
        knife |= ((v0["stash_h"][l].cpu() > 0) != (taps0[f"a{l}"].detach() > 0)).any(dim=1)
    assert int(knife.sum()) <= max(3, P // 100), int(knife.sum())
    d_raw = (d_raw.reshape(-1, 4) * (~knife).float()[:, None]).reshape(n, S, 4).contiguous()
    d_rawd = d_raw.to(DEV)
    raw_want, grads_want, taps = _oracle_backward(net, sd, prefix, rays, z, d_raw)
    assert rel_err(raw.reshape(-1, 4), raw_want) < 2e-5
    v = ops.train_views(net, n, S, stash=stash)
    e_stash = [rel_err(v["stash_h"][l], torch.relu(taps[f"a{l}"]).detach()) for l in range(D)]
    e_stash += [rel_err(v["stash_f"], taps["feat"].detach()), rel_err(v["stash_g"], torch.relu(taps["ad"]).detach())]
    print(f"backward D={D} W={W} skip={skip} P={P}{' (split precision)' if f16s else ''}: knife points {int(knife.sum())}, raw {rel_err(raw.reshape(-1, 4), raw_want):.2e}, "
          f"worst stash row {max(e_stash):.2e}")
    for l in range(D):
        assert e_stash[l] < 2e-5, f"stash_h[{l}]"
    assert e_stash[D] < 2e-5
    assert e_stash[D + 1] < 2e-5

    # 2. backward data: per-layer pre-activation gradients.  A ReLU whose pre-activation is within rounding of zero can
    # flip between the two implementations (its derivative there is either answer): the flipped entry is excluded by comparing
    # only where the oracle's pre-activation is clear of zero, and the POINT it belongs to is excluded from every layer below it
    # (one flipped unit of layer l changes that point's whole gradient row in layers < l).  Such points are rare.
    _, work = ops.mlp_backward(net, packed, packed_bwd, raysd, zd, d_rawd, stash, stage=1, **bw)
    w = ops.train_views(net, n, S, work=work)
    flipped = {l: ((v["stash_h"][l].cpu() > 0) != (taps[f"a{l}"].detach() > 0)).any(dim=1) for l in range(D)}      # [P] per layer
    flipped_d = ((v["stash_g"].cpu() > 0) != (taps["ad"].detach() > 0)).any(dim=1)
    def masked_err(got, tapname, rows_ok):
        want, pre = taps[tapname].grad, taps[tapname].detach()
        clear = (pre.abs() > 1e-4).float() * rows_ok.float()[:, None]
        scale = float(want.abs().max())
        return float(((got.cpu() - want) * clear).abs().max()) / scale
    ok = ~flipped_d
    e_dd = masked_err(w["delta_d"], "ad", torch.ones(P, dtype=torch.bool))
    e_df = float(((w["delta_f"].cpu() - taps["feat"].grad) * ok.float()[:, None]).abs().max()) / float(taps["feat"].grad.abs().max())
    e_dh = {}
    for l in range(D - 1, -1, -1):
        e_dh[l] = masked_err(w["delta_h"][l], f"a{l}", ok)
        ok = ok & ~flipped[l]
    print(f"  delta_d {e_dd:.2e}, delta_f {e_df:.2e}, worst delta_h {max(e_dh.values()):.2e} (layer {max(e_dh, key=e_dh.get)}), points dropped {int((~ok).sum())}")
    assert e_dd < 1e-5
    assert e_df < 5e-5
    for l in range(D - 1, -1, -1):
        assert e_dh[l] < 1e-4, f"delta_h[{l}]"
    assert int((~ok).sum()) <= max(2, P // 200), int((~ok).sum())

    # 3. full backward: flat parameter gradient in module.parameters() order
    grads, _ = ops.mlp_backward(net, packed, packed_bwd, raysd, zd, d_rawd, stash, **bw)
    off, e_par = 0, {}
    for k in ops.param_names(net):
        want = grads_want[k]
        got = grads[off:off + want.numel()].reshape(want.shape)
        off += want.numel()
        e_par[k] = rel_err(got, want)
    print(f"  worst parameter gradient {max(e_par.values()):.2e} ({max(e_par, key=e_par.get)}; relative to the tensor's largest entry)")
    for k, e in e_par.items():
        assert e < 2e-4, k
    assert off == grads.numel() == ops.param_count(net)
    # the flat vector is allocated uninitialised (torch.empty): every element must be WRITTEN by the weight-gradient kernels
    poison = torch.full((ops.param_count(net),), float("nan"), device=DEV)
    again, _ = ops.mlp_backward(net, packed, packed_bwd, raysd, zd, d_rawd, stash, grads=poison, **bw)
    assert again.data_ptr() == poison.data_ptr() and torch.isfinite(poison).all() and torch.equal(poison, grads)


def _device_pack_matches_host_pack(D, W, skip):
    net = ops.make_net(D, W, skip)
    sd = synthetic.make_state_dict(3, D, W, skips=(skip,))
    prefix = "model_fine."
    flat = ops.flatten_params(sd, prefix, net, DEV)
    for backward in (False, True):
        host = ops.pack_module(sd, prefix, net, backward=backward)
        dev = ops.pack_apply(ops.pack_map(net, backward).to(DEV), flat).cpu()
        assert torch.equal(host[1024:], dev[1024:])            # everything but the (unused on device) header
    return net, sd, prefix, flat


def test_device_pack_matches_host_pack():
    _device_pack_matches_host_pack(8, 256, 4)


@pytest.mark.parametrize("W", [256, 128])
def test_device_pack_matches_host_pack_at_the_maximum_depth(W):
    """D = 16, skip at the last position at which one fires: the depth-indexed tables (w_x[16], b_x[16], in_l[16]) at their last entry and the
    longest streams (bwd_stream_bytes(16, W)) through the gather maps -- fp32 forward and backward blobs, and (W = 256) the bf16 blob."""
    net, sd, prefix, flat = _device_pack_matches_host_pack(16, W, 14)
    assert flat.numel() == ops.param_count(net) == sum(torch.as_tensor(sd[prefix + k]).numel() for k in ops.param_names(net))
    if W == 256:
        assert torch.equal(ops.pack_module(sd, prefix, net, bf16=True), ops.pack_apply_bf16(net, ops.pack_map_bf16(net).to(DEV), flat).cpu())


def test_device_bf16_pack_matches_host_pack_and_serves_module_models():
    """The bf16 blob packed on the device from the flat parameter vector equals the host packer's, header included; an nn.Module
    model rendered with bf16=True goes through it (no host round trip per call) and gives the PackedNeRF result."""
    from types import SimpleNamespace
    from nerf_pytorch_paeng_amd import nerf_process as NP, weights
    from nerf_pytorch_paeng_amd.model import NeRF
    net = ops.make_net(8, 256, 4)
    sd = synthetic.make_state_dict(3, 8, 256)
    m = ops.pack_map_bf16(net).to(DEV)
    for prefix in ("model_coarse.", "model_fine."):
        host = ops.pack_module(sd, prefix, net, bf16=True)
        dev = ops.pack_apply_bf16(net, m, ops.flatten_params(sd, prefix, net, DEV)).cpu()
        assert torch.equal(host, dev)
    model = NeRF(8, 256, 63, 27).to(DEV)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    packed = weights.PackedNeRF.from_state_dict(sd, DEV)
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=16, N_samples_f=16, perturb=1.0, chunk_rays=4096, chunk_pts=524288,
                           data_type="blender", gpu_ids=[0], rank=0)
    K, H, Wd = synthetic.lego_camera()
    pix = torch.from_numpy(synthetic.pixel_batch(H, Wd, 128, 1)).to(DEV)
    o, d = ops.make_o_d_pixels(Wd, H, K, synthetic.pose_spherical(30.0, -30.0, 4.0), pix)
    with torch.no_grad():
        a = NP.batchify_rays_and_render_by_chunk(o, d, model, None, H, Wd, K, opts, seed=5, bf16=True)
        b = NP.batchify_rays_and_render_by_chunk(o, d, packed, None, H, Wd, K, opts, seed=5, bf16=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------
# whole training step through the drop-in surface (train.py:53-70)
# ---------------------------------------------------------------------------------------------------
def _train_setup(D=8, W=256, n=96, Sc=32, Nf=48, seed=0):
    from types import SimpleNamespace
    from nerf_pytorch_paeng_amd.model import NeRF, get_positional_encoder
    sd = synthetic.make_state_dict(seed, D, W)
    model = NeRF(D, W, 63, 27).to(DEV)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    posenc = get_positional_encoder(10), get_positional_encoder(4)
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=Sc, N_samples_f=Nf, perturb=1.0, chunk_rays=4096, chunk_pts=524288,
                           data_type="blender", gpu_ids=[0], rank=0)
    K, H, Wd = synthetic.lego_camera()
    pose = synthetic.pose_spherical(30.0, -30.0, 4.0)
    pix = torch.from_numpy(synthetic.pixel_batch(H, Wd, n, 1)).to(DEV)
    o, d = ops.make_o_d_pixels(Wd, H, K, pose, pix)
    g = torch.Generator().manual_seed(seed + 1)
    t_rand, u, target = torch.rand(n, Sc, generator=g), torch.rand(n, Nf, generator=g), torch.rand(n, 3, generator=g)
    cfg = R.PathConfig(near=2.0, far=6.0, N_samples_c=Sc, N_samples_f=Nf, perturb=1.0, netDepth=D, netWidth=W)
    return sd, model, posenc, opts, o, d, t_rand, u, target, cfg


# Xavier networks of 12 and more layers are mostly badly conditioned for a whole step: on this batch, over seeds 0..44, the density of one of
# the two networks is dead on every sample for about half the seeds (all-zero gradients), and where it is not, the reference's OWN fp32
# gradients sit 1e-4 .. 1e-2 (of a tensor's largest entry) from the same step with the MLP in fp64 -- seed 0: D = 12 1.9e-4, D = 14 and 16
# dead coarse networks.  The deep cases therefore use, per depth, a seed chosen on the CPU from the reference alone: both densities alive,
# no all-zero gradient tensor, and the smallest fp32-to-fp64 distance of the scan (D = 12 seed 1: 1.2e-5, densities positive at 0.63 / 0.59
# of the samples; D = 14 seed 3: 7e-7, 0.08 / 0.03; D = 16 seed 35: 1.1e-6, 0.79 / 0.45).  The bar is the function's, 1e-4.
DEEP_STEP_SEEDS = {12: 1, 14: 3, 16: 35}


@pytest.mark.parametrize("D,W,f16s", [(8, 256, False), (8, 256, True), (8, 64, False), (6, 100, False), (8, 200, False), (8, 200, True), (8, 64, True),
                                      (12, 256, False), (16, 256, True), (16, 256, False), (14, 256, True)])
def test_train_step_gradients_match_oracle_autograd(D, W, f16s):
    """``f16s``: the same step with its three MFMA kernels in split precision, same bars.  Widths without training kernels of their own
    (--netWidth 64 / 100 / 200, config.py:57) train as the next wider network, the parameters scattered into zeros and the gradient gathered
    back (weights.pad_index_map): same bars, per parameter tensor of the MODULE's own shape.
    Depths past 11 split the weight-gradient batch (12: behind linear_feat; 16: inside the trunk loop, the maximum depth).  The split-precision
    forward has LDS for D <= 14: (14, f16s) is its largest footprint and ends in the range-word read of end_f16s_step; (16, f16s) is refused
    by name before the step starts."""
    from nerf_pytorch_paeng_amd import nerf_process as NP, train_path
    sd, model, posenc, opts, o, d, t_rand, u, target, cfg = _train_setup(D=D, W=W, seed=DEEP_STEP_SEEDS.get(D, 0))
    rays = torch.cat([o, d], -1).contiguous()
    if f16s and D > ops.F16S_FWD_MAX_D:
        with pytest.raises(ops.MiNerfError, match=r"D = %d does not fit \(D <= 14\)" % D):
            train_path.render_train(rays, model, opts, t_rand=t_rand, u=u, f16s=True)
        assert train_path.render_train(rays, model, opts, t_rand=t_rand, u=u)["rgb_f"].requires_grad      # ... and the same model still trains in fp32
        return
    # the oracle's coarse depths and OUR fine depths are pinned on both sides: the forward is ill-conditioned in z
    # (1 ulp of z moves raw by up to 5e-4 through the 2^9 frequency) and sample_pdf is discontinuous, neither of which is
    # what this test is about
    with torch.no_grad():
        z_f = NP.render_rays(rays, model, posenc, opts, t_rand=t_rand, u=u, return_intermediates=True)["_z_f"]
    z_c = R.stratified_z(rays.shape[0], cfg.near, cfg.far, cfg.N_samples_c, t_rand)
    psd = {k: torch.as_tensor(v).clone().float().requires_grad_(True) for k, v in sd.items()}
    ref = R.render_rays(rays.cpu(), psd, cfg, t_rand, u, z_fine_override=z_f.cpu())
    loss_ref = torch.mean((ref["rgb_c"] - target) ** 2) + torch.mean((ref["rgb_f"] - target) ** 2)      # train.py:60-66
    loss_ref.backward()

    out = train_path.render_train(rays, model, opts, t_rand=t_rand, u=u, z_override=(z_c.to(DEV), z_f), f16s=f16s)
    tgt = target.to(DEV)
    loss = torch.mean((out["rgb_c"] - tgt) ** 2) + torch.mean((out["rgb_f"] - tgt) ** 2)
    loss.backward()
    assert abs(loss.item() - loss_ref.item()) < 1e-5
    assert not out["disp_c"].requires_grad and not out["disp_f"].requires_grad
    worst = 0.0
    for k, p in model.named_parameters():
        assert p.grad is not None and p.grad.shape == psd[k].grad.shape, k
        e = rel_err(p.grad, psd[k].grad)
        worst = max(worst, e)
        assert e < 1e-4, (k, e)                                      # relative to the largest entry of that gradient
    print(f"train step D={D} W={W}{' (split precision)' if f16s else ''}: worst per-tensor gradient error {worst:.2e} (relative to max)")
    if f16s and D > 8:                                               # the step ended in end_f16s_step's read (it raises on saturation): one step counted, nothing out of range
        st = train_path._states[model][256]
        assert st.f16s_steps == 1 and st.f16s_steps_since_read == 0 and train_path.f16s_status(model, reset=False)["saturated"] is False
    if W not in (128, 256):                                          # ... and an optimizer step on it keeps working (the state is re-padded per step)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        opt.step()
        out2 = train_path.render_train(rays, model, opts, t_rand=t_rand, u=u, z_override=(z_c.to(DEV), z_f), f16s=f16s)
        assert torch.isfinite(out2["rgb_f"]).all() and not torch.equal(out2["rgb_f"], out["rgb_f"])
    if W == 64 and f16s:
        # the training width depends on the precision: netWidth 64 trains 256 wide in split precision (the only width those kernels have)
        # and 128 wide in fp32 -- one state per kernel width for the same module, either order
        out3 = train_path.render_train(rays, model, opts, t_rand=t_rand, u=u, z_override=(z_c.to(DEV), z_f), f16s=False)
        assert torch.isfinite(out3["rgb_f"]).all() and float((out3["rgb_f"] - out2["rgb_f"]).abs().max()) < 1e-4
        assert sorted(train_path._states[model]) == [128, 256]
        assert train_path.f16s_status(model, reset=False)["weights_out_of_range"] == 0


def test_drop_in_training_loop_runs_and_repacks():
    """loss.backward(); optimizer.step() through batchify_rays_and_render_by_chunk, as train.py:53-70 does."""
    from nerf_pytorch_paeng_amd import nerf_process as NP
    sd, model, posenc, opts, o, d, t_rand, u, target, cfg = _train_setup(D=4, W=128, n=64)
    K, H, Wd = synthetic.lego_camera()
    optim = torch.optim.Adam(model.parameters(), lr=5e-4, betas=(0.9, 0.999))           # main.py:79-80
    tgt = target.to(DEV)
    losses = []
    for it in range(3):
        rgb_c, disp_c, rgb_f, disp_f = NP.batchify_rays_and_render_by_chunk(o, d, model, posenc, H, Wd, K, opts, t_rand=t_rand, u=u)
        optim.zero_grad()
        loss = torch.nn.functional.mse_loss(rgb_c, tgt) + torch.nn.functional.mse_loss(rgb_f, tgt)
        loss.backward()
        optim.step()
        losses.append(loss.item())
    assert losses[2] < losses[0], losses                            # same batch, same jitter: Adam must make progress
    # after the step the inference path (re-packed on the parameter version bump) sees the same new weights
    with torch.no_grad():
        a = NP.batchify_rays_and_render_by_chunk(o, d, model, posenc, H, Wd, K, opts, t_rand=t_rand, u=u)
    b = NP.batchify_rays_and_render_by_chunk(o, d, model, posenc, H, Wd, K, opts, t_rand=t_rand, u=u)
    assert b[0].requires_grad and not a[0].requires_grad
    assert torch.equal(a[0], b[0].detach()) and torch.equal(a[2], b[2].detach())


@pytest.mark.parametrize("Sc,Nf", [(40, 0), (24, 17)])
def test_train_step_variants_small_net(Sc, Nf):
    """4x128 network, sample counts that are not multiples of the 32-point tile, coarse-only training (N_samples_f = 0,
    nerf_process.py:249-252 returns None for the fine outputs)."""
    from nerf_pytorch_paeng_amd import nerf_process as NP, train_path
    sd, model, posenc, opts, o, d, t_rand, u, target, cfg = _train_setup(D=4, W=128, n=50, Sc=Sc, Nf=max(Nf, 1), seed=5)
    opts.N_samples_f = Nf
    cfg = R.PathConfig(near=2.0, far=6.0, N_samples_c=Sc, N_samples_f=Nf, perturb=1.0, netDepth=4, netWidth=128)
    u = u[:, :Nf] if Nf else None
    rays = torch.cat([o, d], -1).contiguous()
    z_c = R.stratified_z(rays.shape[0], cfg.near, cfg.far, Sc, t_rand)
    z_f = None
    if Nf:
        with torch.no_grad():
            z_f = NP.render_rays(rays, model, posenc, opts, t_rand=t_rand, u=u, return_intermediates=True)["_z_f"]
    psd = {k: torch.as_tensor(v).clone().float().requires_grad_(True) for k, v in sd.items()}
    ref = R.render_rays(rays.cpu(), psd, cfg, t_rand, u, z_fine_override=None if z_f is None else z_f.cpu())
    loss_ref = torch.mean((ref["rgb_c"] - target) ** 2)
    if Nf:
        loss_ref = loss_ref + torch.mean((ref["rgb_f"] - target) ** 2)
    loss_ref.backward()
    out = train_path.render_train(rays, model, opts, t_rand=t_rand, u=u, z_override=(z_c.to(DEV), z_f))
    tgt = target.to(DEV)
    loss = torch.mean((out["rgb_c"] - tgt) ** 2)
    if Nf:
        loss = loss + torch.mean((out["rgb_f"] - tgt) ** 2)
    else:
        assert "rgb_f" not in out
    loss.backward()
    assert abs(loss.item() - loss_ref.item()) < 1e-5
    for k, p in model.named_parameters():
        if not Nf and k.startswith("model_fine."):
            assert p.grad is None and psd[k].grad is None            # the fine network takes no part in a coarse-only step
            continue
        assert rel_err(p.grad, psd[k].grad) < 1e-4, k
    # drop-in surface: 4-tuple with None for the fine outputs when N_samples_f == 0
    K, H, Wd = synthetic.lego_camera()
    res = NP.batchify_rays_and_render_by_chunk(o, d, model, posenc, H, Wd, K, opts, t_rand=t_rand, u=u)
    assert res[0].requires_grad and (res[2] is None) == (Nf == 0)


def test_fine_loss_does_not_reach_coarse_network():
    """nerf_process.py:66 detaches the resampled depths: with a loss on rgb_f only, the coarse network gets no gradient --
    in the oracle (autograd through its own, un-pinned resampling) and in the product."""
    from nerf_pytorch_paeng_amd import train_path
    sd, model, posenc, opts, o, d, t_rand, u, target, cfg = _train_setup(D=4, W=128, n=40, Sc=24, Nf=24, seed=2)
    rays = torch.cat([o, d], -1).contiguous()
    psd = {k: torch.as_tensor(v).clone().float().requires_grad_(True) for k, v in sd.items()}
    ref = R.render_rays(rays.cpu(), psd, cfg, t_rand, u)
    torch.mean((ref["rgb_f"] - target) ** 2).backward()
    assert all(psd[k].grad is None for k in psd if k.startswith("model_coarse."))
    assert all(psd[k].grad is not None for k in psd if k.startswith("model_fine."))
    out = train_path.render_train(rays, model, opts, t_rand=t_rand, u=u)
    torch.mean((out["rgb_f"] - target.to(DEV)) ** 2).backward()
    for k, p in model.named_parameters():
        assert (p.grad is None) == k.startswith("model_coarse."), k


@pytest.mark.parametrize("P,M,N", [(5000, 256, 256), (4099, 128, 256), (3001, 256, 63), (777, 128, 27), (2500, 3, 128), (1999, 1, 256), (11, 256, 256), (1237, 192, 160), (1, 256, 256)])
def test_wgrad_product_vs_float64(P, M, N):
    """One weight-gradient product on its own (mi_nerf_wgrad_product) against a float64 matmul: every operand shape of the
    network, point counts that are not multiples of the 12-row load group."""
    g = torch.Generator().manual_seed(P + M)
    ldd = 256 if M > 4 else 4                      # d_raw has a row pitch of 4 floats
    ldx = 90 if N in (63, 27) else (256 if N > 128 else 128)
    d = torch.randn(P + 64, ldd, generator=g)
    x = torch.randn(P + 64, ldx, generator=g)
    d[P:] = float("nan")                           # rows past P must not contribute
    x[P:] = float("nan")
    want = d[:P, :M].double().T @ x[:P, :N].double()
    out, bias, _ = ops.wgrad_product(d.to(DEV), M, x.to(DEV), N, P)
    assert rel_err(out, want.float()) < 2e-6 * max(1.0, P ** 0.5 / 10)
    assert rel_err(bias, d[:P, :M].double().sum(0).float()) < 1e-5


def test_wgrad_products_batched_entry_equals_the_single_products():
    """mi_nerf_wgrad_products (several wide products over the same points in one launch -- the form the backward pass uses) against
    the same entry with ONE product per call, product by product, and against float64."""
    g = torch.Generator().manual_seed(5)
    P = 5000
    shapes = [(256, 256), (256, 128), (128, 256), (200, 252), (256, 256)]
    deltas = [torch.randn(P + 3, M, generator=g).to(DEV) for M, _ in shapes]
    xs = [torch.randn(P + 3, N, generator=g).to(DEV) for _, N in shapes]
    outs, biases, _ = ops.wgrad_products(deltas, xs, P)
    for d, x, o, b in zip(deltas, xs, outs, biases):
        o1, b1, _ = ops.wgrad_product(d, d.shape[1], x, x.shape[1], P)
        want = d[:P].double().T @ x[:P].double()
        assert rel_err(o, want) < 2e-5 and rel_err(b, d[:P].double().sum(0)) < 2e-5
        assert rel_err(o, o1) < 1e-5 and rel_err(b, b1) < 1e-5                   # different slice counts: same sums up to summation order
    # products with a narrow side (gamma(x), gamma(d), the heads) in the same call: each in a launch of its own behind the wide batch (the
    # wide ones share the CUs, so their slice counts -- and summation order -- differ from a lone product's); not in split precision
    nd, nx = deltas[0][:, :32].contiguous(), xs[0][:, :63].contiguous()
    mixed, mb, _ = ops.wgrad_products([deltas[0], nd, deltas[1], deltas[2]], [xs[0], xs[0], nx, xs[2]], P)
    assert rel_err(mixed[0], ops.wgrad_product(deltas[0], 256, xs[0], 256, P)[0]) < 1e-5 and rel_err(mixed[3], ops.wgrad_product(deltas[2], 128, xs[2], 256, P)[0]) < 1e-5
    assert torch.equal(mixed[1], ops.wgrad_product(nd, 32, xs[0], 256, P)[0])           # a narrow product is the same launch either way
    assert rel_err(mixed[1], nd[:P].double().T @ xs[0][:P].double()) < 2e-5 and rel_err(mixed[2], deltas[1][:P].double().T @ nx[:P].double()) < 2e-5
    assert rel_err(mb[1], nd[:P].double().sum(0)) < 2e-5 and rel_err(mb[2], deltas[1][:P].double().sum(0)) < 2e-5
    with pytest.raises(Exception, match="split-precision entry takes wide products"):
        ops.wgrad_products([nd], [xs[0]], P, f16s=True)
    # the same batch in split precision (wgrad_f16s_kernel through mi_nerf_wgrad_products_f16s): fp32-grade against float64, also with
    # gradient operands of very different magnitudes in one batch (one scale for the batch, from its largest entry) and tiny ones
    for scale in (1.0, 1e-6):
        ds = [d * (scale * (10.0 ** -i)) for i, d in enumerate(deltas)]
        outs_s, biases_s, _ = ops.wgrad_products(ds, xs, P, f16s=True)
        for d, x, o, b in zip(ds, xs, outs_s, biases_s):
            want = d[:P].double().T @ x[:P].double()
            assert rel_err(o, want) < 2e-5 and rel_err(b, d[:P].double().sum(0)) < 2e-5


def test_wgrad_product_beyond_4GiB_operands():
    """Operands larger than 4 GiB (the point count of a MAX_TRAIN_RAYS slab: 16384 rays x 256 samples x 1 KiB rows): the kernels
    rebase their buffer descriptors per 12-row group, so byte offsets never need more than 32 bits.  Rows are drawn from a short
    cycle so that the expected product is cheap: sum_p d[p]^T x[p] = sum over the cycle, weighted by how often each row occurs."""
    P, M, N, cyc = 4_300_001, 256, 256, 977                       # P * 1 KiB > 4 GiB; 977 prime: groups and slices see every phase
    g = torch.Generator().manual_seed(7)
    dc = torch.randn(cyc, M, generator=g).to(DEV)
    xc = torch.randn(cyc, N, generator=g).to(DEV)
    idx = torch.arange(P, device=DEV) % cyc
    d, x = dc[idx], xc[idx]                                       # [P, 256] each, 4.4 GB
    counts = torch.bincount(idx, minlength=cyc).double()
    want = (dc.double() * counts[:, None]).T @ xc.double()
    out, bias, _ = ops.wgrad_product(d, M, x, N, P)
    assert rel_err(out, want.float()) < 5e-5, rel_err(out, want.float())
    assert rel_err(bias, (dc.double() * counts[:, None]).sum(0).float()) < 5e-5
    # the far end alone (rows past the 4 GiB mark must be the ones read, not an alias of the start)
    d[: P - 1000] = 0
    out2, _, _ = ops.wgrad_product(d, M, x, N, P)
    tail_idx = idx[P - 1000:]
    want2 = dc[tail_idx].double().T @ xc[tail_idx].double()
    assert rel_err(out2, want2.float()) < 1e-5
    del d, x


def test_training_slabs_accumulate_like_one_node(monkeypatch):
    """Rays beyond MAX_TRAIN_RAYS are rendered as several autograd nodes; the parameter gradients must equal the
    single-node ones (jitter is keyed on the global ray index, so the slabs see the same samples)."""
    from nerf_pytorch_paeng_amd import nerf_process as NP, train_path
    sd, model, posenc, opts, o, d, t_rand, u, target, cfg = _train_setup(D=4, W=128, n=90, Sc=16, Nf=16, seed=8)
    K, H, Wd = synthetic.lego_camera()
    tgt = target.to(DEV)

    def grads(seed):
        model.zero_grad(set_to_none=True)
        rgb_c, _, rgb_f, _ = NP.batchify_rays_and_render_by_chunk(o, d, model, posenc, H, Wd, K, opts, seed=seed)
        (torch.nn.functional.mse_loss(rgb_c, tgt) + torch.nn.functional.mse_loss(rgb_f, tgt)).backward()
        return {k: p.grad.clone() for k, p in model.named_parameters()}, rgb_f.detach().clone()

    one, rgb_one = grads(5)
    monkeypatch.setattr(train_path, "MAX_TRAIN_RAYS", 32)              # 90 rays -> slabs of 32, 32, 26
    many, rgb_many = grads(5)
    assert torch.equal(rgb_one, rgb_many)
    for k in one:
        assert rel_err(many[k], one[k]) < 5e-5, k                      # same kernels; fp32 sums regrouped (scalar bias gradients cancel heavily)


def test_largest_training_slab_matches_smaller_slabs(monkeypatch):
    """One autograd node at MAX_TRAIN_RAYS (16384 rays x (64 + 256) points: 4.2 M fine rows, 88 GiB of stash and gradient
    workspace, operands past the 4 GiB mark) against the same rays rendered as four nodes of 4096."""
    from nerf_pytorch_paeng_amd import nerf_process as NP, train_path
    free, _ = torch.cuda.mem_get_info()
    if free < 120 * 2 ** 30:
        pytest.skip("needs ~90 GB of device memory")
    n = train_path.MAX_TRAIN_RAYS
    sd, model, posenc, opts, _, _, _, _, _, _ = _train_setup(D=8, W=256, n=8, Sc=64, Nf=128, seed=2)
    opts.N_samples_f = 192                                             # fine net: 64 + 192 = 256 points per ray
    opts.chunk_rays = n
    K, H, Wd = synthetic.lego_camera()
    pix = torch.from_numpy(synthetic.pixel_batch(H, Wd, n, 3)).to(DEV)
    o, d = ops.make_o_d_pixels(Wd, H, K, synthetic.pose_spherical(10.0, -30.0, 4.0), pix)
    tgt = torch.rand(n, 3, generator=torch.Generator().manual_seed(4)).to(DEV)

    def grads():
        model.zero_grad(set_to_none=True)
        rgb_c, _, rgb_f, _ = NP.batchify_rays_and_render_by_chunk(o, d, model, posenc, H, Wd, K, opts, seed=9)
        (torch.nn.functional.mse_loss(rgb_c, tgt) + torch.nn.functional.mse_loss(rgb_f, tgt)).backward()
        out = {k: p.grad.clone() for k, p in model.named_parameters()}, rgb_f.detach().clone()
        torch.cuda.synchronize()
        return out

    torch.cuda.reset_peak_memory_stats()
    one, rgb_one = grads()
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    torch.cuda.empty_cache()
    monkeypatch.setattr(train_path, "MAX_TRAIN_RAYS", 4096)
    many, rgb_many = grads()
    assert torch.equal(rgb_one, rgb_many)
    worst = max(rel_err(many[k], one[k]) for k in one)
    print(f"16384-ray node vs 4 x 4096: worst gradient difference {worst:.2e}, peak memory of the single node {peak:.1f} GiB")
    assert worst < 2e-4
    torch.cuda.empty_cache()


def test_training_path_refuses_what_it_does_not_support():
    from nerf_pytorch_paeng_amd import nerf_process as NP
    sd, model, posenc, opts, o, d, t_rand, u, target, cfg = _train_setup(D=4, W=128, n=8, Sc=8, Nf=8)
    K, H, Wd = synthetic.lego_camera()
    with pytest.raises(ops.MiNerfError):
        NP.batchify_rays_and_render_by_chunk(o, d, model, posenc, H, Wd, K, opts, bf16=True)          # training is fp32 only
    with pytest.raises(ops.MiNerfError):
        NP.render_rays(torch.cat([o, d], -1), model, posenc, opts, return_intermediates=True)
    cpu_model = type(model)(4, 128, 63, 27)
    with pytest.raises(ops.MiNerfError):
        NP.batchify_rays_and_render_by_chunk(o, d, cpu_model, posenc, H, Wd, K, opts)                 # no CPU fallback
    wide = type(model)(4, 320, 63, 27).to(DEV)                                                       # inference only beyond netWidth 256
    with pytest.raises(ops.MiNerfError, match="training kernels exist for netWidth <= 256"):
        NP.batchify_rays_and_render_by_chunk(o, d, wide, posenc, H, Wd, K, opts)


def test_rays_that_require_grad_are_refused():
    from nerf_pytorch_paeng_amd import nerf_process as NP
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    sd, model, posenc, opts, o, d, t_rand, u, target, cfg = _train_setup(D=4, W=128, n=16, Sc=8, Nf=8)
    K, H, Wd = synthetic.lego_camera()
    with pytest.raises(MiNerfError, match="rays require grad"):
        NP.batchify_rays_and_render_by_chunk(o, d.clone().requires_grad_(True), model, posenc, H, Wd, K, opts)


def test_llff_training_step_through_ndc():
    """data_type == 'llff': the NDC warp (nerf_process.py:224-226) precedes the differentiable render; gradients reach both nets."""
    from nerf_pytorch_paeng_amd import nerf_process as NP
    sd, model, posenc, opts, o, d, t_rand, u, target, cfg = _train_setup(D=4, W=128, n=40, Sc=16, Nf=16, seed=6)
    K, H, Wd = synthetic.fern_camera()
    pose = torch.from_numpy(synthetic.fern_pose()).float()
    pix = torch.from_numpy(synthetic.pixel_batch(H, Wd, 40, 2)).to(DEV)
    o, d = ops.make_o_d_pixels(Wd, H, K, pose, pix)
    opts.data_type, opts.near, opts.far = "llff", 0.0, 1.0
    rgb_c, _, rgb_f, _ = NP.batchify_rays_and_render_by_chunk(o, d, model, posenc, H, Wd, K, opts, t_rand=t_rand, u=u)
    (torch.nn.functional.mse_loss(rgb_c, target.to(DEV)) + torch.nn.functional.mse_loss(rgb_f, target.to(DEV))).backward()
    # same rays through the oracle's NDC warp and render, depths pinned to the product's
    with torch.no_grad():
        oo, dd = NP.ndc_rays(H, Wd, float(K[0][0]), 1.0, o, d)
        rays_ndc = torch.cat([oo, dd], -1).contiguous()
        z_f = NP.render_rays(rays_ndc, model, posenc, opts, t_rand=t_rand, u=u, return_intermediates=True)["_z_f"]
    ro, rd = R.ndc_rays(H, Wd, float(K[0][0]), 1.0, o.cpu(), d.cpu())
    psd = {k: torch.as_tensor(v).clone().float().requires_grad_(True) for k, v in sd.items()}
    cfg = R.PathConfig(near=0.0, far=1.0, N_samples_c=16, N_samples_f=16, perturb=1.0, netDepth=4, netWidth=128, data_type="llff")
    ref = R.render_rays(torch.cat([ro, rd], -1), psd, cfg, t_rand, u, z_fine_override=z_f.cpu())
    (torch.mean((ref["rgb_c"] - target) ** 2) + torch.mean((ref["rgb_f"] - target) ** 2)).backward()
    # un-pinned coarse depths: the forward is ill-conditioned in z (see test_train_step_gradients_match_oracle_autograd),
    # so this end-to-end comparison through the drop-in surface carries a loose bar
    for k, p in model.named_parameters():
        assert p.grad is not None and rel_err(p.grad, psd[k].grad) < 2e-2, k


def test_backward_full_size_properties():
    """BASELINE config #2 sizes (4096 rays, 64 + 128 samples, 8x256): the oracle's autograd is too slow there, so the backward is
    checked through properties: bit-reproducible, linear in the incoming gradient, zero for a zero gradient, finite."""
    net = ops.make_net(8, 256, 4)
    sd = synthetic.make_state_dict(0, 8, 256)
    prefix = "model_fine."
    packed = ops.pack_module(sd, prefix, net).to(DEV)
    packed_bwd = ops.pack_module(sd, prefix, net, backward=True).to(DEV)
    K, H, W = synthetic.lego_camera()
    pix = torch.from_numpy(synthetic.pixel_batch(H, W, 4096, 0)).to(DEV)
    o, d = ops.make_o_d_pixels(W, H, K, synthetic.pose_spherical(0.0, -30.0, 4.0), pix)
    rays = torch.cat([o, d], -1).contiguous()
    z = torch.sort(2.0 + 4.0 * torch.rand(4096, 192, generator=torch.Generator().manual_seed(0)), -1).values.to(DEV)
    raw, stash = ops.mlp_rays_train(net, packed, rays, z)
    G = torch.randn(4096, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    d_raw = ops.composite_backward(raw, z, rays, G)
    assert torch.isfinite(d_raw).all()
    g1, work = ops.mlp_backward(net, packed, packed_bwd, rays, z, d_raw, stash)
    g1b, _ = ops.mlp_backward(net, packed, packed_bwd, rays, z, d_raw, stash, work)
    assert torch.isfinite(g1).all() and torch.equal(g1, g1b)                       # deterministic reductions
    g2, _ = ops.mlp_backward(net, packed, packed_bwd, rays, z, (2.0 * d_raw).contiguous(), stash, work)
    assert torch.equal(g2, 2.0 * g1)                                                # scaling by 2 is exact in fp32
    g0, _ = ops.mlp_backward(net, packed, packed_bwd, rays, z, torch.zeros_like(d_raw), stash, work)
    assert float(g0.abs().max()) == 0.0
    assert torch.equal(ops.composite_backward(raw, z, rays, 2.0 * G), 2.0 * d_raw)


def test_post_process_is_differentiable_in_rgb():
    """The drop-in post_process carries the colour gradient (what train.py's loss reads) back to its `outputs` argument."""
    from nerf_pytorch_paeng_amd import nerf_process as NP
    raw, z, rays, G = _composite_case(21, 64, 5)
    raw_a = raw.clone().requires_grad_(True)
    (R.post_process(raw_a, z, rays[:, 3:])[0] * G).sum().backward()
    raw_d = raw.to(DEV).requires_grad_(True)
    out = NP.post_process(raw_d, z.to(DEV), rays[:, 3:].contiguous().to(DEV))
    assert out[0].requires_grad and not out[1].requires_grad and not out[3].requires_grad
    (out[0] * G.to(DEV)).sum().backward()
    assert rel_err(raw_d.grad[..., :3], raw_a.grad[..., :3]) < 1e-5 and rel_err(raw_d.grad[..., 3], raw_a.grad[..., 3]) < 1e-4
    with torch.no_grad():
        assert not NP.post_process(raw_d, z.to(DEV), rays[:, 3:].contiguous().to(DEV))[0].requires_grad


def test_empty_batch_backward_is_zero_not_uninitialised_memory():
    """An empty slab / an empty embedded batch: the library returns before any weight-gradient kernel runs, and ops.mlp_backward allocates
    the flat gradient uninitialised -- so the library zero-fills it (autograd's answer for the gradient of nothing).  Poisoned buffers
    through both entry points, and model(x[0:0]) under autograd."""
    from nerf_pytorch_paeng_amd.model import NeRF
    net = ops.make_net(4, 128, 1)
    sd = synthetic.make_state_dict(5, 4, 128, skips=(1,))
    packed = ops.pack_module(sd, "model_fine.", net).to(DEV)
    packed_bwd = ops.pack_module(sd, "model_fine.", net, backward=True).to(DEV)
    S = 24
    rays, z, d_raw = torch.empty(0, 6, device=DEV), torch.empty(0, S, device=DEV), torch.empty(0, S, 4, device=DEV)
    raw, stash = ops.mlp_rays_train(net, packed, rays, z)
    assert raw.shape == (0, S, 4)
    poison = torch.full((ops.param_count(net),), float("nan"), device=DEV)
    grads, _ = ops.mlp_backward(net, packed, packed_bwd, rays, z, d_raw, stash, grads=poison)
    assert grads.data_ptr() == poison.data_ptr() and torch.count_nonzero(poison).item() == 0
    assert ops.mlp_backward(net, packed, packed_bwd, rays, z, d_raw, stash, stage=1)[0] is None      # deltas only: no gradient vector to mistake for one
    # split-precision backward over an empty slab: the two range words the training path folds into its saturation monitor read "nothing
    # seen", not the allocator's leftovers (NaN here), and the training path does not fold them at all
    net256 = ops.make_net(4, 256, 1)
    sd256 = synthetic.make_state_dict(5, 4, 256, skips=(1,))
    p256, pb256 = ops.pack_module(sd256, "model_fine.", net256).to(DEV), ops.pack_module(sd256, "model_fine.", net256, backward=True).to(DEV)
    _, stash256 = ops.mlp_rays_train(net256, p256, rays, z)
    work = torch.full((ops.train_layout(net256, 0, S).work_bytes,), 0xFF, dtype=torch.uint8, device=DEV)
    g256, _ = ops.mlp_backward(net256, p256, pb256, rays, z, d_raw, stash256, work=work, f16s_wgrad=True)
    assert torch.count_nonzero(g256).item() == 0 and ops.backward_range(net256, 0, S, work) == (0.0, 0.0)
    x = torch.empty(0, 90, device=DEV)
    out, st = ops.mlp_embedded_train(net, packed, x)
    poison.fill_(float("nan"))
    g2 = ops.mlp_embedded_backward(net, packed, packed_bwd, x, torch.empty(0, 4, device=DEV), st, grads=poison)
    assert torch.count_nonzero(g2).item() == 0
    model = NeRF(4, 128, 63, 27, skips=[1]).to(DEV)
    y = model(x, True)
    assert y.shape == (0, 4) and y.requires_grad
    y.sum().backward()
    assert all(p.grad is not None and torch.count_nonzero(p.grad).item() == 0 for p in model.model_fine.parameters())


@pytest.mark.parametrize("D,W,skip,n", [(8, 256, 4, 777), (4, 128, 1, 64), (4, 128, 1, 33)])
def test_model_forward_is_differentiable_like_the_reference_module(D, W, skip, n):
    """model(embedded, is_fine) with gradients enabled -- the call the reference's own render_rays makes (nerf_process.py:190-192):
    output equals the inference kernel's, parameter gradients equal CPU autograd on the oracle; row counts that are not a
    multiple of the 32-row tile."""
    from nerf_pytorch_paeng_amd.model import NeRF
    sd = synthetic.make_state_dict(31 + D, D, W, skips=(skip,))
    model = NeRF(D, W, 63, 27, skips=[skip]).to(DEV)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    g = torch.Generator().manual_seed(n)
    rays = torch.cat([torch.tensor([0.0, 0.0, 4.0]) + 0.2 * torch.randn(n, 3, generator=g),
                      torch.nn.functional.normalize(torch.tensor([0.0, 0.0, -1.0]) + 0.3 * torch.randn(n, 3, generator=g), dim=-1)], -1)
    x = R.embed(rays, 2.0 + 4.0 * torch.rand(n, 1, generator=g), 10, 4)                    # [n, 90]
    G = torch.randn(n, 4, generator=g)
    for is_fine, prefix in ((False, "model_coarse."), (True, "model_fine.")):
        names = ops.param_names(ops.make_net(D, W, skip))
        psd = {prefix + k: torch.as_tensor(sd[prefix + k]).clone().float().requires_grad_(True) for k in names}
        ref = R.mlp_forward(psd, prefix, x, D, 63, 27, (skip,))
        (ref * G).sum().backward()
        model.zero_grad(set_to_none=True)
        out = model(x.to(DEV), is_fine)
        assert out.requires_grad and out.shape == (n, 4)
        with torch.no_grad():
            assert torch.equal(out.detach(), model(x.to(DEV), is_fine))
        (out * G.to(DEV)).sum().backward()
        sub = model.model_fine if is_fine else model.model_coarse
        other = model.model_coarse if is_fine else model.model_fine
        for k, p in sub.named_parameters():
            assert rel_err(p.grad, psd[prefix + k].grad) < 2e-4, (prefix, k)
        assert all(p.grad is None for p in other.parameters())


@pytest.mark.parametrize("tag,f16s", [("d8w256", False), ("d4w128", False), ("d8w256", True)])
def test_F11_backward_matches_the_reference_training_step(golden, tag, f16s):
    """The HIP backward against the gradients of the reference's OWN loss.backward() (fixture F11: train.py:53-70 executed by
    oracle/gen_fixtures.py on 64 rays with injected randoms).  Depths are pinned to the ones the reference sampled.
    ``f16s``: the same bars with the two forward launches in split precision (fp32-grade outputs and stash; the backward is unchanged)."""
    from nerf_pytorch_paeng_amd import train_path
    from nerf_pytorch_paeng_amd.model import NeRF
    from types import SimpleNamespace
    g = golden("F11_train_grads")
    D, W, seed, Sc, Nf = (int(v) for v in g[f"{tag}_cfg"])
    sd = synthetic.make_state_dict(seed, D, W)
    model = NeRF(D, W, 63, 27).to(DEV)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    # the reference's own rays (fixture F8, the same 64 pixels): the path is ill-conditioned in the ray / depth bits (one ulp of a
    # point moves the top octave of gamma(x) by 5e-4), so both sides must start from identical inputs
    rays = torch.from_numpy(golden("F8_render_rays")["legoA_rays"]).to(DEV).contiguous()
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=Sc, N_samples_f=Nf, perturb=1.0)
    t_rand, u = torch.from_numpy(R.counter_uniform(0, 0, 0, 64, Sc)).to(DEV), torch.from_numpy(R.counter_uniform(0, 1, 0, 64, Nf)).to(DEV)
    out = train_path.render_train(rays, model, opts, t_rand=t_rand, u=u, f16s=f16s,
                                  z_override=(torch.from_numpy(g[f"{tag}_z_c"]).to(DEV), torch.from_numpy(g[f"{tag}_z_f"]).to(DEV)))
    tgt = torch.from_numpy(g[f"{tag}_target"]).to(DEV)
    loss_c, loss_f = torch.mean((out["rgb_c"] - tgt) ** 2), torch.mean((out["rgb_f"] - tgt) ** 2)          # train.py:60-66
    (loss_c + loss_f).backward()
    assert abs(loss_c.item() - float(g[f"{tag}_loss_c"])) < 2e-6 and abs(loss_f.item() - float(g[f"{tag}_loss_f"])) < 2e-6
    assert float((out["rgb_f"].detach().cpu() - torch.from_numpy(g[f"{tag}_rgb_f"])).abs().max()) < 2e-5
    # The 8x256 fine network's trunk gradients on this batch are sums that almost cancel (largest entry 1e-4 .. 3e-3 from terms
    # a hundred times larger), so the REFERENCE's own fp32 result sits 5e-4 .. 1.6e-3 (relative to the tensor's largest entry)
    # away from the same computation with the MLP in fp64.  Each gradient is therefore held against that fp64 evaluation with the
    # reference's own distance from it as the yardstick; where the reference is well conditioned (every coarse tensor, the heads,
    # the whole 4x128 case: 2e-7) this is a 2e-5 bound.
    psd = {k: torch.as_tensor(v).clone().float().requires_grad_(True) for k, v in sd.items()}
    cfg = R.PathConfig(near=2.0, far=6.0, N_samples_c=Sc, N_samples_f=Nf, perturb=1.0, netDepth=D, netWidth=W)
    ref64 = R.render_rays(rays.cpu(), psd, cfg, t_rand.cpu(), u.cpu(), z_fine_override=torch.from_numpy(g[f"{tag}_z_f"]), mlp_dtype=torch.float64)
    (torch.mean((ref64["rgb_c"] - tgt.cpu()) ** 2) + torch.mean((ref64["rgb_f"] - tgt.cpu()) ** 2)).backward()
    worst, worst_ref, n = 0.0, 0.0, 0
    for k, p in model.named_parameters():
        want = torch.from_numpy(g[f"{tag}_grad.{k}"])
        e_ref = rel_err(want, psd[k].grad)                 # the reference's fp32 noise on this tensor
        e = float((p.grad.cpu().double() - psd[k].grad.double()).abs().max()) / float(want.abs().max())
        worst, worst_ref = max(worst, e), max(worst_ref, e_ref)
        # ... capped in absolute terms from what is observed (fp32 forward 3.7e-5 on the cancelling trunk tensors, split-precision forward
        # 5.8e-6): a tenfold regression fails whatever the reference's own noise on the tensor
        assert e <= min(3.0 * e_ref + 2e-5, 2e-5 if f16s else 1.5e-4), (k, e, e_ref)
        assert rel_err(p.grad, want) <= 4.0 * e_ref + 2e-5, (k, rel_err(p.grad, want), e_ref)
        n += 1
    assert n == (48 if D == 8 else 32)
    print(f"F11 {tag}{' (split-precision forward)' if f16s else ''}: worst per-tensor gradient error vs the fp64-MLP evaluation {worst:.2e} "
          f"(the reference's own: {worst_ref:.2e})")
