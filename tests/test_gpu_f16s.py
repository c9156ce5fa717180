"""The split-precision variant (csrc/mlp_f16s.hip): fp32-grade results on the f16 matrix pipe.

Weights and activations travel as f16 pairs x = hi + lo * 2^-11; a product is three v_mfma_f32_16x16x32_f16 with fp32 accumulation.
It is held to the bars of the fp32 path itself (tests/test_gpu_parity.py): raw network outputs against an fp64 evaluation within
4x the distance of the reference's own fp32 arithmetic, rendered colours against the CPU oracle within 2e-5 with pinned depths, at
most 1 % of un-pinned rays off by more than 1e-4 -- and, tightly, to the oracle restatement with the same rounding points
(R.mlp_forward_f16split), which a packing or ordering error cannot pass."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import nerf_process as NP
from nerf_pytorch_paeng_amd import ops, synthetic, weights
from nerf_pytorch_paeng_amd._lib import MiNerfError
from oracle import restate as R
from tests import sampling_account as SA

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.from_numpy


def make_opts(**kw):
    base = dict(near=2.0, far=6.0, N_samples_c=64, N_samples_f=128, perturb=1.0, chunk_rays=4096, chunk_pts=524288,
                data_type="blender", gpu_ids=[0], rank=0)
    base.update(kw)
    return SimpleNamespace(**base)


@pytest.fixture(scope="module")
def lego_rays():
    K, H, W = synthetic.lego_camera()
    pix = T(synthetic.pixel_batch(H, W, 4096, 0)).to(DEV)
    o, d = ops.make_o_d_pixels(W, H, K, synthetic.pose_spherical(0.0, -30.0, 4.0), pix)
    return torch.cat([o, d], -1).contiguous()


@pytest.fixture(scope="module")
def packed_big():
    return weights.PackedNeRF.from_state_dict(synthetic.make_state_dict(0, 8, 256), DEV)


@pytest.mark.parametrize("D,skip,L_x,L_d,n,S", [(8, 4, 10, 4, 64, 192), (8, 4, 10, 4, 33, 100), (8, 4, 10, 4, 5, 64), (8, 4, 10, 4, 700, 33),
                                                 (7, 5, 10, 4, 37, 96), (3, -1, 10, 4, 37, 96), (8, 3, 10, 4, 37, 96), (2, -1, 10, 4, 37, 96),
                                                 (9, 0, 10, 4, 37, 96), (8, 4, 6, 2, 37, 96), (4, -1, 0, 4, 37, 96),
                                                 (16, 14, 10, 4, 37, 96), (15, 7, 10, 4, 37, 96), (12, -1, 10, 4, 37, 96), (14, 12, 10, 4, 37, 96)])
def test_f16s_mlp_vs_oracles(D, skip, L_x, L_d, n, S, lego_rays):
    """Raw network outputs of the split-precision kernel: (1) against the restatement with its rounding points (fp64 accumulation):
    what is left is fp32 summation order; (2) against the fp64 evaluation of the network: no further than 4x the reference's own fp32
    arithmetic (and than the fp32 MFMA kernel).  Both trunk polarities, the skip layer at odd / even l, no skip, fewer frequencies,
    ragged sample counts, flat and ray-major tile walks.
    The kernel keeps D x 256 biases beside its weight ring and per-wave buffers in LDS, which holds 14 layers (ops.F16S_FWD_MAX_D; D = 15
    misses the 160 KiB by 16 bytes): D = 14, skip at D - 2, is its largest footprint; D = 15 and 16 are refused by name before any launch --
    the blob itself packs at any depth up to 16 (the f16 kernel reads it: tests/test_gpu_f16.py)."""
    skips = (skip,) if skip >= 0 else ()
    in_x, in_d = 3 + 6 * L_x, 3 + 6 * L_d
    sd = synthetic.make_state_dict(17 + D + L_x, D, 256, in_x=in_x, in_d=in_d, skips=skips)
    packed = weights.PackedNeRF.from_state_dict(sd, DEV)
    rays = lego_rays[:n].contiguous()
    z = torch.sort(T(R.counter_uniform(3, 0, 0, n, S)) * 4 + 2, -1)[0]
    if D > ops.F16S_FWD_MAX_D:
        with pytest.raises(MiNerfError, match=r"D = %d does not fit \(D <= 14\)" % D):
            ops.mlp_rays(packed.net, packed.f16s()[1], rays, z.to(DEV), f16s=True)
        with pytest.raises(MiNerfError, match=r"D = %d does not fit \(D <= 14\)" % D):        # ... and a render in that mode, before anything is packed
            NP.render_rays(rays, packed, None, make_opts(N_samples_c=16, N_samples_f=16), f16s=True)
        print(f"f16s D={D}: refused by name (LDS holds {ops.F16S_FWD_MAX_D} layers)")
        return
    x = R.embed(rays.cpu(), z, L_x, L_d)
    ref64 = R.mlp_forward(sd, "model_fine.", x.double(), D, in_x, in_d, skips=skips, dtype=torch.float64)
    ref32 = R.mlp_forward(sd, "model_fine.", x, D, in_x, in_d, skips=skips)
    emu = R.mlp_forward_f16split(sd, "model_fine.", x, D, in_x, in_d, skips=skips)
    got = ops.mlp_rays(packed.net, packed.f16s()[1], rays, z.to(DEV), f16s=True).cpu().reshape(-1, 4)
    fp32k = ops.mlp_rays(packed.net, packed.fine, rays, z.to(DEV)).cpu().reshape(-1, 4)
    assert torch.isfinite(got).all()
    e_emu = float((got.double() - emu.double()).abs().max())
    e64 = float((got.double() - ref64).abs().max())
    e_ref = float((ref32.double() - ref64).abs().max())
    e_k32 = float((fp32k.double() - ref64).abs().max())
    print(f"f16s D={D} skip={skip} L={L_x}/{L_d} n={n} S={S}: vs its restatement {e_emu:.2e}; vs fp64 {e64:.2e} (reference fp32 {e_ref:.2e}, fp32 kernel {e_k32:.2e})")
    # gamma(x) is evaluated by the kernel (sin / cos of arguments up to 3e3 rad) and by torch on the oracle side: the encoded inputs
    # differ by a few 1e-7, which the network amplifies alike for every implementation
    assert e_emu <= 3e-5, e_emu
    assert e64 <= 4.0 * max(e_ref, e_k32) + 1e-6, (e64, e_ref, e_k32)


@pytest.mark.parametrize("stash", [False, True])
def test_f16s_forward_out_of_range_is_never_a_finite_colour(stash, lego_rays):
    """RANGE CONTRACT of the split-precision forward (mlp_f16s_core.h), both instantiations (inference, training forward with stash): an
    activation at or beyond 65 520 -- here one unit's bias -- comes out as NaN in EVERY output that depends on it, never as a finite value:
      * a trunk unit (layer 3 of 8)       -> all four raw outputs of every point are NaN
      * the LAST trunk unit layer         -> same (density reads it directly)
      * a linear_feat unit (no ReLU)      -> the three colours are NaN, the density (which does not depend on it) is finite and right
      * a linear_d unit (ReLU)            -> the three colours are NaN
    y <= -65 520 in front of a ReLU is exact (the unit is off, as in fp32), and 65 000 stays in range: both equal the fp32 kernel.
    The fp32 kernel itself is finite on all of these networks.  (Until round 4 the ReLU was v_pk_max_f16 / v_max_f32, which return the
    OTHER operand for a NaN: the layer behind an overflow came out as zeros and the network as plausible finite colours.)"""
    n, S, D = 40, 64, 8
    rays = lego_rays[:n].contiguous()
    z = torch.sort(T(R.counter_uniform(5, 0, 0, n, S)) * 4 + 2, -1)[0].to(DEV)

    def run(sd):
        packed = weights.PackedNeRF.from_state_dict(sd, DEV)
        blob = packed.f16s()[1]
        if stash:
            got = ops.mlp_rays_train(packed.net, blob, rays, z, f16s=True)[0]
        else:
            got = ops.mlp_rays(packed.net, blob, rays, z, f16s=True)
        return got.reshape(-1, 4), ops.mlp_rays(packed.net, packed.fine, rays, z).reshape(-1, 4)

    def with_bias(name, unit, value):
        sd = synthetic.make_state_dict(23, D, 256)
        b = sd["model_fine." + name].copy()
        b[unit] = value
        sd["model_fine." + name] = b
        return sd

    base16, base32 = run(synthetic.make_state_dict(23, D, 256))
    assert torch.isfinite(base16).all() and float((base16 - base32).abs().max()) < 1e-4
    for name, unit in (("linear_x.3.bias", 7), ("linear_x.7.bias", 200), ("linear_x.0.bias", 0)):
        got, ref = run(with_bias(name, unit, 70000.0))
        assert torch.isfinite(ref).all()                                        # fp32 carries it
        assert torch.isnan(got).all(), (name, int(torch.isfinite(got).sum()))   # every output of every point
    got, ref = run(with_bias("linear_feat.bias", 11, 70000.0))
    assert torch.isnan(got[:, :3]).all() and torch.isfinite(got[:, 3]).all()
    assert float((got[:, 3] - ref[:, 3]).abs().max()) <= 1e-4 * max(1.0, float(ref[:, 3].abs().max()))
    got, ref = run(with_bias("linear_d.bias", 5, 70000.0))
    assert torch.isnan(got[:, :3]).all() and torch.isfinite(got[:, 3]).all()
    # negative overflow in front of a ReLU: the unit is off, exactly as in fp32; just inside the range: ordinary accuracy
    for value in (-70000.0, -1e9, 65000.0):
        got, ref = run(with_bias("linear_x.3.bias", 7, value))
        assert torch.isfinite(got).all(), value
        assert float((got - ref).abs().max()) <= 2e-4 * max(1.0, float(ref.abs().max())), (value, float((got - ref).abs().max()))


def test_module_source_f16s_blobs_are_packed_on_the_device(lego_rays):
    """packed_for(nn.Module).f16s() builds the split-precision blobs on the device from the flat parameter vectors (no host round trip per
    render call): bit-identical to the host packer's blobs; a weight beyond the f16 range, which the host packer refuses, is COUNTED by the
    device packer and raised by check_f16s_range(), which f16s() itself calls once per packing: the harness, render_rays and batchify all refuse."""
    from nerf_pytorch_paeng_amd import harness
    from nerf_pytorch_paeng_amd.model import NeRF, get_positional_encoder
    from nerf_pytorch_paeng_amd.weights import packed_for
    sd = synthetic.make_state_dict(4, 8, 256)
    model = NeRF(8, 256, 63, 27).to(DEV)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    dev_blobs = packed_for(model)
    got = dev_blobs.f16s()
    want = weights.PackedNeRF.from_state_dict(sd, DEV).f16s()
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert dev_blobs.check_f16s_range() == 0
    # the range read synchronises the host: it is paid once per VERSION of the parameters, not once per render call
    reads = []
    orig = weights.PackedNeRF.check_f16s_range
    weights.PackedNeRF.check_f16s_range = lambda self: (reads.append(1), orig(self))[1]
    try:
        with torch.no_grad():
            for _ in range(3):
                NP.render_rays(lego_rays[:64].contiguous(), model, None, make_opts(), seed=1, f16s=True)
        assert reads == []                                           # verdict of this parameter version already on record (f16s() above)
        with torch.no_grad():
            model.model_fine.linear_x[2].bias[0] += 0.5              # an in-place update = a new version: checked again, once
            for _ in range(2):
                NP.render_rays(lego_rays[:64].contiguous(), model, None, make_opts(), seed=1, f16s=True)
        assert reads == [1]
    finally:
        weights.PackedNeRF.check_f16s_range = orig
    with torch.no_grad():
        model.model_fine.linear_x[2].weight[3, 5] = 1.0e6
    bad = packed_for(model)
    with pytest.raises(MiNerfError, match="beyond the f16 range"):
        bad.f16s()                                                   # the refusal the host packer gives, at packing time
    # ... so EVERY no-grad caller with an nn.Module gets it (round 4: only the eval harness checked; render_rays rendered NaN frames)
    with torch.no_grad(), pytest.raises(MiNerfError, match="beyond the f16 range"):
        NP.render_rays(lego_rays[:64].contiguous(), model, None, make_opts(), seed=1, f16s=True)
    with torch.no_grad(), pytest.raises(MiNerfError, match="beyond the f16 range"):
        NP.batchify_rays_and_render_by_chunk(lego_rays[:64, :3], lego_rays[:64, 3:], model, None, 8, 8, np.eye(3), make_opts(), seed=1, f16s=True)
    K, H, W = synthetic.lego_camera()
    opts = make_opts(precision="f16s", exp_name="x")
    pose = torch.as_tensor(synthetic.pose_spherical(0.0, -30.0, 4.0), dtype=torch.float32)
    posenc = get_positional_encoder(10), get_positional_encoder(4)
    with pytest.raises(MiNerfError, match="beyond the f16 range"):
        harness.test(0, [0], posenc, model, torch.zeros(1, 8, 8, 3), K, pose[None], (8, 8), opts)


def test_f16s_config2_all_rays_vs_oracle(packed_big, lego_rays, oracle_cache):
    """BASELINE config #2 at full size through the split-precision variant, EVERY ray against the CPU oracle, to the bars the fp32
    path is held to (test_config2_all_rays_vs_oracle): coarse colours and disparities directly; fine outputs with the depths pinned to
    the ones the HIP path sampled; un-pinned rays more than 1e-4 off: at most 1 %."""
    opts = make_opts()
    a = NP.render_rays(lego_rays, packed_big, None, opts, seed=11, return_intermediates=True, f16s=True)
    b = NP.render_rays(lego_rays, packed_big, None, opts, seed=11, return_intermediates=True)
    sd = synthetic.make_state_dict(0, 8, 256)
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    rc, tr, uu = lego_rays.cpu(), a["_t_rand"].cpu(), a["_u"].cpu()
    with torch.no_grad():
        if "config2_seed11" not in oracle_cache:             # shared with tests/test_gpu_parity.py::test_config2_all_rays_vs_oracle (same rays, same jitter)
            oracle_cache["config2_seed11"] = (tr, uu, R.render_rays(rc, sd, R.PathConfig(), tr, uu))
        tr0, uu0, ref = oracle_cache["config2_seed11"]
        assert torch.equal(tr0, tr) and torch.equal(uu0, uu)
        pin = R.render_rays(rc, sd, R.PathConfig(), tr, uu, z_fine_override=a["_z_f"].cpu())
    e_c = float((a["rgb_c"].cpu() - ref["rgb_c"]).abs().max())
    e_dc = float((a["disp_c"].cpu() - ref["disp_c"]).abs().max())
    e_f = float((a["rgb_f"].cpu() - pin["rgb_f"]).abs().max())
    bad = float(SA.rays_beyond(a["rgb_f"], ref["rgb_f"]).float().mean())           # a non-finite colour counts
    mse = float(((a["rgb_f"].cpu() - ref["rgb_f"]) ** 2).mean())
    # all 4096 x 128 samples: exactly fine_z of the run's own coarse depths, weights and uniforms, every one accounted for (no allowance)
    z_f_own, z_s_own = ops.fine_z(a["_z_c"].contiguous(), a["_weights_c"].contiguous(), 128, False, a["_u"], want_samples=True)
    assert torch.equal(z_f_own, a["_z_f"])
    acc = SA.fine_account(a["_z_c"], a["_weights_c"], uu, z_s_own)
    print(f"f16s config #2 fine depths: {acc.worst()}")
    assert int(acc.bad.sum()) == 0, acc.bad.nonzero()[:8].tolist()
    no_flip = SA.bad_rays_without_a_flip(a["rgb_f"], ref["rgb_f"], a["_z_f"], ref["_z_f"])       # a ray off by > 1e-4 has a fine depth off by > 5e-6
    assert not bool(no_flip.any()), no_flip.nonzero().flatten().tolist()
    mse32 = float(((a["rgb_f"] - b["rgb_f"]) ** 2).mean())
    print(f"f16s config #2, 4096 rays vs oracle: rgb_c {e_c:.2e}, disp_c {e_dc:.2e}; pinned rgb_f {e_f:.2e}; un-pinned rays off by >1e-4: {bad:.4f}, "
          f"PSNR vs oracle {R.mse2psnr(mse):.1f} dB, vs the fp32 HIP path {R.mse2psnr(max(mse32, 1e-30)):.1f} dB")
    assert e_c <= 2e-5 and e_dc <= 2e-4, (e_c, e_dc)
    assert e_f <= 2e-5, e_f
    assert bad <= 0.01 and R.mse2psnr(mse) > 90.0, (bad, R.mse2psnr(mse))


def test_f16s_surface(packed_big, lego_rays):
    """Chunk / shard invariance, the frame path, module models, refusals."""
    from nerf_pytorch_paeng_amd import dist as mdist
    from nerf_pytorch_paeng_amd.model import NeRF
    opts = make_opts(N_samples_c=32, N_samples_f=32)
    rays = lego_rays[:300].contiguous()
    whole = NP.render_rays(rays, packed_big, None, opts, seed=5, f16s=True)
    part = NP.render_rays(rays[100:250].contiguous(), packed_big, None, opts, seed=5, ray_offset=100, f16s=True)
    assert torch.equal(part["rgb_f"], whole["rgb_f"][100:250])
    K, H, W = synthetic.lego_camera()
    s = 24.0 / W
    Ks = K.copy(); Ks[0, 0] *= s; Ks[1, 1] *= s; Ks[0, 2] = 12.0; Ks[1, 2] = 10.0
    pose = synthetic.pose_spherical(30.0, -30.0, 4.0)
    rgb, disp = mdist.render_frame(20, 24, Ks, pose, packed_big, opts, seed=5, f16s=True)
    rgb32, _ = mdist.render_frame(20, 24, Ks, pose, packed_big, opts, seed=5)
    assert rgb.shape == (20, 24, 3) and float((rgb - rgb32).abs().max()) < 5e-3          # a sample_pdf bin flip at worst
    sd = synthetic.make_state_dict(0, 8, 256)
    model = NeRF(8, 256, 63, 27).to(DEV)
    model.load_state_dict({k: T(v) for k, v in sd.items()})
    with torch.no_grad():
        m = NP.render_rays(rays, model, None, opts, seed=5, f16s=True)
    assert torch.equal(m["rgb_f"], whole["rgb_f"])
    with pytest.raises(MiNerfError):
        NP.render_rays(rays, packed_big, None, opts, seed=5, f16s=True, bf16=True)
    with pytest.raises(MiNerfError, match="netWidth <= 256"):                               # wider than the variant's one kernel width: refused (narrower pads)
        weights.PackedNeRF.from_state_dict(synthetic.make_state_dict(1, 4, 320), DEV).f16s()
    narrow = weights.PackedNeRF.from_state_dict(synthetic.make_state_dict(1, 4, 128), DEV)
    assert narrow.kernel_net(f16s=True).W == 256 and narrow.f16s()[0].numel() == weights.PackedNeRF.from_state_dict(synthetic.make_state_dict(1, 4, 256), DEV).f16s()[0].numel()
    big = synthetic.make_state_dict(0, 8, 256)
    big["model_fine.linear_feat.weight"] = big["model_fine.linear_feat.weight"].copy()
    big["model_fine.linear_feat.weight"][3, 5] = 7.0e4                                      # beyond the f16 range: refused, not clipped
    with pytest.raises(MiNerfError):
        weights.PackedNeRF.from_state_dict(big, DEV).f16s()


def test_eval_harness_in_split_precision(tmp_path):
    """opts.precision = "f16s" takes the eval / video harness (test.py:17-108, 111-174) through the split-precision kernels: the frames
    are the fp32 harness's within one grey level, PSNR within 0.05 dB (the north star's dataset-level bar)."""
    from nerf_pytorch_paeng_amd import harness
    from nerf_pytorch_paeng_amd.model import NeRF, get_positional_encoder
    D, Wd, Hs, Ws = 4, 256, 20, 24
    sd = synthetic.make_state_dict(13, D, Wd)
    model = NeRF(D, Wd, 63, 27).to(DEV)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    posenc = get_positional_encoder(10), get_positional_encoder(4)
    K = np.array([[30.0, 0, Ws / 2], [0, 30.0, Hs / 2], [0, 0, 1]])
    poses = harness.get_render_pose(n_angle=3, phi=-30.0, nf=4.0)
    gt = torch.rand(3, Hs, Ws, 3, generator=torch.Generator().manual_seed(4)).to(DEV)
    res = {}
    for mode in ("fp32", "f16s"):
        opts = make_opts(N_samples_c=32, N_samples_f=32, perturb=0.0, exp_name="x", n_angle=3, single_angle=-1, phi=-30.0, nf=4.0, precision=mode)
        NP.manual_seed(7)
        res[mode] = harness.test(0, [0, 1, 2], posenc, model, gt, K, poses.to(DEV), (Hs, Ws), opts, keep_frames=True)
    for i in range(3):
        assert abs(res["f16s"]["psnr"][i] - res["fp32"]["psnr"][i]) < 0.05
        diff = np.abs(res["f16s"]["frames"][i][0].astype(np.int32) - res["fp32"]["frames"][i][0].astype(np.int32))
        assert diff.max() <= 1 and (diff > 0).mean() < 0.02
    with pytest.raises(ValueError):
        harness.test(0, [0], posenc, model, gt, K, poses.to(DEV), (Hs, Ws), make_opts(N_samples_c=32, N_samples_f=32, precision="fp8"))


# ---------------------------------------------------------------------------------------------------
# training forward in split precision (mi_nerf_mlp_rays_train_f16s): same stash, same layouts as the fp32 one
# ---------------------------------------------------------------------------------------------------
def _flat_params(sd, prefix, net):
    return torch.cat([torch.as_tensor(sd[prefix + k]).reshape(-1) for k in ops.param_names(net)]).float().to(DEV)


@pytest.mark.parametrize("D,skip", [(8, 4), (4, -1), (3, 0), (16, 14)])
def test_f16s_device_pack_is_the_host_pack(D, skip):
    sd = synthetic.make_state_dict(5, D, 256, skips=() if skip < 0 else (skip,))
    net = weights.infer_net(sd)
    assert (net.D, net.W, net.skip) == (D, 256, skip)
    host = ops.pack_module(sd, "model_fine.", net, f16s=True)
    m = ops.pack_map_f16s(net).to(DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    dev = ops.pack_apply_f16s(net, m, _flat_params(sd, "model_fine.", net), bad)
    assert torch.equal(dev.cpu(), host) and int(bad) == 0
    flat = _flat_params(sd, "model_fine.", net)
    flat[7] = 1e6                                                   # beyond f16: counted, not refused (the step cannot stop for a host check)
    ops.pack_apply_f16s(net, m, flat, bad)
    assert int(bad) > 0


def _one_tile_more_than_the_grid_has_waves():
    """Rays of 32 samples (one 32-point tile = one unit each) for which some wave of the split-precision kernels' grid (a workgroup of four
    waves per CU) runs a SECOND unit: only then is the weight ring's wrap to the head of the stream consumed (wstream_ring.h)."""
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count + 1


@pytest.mark.parametrize("n,S", [(300, 64), (77, 65), (64, 192), (0, 32)])
def test_f16s_training_forward_leaves_the_fp32_stash(n, S, lego_rays):
    """Same raw outputs (fp32 grade), same activation rows, same ReLU' bits in the backward kernel's own lane order: the masks may differ
    only where a pre-activation is within rounding of zero.  (n = 0: one tile more than the grid has waves.)"""
    n = n or _one_tile_more_than_the_grid_has_waves()
    sd = synthetic.make_state_dict(3, 8, 256)
    net = weights.infer_net(sd)
    rays = lego_rays[:n].contiguous()
    z = torch.sort(torch.rand(n, S, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) * 4 + 2, -1)[0]
    blob32 = ops.pack_module(sd, "model_fine.", net).to(DEV)
    blob16 = ops.pack_module(sd, "model_fine.", net, f16s=True).to(DEV)
    raw32, st32 = ops.mlp_rays_train(net, blob32, rays, z)
    lay = ops.train_layout(net, n, S)
    st16 = torch.full((lay.stash_bytes,), 0xCD, dtype=torch.uint8, device=DEV)          # poison: every byte the backward reads must be written
    raw16, st16 = ops.mlp_rays_train(net, blob16, rays, z, stash=st16, f16s=True)
    torch.cuda.synchronize()
    assert float((raw16 - raw32).abs().max()) < 2e-5 * float(raw32.abs().max())
    P, W, Dn = n * S, 256, net.D
    ntile = n * ((S + 31) // 32)

    def view(st, off, count, dtype):
        return st[off:off + count * 4].view(dtype)

    for name, off, cnt in (("stash_h", lay.stash_h, Dn * P * W), ("stash_f", lay.stash_f, P * W), ("stash_g", lay.stash_g, P * W // 2)):
        a, b = view(st32, off, cnt, torch.float32), view(st16, off, cnt, torch.float32)
        assert torch.isfinite(b).all(), name
        assert float((a - b).abs().max()) < 2e-5 * float(a.abs().max()), name
    # masks: bit-identical except where the fp32 kernel's pre-activation sits within rounding of zero
    for name, off, words, rows in (("mask_h", lay.mask_h, Dn * ntile * 64 * 4, None), ("mask_g", lay.mask_g, ntile * 64 * 2, None)):
        a, b = view(st32, off, words, torch.int32), view(st16, off, words, torch.int32)
        diff = (a ^ b)
        nbits = sum(int(((diff >> k) & 1).sum()) for k in range(32))
        assert nbits <= 2e-4 * words * 32, (name, nbits, words * 32)
    # ... and where they differ the stashed activation is (near) zero on both sides: rebuild the fp32 kernel's bit order for layer 0 of stash_h
    h32 = view(st32, lay.stash_h, P * W, torch.float32).reshape(n, S, W)
    m16 = view(st16, lay.mask_h, ntile * 64 * 4, torch.int32).reshape(n, (S + 31) // 32, 64, 4)
    tpr = (S + 31) // 32
    f = torch.arange(W, device=DEV)
    hh, word, bit = (f >> 2) & 1, f >> 6, 31 - (4 * ((f >> 3) & 7) + (f & 3))
    for chunk in range(tpr):
        j = torch.arange(min(32, S - 32 * chunk), device=DEV)
        lanes = j[:, None] + 32 * hh[None, :]                                           # [points, features] -> lane of the backward kernel
        got = (m16[:, chunk][:, lanes, word[None, :].expand_as(lanes)] >> bit[None, :]) & 1
        want = (h32[:, 32 * chunk + j] > 0).to(torch.int32)
        wrong = got != want
        assert float(wrong.float().mean()) < 2e-4
        assert float(h32[:, 32 * chunk + j][wrong].abs().max() if wrong.any() else 0.0) < 1e-5


def test_f16s_training_step_gradients_match_the_fp32_path(lego_rays):
    """loss.backward() through the split-precision forward against the fp32 path's on the same rays and depths; an optimizer step goes
    through; bf16 training is refused."""
    from nerf_pytorch_paeng_amd import train_path
    from nerf_pytorch_paeng_amd.model import NeRF
    sd = synthetic.make_state_dict(11, 8, 256)
    n, Sc, Nf = 256, 64, 128
    rays = lego_rays[:n].contiguous()
    opts = make_opts(perturb=1.0)
    g = torch.Generator(device=DEV).manual_seed(3)
    z_c = torch.sort(torch.rand(n, Sc, device=DEV, generator=g) * 4 + 2, -1)[0]
    z_f = torch.sort(torch.rand(n, Sc + Nf, device=DEV, generator=g) * 4 + 2, -1)[0]
    target = torch.rand(n, 3, device=DEV, generator=g)
    grads = {}
    for mode in (False, True):
        model = NeRF(8, 256, 63, 27).to(DEV)
        model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
        out = train_path.render_train(rays, model, opts, z_override=(z_c, z_f), f16s=mode)
        loss = ((out["rgb_c"] - target) ** 2).mean() + ((out["rgb_f"] - target) ** 2).mean()
        loss.backward()
        grads[mode] = {k: p.grad.clone() for k, p in model.named_parameters()}
        if mode:
            torch.optim.Adam(model.parameters(), lr=5e-4).step()
            st = train_path._state_for(model)
            assert int(st.f16s_out_of_range) == 0
    for k in grads[False]:
        a, b = grads[False][k], grads[True][k]
        assert torch.isfinite(b).all(), k
        # the fine network's trunk gradients on such batches are sums that almost cancel (terms a hundred times the result): two fp32-grade
        # forwards land 1e-4 .. 2e-3 apart there, like the reference's own fp32 result and an fp64 evaluation (the F11
        # test holds both forwards to that fp64 yardstick).  Everything else -- every coarse tensor, the heads, linear_feat / linear_d -- agrees
        # to fp32 rounding (observed <= 8e-7).
        ill = k.startswith("model_fine.linear_x.")
        assert float((a - b).abs().max()) <= (6e-3 if ill else 5e-6) * float(a.abs().max()), (k, float((a - b).abs().max()), float(a.abs().max()))
        assert float((a - b).norm()) <= (1.5e-3 if ill else 5e-6) * float(a.norm()), k
    model = NeRF(8, 256, 63, 27).to(DEV)
    with pytest.raises(MiNerfError):
        NP.render_rays(rays, model, None, opts, bf16=True)


@pytest.mark.parametrize("D,skip", [(8, 4), (3, 0), (2, -1), (16, 14), (15, 0)])
def test_f16s_backward_stream_device_pack_is_the_host_pack(D, skip):
    sd = synthetic.make_state_dict(6, D, 256, skips=() if skip < 0 else (skip,))
    net = weights.infer_net(sd)
    host = ops.pack_module(sd, "model_fine.", net, backward=True, f16s=True)
    m = ops.pack_map_f16s(net, backward=True).to(DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    dev = ops.pack_apply_f16s(net, m, _flat_params(sd, "model_fine.", net), bad, backward=True)
    assert torch.equal(dev.cpu(), host) and int(bad) == 0


@pytest.mark.parametrize("D,skip,n,S", [(8, 4, 200, 64), (8, 4, 64, 192), (3, 0, 77, 65), (2, -1, 40, 33), (8, 4, 0, 32)])
def test_f16s_backward_data_chain_matches_the_fp32_kernel(D, skip, n, S, lego_rays):
    """dgrad_f16s_kernel against mlp_dgrad_kernel on the same stash and the same (tiny) d_raw: every pre-activation gradient row --
    delta_d, delta_f, delta_h[l] -- within 2e-5 of the tensor's largest entry (two fp32-grade evaluations of the same chain).
    (n = 0: one tile more than the grid has waves.)"""
    n = n or _one_tile_more_than_the_grid_has_waves()
    sd = synthetic.make_state_dict(8, D, 256, skips=() if skip < 0 else (skip,))
    net = weights.infer_net(sd)
    rays = lego_rays[:n].contiguous()
    g = torch.Generator(device=DEV).manual_seed(n)
    z = torch.sort(torch.rand(n, S, device=DEV, generator=g) * 4 + 2, -1)[0]
    blob = ops.pack_module(sd, "model_fine.", net).to(DEV)
    _, stash = ops.mlp_rays_train(net, blob, rays, z)
    d_raw = (3e-5 * torch.randn(n, S, 4, device=DEV, generator=g)).contiguous()
    d_raw[:, :, 3] *= 0.05                                                       # density gradients are smaller than colour gradients
    b32 = ops.pack_module(sd, "model_fine.", net, backward=True).to(DEV)
    b16 = ops.pack_module(sd, "model_fine.", net, backward=True, f16s=True).to(DEV)
    lay = ops.train_layout(net, n, S)
    w32 = torch.zeros(lay.work_bytes, dtype=torch.uint8, device=DEV)
    w16 = torch.full((lay.work_bytes,), 0xCD, dtype=torch.uint8, device=DEV)     # poison: every row must be written
    ops.mlp_backward(net, blob, b32, rays, z, d_raw, stash, work=w32, stage=1)
    ops.mlp_backward(net, blob, b16, rays, z, d_raw, stash, work=w16, stage=1, f16s_dgrad=True)
    torch.cuda.synchronize()
    P, W = n * S, 256
    for name, off, cnt in (("delta_d", lay.delta_d, P * W // 2), ("delta_f", lay.delta_f, P * W), ("delta_h", lay.delta_h, D * P * W)):
        a, b = w32[off:off + 4 * cnt].view(torch.float32), w16[off:off + 4 * cnt].view(torch.float32)
        assert torch.isfinite(b).all(), name
        if name == "delta_h":
            for l in range(D):
                al, bl = a[l * P * W:(l + 1) * P * W], b[l * P * W:(l + 1) * P * W]
                assert float((al - bl).abs().max()) <= 2e-5 * float(al.abs().max()), (name, l, float((al - bl).abs().max()), float(al.abs().max()))
        else:
            assert float((a - b).abs().max()) <= 2e-5 * float(a.abs().max()), (name, float((a - b).abs().max()), float(a.abs().max()))


def test_f16s_training_loop_follows_the_fp32_loop(lego_rays):
    """Eight Adam steps through batchify_rays_and_render_by_chunk with f16s=True (all three MFMA kernels of the step in split precision) beside
    the same eight steps in fp32: the loss goes down and the two trajectories stay together."""
    from nerf_pytorch_paeng_amd.model import NeRF, get_positional_encoder
    sd = synthetic.make_state_dict(21, 8, 256)
    K, H, W = synthetic.lego_camera()
    n = 512
    o, d = lego_rays[:n, :3].contiguous(), lego_rays[:n, 3:].contiguous()
    target = torch.rand(n, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)) * 0.5 + 0.25
    opts = make_opts(perturb=1.0, chunk_rays=n)
    posenc = get_positional_encoder(10), get_positional_encoder(4)
    hist = {}
    for mode in (False, True):
        model = NeRF(8, 256, 63, 27).to(DEV)
        model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
        opt = torch.optim.Adam(model.parameters(), lr=5e-4)
        losses = []
        for step in range(8):
            rgb_c, _, rgb_f, _ = NP.batchify_rays_and_render_by_chunk(o, d, model, posenc, H, W, K, opts, seed=100 + step, f16s=mode)
            opt.zero_grad()
            loss = ((rgb_c - target) ** 2).mean() + ((rgb_f - target) ** 2).mean()
            loss.backward()
            opt.step()
            losses.append(float(loss))
        hist[mode] = losses
        assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert max(abs(a - b) for a, b in zip(hist[False], hist[True])) < 2e-3 * max(hist[False]), (hist[False], hist[True])


@pytest.mark.parametrize("gain,exact,n,S", [(16.0, True, 128, 64), (1.0, True, 77, 65), (3000.0, False, 128, 64)])
def test_f16s_backward_gradient_range(gain, exact, n, S, lego_rays):
    """The split-precision backward scales its gradient operands from max|d_raw| with seven binades of room for what the transposed weights
    add.  A layer that amplifies the gradient 16x stays inside (results of fp32 grade); one that amplifies it 3000x leaves the f16 range:
    FP16_OVFL saturates the conversion -- the gradients are then wrong in the saturated entries but never inf / NaN."""
    D = 4                                                                       # (77 x 65 = 5005 points: not a multiple of the 32-row load group)
    sd = synthetic.make_state_dict(9, D, 256, skips=())
    sd["model_fine.linear_feat.weight"] = (sd["model_fine.linear_feat.weight"] * gain).astype(np.float32)
    if exact:                                                                   # (the saturating case amplifies the forward too: it runs in fp32 here)
        sd["model_fine.linear_d.weight"] = (sd["model_fine.linear_d.weight"] / gain).astype(np.float32)   # compensated: the net amplification is in the backward chain's middle only
    net = weights.infer_net(sd)
    rays = lego_rays[:n].contiguous()
    g = torch.Generator(device=DEV).manual_seed(4)
    z = torch.sort(torch.rand(n, S, device=DEV, generator=g) * 4 + 2, -1)[0]
    blob = ops.pack_module(sd, "model_fine.", net).to(DEV)
    _, stash = ops.mlp_rays_train(net, blob, rays, z)
    d_raw = (1e-4 * torch.randn(n, S, 4, device=DEV, generator=g)).contiguous()
    b32 = ops.pack_module(sd, "model_fine.", net, backward=True).to(DEV)
    b16 = ops.pack_module(sd, "model_fine.", net, backward=True, f16s=True).to(DEV)
    g32, _ = ops.mlp_backward(net, blob, b32, rays, z, d_raw, stash)
    g16, work = ops.mlp_backward(net, blob, b16, rays, z, d_raw, stash, f16s_wgrad=True, f16s_dgrad=True)
    assert torch.isfinite(g16).all()
    top_raw, top_scaled = ops.backward_range(net, n, S, work)                    # what the scaled chain used of the f16 range
    assert abs(top_raw - float(d_raw.abs().max())) <= 1e-12
    if exact:
        assert float((g16 - g32).abs().max()) <= 1e-4 * float(g32.abs().max())
        assert 128.0 <= top_scaled < 65504.0, top_scaled
    else:
        assert top_scaled >= 65504.0, top_scaled                                 # the saturation is visible to the caller


def test_training_path_notices_a_saturated_f16s_backward(lego_rays, monkeypatch):
    """A 4000x amplification inside the backward chain, through the TRAINING path (render_train -> loss.backward()): the step reads the range words the
    split-precision backward left behind after each of the first F16S_CHECK_FIRST steps (and every F16S_CHECK_EVERY-th after them) and raises; in "warn" mode it
    warns and f16s_status() reports the numbers; a well-scaled network passes with the scaled chain inside the f16 range."""
    import warnings
    from types import SimpleNamespace
    from nerf_pytorch_paeng_amd import train_path
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    from nerf_pytorch_paeng_amd.model import NeRF
    n, Sc, Nf = 128, 32, 32
    rays = lego_rays[:n].contiguous()
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=Sc, N_samples_f=Nf, perturb=1.0)
    tgt = torch.rand(n, 3, generator=torch.Generator().manual_seed(2)).to(DEV)

    def step(model):
        model.zero_grad(set_to_none=True)
        out = train_path.render_train(rays, model, opts, seed=3, f16s=True)
        (torch.mean((out["rgb_c"] - tgt) ** 2) + torch.mean((out["rgb_f"] - tgt) ** 2)).backward()

    def make(gain):
        sd = synthetic.make_state_dict(9, 4, 256, skips=())
        for pre in ("model_coarse.", "model_fine."):
            # amplification in the BACKWARD chain's middle only: linear_feat / gain, linear_d's feature columns x gain -- the forward sees small
            # features and ordinary activations either side (in range for the f16s forward), the backward sees delta_f = gain x (...)
            sd[pre + "linear_feat.weight"] = (sd[pre + "linear_feat.weight"] / gain).astype(np.float32)
            sd[pre + "linear_feat.bias"] = (sd[pre + "linear_feat.bias"] / gain).astype(np.float32)
            w = sd[pre + "linear_d.weight"].copy()
            w[:, :256] *= gain
            sd[pre + "linear_d.weight"] = w.astype(np.float32)
        m = NeRF(4, 256, 63, 27, skips=[]).to(DEV)
        m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
        return m

    good = make(16.0)
    monkeypatch.setattr(train_path, "F16S_CHECK_FIRST", 0)                         # leave the words for the on-demand read
    monkeypatch.setattr(train_path, "F16S_CHECK_EVERY", 1000)
    step(good)
    st = train_path.f16s_status(good)
    assert not st["saturated"] and 128.0 <= st["max_abs_delta_scaled"] < 65504.0 and st["weights_out_of_range"] == 0, st
    assert all(torch.isfinite(p.grad).all() for p in good.parameters())

    # the default cadence: the words are read after BOTH nets' backward launches of each of the first F16S_CHECK_FIRST steps -- the very first
    # step raises, before any optimizer.step() has applied a clipped gradient (the message counts the steps already applied)
    monkeypatch.setattr(train_path, "F16S_CHECK_FIRST", 3)
    monkeypatch.setattr(train_path, "F16S_CHECK_EVERY", 50)
    bad = make(4000.0)
    with pytest.raises((MiNerfError, RuntimeError), match=r"split-precision training step out of range.*within the last 1 training step.*applied up to 0 of them"):
        step(bad)
    # only the FINE net amplifies: its words are in the first read too (until round 5 the first read came after the coarse launch alone)
    fine_only = make(4000.0)
    fine_only.model_coarse.load_state_dict(make(16.0).model_coarse.state_dict())
    with pytest.raises((MiNerfError, RuntimeError), match="split-precision training step out of range"):
        step(fine_only)
    monkeypatch.setattr(train_path, "F16S_ON_SATURATION", "warn")
    bad2 = make(4000.0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        step(bad2)
    assert any("out of range" in str(x.message) for x in w)
    # the cadence: behind the first F16S_CHECK_FIRST steps only every F16S_CHECK_EVERY-th is read; f16s_status reads on demand
    monkeypatch.setattr(train_path, "F16S_CHECK_FIRST", 1)
    monkeypatch.setattr(train_path, "F16S_CHECK_EVERY", 1000)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        step(bad2)
    assert not w
    st = train_path.f16s_status(bad2)
    assert st["saturated"] and st["max_abs_delta_scaled"] >= 65504.0, st
    assert not train_path.f16s_status(bad2)["saturated"]                         # read and reset


def test_f16s_training_llff_two_slabs_and_precision_flags(monkeypatch):
    """The split-precision step through the NDC (llff) entry, with the batch cut into two autograd nodes (slab size lowered): losses and
    coarse-network gradients equal the fp32 path's to fp32 rounding; harness.train takes the mode as opts.precision."""
    from nerf_pytorch_paeng_amd import harness, train_path
    from nerf_pytorch_paeng_amd.model import NeRF, get_positional_encoder
    monkeypatch.setattr(train_path, "MAX_TRAIN_RAYS", 96)
    sd = synthetic.make_state_dict(33, 4, 256, skips=(1,))
    K, H, W = synthetic.fern_camera()
    pose = torch.as_tensor(synthetic.fern_pose()[:3, :4], dtype=torch.float32)
    pix = T(synthetic.pixel_batch(H, W, 160, 3)).to(DEV)
    o, d = ops.make_o_d_pixels(W, H, K, synthetic.fern_pose(), pix)
    target = torch.rand(160, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    opts = make_opts(near=0.0, far=1.0, N_samples_c=32, N_samples_f=33, perturb=1.0, data_type="llff", chunk_rays=160)
    posenc = get_positional_encoder(10), get_positional_encoder(4)
    res = {}
    for mode in (False, True):
        model = NeRF(4, 256, 63, 27, skips=[1]).to(DEV)
        model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
        rgb_c, _, rgb_f, _ = NP.batchify_rays_and_render_by_chunk(o, d, model, posenc, H, W, K, opts, seed=9, f16s=mode)
        lc, lf = ((rgb_c - target) ** 2).mean(), ((rgb_f - target) ** 2).mean()
        (lc + lf).backward()
        res[mode] = (float(lc), float(lf), {k: p.grad.clone() for k, p in model.model_coarse.named_parameters()})
    assert abs(res[True][0] - res[False][0]) < 1e-6 and abs(res[True][1] - res[False][1]) < 2e-5
    for k, a in res[False][2].items():
        b = res[True][2][k]
        assert torch.isfinite(b).all() and float((a - b).abs().max()) <= 2e-5 * float(a.abs().max()) + 1e-12, k
    assert harness._precision(make_opts(precision="f16s")) == {"bf16": False, "f16s": True, "coarse_f16s": False, "f16": False, "coarse_f16": False}
    assert harness._precision(make_opts(precision="f16s+bf16")) == {"bf16": True, "f16s": False, "coarse_f16s": True, "f16": False, "coarse_f16": False}
