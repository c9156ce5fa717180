"""The f16 render modes on the GPU: MI_NERF_MODE_F16 (both networks on the f16 MFMA kernel, csrc/mlp_f16.hip) and MI_NERF_MODE_F16_BF16
(coarse network in f16, fine network in bf16; BASELINE config #5).  The kernel against its rounding-point oracle (tests/test_f16_mode_cpu.py
mlp_forward_f16) with a measured comparator, against the bf16 kernel's error, the mode 9 composition, ray-count invariance, the range
contract, the Python surface, and the held-out frame of a trained network against ground truth."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import harness, ops, synthetic, weights
from nerf_pytorch_paeng_amd import nerf_process as NP
from nerf_pytorch_paeng_amd._lib import MiNerfError
from nerf_pytorch_paeng_amd.model import NeRF, get_positional_encoder
from oracle import restate as R
from tests.test_f16_mode_cpu import mlp_forward_f16

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


def f16_net_alone(packed, rays, z):
    """The f16 network alone: mi_nerf_time_mlp_rays in MI_NERF_MODE_F16, one launch (the launcher picks the shape)."""
    n, S = z.shape
    raw = torch.empty(n, S, 4, dtype=torch.float32, device=DEV)
    ops.time_mlp_rays(packed.kernel_net(f16s=True), packed.f16s()[1], rays, z, raw, 1, f16=True)
    torch.cuda.synchronize()
    return raw


# ---------------------------------------------------------------------------------------------------
# the network against its oracle, and against the bf16 kernel
# ---------------------------------------------------------------------------------------------------
def launch_shape(n, S):
    """The launch the f16 / bf16 launch plan picks for n rays of S samples (mlp_half_core.h mlp_rays_half, points_per_wave 0): "64" (whole
    rounds of the 64-point shape, or one partial one), "32" (one round of the 32-point shape) or "64+32" (both phases in one launch)."""
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    tiles, round4, round2 = n * ((S + 31) // 32), cus * 8, cus * 4
    main = tiles // round4 * round4
    rem = tiles - main
    if rem == 0 or rem > round2:
        return "64"
    return "32" if main == 0 else "64+32"


ORACLE_CASES = [(8, 4, 10, 4, 300, 64), (8, 4, 10, 4, 64, 192), (3, 0, 10, 4, 77, 65), (2, -1, 6, 2, 40, 33),
                (8, 4, 10, 4, 1024, 64), (8, 4, 10, 4, 1100, 64), (16, 14, 10, 4, 77, 65)]


def test_oracle_cases_cover_every_launch_shape():
    """On this device the cases below run all three launches of the plan: the 32-point shape alone, the 64-point shape alone, and the
    two-phase 64 + 32 launch (on 256 CUs: <= 1024 tiles; 1024 x 64 = 2048 tiles; 1100 x 64 = 2200 tiles)."""
    shapes = {launch_shape(n, S) for *_, n, S in ORACLE_CASES}
    assert shapes == {"32", "64", "64+32"}, shapes


@pytest.mark.parametrize("D,skip,L_x,L_d,n,S", ORACLE_CASES)
def test_f16_network_vs_oracle(D, skip, L_x, L_d, n, S, lego_rays):
    """max |gpu - oracle_fp64| <= max(4 e_ref, 2e-5), e_ref = max |oracle_fp32 - oracle_fp64|: the oracle's own fp32 accumulation noise, rounding-
    boundary flips included, measured on the same inputs.  The launch shape each case takes is printed (launch_shape; on 256 CUs the first
    four run the 32-point shape, 1024 x 64 the 64-point shape alone, 1100 x 64 the two-phase 64 + 32 launch)."""
    skips = (skip,) if skip >= 0 else ()
    in_x, in_d = 3 + 6 * L_x, 3 + 6 * L_d
    sd = synthetic.make_state_dict(40 + D, D, 256, in_x=in_x, in_d=in_d, skips=skips)
    packed = weights.PackedNeRF.from_state_dict(sd, DEV)
    assert (packed.net.L_x, packed.net.L_d, packed.net.skip) == (L_x, L_d, skip)
    rays = lego_rays[:n].contiguous()
    z = torch.sort(T(R.counter_uniform(6, 0, 0, n, S)) * 4 + 2, -1)[0]
    got = f16_net_alone(packed, rays, z.to(DEV)).cpu().double().reshape(-1, 4)
    x = R.embed(rays.cpu(), z, L_x, L_d)
    ref64 = mlp_forward_f16(sd, "model_fine.", x, D, in_x, in_d, skips=skips, dtype=torch.float64)
    ref32 = mlp_forward_f16(sd, "model_fine.", x, D, in_x, in_d, skips=skips, dtype=torch.float32).double()
    e_ref, e_gpu = float((ref32 - ref64).abs().max()), float((got - ref64).abs().max())
    print(f"f16 kernel D={D} skip={skip} L={L_x}/{L_d} n={n} S={S} ({launch_shape(n, S)}-point launch): max |gpu - oracle64| {e_gpu:.3e}, "
          f"max |oracle32 - oracle64| {e_ref:.3e}")
    assert torch.isfinite(got).all()
    assert e_gpu <= max(4 * e_ref, 2e-5), (e_gpu, e_ref)
    if D > ops.HALF_64PT_MAX_D:
        # The 64-point shape's LDS holds 12 layers' side tables: the plan runs a deeper network at 32 points per wave whatever the launch size
        # (launch_shape() above describes D <= 12).  2200 rays x 3 tiles is where it would open with whole 64-point rounds: same rays, same bits.
        big, zb = lego_rays[:2200].contiguous(), z[torch.arange(2200) % n].to(DEV)
        assert torch.equal(f16_net_alone(packed, big, zb)[:n].cpu().double().reshape(-1, 4), got)


@pytest.mark.parametrize("n", [300, 1100])
def test_f16_error_is_well_below_bf16s(n, lego_rays):
    """The mode is what it says: against the fp32 kernel, the f16 network's |d raw| is >= 4x smaller than the bf16 kernel's (median and p99).
    300 rays: the 32-point shape; 1100 rays: the two-phase launch (on 256 CUs)."""
    sd = synthetic.make_state_dict(0, 8, 256)
    packed = weights.PackedNeRF.from_state_dict(sd, DEV)
    S = 64
    rays = lego_rays[:n].contiguous()
    z = torch.sort(T(R.counter_uniform(7, 0, 0, n, S)) * 4 + 2, -1)[0].to(DEV)
    raw32 = ops.mlp_rays(packed.net, packed.fine, rays, z)
    d16 = (f16_net_alone(packed, rays, z) - raw32).abs().flatten().double()
    db16 = (ops.mlp_rays(packed.net, packed.bf16()[1], rays, z, bf16=True) - raw32).abs().flatten().double()
    q = lambda t, p: float(torch.quantile(t.cpu(), p))
    print(f"n={n} ({launch_shape(n, S)}-point launch) |d raw| vs fp32: f16 median {q(d16, 0.5):.2e} p99 {q(d16, 0.99):.2e}; bf16 median {q(db16, 0.5):.2e} p99 {q(db16, 0.99):.2e}")
    assert q(d16, 0.5) * 4 <= q(db16, 0.5) and q(d16, 0.99) * 4 <= q(db16, 0.99)


# ---------------------------------------------------------------------------------------------------
# render_rays in modes 8 and 9
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 1024, 4096])
def test_mode9_is_mode8_coarse_and_bf16_fine(n, lego_rays):
    """Mode 9's coarse pass is mode 8's bit for bit (rgb_c, disp_c); its fine raw output is the bf16 kernel alone on the same fine depths."""
    packed = weights.PackedNeRF.from_state_dict(synthetic.make_state_dict(0, 8, 256), DEV)
    rays = lego_rays[:n].contiguous()
    a = NP.render_rays(rays, packed, None, make_opts(), seed=4, f16=True)
    b = NP.render_rays(rays, packed, None, make_opts(), seed=4, bf16=True, coarse_f16=True, return_intermediates=True)
    assert torch.equal(a["rgb_c"], b["rgb_c"]) and torch.equal(a["disp_c"], b["disp_c"])
    fine = ops.mlp_rays(packed.net, packed.bf16()[1], rays, b["_z_f"].contiguous(), bf16=True)
    assert torch.equal(b["_raw_f"], fine)
    assert torch.isfinite(b["rgb_f"]).all() and torch.isfinite(a["rgb_f"]).all()


def test_mode9_results_do_not_depend_on_the_ray_count(lego_rays):
    """512 and 1024 rays (the launches whose coarse kernel does render_rays' middle in its epilogue) give the per-ray outputs of the same rays
    inside a 4096-ray call: same seed, same global ray index."""
    packed = weights.PackedNeRF.from_state_dict(synthetic.make_state_dict(0, 8, 256), DEV)
    whole = NP.render_rays(lego_rays, packed, None, make_opts(), seed=8, bf16=True, coarse_f16=True)
    for lo, hi in ((0, 512), (1024, 2048), (3584, 4096)):
        part = NP.render_rays(lego_rays[lo:hi].contiguous(), packed, None, make_opts(), seed=8, ray_offset=lo, bf16=True, coarse_f16=True)
        for k in ("rgb_c", "disp_c", "rgb_f", "disp_f"):
            assert torch.equal(part[k], whole[k][lo:hi]), (lo, hi, k)


def test_f16_forward_out_of_range_is_never_a_finite_colour(lego_rays):
    """RANGE CONTRACT (the split-precision one, include/mi_nerf.h): an activation at or beyond 65 520 -- one unit's bias -- is NaN in every
    output that depends on it, never finite: a trunk unit -> all four raw values; a linear_feat unit (no ReLU, either sign) or a linear_d unit
    -> the three colours, the density finite and unchanged.  Below -65 520 in front of a ReLU is exact: the unit is off.  Both modes, through
    render_rays too; the 32-point shape (40 rays) and the two-phase launch (1100 rays); a weight beyond the f16 range is refused."""
    n, S, D = 40, 64, 8
    rays = lego_rays[:n].contiguous()
    z = torch.sort(T(R.counter_uniform(5, 0, 0, n, S)) * 4 + 2, -1)[0].to(DEV)

    def net_with(name, unit, value):
        sd = synthetic.make_state_dict(23, D, 256)
        for prefix in ("model_coarse.", "model_fine."):
            b = sd[prefix + name].copy()
            b[unit] = value
            sd[prefix + name] = b
        return weights.PackedNeRF.from_state_dict(sd, DEV)

    base = f16_net_alone(weights.PackedNeRF.from_state_dict(synthetic.make_state_dict(23, D, 256), DEV), rays, z).reshape(-1, 4)
    coarse_only = make_opts(N_samples_f=0)                                      # render_rays' coarse pass (NaN weights would feed sample_pdf)
    assert torch.isfinite(base).all()
    for name, unit in (("linear_x.3.bias", 7), ("linear_x.7.bias", 200), ("linear_x.0.bias", 0)):
        packed = net_with(name, unit, 70000.0)
        got = f16_net_alone(packed, rays, z)
        assert torch.isfinite(ops.mlp_rays(packed.net, packed.fine, rays, z)).all()                   # fp32 carries it
        assert torch.isnan(got).all(), (name, int(torch.isfinite(got).sum()))
        for kw in (dict(f16=True), dict(bf16=True, coarse_f16=True)):
            out = NP.render_rays(rays, packed, None, coarse_only, seed=1, **kw)
            assert torch.isnan(out["rgb_c"]).all(), (name, kw)
    off = f16_net_alone(net_with("linear_x.3.bias", 7, -70000.0), rays, z)
    assert torch.equal(off, f16_net_alone(net_with("linear_x.3.bias", 7, -1000.0), rays, z)) and torch.isfinite(off).all()
    for name, unit, value in (("linear_feat.bias", 11, 70000.0), ("linear_feat.bias", 11, -70000.0), ("linear_d.bias", 5, 70000.0)):
        got = f16_net_alone(net_with(name, unit, value), rays, z).reshape(-1, 4)
        assert torch.isnan(got[:, :3]).all() and torch.equal(got[:, 3], base[:, 3]), (name, value)
        for kw in (dict(f16=True), dict(bf16=True, coarse_f16=True)):
            out = NP.render_rays(rays, net_with(name, unit, value), None, coarse_only, seed=1, **kw)
            assert torch.isnan(out["rgb_c"]).all(), (name, value, kw)
    # the same on the two-phase launch (64-point rounds + a 32-point remainder; the packing schedules of both shapes)
    rays_l = lego_rays[:1100].contiguous()
    z_l = torch.sort(T(R.counter_uniform(5, 0, 0, 1100, S)) * 4 + 2, -1)[0].to(DEV)
    base_l = f16_net_alone(weights.PackedNeRF.from_state_dict(synthetic.make_state_dict(23, D, 256), DEV), rays_l, z_l).reshape(-1, 4)
    assert launch_shape(1100, S) == "64+32" and torch.isfinite(base_l).all()
    assert torch.isnan(f16_net_alone(net_with("linear_x.3.bias", 7, 70000.0), rays_l, z_l)).all()
    for value in (70000.0, -70000.0):
        got = f16_net_alone(net_with("linear_feat.bias", 11, value), rays_l, z_l).reshape(-1, 4)
        assert torch.isnan(got[:, :3]).all() and torch.equal(got[:, 3], base_l[:, 3]), value
    assert torch.equal(f16_net_alone(net_with("linear_x.3.bias", 7, -70000.0), rays_l, z_l),
                       f16_net_alone(net_with("linear_x.3.bias", 7, -1000.0), rays_l, z_l))
    sd = synthetic.make_state_dict(23, D, 256)
    w = sd["model_coarse.linear_x.2.weight"].copy()
    w[3, 4] = 65504.0
    sd["model_coarse.linear_x.2.weight"] = w
    big = weights.PackedNeRF.from_state_dict(sd, DEV)
    for kw in (dict(f16=True), dict(bf16=True, coarse_f16=True)):
        with pytest.raises(MiNerfError):
            NP.render_rays(rays, big, None, make_opts(), seed=1, **kw)


def test_f16_modes_through_the_module_and_the_harness(lego_rays, tmp_path):
    """nn.Module (device-packed blobs) and PackedNeRF (host-packed) give the same frames in both modes; the training path refuses them; the
    eval harness renders "f16+bf16" frames."""
    sd = synthetic.make_state_dict(2, 8, 256)
    model = NeRF(8, 256, 63, 27).to(DEV)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    packed = weights.PackedNeRF.from_state_dict(sd, DEV)
    rays = lego_rays[:600].contiguous()
    for kw in (dict(f16=True), dict(bf16=True, coarse_f16=True)):
        with torch.no_grad():
            a = NP.render_rays(rays, model, None, make_opts(), seed=2, **kw)
        b = NP.render_rays(rays, packed, None, make_opts(), seed=2, **kw)
        for k in a:
            assert torch.equal(a[k], b[k]), (kw, k)
        with pytest.raises(MiNerfError):                                           # gradients enabled, trainable parameters: the training path
            NP.render_rays(rays, model, None, make_opts(), seed=2, **kw)
        with pytest.raises(MiNerfError):
            NP.batchify_rays_and_render_by_chunk(rays[:, :3], rays[:, 3:], model, None, 1, 600, None, make_opts(), seed=2, **kw)
    posenc = get_positional_encoder(10), get_positional_encoder(4)
    Hs, Ws = 20, 24
    K = np.array([[30.0, 0, Ws / 2], [0, 30.0, Hs / 2], [0, 0, 1]])
    poses = harness.get_render_pose(n_angle=2, phi=-30.0, nf=4.0)
    gt = torch.rand(2, Hs, Ws, 3, generator=torch.Generator().manual_seed(4)).to(DEV)
    opts = make_opts(N_samples_c=32, N_samples_f=32, perturb=0.0, exp_name="x", n_angle=2, single_angle=-1, phi=-30.0, nf=4.0, precision="f16+bf16")
    res = harness.test(0, [0, 1], posenc, model, gt, K, poses.to(DEV), (Hs, Ws), opts, save_dir=str(tmp_path), keep_frames=True)
    assert len(res["frames"]) == 2 and all(np.isfinite(p) for p in res["psnr"])
    written = sorted(p.name for p in tmp_path.rglob("*.png"))
    assert len(written) >= 2, written


# ---------------------------------------------------------------------------------------------------
# a trained network: the held-out frame of the sharp solids scene against ground truth
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solids(tmp_path_factory):
    """tests/test_gpu_trained.py's training fixture (its TRAINED_STEPS / TRAINED_VIEWS / TRAINED_SIZE honoured), for the solids scene only."""
    import tests.test_gpu_trained as TG
    return TG.trained.__wrapped__(SimpleNamespace(param="solids"), tmp_path_factory)


def test_trained_f16_frames_vs_ground_truth(solids):
    """The f16 and f16+bf16 held-out frames: finite, closer to the fp32 frame than the bf16 frame is, and f16+bf16 within 0.05 dB of the fp32
    frame against ground truth (the north star's bar, which all-bf16 misses on this scene)."""
    import tests.test_gpu_trained as TG
    gt = solids.test_img[0].reshape(-1, 3)
    pose = solids.poses[TG.N_IMG].to(DEV)
    geo = solids.geo
    frames = {}
    with torch.no_grad():
        for mode in ("fp32", "bf16", "f16", "f16+bf16"):
            opts = TG._opts(geo, precision=mode)
            NP.manual_seed(9)
            frames[mode] = harness._render_pose(harness._frozen(solids.model, opts), solids.posenc, solids.K, pose, (geo.HS, geo.WS), opts)[0]
    psnr = lambda a, b: float(-10.0 * torch.log10(torch.mean((a - b) ** 2)))
    base = psnr(frames["fp32"], gt)
    line, vs32 = [f"fp32 {base:.3f} dB vs ground truth"], {}
    for mode in ("bf16", "f16", "f16+bf16"):
        vs32[mode] = psnr(frames[mode], frames["fp32"])
        line.append(f"{mode}: {vs32[mode]:.1f} dB vs fp32 (max |d rgb| {float((frames[mode] - frames['fp32']).abs().max()):.2e}), "
                    f"{psnr(frames[mode], gt):.3f} dB vs ground truth ({psnr(frames[mode], gt) - base:+.3f})")
    print(f"\n[solids, {TG.N_STEPS} steps] held-out frame: " + "; ".join(line))
    for mode in ("f16", "f16+bf16"):
        assert torch.isfinite(frames[mode]).all()
        assert vs32[mode] > vs32["bf16"], (mode, vs32)
    assert abs(psnr(frames["f16+bf16"], gt) - base) < 0.05, (psnr(frames["f16+bf16"], gt), base)
