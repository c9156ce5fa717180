"""ops.ssim / mi_iqa_ssim on the GPU against the float64 oracle of tests/test_iqa_cpu.py (torch on the CPU, written from the definition in
include/mi_nerf_iqa.h).  The bar is the one tests/test_gpu_parity.py uses for fp32 results: |hip - f64| <= max(4 * e_ref, 2e-5), where
e_ref = |f32_cpu - f64| is the error of the same computation in float32 on the CPU, on the same inputs -- for the scalar, and pixel by
pixel for the map (var = E[x^2] - mu^2 cancels, so the map's bound comes from the comparator's error at that pixel, not from the scalar's)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nerf_pytorch_paeng_amd import harness, ops, synthetic
from nerf_pytorch_paeng_amd import nerf_process as NP
from nerf_pytorch_paeng_amd.model import NeRF, get_positional_encoder
from tests.test_iqa_cpu import C1, matlab_factor, ssim_oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FLOOR = 2e-5                                                           # the project's floor for fp32 results (tests/test_gpu_parity.py)
SHAPES = [(11, 11), (12, 37), (48, 48), (97, 131), (378, 504), (800, 800)]
OPTIONS = {"plain": {}, "clamp_cs": {"clamp_cs": True}, "matlab": {"downsample": 0}, "pool2": {"downsample": 2}, "pool3": {"downsample": 3},
           "pool2_clamp": {"downsample": 2, "clamp_cs": True}}


@pytest.fixture(scope="module", autouse=True)
def _built():
    from nerf_pytorch_paeng_amd.build import build_iqa_library
    build_iqa_library()


_frames = {}


def rendered_frame(H, W):
    """A frame of the synthetic network (synthetic.make_state_dict) seen from the lego camera's pose, rendered by the product at H x W."""
    if (H, W) not in _frames:
        D, Wd = 4, 128
        model = NeRF(D, Wd, 63, 27).to(DEV)
        model.load_state_dict({k: torch.as_tensor(v) for k, v in synthetic.make_state_dict(5, D, Wd).items()})
        model.eval()
        K = np.array([[1.2 * W, 0, W / 2], [0, 1.2 * W, H / 2], [0, 0, 1]])
        pose = torch.from_numpy(synthetic.pose_spherical(30.0, -30.0, 4.0)).float().to(DEV)
        opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=16, N_samples_f=16, perturb=0.0, chunk_rays=32768, chunk_pts=524288,
                               data_type="blender", gpu_ids=[0], rank=0)
        posenc = get_positional_encoder(10), get_positional_encoder(4)
        with torch.no_grad():
            NP.manual_seed(11)
            rgb, _ = harness._render_pose(model, posenc, K, pose, (H, W), opts)
        _frames[(H, W)] = rgb.reshape(H, W, 3).cpu()
    return _frames[(H, W)]


def make_pair(kind, H, W):
    g = torch.Generator().manual_seed(H * 1000 + W)
    if kind == "random":                                               # beyond [0, 1] on both sides: nothing is clamped
        return torch.rand(H, W, 3, generator=g) * 1.2 - 0.1, torch.rand(H, W, 3, generator=g) * 1.2 - 0.1
    frame = rendered_frame(H, W)
    if kind == "blurred":
        other = F.avg_pool2d(frame.permute(2, 0, 1)[None], 3, stride=1, padding=1, count_include_pad=False)[0].permute(1, 2, 0).contiguous()
    else:
        other = frame + 0.05 * torch.randn(H, W, 3, generator=g)
    return other, frame


def check_scalar(tag, got, pred, target, **kw):
    v64, _ = ssim_oracle(pred, target, **kw)
    v32, _ = ssim_oracle(pred, target, dtype=torch.float32, **kw)
    e_ref, e_hip = abs(float(v32) - float(v64)), abs(float(got) - float(v64))
    print(f"{tag}: ssim {float(v64):+.7f}  e_ref {e_ref:.2e}  |hip - f64| {e_hip:.2e}")
    assert e_hip <= max(4 * e_ref, FLOOR), (tag, float(got), float(v64), e_ref)
    return float(v64)


@pytest.mark.parametrize("opt", sorted(OPTIONS))
@pytest.mark.parametrize("kind", ["random", "blurred", "noised"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_ssim_and_map_match_the_float64_oracle(H, W, kind, opt):
    kw = OPTIONS[opt]
    pred, target = make_pair(kind, H, W)
    ds = kw.get("downsample", 1)
    f = matlab_factor(H, W) if ds == 0 else ds
    if H // f < 11 or W // f < 11:                                     # pooled below the window: refused, nothing computed
        with pytest.raises(ops.MiNerfError, match="window"):
            ops.ssim(pred.to(DEV), target.to(DEV), **kw)
        return
    got, gmap = ops.ssim(pred.to(DEV), target.to(DEV), return_map=True, **kw)
    assert got.shape == (1,) and gmap.shape == (1, H // f - 10, W // f - 10, 3) and got.is_cuda
    tag = f"{H}x{W} {kind} {opt}"
    check_scalar(tag, got.cpu()[0], pred, target, **kw)
    _, m64 = ssim_oracle(pred, target, **kw)
    _, m32 = ssim_oracle(pred, target, dtype=torch.float32, **kw)
    e_ref = (m32.double() - m64).abs()
    e_hip = (gmap[0].cpu().double() - m64).abs()
    print(f"{tag}: map max e_ref {float(e_ref.max()):.2e}  max |hip - f64| {float(e_hip.max()):.2e}")
    assert bool((e_hip <= torch.clamp(4 * e_ref, min=FLOOR)).all()), (tag, float(e_hip.max()))
    assert torch.equal(ops.ssim(pred.to(DEV), target.to(DEV), **kw), got)          # without the map: the same bits


def test_exact_cases():
    g = torch.Generator().manual_seed(1)
    img = torch.rand(97, 131, 3, generator=g)
    for kw in ({}, {"clamp_cs": True}, {"downsample": 2}):
        v = check_scalar(f"identical {kw}", ops.ssim(img.to(DEV), img.to(DEV), **kw).cpu()[0], img, img, **kw)
        assert abs(v - 1.0) < 1e-12
    for a, b in ((0.2, 0.9), (0.5, 0.5), (0.0, 1.0), (0.03, 0.04), (1.5, -0.25)):
        x, y = torch.full((40, 75, 3), a), torch.full((40, 75, 3), b)
        v = check_scalar(f"constant {a} {b}", ops.ssim(x.to(DEV), y.to(DEV)).cpu()[0], x, y)
        xa, xb = float(x[0, 0, 0]), float(y[0, 0, 0])
        assert abs(v - (2 * xa * xb + C1) / (xa * xa + xb * xb + C1)) < 1e-12


def test_nan_pixel_gives_nan_for_that_frame_only():
    g = torch.Generator().manual_seed(2)
    pred, target = torch.rand(3, 48, 70, 3, generator=g), torch.rand(3, 48, 70, 3, generator=g)
    clean = ops.ssim(pred.to(DEV), target.to(DEV)).cpu()
    for where in ((0, 0), (47, 69), (20, 33)):
        bad = pred.clone()
        bad[1, where[0], where[1], 2] = float("nan")
        for kw in ({}, {"clamp_cs": True}, {"downsample": 2}):
            got = ops.ssim(bad.to(DEV), target.to(DEV), **kw).cpu()
            ref = ops.ssim(pred.to(DEV), target.to(DEV), **kw).cpu()
            assert torch.isnan(got[1]) and got[0] == ref[0] and got[2] == ref[2], (where, kw, got)
    assert torch.isfinite(clean).all()
    got = ops.ssim(pred.to(DEV), torch.where(torch.arange(3)[:, None, None, None] == 2, torch.tensor(float("nan")), target).to(DEV)).cpu()
    assert torch.isnan(got[2]) and torch.equal(got[:2], clean[:2])                  # in the target just as well


def test_batches_runs_and_streams_give_the_same_bits():
    g = torch.Generator().manual_seed(3)
    N, H, W = 5, 97, 131
    pred, target = torch.rand(N, H, W, 3, generator=g).to(DEV), torch.rand(N, H, W, 3, generator=g).to(DEV)
    for kw in ({}, {"downsample": 2, "clamp_cs": True}):
        both, bmap = ops.ssim(pred, target, return_map=True, **kw)
        assert both.shape == (N,)
        for i in range(N):
            one, omap = ops.ssim(pred[i], target[i], return_map=True, **kw)
            assert torch.equal(one[0], both[i]) and torch.equal(omap[0], bmap[i])                          # a batch == N single calls
            assert torch.equal(ops.ssim(pred[i].reshape(-1, 3), target[i].reshape(-1, 3), hw=(H, W), **kw), one)   # the flat frame of test()
            check_scalar(f"batch frame {i} {kw}", both[i].cpu(), pred[i].cpu(), target[i].cpu(), **kw)
        assert torch.equal(ops.ssim(pred, target, **kw), both)                                             # run to run
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            on_side = ops.ssim(pred, target, **kw)
        side.synchronize()
        assert torch.equal(on_side, both)                                                                  # on a side stream
    with pytest.raises(ops.MiNerfError):
        ops.ssim(pred, target[:, :, :100])
    with pytest.raises(ops.MiNerfError, match="downsample"):
        ops.ssim(pred, target, downsample=-2)


def _small_scene(tmp_path):
    """The 20 x 24 scene of tests/test_gpu_harness.py::test_eval_and_video_harness_from_reference_checkpoint."""
    D, Wd, Hs, Ws = 4, 128, 20, 24
    sd = synthetic.make_state_dict(13, D, Wd)
    src = NeRF(D, Wd, 63, 27)
    src.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    exp, idx = "lego_t", 2000
    os.makedirs(tmp_path / exp)
    torch.save({"idx": idx, "model_state_dict": src.state_dict(), "optimizer_state_dict": {}}, harness._ckpt_path(str(tmp_path), exp, idx))
    model = NeRF(D, Wd, 63, 27).to(DEV)
    posenc = get_positional_encoder(10), get_positional_encoder(4)
    K = np.array([[30.0, 0, Ws / 2], [0, 30.0, Hs / 2], [0, 0, 1]])
    poses = harness.get_render_pose(n_angle=3, phi=-30.0, nf=4.0)
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=32, N_samples_f=32, perturb=0.0, chunk_rays=4096, chunk_pts=524288,
                           data_type="blender", gpu_ids=[0], rank=0, exp_name=exp, n_angle=3, single_angle=-1, phi=-30.0, nf=4.0)
    gt = torch.rand(3, Hs, Ws, 3, generator=torch.Generator().manual_seed(4))
    return idx, posenc, model, gt, K, poses, (Hs, Ws), opts


def test_harness_reports_ssim_when_asked_and_nothing_new_otherwise(tmp_path):
    idx, posenc, model, gt, K, poses, hw, opts = _small_scene(tmp_path)
    save_dir, plain_dir, opts_dir = str(tmp_path / "with_ssim"), str(tmp_path / "plain"), str(tmp_path / "by_opts")
    NP.manual_seed(7)
    res = harness.test(idx, [0, 1, 2], posenc, model, gt.to(DEV), K, poses.to(DEV), hw, opts, log_dir=str(tmp_path), save_dir=save_dir, ssim=True)
    assert len(res["ssim"]) == 3 and all(isinstance(v, float) and np.isfinite(v) and -1.0 < v <= 1.0 for v in res["ssim"])
    # the float frames the harness rendered: the same poses, the same seed, the checkpoint the harness loaded
    NP.manual_seed(7)
    with torch.no_grad():
        for i in range(3):
            rgb, _ = harness._render_pose(model, posenc, K, poses[i].float().to(DEV), hw, opts)
            check_scalar(f"harness frame {i}", res["ssim"][i], rgb.reshape(hw[0], hw[1], 3).cpu(), gt[i])
    assert res["best_ssim"] == max(res["ssim"]) and abs(res["mean_ssim"] - float(np.mean(res["ssim"]))) < 1e-12
    lines = open(os.path.join(save_dir, "_result.txt")).read().split("\n")
    for i in range(3):
        assert lines[i] == f"idx:{i}\tloss:{res['loss'][i]}\tpsnr:{res['psnr'][i]}\tssim:{res['ssim'][i]}\tlpips:n/a"
    assert lines[4] == f"Best Value ) PSNR : {res['best_psnr']}\tSSIM : {res['best_ssim']}\tLPIPS : n/a"
    assert lines[5] == f"Mean Value ) PSNR : {res['mean_psnr']}\tSSIM : {res['mean_ssim']}\tLPIPS : n/a"
    # the default: no SSIM, the file text of before
    NP.manual_seed(7)
    plain = harness.test(idx, [0, 1, 2], posenc, model, gt.to(DEV), K, poses.to(DEV), hw, opts, log_dir=str(tmp_path), save_dir=plain_dir)
    assert plain["ssim"] is None and "best_ssim" not in plain and "mean_ssim" not in plain
    assert plain["psnr"] == res["psnr"] and plain["loss"] == res["loss"]
    want = "".join(f"idx:{i}\tloss:{plain['loss'][i]}\tpsnr:{plain['psnr'][i]}\tssim:n/a\tlpips:n/a\n" for i in range(3))
    want += f"\nBest Value ) PSNR : {plain['best_psnr']}\tSSIM : n/a\tLPIPS : n/a\nMean Value ) PSNR : {plain['mean_psnr']}\tSSIM : n/a\tLPIPS : n/a"
    assert open(os.path.join(plain_dir, "_result.txt")).read() == want
    # a reference-style options object can ask for it
    NP.manual_seed(7)
    by_opts = harness.test(idx, [0, 1, 2], posenc, model, gt.to(DEV), K, poses.to(DEV), hw, SimpleNamespace(**vars(opts), ssim=True),
                           log_dir=str(tmp_path), save_dir=opts_dir)
    assert by_opts["ssim"] == res["ssim"]
