"""perceptual.Lpips / libmi_nerf_lpips.so on the GPU against the float64 restatement of tests/lpips_restate.py (torch on the CPU, written from
the definition in include/mi_nerf_lpips.h), on seeded random weights.  The bar is the one tests/test_gpu_parity.py uses for fp32 results:
with e_ref = max|f32 restatement - f64| and e_hip = max|HIP - f64| on the same inputs, e_hip <= max(4 * e_ref, 2e-5 * max|f64|); the factor
4 covers a different summation order over K = 9 * cin.  The shapes are the smallest at which the kernels can go wrong: the full VGG-16
channel plan at 32 x 40 (every N-tile grouping of the convolution kernel, 0.8 GFLOP per image), and a narrow plan at sizes that are no
multiple of the 8 x 16 tile and where the pool floor drops a row or a column.

One case of the issue cannot be built: "a NaN where only a max-pool's discarded remainder row would read it".  The first operation of every
accepted plan is a 3 x 3 convolution, which reads every pixel of the image, so no input pixel is read by a pool's remainder alone, and a
caller cannot plant a value into a feature map.  What the remainder does is held by the feature comparisons at odd sizes."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import harness, ops, synthetic
from nerf_pytorch_paeng_amd import nerf_process as NP
from nerf_pytorch_paeng_amd.model import NeRF, get_positional_encoder
from tests import lpips_restate as LR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FLOOR = 2e-5                                                           # relative to max|f64| (tests/test_gpu_parity.py)
# a POOL directly after a convolution (fused into its epilogue), a 96-channel layer (three N-tiles: one per workgroup)
FUSED = [("conv", 32), ("conv", 32), "pool", ("conv", 64), "tap", ("conv", 96), "tap"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    from nerf_pytorch_paeng_amd.build import build_lpips_library
    build_lpips_library()


_models, _refs = {}, {}


def model_of(plan, seed=0):
    from nerf_pytorch_paeng_amd.perceptual import Lpips
    key = (plan[0], tuple(plan[1]), seed)
    if key not in _models:
        w = LR.random_weights(plan, seed)
        _models[key] = (w, Lpips.from_arrays(plan, w["conv_w"], w["conv_b"], w["tap_w"], w["a"], w["b"], device=DEV))
    return _models[key]


def reference(plan, H, W, n=1, seed=0):
    """Images, and the restatement's features and distances in float64 and float32: computed once, shared, never changed."""
    key = (plan[0], tuple(plan[1]), H, W, n, seed)
    if key not in _refs:
        w, _ = model_of(plan, seed)
        pred, target = LR.smooth_images(n, H, W, plan[0], seed)
        r = {"pred": pred, "target": target}
        for name, dt in (("64", torch.float64), ("32", torch.float32)):
            r["f" + name] = LR.features(plan, w, pred, dt)
            r["d" + name], r["t" + name] = LR.distance(plan, w, pred, target, dt)
        _refs[key] = r
    return _refs[key]


def held(what, got, f64, f32):
    e_ref = float((f32.double() - f64).abs().max())
    e_hip = float((got.double().cpu() - f64).abs().max())
    bar = max(4 * e_ref, FLOOR * float(f64.abs().max()))
    print(f"{what}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  max|f64| {float(f64.abs().max()):.3e}  bar {bar:.3e}")
    assert torch.isfinite(got).all() and e_hip <= bar, (what, e_hip, e_ref, bar)


def check_plan(plan, H, W, n=1, seed=0):
    _, m = model_of(plan, seed)
    r = reference(plan, H, W, n, seed)
    tag = f"cin0 {plan[0]} {len(plan[1])} ops {H}x{W}"
    for t in range(len(m.tap_channels)):
        got = m.features(r["pred"].to(DEV), t)
        assert tuple(got.shape) == tuple(r["f64"][t].shape)
        held(f"{tag} features tap {t}", got, r["f64"][t], r["f32"][t])
    d, terms = m(r["pred"].to(DEV), r["target"].to(DEV), per_tap=True)
    held(f"{tag} distance", d, r["d64"], r["d32"])
    held(f"{tag} per-tap terms", terms, r["t64"], r["t32"])
    assert bool((d > 0).all())


@pytest.mark.parametrize("tap", range(5))
def test_vgg16_features_at_each_tap(tap):
    _, m = model_of(LR.VGG16)
    r = reference(LR.VGG16, 32, 40)
    got = m.features(r["pred"].to(DEV), tap)
    assert tuple(got.shape) == (1, 32 >> tap, 40 >> tap, [64, 128, 256, 512, 512][tap])
    held(f"vgg16 32x40 features tap {tap}", got, r["f64"][tap], r["f32"][tap])
    assert float(r["f64"][tap].abs().max()) > 0.1                   # the seeded weights keep the activations alive through 13 layers


def test_vgg16_distance_and_per_tap_terms():
    _, m = model_of(LR.VGG16)
    r = reference(LR.VGG16, 32, 40)
    d, terms = m(r["pred"].to(DEV), r["target"].to(DEV), per_tap=True)
    assert tuple(d.shape) == (1,) and tuple(terms.shape) == (1, 5)
    held("vgg16 32x40 distance", d, r["d64"], r["d32"])
    held("vgg16 32x40 per-tap terms", terms, r["t64"], r["t32"])
    # the flat frames test() holds, through ops.lpips
    flat = ops.lpips(r["pred"][0].reshape(-1, 3).to(DEV), r["target"][0].reshape(-1, 3).to(DEV), hw=(32, 40), model=m)
    assert torch.equal(flat, d)


@pytest.mark.parametrize("H,W", [(37, 45), (17, 16), (4, 4), (5, 131)])
def test_narrow_plan_at_sizes_off_the_tile_and_with_a_pool_remainder(H, W):
    check_plan(LR.NARROW, H, W, n=2)
    _, m = model_of(LR.NARROW)
    assert tuple(m.features(reference(LR.NARROW, H, W, 2)["pred"].to(DEV), 2).shape) == (2, H // 4, W // 4, 32)


@pytest.mark.parametrize("cin0", [1, 4])
def test_one_and_four_input_channels_and_a_pool_fused_into_the_convolution(cin0):
    check_plan((cin0, FUSED), 19, 35)
    check_plan((cin0, FUSED), 2, 2)


@pytest.mark.parametrize("name,ops", [("four N-tiles per workgroup", [("conv", 32), ("conv", 128), "tap"]),
                                      ("two N-tiles per workgroup", [("conv", 32), ("conv", 64), "tap"]),
                                      ("four N-tiles and a fused pool", [("conv", 32), ("conv", 128), "pool", ("conv", 32), "tap"]),
                                      ("two N-tiles and a fused pool", [("conv", 32), ("conv", 64), "pool", ("conv", 32), "tap"])])
def test_the_wide_channel_groups_a_launch_takes_once_it_fills_the_device(name, ops):
    """A convolution launch takes 128 or 64 output channels per workgroup only from 256 workgroups on (FILL_BLOCKS of csrc/lpips.hip):
    128 x 256 is 16 x 16 tiles, the smallest map at which one image's 128- and 64-channel layers do."""
    plan = (3, ops)
    _, m = model_of(plan)
    w, _ = model_of(plan)
    pred, _ = LR.smooth_images(1, 128, 256)
    f64, f32 = LR.features(plan, w, pred, torch.float64)[0], LR.features(plan, w, pred, torch.float32)[0]
    got = m.features(pred.to(DEV), 0)
    assert tuple(got.shape) == tuple(f64.shape)
    held(f"{name} 128x256 features", got, f64, f32)


def test_a_single_convolution_with_a_single_tap():
    check_plan((3, [("conv", 32), "tap"]), 9, 21)
    check_plan((3, [("conv", 32), "tap"]), 1, 1)


def test_pairs_do_not_depend_on_their_batch_and_runs_are_bit_identical():
    _, m = model_of(LR.NARROW)
    r = reference(LR.NARROW, 37, 45, n=3, seed=5)
    pred, target = r["pred"].to(DEV), r["target"].to(DEV)
    d, terms = m(pred, target, per_tap=True)
    for i in range(3):
        di, ti = m(pred[i:i + 1].contiguous(), target[i:i + 1].contiguous(), per_tap=True)
        assert torch.equal(di, d[i:i + 1]) and torch.equal(ti, terms[i:i + 1])
    again = m(pred, target)
    assert torch.equal(again, d)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = m(pred, target)
    side.synchronize()
    assert torch.equal(other, d)
    f0 = m.features(pred, 1)
    assert torch.equal(m.features(pred, 1), f0) and torch.equal(m.features(pred[1:2].contiguous(), 1), f0[1:2])


def test_identical_inputs_give_exactly_zero():
    for plan, H, W in ((LR.NARROW, 37, 45), (LR.VGG16, 32, 40)):
        _, m = model_of(plan)
        pred = reference(plan, H, W, n=3 if plan is LR.NARROW else 1, seed=5 if plan is LR.NARROW else 0)["pred"].to(DEV)
        d, terms = m(pred, pred.clone(), per_tap=True)
        assert float(d.abs().max()) == 0.0 and float(terms.abs().max()) == 0.0


@pytest.mark.parametrize("where", ["interior", "corner", "last row and column"])
def test_a_nan_reaches_its_own_pair_and_no_other(where):
    _, m = model_of(LR.NARROW)
    r = reference(LR.NARROW, 37, 45, n=3, seed=5)
    pred, target = r["pred"].to(DEV), r["target"].to(DEV)
    clean, clean_terms = m(pred, target, per_tap=True)
    y, x = {"interior": (20, 23), "corner": (0, 0), "last row and column": (36, 44)}[where]
    for victim in (pred, target):
        bad = victim.clone()
        bad[1, y, x, 1] = float("nan")
        d, terms = m(bad, target, per_tap=True) if victim is pred else m(pred, bad, per_tap=True)
        assert bool(torch.isnan(d[1])) and bool(torch.isnan(terms[1, 0]))
        assert torch.equal(d[[0, 2]], clean[[0, 2]]) and torch.equal(terms[[0, 2]], clean_terms[[0, 2]])
    # the NaN spreads by one pixel per convolution and survives ReLU and the pools: every tap of that image sees it
    bad = pred.clone()
    bad[1, y, x, 1] = float("nan")
    for t in range(3):
        f = m.features(bad, t)
        assert bool(torch.isnan(f[1]).any()) and not bool(torch.isnan(f[[0, 2]]).any())


def test_a_nan_survives_the_pool_fused_into_a_convolution_and_stays_local():
    _, m = model_of((3, FUSED))
    img = reference((3, FUSED), 19, 35)["pred"].clone()
    img[0, 7, 9, 2] = float("nan")
    # rows 5..9 x columns 7..11 after two convolutions, pooled rows 2..4 x columns 3..5, one more convolution: 5 x 5 pixels of the 9 x 17 map
    f = m.features(img.to(DEV), 0)
    nan = torch.isnan(f[0]).any(-1).cpu()
    assert bool(nan[1:6, 2:7].all()) and int(nan.sum()) == 25 and bool(torch.isnan(f[0, 1:6, 2:7]).all())


def test_all_zero_weights_give_zero_features_and_a_distance_of_exactly_zero():
    from nerf_pytorch_paeng_amd.perceptual import Lpips
    w, _ = model_of(LR.NARROW)
    m = Lpips.from_arrays(LR.NARROW, [torch.zeros_like(v) for v in w["conv_w"]], [torch.zeros_like(v) for v in w["conv_b"]], w["tap_w"], w["a"],
                          w["b"], device=DEV)
    r = reference(LR.NARROW, 17, 16, n=2)
    pred, target = r["pred"].to(DEV), r["target"].to(DEV)
    for t in range(3):
        assert float(m.features(pred, t).abs().max()) == 0.0
    d, terms = m(pred, target, per_tap=True)
    assert float(d.abs().max()) == 0.0 and float(terms.abs().max()) == 0.0 and not bool(torch.isnan(d).any())


def _small_scene(tmp_path):
    """The 20 x 24 scene of tests/test_gpu_iqa.py."""
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


def test_harness_reports_lpips_when_given_a_model_and_nothing_new_otherwise(tmp_path):
    idx, posenc, model, gt, K, poses, hw, opts = _small_scene(tmp_path)
    _, lp = model_of(LR.VGG16)
    save_dir, plain_dir, opts_dir = str(tmp_path / "with_lpips"), str(tmp_path / "plain"), str(tmp_path / "by_opts")
    NP.manual_seed(7)
    res = harness.test(idx, [0, 1, 2], posenc, model, gt.to(DEV), K, poses.to(DEV), hw, opts, log_dir=str(tmp_path), save_dir=save_dir, ssim=True,
                       lpips=lp)
    assert len(res["lpips"]) == 3 and all(isinstance(v, float) and np.isfinite(v) and v > 0 for v in res["lpips"])
    # the float frames the harness rendered: the same poses, the same seed, the checkpoint the harness loaded
    NP.manual_seed(7)
    with torch.no_grad():
        for i in range(3):
            rgb, _ = harness._render_pose(model, posenc, K, poses[i].float().to(DEV), hw, opts)
            want = ops.lpips(rgb.reshape(-1, 3), gt[i].reshape(-1, 3).to(DEV), hw=hw, model=lp)
            assert float(want[0]) == res["lpips"][i]
    assert res["best_lpips"] == min(res["lpips"]) and abs(res["mean_lpips"] - float(np.mean(res["lpips"]))) < 1e-12
    assert len(res["ssim"]) == 3 and res["best_ssim"] == max(res["ssim"])
    lines = open(os.path.join(save_dir, "_result.txt")).read().split("\n")
    for i in range(3):
        assert lines[i] == f"idx:{i}\tloss:{res['loss'][i]}\tpsnr:{res['psnr'][i]}\tssim:{res['ssim'][i]}\tlpips:{res['lpips'][i]}"
    assert lines[4] == f"Best Value ) PSNR : {res['best_psnr']}\tSSIM : {res['best_ssim']}\tLPIPS : {res['best_lpips']}"
    assert lines[5] == f"Mean Value ) PSNR : {res['mean_psnr']}\tSSIM : {res['mean_ssim']}\tLPIPS : {res['mean_lpips']}"
    # the default: no LPIPS, the file text of before
    NP.manual_seed(7)
    plain = harness.test(idx, [0, 1, 2], posenc, model, gt.to(DEV), K, poses.to(DEV), hw, opts, log_dir=str(tmp_path), save_dir=plain_dir)
    assert plain["lpips"] is None and "best_lpips" not in plain and "mean_lpips" not in plain
    assert plain["psnr"] == res["psnr"] and plain["loss"] == res["loss"]
    want = "".join(f"idx:{i}\tloss:{plain['loss'][i]}\tpsnr:{plain['psnr'][i]}\tssim:n/a\tlpips:n/a\n" for i in range(3))
    want += f"\nBest Value ) PSNR : {plain['best_psnr']}\tSSIM : n/a\tLPIPS : n/a\nMean Value ) PSNR : {plain['mean_psnr']}\tSSIM : n/a\tLPIPS : n/a"
    assert open(os.path.join(plain_dir, "_result.txt")).read() == want
    # a reference-style options object can carry the model; without SSIM the LPIPS column follows PSNR
    NP.manual_seed(7)
    by_opts = harness.test(idx, [0, 1, 2], posenc, model, gt.to(DEV), K, poses.to(DEV), hw, SimpleNamespace(**vars(opts), lpips=lp),
                           log_dir=str(tmp_path), save_dir=opts_dir)
    assert by_opts["lpips"] == res["lpips"] and by_opts["ssim"] is None
    assert open(os.path.join(opts_dir, "_result.txt")).read().split("\n")[0].endswith(f"ssim:n/a\tlpips:{res['lpips'][0]}")
