"""The reference's main loop (main.py:17-161: train -> test -> render) on this package, end to end on one MI355X, with a synthetic scene
standing in for the dataset loaders (no dataset ships with either repository).  Everything below `from nerf_pytorch_paeng_amd ...` keeps the
reference's names and call shapes (train.py:12, test.py:17, test.py:111); swap the imports back and the same script drives the reference.

    python examples/train_eval_render.py [--steps 2000] [--size 64] [--out /tmp/nerf_demo] [--precision fp32|f16s] [--net-width 256]
                                             [--scene teacher|solid] [--mesh PATH.ply [--mesh-res 128] [--mesh-iso 10] [--mesh-view]]
                                             [--train-occupancy WARMUP:EVERY] [--geometry ACC:DEPTH:DIST]
                                             [--fused-adam] [--lr-min LR --warmup STEPS] [--bake RES[:B[:STORAGE]] [--bake-finetune STEPS [--bake-reg TV_SIGMA:TV_COEF:SPARSITY] [--bake-optimizer adam|lazy]
                                             [--bake-levels RES:STEPS[,RES:STEPS...]] [--bake-prune TAU]] [--bake-prune-seen T_VIS] [--bake-locate DEG:DIST] [--bake-signed [CLIP]]]

``--scene solid``: the dataset is scenes.SolidScene.default() -- opaque solids in empty space on a white background, ground truth rendered by
mi_scene_render -- instead of views of a random network.  ``--mesh PATH``: after training, the fine network's density on a (mesh-res + 1)^3 lattice of the box
+-``--mesh-box`` is turned into a triangle mesh at the level ``--mesh-iso`` (mesh.extract: marching tetrahedra on the device), coloured by the
network and written as a binary PLY; with ``--mesh-view`` the video poses are then rasterised from the mesh (Mesh.render, the network left out) into
``render_mesh`` and the PSNR of each frame against the network's frame of the same pose is printed.  No counterpart in the reference.  ``--train-occupancy WARMUP:EVERY``: WARMUP full steps, then an
occupancy grid is baked from the model (128^3 cells; ``--scene solid``: the box +-1.5 with everything outside it skipped, otherwise a box that
holds every sample) and the remaining steps skip the samples it marks empty (occupancy_train.py), re-baking every EVERY steps (0: never).
``--geometry ACC:DEPTH:DIST``: the weights of the opacity, depth and distortion losses (geometry.py; e.g. 0.1:0:0.01); ACC and DEPTH are
supervised by the analytic scene's own opacity and depth, so they need ``--scene solid``.  ``--fused-adam``: optim.FusedAdam (one launch per
step, skipping a step whose gradients are not finite) instead of torch.optim.Adam.  ``--lr-min LR`` / ``--warmup STEPS``: the reference's
schedule (main.py:83-90, optim.CosineAnnealingWarmupRestarts) over one cycle of ``--steps``, from LR up to 5e-4 in STEPS steps and back; with
none of the three the run is what it was.  ``--bake RES[:B[:dense|sparse|sparse16]]``: after training, the fine network is baked into a radiance grid (baked.py:
density and B = 1, 4 or 9 spherical-harmonic colour coefficients, default 9, on a (RES + 1)^3 lattice of the box +-``--mesh-box``), the video poses
are rendered from the grid as well, with no network, and the PSNR of the grid's frames against the network's and both times are printed.
``--bake-finetune STEPS`` (dense storage): the baked grid is then fine-tuned on the training views' rays for STEPS steps
(baked_train.finetune: the backward pass of the grid renderer) and its PSNR on the test views is printed before and after;
``--bake-reg TV_SIGMA:TV_COEF:SPARSITY`` adds the lattice regularisers to those steps (total variation of the density plane and of the
records, Cauchy sparsity of the density; e.g. 0.01:0.01:0.01) and is refused without ``--bake-finetune``.
``--bake-optimizer lazy`` runs those steps with optim.LazyAdam on finetune's direct path (docs/design/26_lazy_optimizer.md); the default is torch.optim.Adam.
``--bake-levels RES:STEPS[,RES:STEPS...]`` trains the grid coarse to fine (baked_train.coarse_to_fine): the network is baked at the first
level's resolution -- eight times fewer evaluations per halving -- and each level's steps are followed by a resample to the next
(RadianceGrid.resample); the final level is ``--bake`` RES with ``--bake-finetune`` STEPS.  ``--bake-prune TAU`` ends every level with
RadianceGrid.prune(TAU): density and records are cleared away from density above TAU.  Both are refused without ``--bake RES --bake-finetune STEPS``.
``--bake-signed [CLIP]`` (any storage) bakes A SIGNED GRID (docs/design/29_signed_density.md): the plane is the network's density before its
ReLU, clamped to [-CLIP, CLIP] when CLIP is given, the ReLU is applied after the interpolation, and ``--bake-finetune`` trains it without the
clamp at 0.  It is refused together with ``--bake-prune-seen`` and ``--bake-locate``, whose rules read the density without the ReLU.
``--bake-prune-seen T_VIS`` (dense storage) prunes the grid by the training views (RadianceGrid.seen, RadianceGrid.prune(seen=...)): after the
bake, and with ``--bake-levels`` after every level instead; active points, record MiB and the held-out PSNR are printed before and after.
``--bake-locate DEG:DIST`` (any storage) turns the first held-out pose by DEG degrees and moves it by DIST, then recovers it against the
grid from that view's image alone (baked_pose.locate, docs/design/28_grid_ray_gradients.md); the image error and both pose errors are
printed before and after.
"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pytorch_paeng_amd import harness, scenes, synthetic                                  # noqa: E402
from nerf_pytorch_paeng_amd.model import NeRF, get_positional_encoder                          # noqa: E402  (model/NeRF.py, model/PositionalEncoding.py)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--size", type=int, default=64, help="training / test image side")
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--out", default="/tmp/nerf_demo")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "f16s"])
    ap.add_argument("--net-width", type=int, default=256)
    ap.add_argument("--render-views", type=int, default=8)
    ap.add_argument("--scene", default="teacher", choices=["teacher", "solid"], help="teacher: views of a random network; solid: scenes.SolidScene.default()")
    ap.add_argument("--mesh", default=None, metavar="PATH", help="write the trained scene's surface as a coloured PLY")
    ap.add_argument("--mesh-res", type=int, default=128, help="lattice cells per axis (1..512)")
    ap.add_argument("--mesh-iso", type=float, default=10.0, help="raw density of the surface")
    ap.add_argument("--mesh-box", type=float, default=1.5, help="the lattice spans +-this on every axis")
    ap.add_argument("--mesh-view", action="store_true", help="with --mesh: rasterise the video poses from the mesh too (Mesh.render) and compare with the network's frames")
    ap.add_argument("--train-occupancy", default=None, metavar="WARMUP:EVERY", help="train with an occupancy grid baked after WARMUP full steps, re-baked every EVERY steps")
    ap.add_argument("--geometry", default=None, metavar="ACC:DEPTH:DIST", help="weights of the opacity, depth and distortion losses (ACC, DEPTH: --scene solid only)")
    ap.add_argument("--fused-adam", action="store_true", help="optim.FusedAdam instead of torch.optim.Adam")
    ap.add_argument("--lr-min", type=float, default=None, help="warm-up cosine schedule from this rate up to 5e-4 and back over --steps")
    ap.add_argument("--warmup", type=int, default=None, help="warm-up steps of the schedule (default with --lr-min: a twentieth of --steps)")
    ap.add_argument("--bake", default=None, metavar="RES[:B[:STORAGE]]",
                    help="bake the fine network into a radiance grid and render the video from it too; STORAGE: dense (default), sparse or sparse16 (records of active points only, fp32 or f16)")
    ap.add_argument("--lpips", default=None, metavar="VGG_PTH:LIN_PTH", help="also report LPIPS: a torchvision vgg16 state dict and the lpips package's linear layers, two files for torch.load")
    ap.add_argument("--bake-finetune", type=int, default=0, metavar="STEPS", help="after --bake (dense), fine-tune the grid on the training views for STEPS steps")
    ap.add_argument("--bake-reg", default=None, metavar="TV_SIGMA:TV_COEF:SPARSITY",
                    help="with --bake-finetune: weights of the total variation of the density plane and of the records and of the density's sparsity prior")
    ap.add_argument("--bake-optimizer", choices=("adam", "lazy"), default="adam",
                    help="with --bake-finetune: torch.optim.Adam (default) or optim.LazyAdam, which steps only the grid elements a gradient reached")
    ap.add_argument("--bake-levels", default=None, metavar="RES:STEPS[,RES:STEPS...]",
                    help="with --bake RES --bake-finetune STEPS: bake at the first level's resolution and train coarse to fine through these levels; the final level is RES with STEPS steps")
    ap.add_argument("--bake-prune", type=float, default=None, metavar="TAU", help="with --bake-finetune: after each level, clear density and records away from density above TAU")
    ap.add_argument("--bake-signed", type=float, nargs="?", const=0.0, default=None, metavar="CLIP",
                    help="with --bake: a signed grid -- the density before its ReLU, clamped to [-CLIP, CLIP] when CLIP is given, the ReLU after the interpolation")
    ap.add_argument("--bake-prune-seen", type=float, default=None, metavar="T_VIS",
                    help="with --bake (dense): prune the grid by the training views -- density stays only around points that some training view sees with "
                         "transmittance at least T_VIS; after the bake, and after every level with --bake-levels")
    ap.add_argument("--bake-locate", default=None, metavar="DEG:DIST",
                    help="with --bake: perturb the first held-out pose by DEG degrees and DIST, recover it against the grid, print the errors before and after")
    a = ap.parse_args(argv)
    bake_locate = None
    if a.bake_locate is not None:
        try:
            bake_locate = tuple(float(v) for v in a.bake_locate.split(":"))
        except ValueError:
            bake_locate = ()
        if a.bake is None or len(bake_locate) != 2 or not all(np.isfinite(v) and v >= 0 for v in bake_locate):
            ap.error("--bake-locate takes DEG:DIST, two finite numbers >= 0, and needs --bake RES")
    if a.warmup is not None and not 0 <= a.warmup < a.steps:
        ap.error("--warmup takes a number of steps below --steps")
    if a.mesh_view and not a.mesh:
        ap.error("--mesh-view renders the mesh that --mesh PATH extracts: give both")
    bake_res = bake_B = None
    bake_storage = "dense"
    if a.bake_finetune and (a.bake is None or len(a.bake.split(":")) > 2 and a.bake.split(":")[2] != "dense"):
        ap.error("--bake-finetune needs --bake with dense storage (fine-tune dense, then compact)")
    if a.bake_prune_seen is not None:
        if a.bake is None or len(a.bake.split(":")) > 2 and a.bake.split(":")[2] != "dense":
            ap.error("--bake-prune-seen needs --bake with dense storage (prune dense, then compact)")
        if not 0.0 <= a.bake_prune_seen <= 1.0:
            ap.error("--bake-prune-seen takes a transmittance, 0 .. 1")
    if a.bake_signed is not None:
        if a.bake is None or not (np.isfinite(a.bake_signed) and a.bake_signed >= 0):
            ap.error("--bake-signed takes an optional CLIP, a finite number > 0, and needs --bake RES")
        if a.bake_prune_seen is not None or a.bake_locate is not None:
            ap.error("--bake-signed: --bake-prune-seen and --bake-locate read the density without the ReLU and refuse a signed grid")
    bake_reg = {}
    if a.bake_reg is not None:
        if not a.bake_finetune:
            ap.error("--bake-reg weighs the regularisers of --bake-finetune STEPS: give both")
        try:
            w_tvs, w_tvc, w_sp = (float(v) for v in a.bake_reg.split(":"))
        except ValueError:
            ap.error("--bake-reg takes TV_SIGMA:TV_COEF:SPARSITY, three numbers")
        if not all(np.isfinite(w) and w >= 0 for w in (w_tvs, w_tvc, w_sp)):
            ap.error("--bake-reg takes three non-negative numbers")
        bake_reg = {"tv_sigma": w_tvs, "tv_coef": w_tvc, "sparsity": w_sp}
    bake_levels = []
    if a.bake_levels is not None or a.bake_prune is not None:
        if not a.bake_finetune:                                                                  # (without --bake, --bake-finetune was refused above)
            ap.error("--bake-levels and --bake-prune shape the steps of --bake RES --bake-finetune STEPS: give those too")
        if a.bake_prune is not None and not (np.isfinite(a.bake_prune) and a.bake_prune >= 0):
            ap.error("--bake-prune takes a finite number >= 0")
        try:
            bake_levels = [tuple(int(v) for v in lv.split(":")) for lv in a.bake_levels.split(",")] if a.bake_levels else []
        except ValueError:
            ap.error("--bake-levels takes RES:STEPS[,RES:STEPS...], pairs of integers")
        if any(len(lv) != 2 or not 1 <= lv[0] <= 512 or lv[1] < 0 for lv in bake_levels):
            ap.error("--bake-levels takes RES in 1..512 and STEPS >= 0 per level")
    if a.bake is not None:
        fields = a.bake.split(":")
        try:
            bake_res, bake_B = (int(v) for v in (fields + ["9"])[:2])
        except ValueError:
            ap.error("--bake takes RES[:B[:STORAGE]], one or two integers and a storage")
        if len(fields) == 3:
            bake_storage = fields[2]
        if not 1 <= bake_res <= 512 or bake_B not in (1, 4, 9) or len(fields) > 3 or bake_storage not in ("dense", "sparse", "sparse16"):
            ap.error("--bake takes RES in 1..512, B in 1, 4, 9 and STORAGE in dense, sparse, sparse16")
    geometry = None
    if a.geometry is not None:
        try:
            w_acc, w_depth, w_dist = (float(v) for v in a.geometry.split(":"))
        except ValueError:
            ap.error("--geometry takes ACC:DEPTH:DIST, three numbers")
        if min(w_acc, w_depth, w_dist) < 0:
            ap.error("--geometry takes three non-negative numbers")
        if (w_acc or w_depth) and a.scene != "solid":
            ap.error("--geometry with ACC or DEPTH above zero needs --scene solid (the targets come from the analytic scene)")
        geometry = {"acc_weight": w_acc, "depth_weight": w_depth, "distortion_weight": w_dist}
    occ_warmup = occ_every = None
    if a.train_occupancy is not None:
        try:
            occ_warmup, occ_every = (int(v) for v in a.train_occupancy.split(":"))
        except ValueError:
            ap.error("--train-occupancy takes WARMUP:EVERY, two integers")
        if occ_warmup < 0 or occ_every < 0:
            ap.error("--train-occupancy takes two non-negative integers")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lpips_model = None
    if a.lpips is not None:
        if a.lpips.count(":") != 1:
            ap.error("--lpips takes VGG_PTH:LIN_PTH, two files")
        from nerf_pytorch_paeng_amd.perceptual import Lpips
        vgg_pth, lin_pth = a.lpips.split(":")
        lpips_model = Lpips.from_state_dicts(torch.load(vgg_pth, map_location="cpu"), torch.load(lin_pth, map_location="cpu"), input="lpips", device=dev)
    H = W = a.size
    # config.py:105-111 -- the fields the path reads, with lego.txt's values
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=64, N_samples_f=128, perturb=1.0, chunk_rays=4096, chunk_pts=524288, data_type="blender",
                           gpu_ids=[0], rank=0, exp_name="demo", N_rays=1024, global_batch=True, idx_save=a.steps, idx_print=500, n_angle=a.render_views,
                           single_angle=-1, phi=-30.0, nf=4.0, precision=a.precision)
    K800, _, _ = synthetic.lego_camera()
    K = np.array([[K800[0][0] * W / 800.0, 0, W / 2], [0, K800[1][1] * H / 800.0, H / 2], [0, 0, 1]])
    posenc = get_positional_encoder(10), get_positional_encoder(4)                               # main.py:133
    poses = harness.get_render_pose(n_angle=a.views + 2, phi=-30.0, nf=4.0)                      # stand-in for load_blender's camera list
    # the "dataset": views of a fixed random NeRF rendered by the inference kernels (the teacher); the last two views are the test set
    if a.scene == "solid":                                                                       # the same cameras, the analytic scene
        images = scenes.SolidScene.default().render_views(poses, K, (H, W), opts.near, opts.far, 1024, dev)
        if geometry is not None:
            geometry["targets"] = scenes.SolidScene.default()                                    # its acc and depth along each training ray
    else:
        teacher = NeRF(8, 256, 63, 27).to(dev)
        teacher.load_state_dict({k: torch.as_tensor(v) for k, v in synthetic.make_state_dict(77, 8, 256).items()})
        with torch.no_grad():
            images = torch.stack([harness._render_pose(teacher, posenc, K, poses[i].to(dev), (H, W), opts)[0].reshape(H, W, 3) for i in range(a.views + 2)], 0)
    if geometry is not None:
        opts.geometry = geometry
    i_train, i_test = list(range(a.views)), [a.views, a.views + 1]

    model = NeRF(8, a.net_width, 63, 27, skips=[4]).to(dev)                                      # main.py:67-73
    if a.fused_adam:
        from nerf_pytorch_paeng_amd.optim import FusedAdam
        optimizer = FusedAdam(model.parameters(), lr=5e-4, betas=(0.9, 0.999), skip_nonfinite=True)
    else:
        optimizer = torch.optim.Adam(model.parameters(), lr=5e-4, betas=(0.9, 0.999))            # main.py:79-80
    scheduler = None
    if a.lr_min is not None or a.warmup is not None:                                             # main.py:83-90
        from nerf_pytorch_paeng_amd.optim import CosineAnnealingWarmupRestarts
        scheduler = CosineAnnealingWarmupRestarts(optimizer, first_cycle_steps=a.steps + 1, max_lr=5e-4, min_lr=5e-5 if a.lr_min is None else a.lr_min,
                                                  warmup_steps=a.steps // 20 if a.warmup is None else a.warmup)
    criterion = torch.nn.MSELoss()
    getter = harness.global_batch(images, K, poses, i_train, (H, W), dev)                        # main.py:92-106
    t0 = time.perf_counter()
    for i in range(1, a.steps + 1):                                                              # main.py:136-139
        if occ_warmup is not None and i == occ_warmup + 1:                                       # the warm-up is over: bake, and train with the grid from here on
            from nerf_pytorch_paeng_amd import occupancy
            box, outside = (1.5, False) if a.scene == "solid" else (4.5, True)
            with torch.no_grad():
                opts.train_occupancy = occupancy.OccupancyGrid(-box, box, 128, outside_occupied=outside).bake(model, f16s=a.precision == "f16s")
            opts.occupancy_rebake_every = occ_every
            opts.occupancy_bake_args = {"f16s": a.precision == "f16s"}
            print(f"step {i:6d}  occupancy grid baked: {opts.train_occupancy.fraction():.4f} of the cells occupied", flush=True)
        out = harness.train(i, i_train, images, (K, poses.numpy()), (H, W), model, criterion, posenc, optimizer, getter, None, opts, log_dir=a.out)
        if scheduler is not None:
            scheduler.step()                                                                     # main.py:161
        if i % opts.idx_print == 0:
            torch.cuda.synchronize()
            print(f"step {i:6d}  loss {float(out['loss']):.5f}  psnr_f {float(out['psnr_f']):.2f} dB  {(time.perf_counter() - t0) / i * 1e3:.1f} ms/step", flush=True)
            if geometry is not None:
                print("             " + "  ".join(f"{k} {float(out[k]):.3e}" for k in ("loss_acc", "loss_depth", "loss_distortion") if k in out), flush=True)
            grid = getattr(opts, "train_occupancy", None)
            if grid is not None and grid.last_stats:
                from nerf_pytorch_paeng_amd import occupancy
                print(f"             evaluated share {occupancy.evaluated_share(grid.last_stats):.3f}, padded share {occupancy.padded_share(grid.last_stats):.3f}", flush=True)
    fresh = NeRF(8, a.net_width, 63, 27, skips=[4]).to(dev)                                      # test() loads the checkpoint train() saved (test.py:20-21)
    res = harness.test(a.steps, i_test, posenc, fresh, images[i_test], K, poses[i_test].to(dev), (H, W), opts, log_dir=a.out,
                       save_dir=os.path.join(a.out, "test_result"), ssim=True, lpips=lpips_model)   # main.py:140-149
    print(f"test: PSNR {['%.2f' % p for p in res['psnr']]} dB (mean {res['mean_psnr']:.2f}), SSIM {['%.4f' % v for v in res['ssim']]} "
          f"(mean {res['mean_ssim']:.4f}); PNGs and _result.txt in {a.out}/test_result")
    if lpips_model is not None:
        print(f"test: LPIPS {['%.4f' % v for v in res['lpips']]} (mean {res['mean_lpips']:.4f})")
    torch.cuda.synchronize()
    t_net = time.perf_counter()
    rgbs, disps = harness.render(a.steps, posenc, fresh, K, None, (H, W), opts, log_dir=a.out, save_dir=os.path.join(a.out, "render_result"))   # main.py:150-158
    t_net = time.perf_counter() - t_net
    print(f"render: {rgbs.shape[0]} frames {rgbs.shape[1]}x{rgbs.shape[2]} in {a.out}/render_result")
    if bake_res is not None:
        from nerf_pytorch_paeng_amd import baked
        t_bake = time.perf_counter()
        if bake_storage == "dense":
            grid = baked.RadianceGrid(-a.mesh_box, a.mesh_box, bake_levels[0][0] if bake_levels else bake_res, B=bake_B,
                                      signed=a.bake_signed is not None)                                                      # coarse to fine: the first level's lattice
        else:
            grid = baked.SparseRadianceGrid(-a.mesh_box, a.mesh_box, bake_res, B=bake_B, storage="f16" if bake_storage == "sparse16" else "fp32",
                                            signed=a.bake_signed is not None)
        grid = grid.bake(fresh, network="fine", precision=a.precision, clip=a.bake_signed or None)
        torch.cuda.synchronize()
        t_bake = time.perf_counter() - t_bake
        opts.baked = grid                                                                        # the same poses, from the grid alone
        t_grid = time.perf_counter()
        rgbs_g, _ = harness.render(a.steps, posenc, None, K, None, (H, W), opts, save_dir=os.path.join(a.out, "render_baked"))
        t_grid = time.perf_counter() - t_grid
        opts.baked = None
        mse = np.mean((rgbs_g.astype(np.float64) - rgbs.astype(np.float64)) ** 2, axis=(1, 2, 3)) / 255.0 ** 2
        print(f"bake: {grid.res[0]}^3 cells, B={bake_B}, {bake_storage}{', signed' if grid.signed else ''}, {grid.nbytes / 2 ** 20:.1f} MiB in {t_bake:.2f} s; {rgbs_g.shape[0]} frames from the grid in {t_grid * 1e3:.1f} ms "
              f"(the network: {t_net * 1e3:.1f} ms, PNG writing included in both); PSNR of the grid's frames against the network's "
              f"{['%.2f' % (-10.0 * np.log10(max(m, 1e-12))) for m in mse]} dB; {a.out}/render_baked")
        from nerf_pytorch_paeng_amd.rays import make_o_d

        def view_rays(idx):
            return torch.cat([torch.cat([x.reshape(-1, 3) for x in make_o_d(W, H, K, poses[i][:3, :4].to(dev))], -1) for i in idx]).float().contiguous()

        def grid_psnr():
            with torch.no_grad():
                rgb = grid.render(view_rays(i_test), want_all=False).reshape(len(i_test), -1)
            return [float(-10.0 * torch.log10(torch.mean((rgb[j] - images[i].to(dev).reshape(-1)) ** 2))) for j, i in enumerate(i_test)]

        def prune_seen(what):
            """Prune the dense grid by the training views; active points, record MiB and the held-out PSNR before and after."""
            n0, p0 = grid.compact().count, grid_psnr()
            grid.prune(0.0 if a.bake_prune is None else a.bake_prune, seen=grid.seen(train_views), T_vis=a.bake_prune_seen)
            n1 = grid.compact().count
            mib = 4 * grid.record_floats / 2 ** 20
            print(f"bake-prune-seen ({what}): T_vis {a.bake_prune_seen:g}, {len(train_views)} training views; active points {n0} -> {n1}, records "
                  f"{n0 * mib:.1f} -> {n1 * mib:.1f} MiB (fp32), {int(grid.skip.sum())} of {grid.skip.numel()} blocks of the skip plane occupied; the grid's "
                  f"PSNR on the test views {['%.2f' % p for p in p0]} -> {['%.2f' % p for p in grid_psnr()]} dB")

        train_views = baked.Views(H, W, K, poses[i_train]) if a.bake_prune_seen is not None else None
        if train_views is not None and not bake_levels:
            prune_seen("after the bake")
        if a.bake_finetune > 0:
            from nerf_pytorch_paeng_amd import baked_train

            if a.bake_optimizer == "lazy":                                                     # the direct path: steps only where a gradient arrived
                from nerf_pytorch_paeng_amd.optim import LazyAdam
                bake_reg = dict(bake_reg, optimizer=LazyAdam)
            before = grid_psnr()
            t_ft = time.perf_counter()
            if bake_levels or a.bake_prune is not None:
                levels = bake_levels + [(bake_res, a.bake_finetune)]
                grid, losses = baked_train.coarse_to_fine(grid, view_rays(i_train), images[i_train].to(dev).reshape(-1, 3).float(), levels, prune=a.bake_prune, prune_views=train_views,
                                                          prune_T=1e-3 if a.bake_prune_seen is None else a.bake_prune_seen, **bake_reg)
                print(f"bake-levels: {levels}, prune {a.bake_prune}{'' if train_views is None else ', by the training views at T_vis %g' % a.bake_prune_seen}; {int(grid.skip.sum())} of {grid.skip.numel()} blocks of the skip plane occupied at the end")
            else:
                losses = baked_train.finetune(grid, view_rays(i_train), images[i_train].to(dev).reshape(-1, 3).float(), a.bake_finetune, **bake_reg)
            torch.cuda.synchronize()
            t_ft = time.perf_counter() - t_ft
            if bake_reg:
                print(f"bake-reg: {bake_reg}; TV(sigma) {float(baked_train.lattice_tv(grid)):.4g}, TV(coef) {float(baked_train.lattice_tv(grid, 'coef')):.4g}, "
                      f"SP {float(baked_train.lattice_sparsity(grid)):.4g} after the steps")
            print(f"bake-finetune: {int(losses.numel())} steps{' over the levels ' + str(levels) if bake_levels or a.bake_prune is not None else ''} in {t_ft:.2f} s, batch loss {float(losses[0]):.5f} -> {float(losses[-1]):.5f}; the grid's PSNR on the test "
                  f"views {['%.2f' % p for p in before]} -> {['%.2f' % p for p in grid_psnr()]} dB")
        if bake_locate is not None:
            import math

            from nerf_pytorch_paeng_amd import baked_pose
            i = i_test[0]
            true = poses[i][:3, :4].to(dev).float()
            axis = torch.tensor([0.5, -0.7, 0.5], dtype=torch.float64)
            axis = axis / axis.norm() * math.radians(bake_locate[0])
            turn = torch.matrix_exp(torch.tensor([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]], dtype=torch.float64))
            start = true.clone()
            start[:, :3] = (turn @ true[:, :3].double().cpu()).float().to(dev)
            start[:, 3] += torch.tensor([0.6, -0.6, 0.53], device=dev) * (bake_locate[1] / math.sqrt(0.6 ** 2 + 0.6 ** 2 + 0.53 ** 2))
            target = images[i].to(dev).reshape(-1, 3).float()

            def errors(p):
                cos = float(((p[:, :3].double().T @ true[:, :3].double()).trace() - 1.0) / 2.0)
                with torch.no_grad():
                    rgb = grid.render(torch.cat([x.reshape(-1, 3) for x in make_o_d(W, H, K, p)], -1).float().contiguous(), want_all=False)
                return float(torch.mean((rgb - target) ** 2)), math.degrees(math.acos(max(-1.0, min(1.0, cos)))), float((p[:, 3] - true[:, 3]).norm())

            e0 = errors(start)
            t_loc = time.perf_counter()
            found, _ = baked_pose.locate(grid, H, W, K, start, target)
            torch.cuda.synchronize()
            t_loc = time.perf_counter() - t_loc
            e1 = errors(found)
            print(f"bake-locate: test view {i} turned by {bake_locate[0]:g} deg and moved by {bake_locate[1]:g}, 200 steps of 1024 pixels in {t_loc:.2f} s: image MSE "
                  f"{e0[0]:.3e} -> {e1[0]:.3e}, rotation error {e0[1]:.3f} -> {e1[1]:.3f} deg, translation error {e0[2]:.4f} -> {e1[2]:.4f}")
    if a.mesh:
        from nerf_pytorch_paeng_amd import mesh
        with torch.no_grad():
            field = mesh.density_lattice(fresh, -a.mesh_box, a.mesh_box, a.mesh_res, network="fine", precision=a.precision)
            m = mesh.extract(field, -a.mesh_box, a.mesh_box, a.mesh_iso).colorize(fresh, network="fine")
        os.makedirs(os.path.dirname(os.path.abspath(a.mesh)), exist_ok=True)
        m.save_ply(a.mesh)
        print(f"mesh: {m.verts.shape[0]} vertices, {m.tris.shape[0]} triangles at density {a.mesh_iso:g} on a {a.mesh_res}^3 lattice of +-{a.mesh_box:g}; "
              f"area {m.area():.3f}, enclosed volume {m.volume():.4f}; {a.mesh}")
        if a.mesh_view:
            opts.mesh_view = m                                                                   # the same poses, from the mesh alone
            t_view = time.perf_counter()
            rgbs_m, _ = harness.render(a.steps, posenc, None, K, None, (H, W), opts, save_dir=os.path.join(a.out, "render_mesh"))
            t_view = time.perf_counter() - t_view
            opts.mesh_view = None
            mse = np.mean((rgbs_m.astype(np.float64) - rgbs.astype(np.float64)) ** 2, axis=(1, 2, 3)) / 255.0 ** 2
            print(f"mesh view: {rgbs_m.shape[0]} frames from the mesh in {t_view * 1e3:.1f} ms (the network: {t_net * 1e3:.1f} ms, PNG writing included in both); "
                  f"PSNR of the mesh's frames against the network's {['%.2f' % (-10.0 * np.log10(max(v, 1e-12))) for v in mse]} dB; {a.out}/render_mesh")
    return res


if __name__ == "__main__":
    main()
