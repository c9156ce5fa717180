"""Ray gradients of the radiance grid, measured (docs/design/28_grid_ray_gradients.md): one process, interleaved, as medians.

    python tools/vox_raygrad_probe.py [--res 128 256] [--reps 7] [--out profiles/r28_vox_raygrad.txt]

Entries: the cases of tools/voxgrad_probe.py (docs/design/23_radiance_grid_training.md, 23.7) -- scenes.SolidScene.default() baked on the
box +-1.2 with shell="neighbours", B = 1 and 9, 4 096 and 65 536 rays drawn at random from an 800 x 800 frame and the frame's 640 000 rays in
pixel order, skip plane on, T_min = 0, upstream gradients 2 (rgb - truth) / n.  Per case the device time (HIP events) of RadianceGrid.render
(mi_vox_render), of baked_train.backward into arrays that exist (mi_voxgrad_render_backward), of RadianceGrid.render_backward_rays
(mi_vox_render_backward_rays) and of the same on the grid's f16 compact form (mi_vox_render_sparse_backward_rays); every repetition runs
every variant once.
Steps: one pose step against a grid (pose.make_o_d on a pixel batch, baked_pose.render, the mean squared error, backward to the pose;
no optimiser step) beside one pose step of the network path (tools/pose_probe.py's: train_path.render_train with ray_grad on an 8 x 256
network, 64 + 128 samples), alternating, host clock around work that ends in a device synchronise.
Nothing here is asserted.
"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pytorch_paeng_amd import baked, baked_pose, baked_train, pose, scenes, synthetic     # noqa: E402
from nerf_pytorch_paeng_amd.rays import make_o_d                                               # noqa: E402

BOX = 1.2


def frame_rays(H, W, K, az, el, dev, radius=4.0):
    p = torch.from_numpy(np.asarray(synthetic.pose_spherical(az, el, radius), dtype=np.float32)).to(dev)
    o, d = make_o_d(W, H, K, p[:3, :4])
    return torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1).contiguous()


def med(v):
    return float(np.median(v))


def spread(v):
    return f"{med(v):.3f} ms [{min(v):.3f} .. {max(v):.3f}]"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "r28_vox_raygrad.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    scene = scenes.SolidScene.default()
    K, H, W = synthetic.lego_camera()
    frame = frame_rays(H, W, K, 30.0, -30.0, dev)
    n_frame = frame.shape[0]
    perm = torch.randperm(n_frame, generator=torch.Generator().manual_seed(0)).to(dev)
    sets = {"4096 random": frame[perm[:4096]].contiguous(), "65536 random": frame[perm[:65536]].contiguous(), f"{n_frame} frame": frame}
    truth = {k: scene.render(v, 2.0, 6.0, want_all=False) for k, v in sets.items()}
    lines = [f"radiance-grid ray-gradient probe: scenes.SolidScene.default() baked on the box +-{BOX:g} (shell='neighbours'), frame {H} x {W}, azimuth 30, "
             f"elevation -30, radius 4; step = half a cell, skip plane on, T_min = 0; medians of {a.reps} interleaved repetitions after a warm-up"]
    grids = {(res, B): baked.bake_field(scene.field, -BOX, BOX, res, B=B, D=32, device=dev, shell="neighbours") for res in a.res for B in (1, 9)}
    small = {k: g.compact("f16") for k, g in grids.items()}
    grads = {k: (torch.zeros_like(g.sigma), torch.zeros_like(g.coef)) for k, g in grids.items()}
    variants = [(res, B, s) for res in a.res for B in (1, 9) for s in sets]
    t = {v: {"f": [], "b": [], "r": [], "r16": []} for v in variants}
    ups = {}
    with torch.no_grad():
        for v in variants:
            res, B, s = v
            rgb = grids[(res, B)].render(sets[s], want_all=False)
            ups[v] = (2.0 * (rgb - truth[s]) / rgb.shape[0]).contiguous()
        for rep in range(a.reps + 1):                                 # the first pass warms up
            for v in variants:
                res, B, s = v
                g, g16 = grids[(res, B)], small[(res, B)]
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
                ev[0].record()
                g.render(sets[s], want_all=False)
                ev[1].record()
                baked_train.backward(g, sets[s], ups[v], None, None, *grads[(res, B)])
                ev[2].record()
                g.render_backward_rays(sets[s], ups[v])
                ev[3].record()
                g16.render_backward_rays(sets[s], ups[v])
                ev[4].record()
                ev[4].synchronize()
                if rep:
                    for i, k in enumerate(("f", "b", "r", "r16")):
                        t[v][k].append(ev[i].elapsed_time(ev[i + 1]))
    lines.append("  res   B  rays               render ms   parameter backward ms   ray backward ms   ray backward f16 compact ms   ray / render   ray / parameter")
    for v in variants:
        res, B, s = v
        f, b, r, r16 = (med(t[v][k]) for k in ("f", "b", "r", "r16"))
        lines.append(f"  {res:3d}   {B}  {s:16s}  {f:9.3f}   {b:12.3f}          {r:9.3f}         {r16:9.3f}                {r / f:9.2f}      {r / b:9.2f}")
    del grads, small

    # ---- one pose step against a grid beside one of the network path ----------------------------------------------
    from nerf_pytorch_paeng_amd import ops, train_path
    from nerf_pytorch_paeng_amd.model import NeRF
    grid = grids[(a.res[0], 9)]
    base = torch.from_numpy(np.asarray(synthetic.pose_spherical(30.0, -30.0, 4.0), dtype=np.float32)).to(dev)[:3, :4].contiguous()
    target = scene.render(frame, 2.0, 6.0, want_all=False)
    model = NeRF(8, 256, 63, 27, skips=[4]).to(dev)
    model.load_state_dict({k: torch.as_tensor(x) for k, x in synthetic.make_state_dict(0, 8, 256).items()})
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=64, N_samples_f=128, perturb=1.0)
    for n in (1024, 4096):
        pix = torch.from_numpy(synthetic.pixel_batch(H, W, n, 0)).to(dev)
        refiner = pose.CameraRefiner(1).to(dev)

        def grid_step():
            refiner.zero_grad(set_to_none=True)
            o, d = pose.make_o_d(W, H, K, refiner(0, base), pixels=pix)
            rgb = baked_pose.render(grid, torch.cat([o, d], -1))[0]
            torch.mean((rgb - target[pix]) ** 2).backward()

        def net_step(seed=0):
            refiner.zero_grad(set_to_none=True)
            model.zero_grad(set_to_none=True)
            o, d = pose.make_o_d(W, H, K, refiner(0, base), pixels=pix)
            out = train_path.render_train(torch.cat([o, d], -1), model, opts, seed=seed, ray_grad=True)
            (torch.mean((out["rgb_c"] - target[pix]) ** 2) + torch.mean((out["rgb_f"] - target[pix]) ** 2)).backward()

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        for _ in range(3):
            grid_step()
            net_step()
        tg, tn = [], []
        for _ in range(a.step_reps):
            tg.append(timed(grid_step))
            tn.append(timed(net_step))
        lines.append(f"pose step, {n} pixels of the frame, forward + loss + backward to the pose, no optimiser step, host clock, {a.step_reps} steps each, alternating:")
        lines.append(f"  against the {a.res[0]}^3 B=9 grid (baked_pose.render):                     {spread(tg)}")
        lines.append(f"  network path (8 x 256, 64 + 128 samples, fp32, render_train ray_grad): {spread(tn)}   ratio {med(tn) / med(tg):.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
