"""Training with an occupancy grid, measured: train scenes.SolidScene.default() as tools/occ_probe.py --scene solid does, bake a grid, then time
one training step (forward, loss, backward; no optimizer step, so every repetition sees the same weights) of 4096 rays x (64 + 128) samples
with and without the grid -- the two interleaved in one process, in fp32 and in f16s.

    python tools/occ_train_probe.py [--steps 1000] [--res 160] [--reps 20] [--rays 4096] [--out profiles/r12_occ_train.txt]

Reports the evaluated and the padded share of the samples, the step time both ways (host clock around work that ends in a device
synchronise; median and spread of ``--reps`` alternating repetitions after a warm-up of each shape) and the device time of the new kernels
over one step (torch.profiler, in a pass of its own; "not captured" if the profiler does not see them).  The design's expectation is

    step ~ full step x (evaluated + padded share) + the three small kernels + two host reads;

the report puts the measured ratio beside it.  Nothing here is asserted.
"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pytorch_paeng_amd import harness, scenes, train_path                                 # noqa: E402
from nerf_pytorch_paeng_amd import occupancy as OC                                             # noqa: E402
from nerf_pytorch_paeng_amd import occupancy_train as OT                                       # noqa: E402
from nerf_pytorch_paeng_amd.model import NeRF, get_positional_encoder                          # noqa: E402

NEW_KERNELS = ("occ_compact_count_kernel", "cscan_", "occ_compact_emit_kernel", "occ_scatter_kernel", "occ_gather_kernel")


def train_scene(dev, steps, size, views):
    H = W = size
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=64, N_samples_f=128, perturb=1.0, chunk_rays=4096, chunk_pts=524288, data_type="blender",
                           gpu_ids=[0], rank=0, exp_name="occ_train_probe", N_rays=1024, global_batch=True, idx_save=1 << 30, idx_print=1 << 30,
                           precision="fp32")
    images, poses, K = scenes.SolidScene.default().dataset(views, (H, W), radius=4.0, phi=-30.0, near=opts.near, far=opts.far, device=dev)
    posenc = get_positional_encoder(10), get_positional_encoder(4)
    model = NeRF(8, 256, 63, 27, skips=[4]).to(dev)
    optimizer = torch.optim.Adam(model.parameters(), lr=5e-4, betas=(0.9, 0.999))
    getter = harness.global_batch(images, K, poses, list(range(views)), (H, W), dev)
    for i in range(1, steps + 1):
        harness.train(i, list(range(views)), images, (K, poses.numpy()), (H, W), model, torch.nn.MSELoss(), posenc, optimizer, getter, None, opts)
    return model, opts, getter


def one_step(model, opts, rays, tgt, grid, f16s, seed):
    model.zero_grad(set_to_none=True)
    if grid is None:
        out = train_path.render_train(rays, model, opts, seed=seed, f16s=f16s)
    else:
        out = OT.render_train(rays, model, opts, grid, seed=seed, f16s=f16s)
    (torch.mean((out["rgb_c"] - tgt) ** 2) + torch.mean((out["rgb_f"] - tgt) ** 2)).backward()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_times(fn):
    """Device ms of the new kernels over one call of ``fn``; None if the profiler does not report them."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        tot = {k: 0.0 for k in NEW_KERNELS}
        for ev in prof.key_averages():
            for k in tot:
                if k in ev.key:
                    tot[k] += getattr(ev, "device_time_total", getattr(ev, "cuda_time_total", 0.0)) / 1e3
        return tot if any(v > 0 for v in tot.values()) else None
    except Exception as e:                                           # a tool: report, do not fail the measurement
        print(f"profiler: {e}", file=sys.stderr)
        return None


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--res", type=int, default=160)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--size", type=int, default=48, help="training image side")
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--out", default=os.path.join("profiles", "r12_occ_train.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    model, opts, getter = train_scene(dev, a.steps, a.size, a.views)
    i_batch, rays_rgb, _ = getter(a.rays)                            # a batch of the training set, as harness.train draws it
    batch = rays_rgb[i_batch - a.rays:i_batch]
    rays = torch.cat([batch[:, 0], batch[:, 1]], -1).contiguous()
    tgt = batch[:, 2].contiguous()
    lines = [f"occupancy training probe: scenes.SolidScene.default(), {a.views} views {a.size} x {a.size}, an 8 x 256 network after {a.steps} full fp32 training steps; "
             f"one step = forward + MSE(rgb_c) + MSE(rgb_f) + backward of {rays.shape[0]} rays x (64 + 128) samples, no optimizer step",
             f"times: host clock around a step that ends in a device synchronise, median [min .. max] of {a.reps} repetitions, full and grid step alternating"]
    grids = [("box +-1.5, outside skipped", OC.OccupancyGrid(-1.5, 1.5, a.res, outside_occupied=False)),
             ("box +-4.5 (holds every sample)", OC.OccupancyGrid(-4.5, 4.5, a.res))]
    for name, grid in grids:
        with torch.no_grad():
            grid.bake(model, sub=2, sigma_min=0.0, dilate=1)
        lines += ["", f"grid: {name}, res {a.res}^3, sub 2, sigma_min 0, dilate 1: occupied cells {grid.fraction():.4f}"]
        for f16s in (False, True):
            for g in (None, grid):                                   # warm up both shapes
                for _ in range(3):
                    one_step(model, opts, rays, tgt, g, f16s, 5)
            full, occ = [], []
            for rep in range(a.reps):
                full.append(timed(lambda: one_step(model, opts, rays, tgt, None, f16s, 100 + rep)))
                occ.append(timed(lambda: one_step(model, opts, rays, tgt, grid, f16s, 100 + rep)))
            s = grid.last_stats
            share, padded = OC.evaluated_share(s), OC.padded_share(s)
            kt = kernel_times(lambda: one_step(model, opts, rays, tgt, grid, f16s, 100))
            fm, om = float(np.median(full)), float(np.median(occ))
            small = sum(kt.values()) if kt else 0.0
            lines += [
                f"  {'f16s' if f16s else 'fp32'}: full step {fm:.2f} ms [{min(full):.2f} .. {max(full):.2f}]; grid step {om:.2f} ms [{min(occ):.2f} .. {max(occ):.2f}] "
                f"= {om / fm:.3f} x the full step",
                f"        samples: evaluated share {share:.4f} (coarse {s['evaluated_c'] / s['total_c']:.4f}, fine {s['evaluated_f'] / s['total_f']:.4f}), "
                f"padded share {padded:.4f}; evaluated + padded {share + padded:.4f}",
                "        new kernels over one step (two compactions, two scatters, two gathers): "
                + (", ".join(f"{k.rstrip('_')}* {v * 1e3:.1f} us" if k.endswith("_") else f"{k} {v * 1e3:.1f} us" for k, v in kt.items()) + f"; sum {small:.3f} ms"
                   if kt else "not captured"),
                f"        expectation full x (evaluated + padded share) + new kernels = {fm * (share + padded) + small:.2f} ms; "
                f"measured - expectation = {om - fm * (share + padded) - small:+.2f} ms (two host reads, launches of the smaller shapes, what the kernels lose on fewer points)",
            ]
            with open(a.out, "w") as fh:                               # after every row: a run cut short keeps what it measured
                fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
