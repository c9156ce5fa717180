"""Occupancy-grid rendering, measured: train the synthetic scene of examples/train_eval_render.py, bake a grid, render one 800 x 800 frame with
and without it on the same build.

    python tools/occ_probe.py [--steps 1500] [--res 160] [--out profiles/r09_occupancy.txt]

Reports the occupied share of the cells, the evaluated and the padded share of the samples, the frame time with the grid next to the full
path's (nerf_process.batchify_rays_and_render_by_chunk both ways; the full path is mi_nerf_render_rays, unchanged), the PSNR between the
two frames, and the device time of the cull and scatter kernels (torch.profiler; "not captured" if the profiler does not see them).
The expectation is full time x evaluated share + the stage overhead; the report says where the frame falls short of it.
"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pytorch_paeng_amd import harness, synthetic, weights                                 # noqa: E402
from nerf_pytorch_paeng_amd import nerf_process as NP                                          # noqa: E402
from nerf_pytorch_paeng_amd import occupancy as OC                                             # noqa: E402
from nerf_pytorch_paeng_amd.model import NeRF, get_positional_encoder                          # noqa: E402
from nerf_pytorch_paeng_amd.rays import make_o_d                                               # noqa: E402


def train_scene(dev, steps, size=48, views=12):
    H = W = size
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=64, N_samples_f=128, perturb=1.0, chunk_rays=4096, chunk_pts=524288, data_type="blender",
                           gpu_ids=[0], rank=0, exp_name="occ_probe", N_rays=1024, global_batch=True, idx_save=1 << 30, idx_print=1 << 30, precision="fp32")
    K800, _, _ = synthetic.lego_camera()
    K = np.array([[K800[0][0] * W / 800.0, 0, W / 2], [0, K800[1][1] * H / 800.0, H / 2], [0, 0, 1]])
    posenc = get_positional_encoder(10), get_positional_encoder(4)
    poses = harness.get_render_pose(n_angle=views, phi=-30.0, nf=4.0)
    teacher = NeRF(8, 256, 63, 27).to(dev)
    teacher.load_state_dict({k: torch.as_tensor(v) for k, v in synthetic.make_state_dict(77, 8, 256).items()})
    with torch.no_grad():
        images = torch.stack([harness._render_pose(teacher, posenc, K, poses[i].to(dev), (H, W), opts)[0].reshape(H, W, 3) for i in range(views)], 0)
    model = NeRF(8, 256, 63, 27, skips=[4]).to(dev)
    optimizer = torch.optim.Adam(model.parameters(), lr=5e-4, betas=(0.9, 0.999))
    getter = harness.global_batch(images, K, poses, list(range(views)), (H, W), dev)
    for i in range(1, steps + 1):
        harness.train(i, list(range(views)), images, (K, poses.numpy()), (H, W), model, torch.nn.MSELoss(), posenc, optimizer, getter, None, opts)
    model.eval()
    return weights.packed_for(model), opts


def frame(packed, opts, grid, reps):
    K, H, W = synthetic.lego_camera()
    pose = torch.from_numpy(np.asarray(synthetic.pose_spherical(30.0, -30.0, 4.0), dtype=np.float32)).to(packed.device)
    o, d = make_o_d(W, H, K, pose[:3, :4])
    times, rgb = [], None
    with torch.no_grad():
        for _ in range(reps + 1):                                    # the first pass warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, rgb, _ = NP.batchify_rays_and_render_by_chunk(o, d, packed, None, H, W, K, opts, seed=5, occupancy=grid)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    return rgb, float(np.median(times[1:]))


def stage_kernel_times(packed, opts, grid):
    """Device ms of the cull and scatter kernels over one frame; None if the profiler does not report them."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            frame(packed, opts, grid, 0)
        tot = {"occ_cull_kernel": 0.0, "occ_scatter_kernel": 0.0}
        for ev in prof.key_averages():
            for k in tot:
                if k in ev.key:
                    tot[k] += getattr(ev, "device_time_total", getattr(ev, "cuda_time_total", 0.0)) / 1e3
        return tot if all(v > 0 for v in tot.values()) else None
    except Exception as e:                                           # a tool: report, do not fail the measurement
        print(f"profiler: {e}", file=sys.stderr)
        return None


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--res", type=int, default=160)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r09_occupancy.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    packed, opts = train_scene(dev, a.steps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    grid = OC.OccupancyGrid(-4.5, 4.5, a.res).bake(packed, sub=2, sigma_min=0.0, dilate=1)
    occupied = grid.fraction()
    bake_ms = (time.perf_counter() - t0) * 1e3
    full_rgb, full_ms = frame(packed, opts, None, a.reps)
    occ_rgb, occ_ms = frame(packed, opts, grid, a.reps)
    s = grid.last_stats
    share, padded = OC.evaluated_share(s), OC.padded_share(s)
    psnr = float(-10.0 * torch.log10(torch.mean((full_rgb - occ_rgb) ** 2).clamp_min(1e-20)))
    kt = stage_kernel_times(packed, opts, grid)
    expect = full_ms * (share + padded)
    lines = [
        f"occupancy probe: synthetic scene of examples/train_eval_render.py, {a.steps} training steps, fp32, 800 x 800 frame, 64 + 128 samples",
        f"grid: box +-4.5, res {a.res}^3, sub 2, sigma_min 0, dilate 1: occupied cells {occupied:.4f}; bake + count {bake_ms:.1f} ms",
        f"samples: evaluated share {share:.4f} (coarse {s['evaluated_c'] / s['total_c']:.4f}, fine {s['evaluated_f'] / s['total_f']:.4f}), padded share {padded:.4f}",
        f"frame: full path (mi_nerf_render_rays) {full_ms:.1f} ms; with the grid {occ_ms:.1f} ms = {occ_ms / full_ms:.3f} x",
        f"expectation full x (evaluated + padded share) = {expect:.1f} ms; stage overhead and shortfall {occ_ms - expect:.1f} ms "
        f"(two stream synchronisations per slab, cull, scatter, the staged composite / resample launches, slabs of {OC.MAX_RAYS_PER_LAUNCH} rays)",
        "cull / scatter kernels over the frame: " + (f"{kt['occ_cull_kernel']:.2f} ms / {kt['occ_scatter_kernel']:.2f} ms" if kt else "not captured"),
        f"frame with the grid vs the full frame: PSNR {psnr:.2f} dB",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
