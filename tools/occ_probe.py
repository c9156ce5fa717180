"""Occupancy-grid rendering, measured: train the synthetic scene of examples/train_eval_render.py, bake a grid, render one 800 x 800 frame with
and without it on the same build.

    python tools/occ_probe.py [--steps 1500] [--res 160] [--out profiles/r09_occupancy.txt]
    python tools/occ_probe.py --scene solid [--sigma-min 0 0.1 1 10] [--outside empty occupied] [--out profiles/r10_solid_scene.txt]

``--scene solid`` trains on scenes.SolidScene.default() (opaque solids in empty space, ground truth by mi_scene_render) instead of the views of a
random network, bakes with the box +-1.5 once per ``--sigma-min`` / ``--outside`` value, and adds the PSNR of the full and of the grid frame against
the analytic ground truth and the time of mi_scene_render for the 800 x 800 frame at S = 1024.

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
from nerf_pytorch_paeng_amd import scenes                                                      # noqa: E402
from nerf_pytorch_paeng_amd.model import NeRF, get_positional_encoder                          # noqa: E402
from nerf_pytorch_paeng_amd.rays import make_o_d                                               # noqa: E402


def train_scene(dev, steps, size=48, views=12, scene="teacher"):
    H = W = size
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=64, N_samples_f=128, perturb=1.0, chunk_rays=4096, chunk_pts=524288, data_type="blender",
                           gpu_ids=[0], rank=0, exp_name="occ_probe", N_rays=1024, global_batch=True, idx_save=1 << 30, idx_print=1 << 30, precision="fp32")
    K800, _, _ = synthetic.lego_camera()
    K = np.array([[K800[0][0] * W / 800.0, 0, W / 2], [0, K800[1][1] * H / 800.0, H / 2], [0, 0, 1]])
    posenc = get_positional_encoder(10), get_positional_encoder(4)
    poses = harness.get_render_pose(n_angle=views, phi=-30.0, nf=4.0)
    if scene == "solid":
        images, poses, K = scenes.SolidScene.default().dataset(views, (H, W), radius=4.0, phi=-30.0, near=opts.near, far=opts.far, device=dev)
    else:
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


def frame(packed, opts, grid, reps, theta=30.0):
    K, H, W = synthetic.lego_camera()
    pose = torch.from_numpy(np.asarray(synthetic.pose_spherical(theta, -30.0, 4.0), dtype=np.float32)).to(packed.device)
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


def stage_kernel_times(packed, opts, grid, theta=30.0):
    """Device ms of the cull and scatter kernels over one frame; None if the profiler does not report them."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            frame(packed, opts, grid, 0, theta)
        tot = {"occ_cull_kernel": 0.0, "occ_scatter_kernel": 0.0}
        for ev in prof.key_averages():
            for k in tot:
                if k in ev.key:
                    tot[k] += getattr(ev, "device_time_total", getattr(ev, "cuda_time_total", 0.0)) / 1e3
        return tot if all(v > 0 for v in tot.values()) else None
    except Exception as e:                                           # a tool: report, do not fail the measurement
        print(f"profiler: {e}", file=sys.stderr)
        return None


def psnr(a, b) -> float:
    return float(-10.0 * torch.log10(torch.mean((a - b) ** 2).clamp_min(1e-20)))


def ground_truth(dev, opts, theta, reps):
    """The analytic frame (mi_scene_render, 800 x 800, S = 1024) and its device time in ms (median of ``reps`` launches after a warm-up)."""
    K, H, W = synthetic.lego_camera()
    pose = torch.from_numpy(np.asarray(synthetic.pose_spherical(theta, -30.0, 4.0), dtype=np.float32)).to(dev)
    o, d = make_o_d(W, H, K, pose[:3, :4])
    rays = torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1).contiguous()
    scene = scenes.SolidScene.default()
    rgb = scene.render(rays, opts.near, opts.far, 1024, want_all=False)
    times = []
    for _ in range(max(1, reps)):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        scene.render(rays, opts.near, opts.far, 1024, want_all=False)
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return rgb, float(np.median(times))


def main_solid(a):
    """--scene solid: one table per (outside, sigma_min), the full frame and the ground truth measured once."""
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    theta = 45.0                                                       # between two training azimuths (multiples of 30 degrees)
    packed, opts = train_scene(dev, a.steps, a.size, a.views, "solid")
    gt_rgb, gt_ms = ground_truth(dev, opts, theta, a.reps)
    full_rgb, full_ms = frame(packed, opts, None, a.reps, theta)
    lines = [
        f"occupancy probe: scenes.SolidScene.default(), {a.views} views {a.size} x {a.size}, {a.steps} training steps, fp32, 800 x 800 frame at azimuth {theta:g}, 64 + 128 samples",
        f"ground truth: mi_scene_render, 800 x 800 rays, S = 1024: {gt_ms:.3f} ms per frame (device time, for the record)",
        f"frame: full path (mi_nerf_render_rays) {full_ms:.1f} ms; PSNR against the ground truth {psnr(full_rgb, gt_rgb):.2f} dB",
    ]
    for outside in a.outside:
        for sigma_min in a.sigma_min:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            grid = OC.OccupancyGrid(-1.5, 1.5, a.res, outside_occupied=(outside == "occupied")).bake(packed, sub=2, sigma_min=sigma_min, dilate=1)
            occupied = grid.fraction()
            bake_ms = (time.perf_counter() - t0) * 1e3
            occ_rgb, occ_ms = frame(packed, opts, grid, a.reps, theta)
            s = grid.last_stats
            share, padded = OC.evaluated_share(s), OC.padded_share(s)
            kt = stage_kernel_times(packed, opts, grid, theta)
            expect = full_ms * (share + padded)
            lines += [
                "",
                f"grid: box +-1.5, res {a.res}^3, sub 2, sigma_min {sigma_min:g}, dilate 1, outside {outside}: occupied cells {occupied:.4f}; bake + count {bake_ms:.1f} ms",
                f"samples: evaluated share {share:.4f} (coarse {s['evaluated_c'] / s['total_c']:.4f}, fine {s['evaluated_f'] / s['total_f']:.4f}), padded share {padded:.4f}",
                f"frame with the grid {occ_ms:.1f} ms = {occ_ms / full_ms:.3f} x the full frame",
                f"expectation full x (evaluated + padded share) = {expect:.1f} ms; stage overhead and shortfall {occ_ms - expect:.1f} ms",
                "cull / scatter kernels over the frame: " + (f"{kt['occ_cull_kernel']:.2f} ms / {kt['occ_scatter_kernel']:.2f} ms" if kt else "not captured"),
                f"PSNR: grid vs full {psnr(full_rgb, occ_rgb):.2f} dB; grid vs ground truth {psnr(occ_rgb, gt_rgb):.2f} dB; full vs ground truth {psnr(full_rgb, gt_rgb):.2f} dB",
            ]
            text = "\n".join(lines) + "\n"
            with open(a.out, "w") as fh:                                # after every table: a run cut short keeps what it measured
                fh.write(text)
    print(text, end="")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--res", type=int, default=160)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="default: profiles/r09_occupancy.txt (teacher), profiles/r10_solid_scene.txt (solid)")
    ap.add_argument("--scene", default="teacher", choices=["teacher", "solid"])
    ap.add_argument("--sigma-min", type=float, nargs="+", default=None, help="solid: one table per value (default 0 0.1 1 10)")
    ap.add_argument("--outside", nargs="+", default=["empty"], choices=["empty", "occupied"], help="solid: samples outside the box +-1.5 are skipped / evaluated")
    ap.add_argument("--size", type=int, default=48, help="solid: training image side")
    ap.add_argument("--views", type=int, default=12, help="solid: training views")
    a = ap.parse_args(argv)
    if a.out is None:
        a.out = os.path.join("profiles", "r09_occupancy.txt" if a.scene == "teacher" else "r10_solid_scene.txt")
    if a.scene == "solid":
        a.sigma_min = [0.0, 0.1, 1.0, 10.0] if a.sigma_min is None else a.sigma_min
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        return main_solid(a)
    if a.sigma_min is not None:
        ap.error("--sigma-min goes with --scene solid")
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
