"""Geometry losses, measured (docs/design/18_geometry_losses.md).  Three parts, each optional, each written to ``--out`` as soon as it is done:

    python tools/geo_probe.py [--kernels] [--step] [--arms] [--rays 4096] [--reps 20] [--steps 1500] [--size 48] [--out profiles/r13_geo.txt]

--kernels  device time of the compositing kernels at ``--rays`` rays x 192 samples: composite_bwd_kernel (libmi_nerf.so) against
           geo_composite_bwd_kernel with g_rgb alone and with all five gradients, composite_kernel against geo_composite_kernel; the five
           alternate inside one profiler session (torch.profiler; the kernels' template arguments tell the instantiations apart), and the
           bytes each must move are computed from the shapes.
--step     one training step (forward, loss, backward; no optimizer step) of ``--rays`` rays x (64 + 128) samples on an 8 x 256 network with
           geometry off and with all three terms, alternating, fp32 and f16s; host clock around work that ends in a device synchronise.
--arms     scenes.SolidScene.default() trained ``--steps`` steps twice from the same initial weights on the same ray batches, plain and with
           opts.geometry = {acc_weight 0.1, distortion_weight 0.01}: occupied fraction of the box +-1.5 at 160^3, evaluated share and time of
           an 800 x 800 frame with that grid against the full frame, PSNR against the analytic frame.
Nothing here is asserted.
"""
import argparse
import copy
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pytorch_paeng_amd import geometry as G                                               # noqa: E402
from nerf_pytorch_paeng_amd import harness, ops, scenes, synthetic, train_path, weights        # noqa: E402
from nerf_pytorch_paeng_amd import nerf_process as NP                                          # noqa: E402
from nerf_pytorch_paeng_amd import occupancy as OC                                             # noqa: E402
from nerf_pytorch_paeng_amd.model import NeRF, get_positional_encoder                          # noqa: E402
from nerf_pytorch_paeng_amd.rays import make_o_d                                               # noqa: E402

NEAR, FAR = 2.0, 6.0


def flush(path, lines):
    with open(path, "w") as fh:                                      # after every part: a run cut short keeps what it measured
        fh.write("\n".join(lines) + "\n")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return f"{float(np.median(v)):.2f} ms [{min(v):.2f} .. {max(v):.2f}]"


# ---------------------------------------------------------------------------------------------------
def kernels(a, dev, lines):
    n, S = a.rays, 192
    g = torch.Generator().manual_seed(0)
    raw = torch.randn(n, S, 4, generator=g)
    raw[..., 3] *= 3.0
    z = torch.sort(NEAR + (FAR - NEAR) * torch.rand(n, S, generator=g), -1).values
    rays = torch.randn(n, 6, generator=g)
    raw, z, rays = raw.to(dev), z.to(dev), rays.to(dev)
    gr = {k: torch.randn(*shape, generator=g).to(dev) for k, shape in (("rgb", (n, 3)), ("acc", (n,)), ("depth", (n,)), ("distortion", (n,)), ("weights", (n, S)))}
    five = {"g_" + k: v for k, v in gr.items()}
    C = (S + 63) // 64
    common_in = n * S * 4 * 4 + n * S * 4 + n * 6 * 4                # raw, z, rays
    variants = [
        ("composite_bwd_kernel (libmi_nerf.so)", f"composite_bwd_kernel<{C}>", lambda: ops.composite_backward(raw, z, rays, gr["rgb"]), common_in + n * 12 + n * S * 16),
        ("geo backward, g_rgb alone", f"geo_composite_bwd_kernel<{C}, 0>", lambda: G.composite_geo_backward(raw, z, rays, NEAR, FAR, g_rgb=gr["rgb"]),
         common_in + n * 12 + n * S * 16),
        ("geo backward, all five gradients", f"geo_composite_bwd_kernel<{C}, 2>", lambda: G.composite_geo_backward(raw, z, rays, NEAR, FAR, **five),
         common_in + n * 24 + n * S * 4 + n * S * 16),
        ("composite_kernel (libmi_nerf.so), all outputs", f"composite_kernel<{C}>", lambda: ops.composite(raw, z, rays, want_all=True), common_in + n * 24 + n * S * 4),
        ("geo forward, all outputs", f"geo_composite_kernel<{C}>", lambda: G.composite_geo(raw, z, rays, NEAR, FAR), common_in + n * 28 + n * S * 4),
    ]
    for _, _, fn, _ in variants:                                     # warm up every shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    lines += ["", f"kernels: {n} rays x {S} samples (C = {C}), device time per launch from torch.profiler, {a.reps} launches each, the five alternating in one session;",
              "bytes: what the launch must read and write, from the shapes (raw, z, rays, the gradients given, the outputs)"]
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(a.reps):
                for _, _, fn, _ in variants:
                    fn()
            torch.cuda.synchronize()
        seen = {ev.key: (getattr(ev, "device_time_total", getattr(ev, "cuda_time_total", 0.0)), ev.count) for ev in prof.key_averages()}
        for label, needle, _, nbytes in variants:
            hit = [(k, v) for k, v in seen.items() if needle.replace(" ", "") in k.replace(" ", "")]
            if len(hit) != 1:
                lines.append(f"  {label}: not captured ({len(hit)} profiler rows match {needle!r})")
                continue
            us = hit[0][1][0] / max(1, hit[0][1][1])
            lines.append(f"  {label}: {us:.2f} us over {hit[0][1][1]} launches; {nbytes / 1e6:.2f} MB -> {nbytes / us / 1e6:.2f} TB/s")
    except Exception as e:                                           # a tool: report, do not fail the measurement
        lines.append(f"  profiler: {e}")
    flush(a.out, lines)


# ---------------------------------------------------------------------------------------------------
def step(a, dev, lines):
    n = a.rays
    model = NeRF(8, 256, 63, 27, skips=[4]).to(dev)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in synthetic.make_state_dict(0, 8, 256).items()})
    opts = SimpleNamespace(near=NEAR, far=FAR, N_samples_c=64, N_samples_f=128, perturb=1.0)
    K, H, W = synthetic.lego_camera()
    pix = torch.from_numpy(synthetic.pixel_batch(H, W, n, 0)).to(dev)
    o, d = ops.make_o_d_pixels(W, H, K, synthetic.pose_spherical(0.0, -30.0, 4.0), pix)
    rays = torch.cat([o, d], -1).contiguous()
    g = torch.Generator().manual_seed(1)
    tgt, a_t, d_t = torch.rand(n, 3, generator=g).to(dev), torch.rand(n, generator=g).to(dev), (NEAR + (FAR - NEAR) * torch.rand(n, generator=g)).to(dev)

    def one(geometry, f16s, seed):
        model.zero_grad(set_to_none=True)
        out = train_path.render_train(rays, model, opts, seed=seed, f16s=f16s, geometry=geometry)
        loss = torch.mean((out["rgb_c"] - tgt) ** 2) + torch.mean((out["rgb_f"] - tgt) ** 2)
        if geometry:
            for k in ("c", "f"):
                loss = loss + 0.1 * torch.mean((out["acc_" + k] - a_t) ** 2) + 0.1 * torch.mean(a_t * (out["depth_" + k] - d_t) ** 2) \
                    + 0.01 * torch.mean(out["distortion_" + k])
        loss.backward()

    lines += ["", f"training step: {n} rays x (64 + 128) samples, 8 x 256 network, forward + loss + backward, no optimizer step; host clock around a step that ends "
              f"in a device synchronise, median [min .. max] of {a.reps} repetitions, geometry off and on alternating",
              "geometry on: mse(rgb) + 0.1 mse(acc) + 0.1 mean(acc* (depth - depth*)^2) + 0.01 mean(distortion), both networks"]
    for f16s in (False, True):
        for geometry in (False, True):
            for _ in range(3):
                one(geometry, f16s, 5)
        off, on = [], []
        for rep in range(a.reps):
            off.append(timed(lambda: one(False, f16s, 100 + rep)))
            on.append(timed(lambda: one(True, f16s, 100 + rep)))
        lines.append(f"  {'f16s' if f16s else 'fp32'}: geometry off {spread(off)}; geometry on {spread(on)} = {np.median(on) / np.median(off):.4f} x "
                     f"({np.median(on) - np.median(off):+.3f} ms)")
        flush(a.out, lines)


# ---------------------------------------------------------------------------------------------------
def frame(packed, opts, grid, reps, theta):
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
    return rgb, times[1:], torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1).contiguous()


def psnr(x, y) -> float:
    return float(-10.0 * torch.log10(torch.mean((x - y) ** 2).clamp_min(1e-20)))


def arms(a, dev, lines):
    H = W = a.size
    views, theta = 12, 45.0
    torch.manual_seed(0)
    opts = SimpleNamespace(near=NEAR, far=FAR, N_samples_c=64, N_samples_f=128, perturb=1.0, chunk_rays=4096, chunk_pts=524288, data_type="blender",
                           gpu_ids=[0], rank=0, exp_name="geo_probe", N_rays=1024, global_batch=True, idx_save=1 << 30, idx_print=1 << 30, precision="fp32")
    scene = scenes.SolidScene.default()
    images, poses, K = scene.dataset(views, (H, W), radius=4.0, phi=-30.0, near=NEAR, far=FAR, device=dev)
    posenc = get_positional_encoder(10), get_positional_encoder(4)
    first = NeRF(8, 256, 63, 27, skips=[4]).to(dev)
    init = copy.deepcopy(first.state_dict())
    getter0 = harness.global_batch(images, K, poses, list(range(views)), (H, W), dev)
    rng = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    lines += ["", f"two arms: scenes.SolidScene.default(), {views} views {H} x {W}, 8 x 256 network, {a.steps} fp32 steps each from the same initial weights on the same "
              f"ray batches; grid: box +-1.5, {a.res}^3, sub 2, sigma_min 0, dilate 1, outside skipped; 800 x 800 frame at azimuth {theta:g}, {a.reps} repetitions"]
    for name, geometry in (("plain", None), ("geometry acc 0.1, distortion 0.01", {"acc_weight": 0.1, "distortion_weight": 0.01, "targets": scene})):
        model = NeRF(8, 256, 63, 27, skips=[4]).to(dev)
        model.load_state_dict(init)
        optimizer = torch.optim.Adam(model.parameters(), lr=5e-4, betas=(0.9, 0.999))
        getter = copy.deepcopy(getter0)
        torch.set_rng_state(rng[0])
        torch.cuda.set_rng_state(rng[1], dev)
        NP.manual_seed(7)
        o = SimpleNamespace(**vars(opts), geometry=geometry)
        t_train = timed(lambda: [harness.train(i, list(range(views)), images, (K, poses.numpy()), (H, W), model, torch.nn.MSELoss(), posenc, optimizer, getter,
                                               None, o) for i in range(1, a.steps + 1)])
        model.eval()
        packed = weights.packed_for(model)
        with torch.no_grad():
            grid = OC.OccupancyGrid(-1.5, 1.5, a.res, outside_occupied=False).bake(packed, sub=2, sigma_min=0.0, dilate=1)
        full_rgb, full_ms, rays = frame(packed, opts, None, a.reps, theta)
        occ_rgb, occ_ms, _ = frame(packed, opts, grid, a.reps, theta)
        s = grid.last_stats
        gt_rgb, _, gt_acc, _ = scene.render(rays, NEAR, FAR)
        with torch.no_grad():
            acc = NP.render_rays(rays, packed, None, opts, seed=5, geometry=True)["acc_f"]
        lines += [f"  {name}: {t_train / a.steps:.2f} ms per training step; occupied cells {grid.fraction():.4f}; evaluated share {OC.evaluated_share(s):.4f}, padded share "
                  f"{OC.padded_share(s):.4f}",
                  f"      full frame {spread(full_ms)}; grid frame {spread(occ_ms)} = {np.median(occ_ms) / np.median(full_ms):.3f} x the full frame",
                  f"      PSNR vs the analytic frame: full {psnr(full_rgb, gt_rgb):.2f} dB, grid {psnr(occ_rgb, gt_rgb):.2f} dB; mean acc_f over the "
                  f"{int((gt_acc == 0).sum())} rays that meet nothing {float(acc[gt_acc == 0].mean()):.5f}"]
        flush(a.out, lines)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--arms", action="store_true")
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--size", type=int, default=48, help="training image side of --arms")
    ap.add_argument("--res", type=int, default=160, help="grid cells per axis of --arms")
    ap.add_argument("--out", default=os.path.join("profiles", "r13_geo.txt"))
    a = ap.parse_args(argv)
    if not (a.kernels or a.step or a.arms):
        a.kernels = a.step = a.arms = True
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    lines = [f"geometry probe ({torch.cuda.get_device_name(0)})"]
    if a.kernels:
        kernels(a, dev, lines)
    if a.step:
        step(a, dev, lines)
    if a.arms:
        arms(a, dev, lines)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
