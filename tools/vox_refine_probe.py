"""Coarse-to-fine training of a radiance grid, measured: mi_vox_resample and mi_vox_prune against a byte model, and what training through
levels does against training at one resolution -- one process, interleaved, as medians.

    python tools/vox_refine_probe.py [--reps 9] [--steps 300] [--prune-alpha 0.01] [--skip-training] [--out profiles/r23_vox_refine.txt]

Kernels.  Resample 64^3 -> 128^3 and 128^3 -> 256^3 at B = 1 and 9 on the box +-1.2, the source a bake of scenes.SolidScene.default().
The byte model is the destination written once plus the source read once (sigma planes and records, padding included); beside every
resample the same repetition times a device copy that moves the same number of bytes (a copy of half of them: each byte read and
written), and a row reports copy time over resample time.  Prune at 256^3, B = 9, on the bake under a fog of density below 0.5: tau = 0
(every point is kept: the stencil's reads alone) and tau = 1 (the fog and its records go: what is not kept is written as zeros).
Device time by HIP events; every repetition runs every variant once; the first pass warms up.

Training, from nothing (``allocate()``), B = 9, batch 32 768, 20 views of 400 x 400, PSNR to scene.render of two held-out 800 x 800 views:
128^3 alone and 256^3 alone (``finetune`` as it was: the parent's path, measured here and not copied) against 32 -> 64 -> 128 and
64 -> 128 -> 256 with the same total number of steps, a third per level, and once more with the steps of each level chosen so that every level
takes a third of the wall time the single resolution took.  Each schedule runs without and with pruning; tau per level is the density whose
opacity across one cell edge of that level is ``--prune-alpha``: tau = -ln(1 - alpha) / edge.  Levels are driven one at a time through
``baked_train.coarse_to_fine`` so that each can be timed (the probe synchronises between levels; the library does not).  A short untimed
schedule runs first, so that no timed run pays for the process's first launches.
"""
import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pytorch_paeng_amd import _vox, baked, baked_train, scenes, synthetic                # noqa: E402
from nerf_pytorch_paeng_amd._lib import dev_ptr, stream_ptr                                    # noqa: E402
from nerf_pytorch_paeng_amd.rays import make_o_d                                               # noqa: E402

BOX = 1.2


def frame_rays(H, W, K, az, el, dev, radius=4.0):
    pose = torch.from_numpy(np.asarray(synthetic.pose_spherical(az, el, radius), dtype=np.float32)).to(dev)
    o, d = make_o_d(W, H, K, pose[:3, :4])
    return torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1).contiguous()


def psnr(a, b):
    return float(-10.0 * torch.log10(torch.mean((a - b) ** 2)))


def timed(calls, reps):
    """Median device time in us of each call, interleaved: every repetition runs every call once; the first pass warms up."""
    times = [[] for _ in calls]
    for rep in range(reps + 1):
        for i, c in enumerate(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c()
            e1.record()
            e1.synchronize()
            if rep:
                times[i].append(e0.elapsed_time(e1) * 1e3)
    return [float(np.median(t)) for t in times]


def grid_bytes(g):
    n = g.points[0] * g.points[1] * g.points[2]
    return 4 * n * (1 + g.record_floats)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=300, help="total steps of every schedule")
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--lr-sigma", type=float, default=0.5)
    ap.add_argument("--prune-alpha", type=float, default=0.01)
    ap.add_argument("--skip-training", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "r23_vox_refine.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    scene = scenes.SolidScene.default()
    lines = [f"coarse-to-fine probe: scenes.SolidScene.default() on the box +-{BOX:g}; kernels: medians of {a.reps} interleaved repetitions after a warm-up, "
             f"device time by events; byte model: destination written once + source read once, against a device copy moving the same bytes in the same repetition"]

    def out(line):
        lines.append(line)
        print(line, flush=True)

    # ---- resample ----------------------------------------------------------------------------------
    out("  resample        B   source MB   destination MB   model MB   copy us   copy GB/s   resample us   copy / resample")
    for B in (1, 9):
        for res in (64, 128):
            g = baked.bake_field(scene.field, -BOX, BOX, res, B=B, D=32, device=dev, shell="neighbours")
            fine = g.resample(2 * res)
            s_bytes, d_bytes = grid_bytes(g), grid_bytes(fine)
            gs, gd = g.c_grid(), fine.c_grid()
            half = (s_bytes + d_bytes) // 8                         # floats of a copy that reads and writes model / 2 bytes each
            a_buf, b_buf = torch.empty(half, dtype=torch.float32, device=dev).normal_(), torch.empty(half, dtype=torch.float32, device=dev)

            def resample():
                _vox.check(_vox.lib().mi_vox_resample(C.byref(gs), C.byref(gd), B, dev_ptr(g.sigma), dev_ptr(g.coef, "coef", torch.float32, 16), dev_ptr(fine.sigma),
                                                      dev_ptr(fine.coef, "coef", torch.float32, 16), stream_ptr(dev)), "mi_vox_resample")

            t_copy, t_res = timed([lambda: b_buf.copy_(a_buf), resample], a.reps)
            model = s_bytes + d_bytes
            out(f"  {res:3d}^3 -> {2 * res:3d}^3   {B}   {s_bytes / 1e6:9.1f}   {d_bytes / 1e6:14.1f}   {model / 1e6:8.1f}   {t_copy:7.1f}   {model / t_copy / 1e3:9.0f}   "
                f"{t_res:11.1f}   {t_copy / t_res:8.3f}")
            del g, fine, a_buf, b_buf
            torch.cuda.empty_cache()

    # ---- prune -------------------------------------------------------------------------------------
    g = baked.bake_field(scene.field, -BOX, BOX, 256, B=9, D=32, device=dev, shell="neighbours")
    g.sigma.add_(torch.rand(g.sigma.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 0.5)       # a fog below 0.5 everywhere
    g.coef[..., :27].normal_(generator=torch.Generator(device=dev).manual_seed(2))
    sigma_in = g.sigma.clone()
    n = sigma_in.numel()
    # counted as integers: a float32 sum cannot hold 257^3
    kept = {tau: int((torch.nn.functional.max_pool3d((sigma_in > tau).float()[None, None], 3, stride=1, padding=1) > 0).sum()) for tau in (0.0, 1.0)}

    def prune(tau):
        g.sigma = sigma_in                                           # the same input every time; the records a call cleared stay cleared: the next call clears them again
        g.prune(tau)

    out("  prune 256^3 B=9 (sigma_out and the skip plane included, as RadianceGrid.prune runs it)   tau   kept points   of   zeros written MB   us")
    t0, t1 = timed([lambda: prune(0.0), lambda: prune(1.0)], a.reps)
    for tau, t in ((0.0, t0), (1.0, t1)):
        out(f"                                                                                          {tau:3.1f}   {kept[tau]:11d}   {n}   {(n - kept[tau]) * 128 / 1e6:14.1f}   {t:8.1f}")
    del g, sigma_in
    torch.cuda.empty_cache()
    if a.skip_training:
        return finish(lines, a.out)

    # ---- training ----------------------------------------------------------------------------------
    K, H, W = synthetic.lego_camera()
    Kt, Ht, Wt = scenes.scaled_camera((400, 400)), 400, 400
    train = torch.cat([frame_rays(Ht, Wt, Kt, 360.0 * i / a.views + 7.0, -15.0 - 30.0 * (i % 3), dev) for i in range(a.views)]).contiguous()
    target = scene.render(train, 2.0, 6.0, want_all=False)
    held = [frame_rays(H, W, K, az, el, dev) for az, el in ((30.0, -30.0), (200.0, -50.0))]
    held_truth = [scene.render(r, 2.0, 6.0, want_all=False) for r in held]
    out(f"training from nothing, B = 9, batch {a.batch}, lr_sigma {a.lr_sigma:g}, {a.views} views of {Ht} x {Wt}; PSNR to scene.render of two held-out {H} x {W} views "
        f"(azimuth 30 / 200); prune: tau = -ln(1 - {a.prune_alpha:g}) / cell edge per level (the density whose opacity across one cell is {a.prune_alpha:g}); "
        f"skip=False on the first level, the plane from the second on")

    def run(name, levels, pruned):
        """One schedule, level by level; returns the wall time of each level."""
        g = baked.RadianceGrid(-BOX, BOX, levels[0][0], B=9).allocate(dev)
        walls = []
        for i, (res, steps) in enumerate(levels):
            tau = -math.log(1.0 - a.prune_alpha) / (2.0 * BOX / res) if pruned else None
            torch.cuda.synchronize()
            t = time.perf_counter()
            g, losses = baked_train.coarse_to_fine(g, train, target, [(res, steps)], prune=tau, batch=a.batch, lr_sigma=a.lr_sigma, skip=(i > 0))
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t)
            with torch.no_grad():
                p = [psnr(g.render(r, want_all=False), t_) for r, t_ in zip(held, held_truth)]
            out(f"  {name:34s} level {res:3d}^3, {steps:4d} steps: {1e3 * walls[-1] / max(steps, 1):6.2f} ms per step (resample and prune included), held-out PSNR {p[0]:.2f} / {p[1]:.2f} dB, "
                f"occupied blocks {int((g.skip != 0).sum())} of {g.skip.numel()}" + (f", tau {tau:.3f}" if pruned else "")
                + f", last-tenth loss {float(losses[-max(steps // 10, 1):].mean()):.5f}")
        out(f"  {name:34s} total {sum(walls):.2f} s")
        del g
        torch.cuda.empty_cache()
        return walls

    # a warm-up outside every timing: the first steps of a process pay for the allocator and the kernels' first launches
    warm = baked.RadianceGrid(-BOX, BOX, 64, B=9).allocate(dev)
    baked_train.coarse_to_fine(warm, train, target, [(64, 10), (128, 10)], prune=0.1, batch=a.batch, lr_sigma=a.lr_sigma, skip=(False, True))
    torch.cuda.synchronize()
    del warm
    torch.cuda.empty_cache()
    third = a.steps // 3
    for top in (128, 256):
        alone = [(top, a.steps)]
        c2f = [(top // 4, third), (top // 2, third), (top, a.steps - 2 * third)]
        w_alone = run(f"{top}^3 alone", alone, False)
        run(f"{top}^3 alone, pruned at the end", alone, True)
        w = run(f"{top // 4}->{top // 2}->{top}, equal steps", c2f, False)
        run(f"{top // 4}->{top // 2}->{top}, equal steps, pruned", c2f, True)
        # equal wall time: each level gets a third of the single resolution's time, at the rate just measured
        per = [wi / max(s, 1) for wi, (_, s) in zip(w, c2f)]
        timed_levels = [(r, max(int(w_alone[0] / 3.0 / p), 1)) for (r, _), p in zip(c2f, per)]
        run(f"{top // 4}->{top // 2}->{top}, equal time", timed_levels, False)
        run(f"{top // 4}->{top // 2}->{top}, equal time, pruned", timed_levels, True)
    return finish(lines, a.out)


def finish(lines, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
