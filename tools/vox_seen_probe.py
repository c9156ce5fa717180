"""Pruning a radiance grid by visibility, measured: mi_vox_shadow, mi_vox_seen and mi_vox_prune_seen against their byte models, and what the
pruning buys on a baked scene -- one process, interleaved, as medians.

    python tools/vox_seen_probe.py [--reps 9] [--views 20] [--skip-training] [--steps 300] [--out profiles/r25_vox_seen.txt]

Kernels, on bakes of scenes.SolidScene.default() at 128^3 and 256^3 (B = 1: the three kernels read no record but prune's zeros) with one
view of 400 x 400 and of 800 x 800 from the training ring.  Device time by HIP events; every repetition runs every variant once; the
first pass warms up.
  shadow      against a device copy that moves the same bytes in the same repetition: the model is tvol written once, H W K 4 bytes (a copy of
              half of them: each byte read and written).  The sigma reads are left to the caches and are not in the model.
  seen        against its model: the od plane read and written once plus 4 bytes of tvol per lattice point the view looks at (counted).
  prune_seen  against mi_vox_prune on the same planes (B = 9 at 256^3, od_max = -log(1e-3)), both into sigma_out and zeros.
  20 views    RadianceGrid.seen end to end at 256^3 (shadow + seen per view, the fill of the plane included), beside one finetune step of
              the same grid (the thing a per-level prune competes with).
What it buys: the 256^3, B = 9 bake before and after prune(0, seen=seen(views), T_vis=1e-3) with the 20 training views of 400 x 400: active
points, compact("fp32" | "f16") MiB, occupied skip blocks, the median time of an 800 x 800 frame, and the PSNR of both held-out 800 x 800
views to scene.render -- each beside the un-pruned grid of the same process.
Training (unless --skip-training): 64 -> 128 -> 256 from nothing with a third of --steps per level, pruned per level by tau alone and by
tau and the views: wall seconds, held-out PSNR, occupied blocks.
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


def ring_pose(i, n):
    return np.asarray(synthetic.pose_spherical(360.0 * i / n + 7.0, -15.0 - 30.0 * (i % 3), 4.0), dtype=np.float32)


def frame_rays(H, W, K, pose, dev):
    o, d = make_o_d(W, H, K, torch.from_numpy(pose).to(dev)[:3, :4])
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--steps", type=int, default=300, help="total steps of each training schedule")
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--lr-sigma", type=float, default=0.5)
    ap.add_argument("--prune-alpha", type=float, default=0.01)
    ap.add_argument("--T-vis", type=float, default=1e-3)
    ap.add_argument("--skip-training", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "r25_vox_seen.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    scene = scenes.SolidScene.default()
    L = _vox.lib()
    lines = [f"visibility probe: scenes.SolidScene.default() on the box +-{BOX:g}; kernels: medians of {a.reps} interleaved repetitions after a warm-up, device time by "
             f"events; bias 2, step = half a cell edge"]

    def out(line):
        lines.append(line)
        print(line, flush=True)

    # ---- kernels -----------------------------------------------------------------------------------
    out("  res    view        K   tvol MB   copy us   copy GB/s   shadow us   copy/shadow   shadow+skip us | looked at   seen model MB   seen us   seen GB/s")
    for res in (128, 256):
        g = baked.bake_field(scene.field, -BOX, BOX, res, B=1, D=32, device=dev, shell="neighbours")
        cg = g.c_grid()
        for hw in (400, 800):
            cams = baked.Views(hw, hw, scenes.scaled_camera((hw, hw)), ring_pose(3, a.views)[None])
            v = g.view_slices(cams)[0]
            nbytes = int(L.mi_vox_shadow_bytes(C.byref(v)))
            tvol = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
            src, dst = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_(), torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
            od = torch.full(g.points, math.inf, dtype=torch.float32, device=dev)

            def shadow(skip):
                _vox.check(L.mi_vox_shadow(C.byref(cg), dev_ptr(g.sigma), dev_ptr(g.skip, "skip", torch.uint8, 1) if skip else None, C.byref(v),
                                           dev_ptr(tvol, "tvol", torch.float32, 32), stream_ptr(dev)), "mi_vox_shadow")

            def seen():
                _vox.check(L.mi_vox_seen(C.byref(cg), C.byref(v), dev_ptr(tvol, "tvol", torch.float32, 32), 2, dev_ptr(od), stream_ptr(dev)), "mi_vox_seen")

            t_copy, t_plain, t_skip, t_seen = timed([lambda: dst.copy_(src), lambda: shadow(False), lambda: shadow(True), seen], a.reps)
            looked = int(torch.isfinite(od).sum())
            model = 8 * od.numel() + 4 * looked
            out(f"  {res:3d}^3  {hw:3d} x {hw:3d}  {v.slices:4d}  {nbytes / 1e6:8.1f}  {t_copy:8.1f}  {nbytes / t_copy / 1e3:10.0f}  {t_plain:10.1f}  {t_copy / t_plain:12.3f}  "
                f"{t_skip:15.1f} | {looked:9d}  {model / 1e6:14.1f}  {t_seen:8.1f}  {model / t_seen / 1e3:10.0f}")
            del tvol, src, dst, od
            torch.cuda.empty_cache()
        del g
        torch.cuda.empty_cache()

    # ---- the 256^3, B = 9 bake ---------------------------------------------------------------------
    Kt, Ht, Wt = scenes.scaled_camera((400, 400)), 400, 400
    train_poses = np.stack([ring_pose(i, a.views) for i in range(a.views)])
    views = baked.Views(Ht, Wt, Kt, train_poses)
    K8, H8, W8 = synthetic.lego_camera()
    held_poses = [np.asarray(synthetic.pose_spherical(az, el, 4.0), dtype=np.float32) for az, el in ((30.0, -30.0), (200.0, -50.0))]
    held = [frame_rays(H8, W8, K8, p, dev) for p in held_poses]
    held_truth = [scene.render(r, 2.0, 6.0, want_all=False) for r in held]
    g = baked.bake_field(scene.field, -BOX, BOX, 256, B=9, D=32, device=dev, shell="neighbours")
    od_max = float(np.float32(-math.log(a.T_vis)))
    od = g.seen(views)
    cg = g.c_grid()
    kept, coef = torch.empty_like(g.sigma), g.coef.clone()

    def prune(with_od):
        if with_od:
            _vox.check(L.mi_vox_prune_seen(C.byref(cg), 9, 0.0, od_max, dev_ptr(g.sigma), dev_ptr(od), dev_ptr(kept), dev_ptr(coef, "coef", torch.float32, 16),
                                           stream_ptr(dev)), "mi_vox_prune_seen")
        else:
            _vox.check(L.mi_vox_prune(C.byref(cg), 9, 0.0, dev_ptr(g.sigma), dev_ptr(kept), dev_ptr(coef, "coef", torch.float32, 16), stream_ptr(dev)), "mi_vox_prune")

    t_plain, t_seen = timed([lambda: prune(False), lambda: prune(True)], a.reps)
    out(f"  prune 256^3 B=9, tau 0 (the kernel alone, records already cleared by the first pass): mi_vox_prune {t_plain:.1f} us, mi_vox_prune_seen (od_max {od_max:.3f}) "
        f"{t_seen:.1f} us, ratio {t_seen / t_plain:.3f}")
    del kept, coef
    buf = torch.empty_like(od)
    t_views, = timed([lambda: g.seen(views, out=buf)], a.reps)
    rays_b = torch.cat([frame_rays(Ht, Wt, Kt, p, dev) for p in train_poses[:4]]).contiguous()
    target_b = scene.render(rays_b, 2.0, 6.0, want_all=False)
    trial = baked.RadianceGrid(-BOX, BOX, 256, B=9).allocate(dev)
    trial.sigma.copy_(g.sigma), trial.coef.copy_(g.coef)
    trial.build_skip()
    baked_train.finetune(trial, rays_b, target_b, steps=3, batch=a.batch)                  # warm-up
    torch.cuda.synchronize()
    t = time.perf_counter()
    baked_train.finetune(trial, rays_b, target_b, steps=10, batch=a.batch)
    torch.cuda.synchronize()
    t_step = (time.perf_counter() - t) / 10
    del trial
    out(f"  RadianceGrid.seen, {a.views} views of {Ht} x {Wt} at 256^3, end to end: {t_views / 1e3:.2f} ms ({t_views / 1e3 / a.views:.2f} ms per view); one finetune step of "
        f"the same grid (torch.optim.Adam, batch {a.batch}, wall over 10 steps): {t_step * 1e3:.2f} ms")

    def report(name, grid):
        frame = timed([lambda: grid.render(held[0], want_all=False)], a.reps)[0]
        with torch.no_grad():
            p = [psnr(grid.render(r, want_all=False), t_) for r, t_ in zip(held, held_truth)]
        c32, c16 = grid.compact("fp32"), grid.compact("f16")
        out(f"  {name:22s} points with density {int((grid.sigma > 0).sum()):9d}, active {c32.count:9d} of {grid.sigma.numel()}, compact fp32 {c32.nbytes / 2 ** 20:7.1f} MiB, f16 "
            f"{c16.nbytes / 2 ** 20:7.1f} MiB, occupied blocks {int((grid.skip != 0).sum()):6d} of {grid.skip.numel()}, 800 x 800 frame {frame / 1e3:6.2f} ms, held-out PSNR "
            f"{p[0]:.3f} / {p[1]:.3f} dB")

    out(f"what it buys: 256^3, B = 9 bake; prune(0, seen=seen({a.views} views of {Ht} x {Wt}), T_vis={a.T_vis:g}), bias 2")
    report("baked", g)
    seen_share = float(torch.isfinite(od).float().mean())
    hidden = int(((g.sigma > 0) & ~(od <= od_max)).sum())
    g.prune(0.0, seen=od, T_vis=a.T_vis)
    report("pruned by the views", g)
    out(f"  some view looks at {100 * seen_share:.1f} % of the lattice points; {hidden} points with density were no seed (od > {od_max:.3f} or not looked at)")
    del g, od, buf
    torch.cuda.empty_cache()
    if a.skip_training:
        out("training schedules: not measured in this run (--skip-training)")
        return finish(lines, a.out)

    # ---- training ----------------------------------------------------------------------------------
    train = torch.cat([frame_rays(Ht, Wt, Kt, p, dev) for p in train_poses]).contiguous()
    target = scene.render(train, 2.0, 6.0, want_all=False)
    third = a.steps // 3
    levels = [(64, third), (128, third), (256, a.steps - 2 * third)]
    out(f"training from nothing, B = 9, batch {a.batch}, lr_sigma {a.lr_sigma:g}, {a.views} views of {Ht} x {Wt}, levels {levels}; tau = -ln(1 - {a.prune_alpha:g}) / cell edge "
        f"per level; held-out PSNR of two {H8} x {W8} views")

    def run(name, by_views):
        grid = baked.RadianceGrid(-BOX, BOX, levels[0][0], B=9).allocate(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, (res, steps) in enumerate(levels):
            tau = -math.log(1.0 - a.prune_alpha) / (2.0 * BOX / res)
            grid, _ = baked_train.coarse_to_fine(grid, train, target, [(res, steps)], prune=tau, batch=a.batch, lr_sigma=a.lr_sigma, skip=(i > 0),
                                                 prune_views=views if by_views else None, prune_T=a.T_vis)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        with torch.no_grad():
            p = [psnr(grid.render(r, want_all=False), t_) for r, t_ in zip(held, held_truth)]
        out(f"  {name:28s} {wall:6.2f} s, held-out PSNR {p[0]:.2f} / {p[1]:.2f} dB, occupied blocks {int((grid.skip != 0).sum())} of {grid.skip.numel()}, active points "
            f"{grid.compact().count}")

    warm = baked.RadianceGrid(-BOX, BOX, 64, B=9).allocate(dev)
    baked_train.coarse_to_fine(warm, train, target, [(64, 10), (128, 10)], prune=0.1, batch=a.batch, lr_sigma=a.lr_sigma, skip=(False, True), prune_views=views)
    del warm
    for name, by_views in (("pruned by tau", False), ("pruned by tau and the views", True), ("pruned by tau (again)", False), ("pruned by tau and the views (again)", True)):
        run(name, by_views)
    return finish(lines, a.out)


def finish(lines, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
