"""The lattice regularisers of a radiance grid, measured: the kernels against their byte model, and what the priors do to training -- one
process, interleaved, as medians.

    python tools/lattice_reg_probe.py [--res 128 256] [--reps 9] [--steps 300] [--weights TV_SIGMA TV_COEF SPARSITY] [--out profiles/r22_lattice_reg.txt]

The scene is scenes.SolidScene.default() baked on the box +-1.2 with shell="neighbours".  Kernels: per (res, B) the gradient-only call that
``baked_train.finetune`` makes (mi_geo_lattice_tv on the sigma plane and on the records, mi_geo_lattice_sparsity on the plane) and the
value + gradient call, with mask NULL and with the bake's skip plane; device time by HIP events, every repetition runs every variant once.
The byte model is 12 bytes per float of the array (v read once, d_v read and written once; the padding travels with its row), over the
points of the workgroups the mask leaves standing; a row is reported as that model at the copy rate over its time.  Beside them: one step
of ``finetune`` with all weights 0 (the step it was before the regularisers) at batch 32 768, same process.
Training: from nothing (``allocate()``, skip=False) and from the bake (the fine-tune of tools/voxgrad_probe.py), plain against regularised:
the PSNR to scene.render of two held-out 800 x 800 views, the time per step, TV(sigma) and SP of the result.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pytorch_paeng_amd import baked, baked_train, scenes, synthetic                      # noqa: E402
from nerf_pytorch_paeng_amd.rays import make_o_d                                               # noqa: E402

BOX = 1.2
COPY_RATE = 6.29e12             # measured copy rate of the chip, bytes per second (the microarchitecture guide's figure)


def frame_rays(H, W, K, az, el, dev, radius=4.0):
    pose = torch.from_numpy(np.asarray(synthetic.pose_spherical(az, el, radius), dtype=np.float32)).to(dev)
    o, d = make_o_d(W, H, K, pose[:3, :4])
    return torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1).contiguous()


def psnr(a, b):
    return float(-10.0 * torch.log10(torch.mean((a - b) ** 2)))


def standing_points(grid, mask, backward):
    """Points of the blocks a launch does not skip: a block stands when it or (for the gradient) a backward neighbour block is set."""
    P = grid.points
    if mask is None:
        return P[0] * P[1] * P[2]
    m = mask != 0
    if backward:
        s = m.clone()
        s[1:] |= m[:-1]
        s[:, 1:] |= m[:, :-1]
        s[:, :, 1:] |= m[:, :, :-1]
        m = s
    ext = [torch.full((n,), 8, device=mask.device) for n in m.shape]
    for a, e in enumerate(ext):
        e[-1] = P[a] - 8 * (m.shape[a] - 1)
    pts = ext[0][:, None, None] * ext[1][None, :, None] * ext[2][None, None, :]
    return int((pts * m).sum())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--weights", type=float, nargs=3, default=[0.01, 0.01, 0.01], metavar=("TV_SIGMA", "TV_COEF", "SPARSITY"))
    ap.add_argument("--lr-sigma-nothing", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join("profiles", "r22_lattice_reg.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    scene = scenes.SolidScene.default()
    K, H, W = synthetic.lego_camera()
    Kt, Ht, Wt = scenes.scaled_camera((400, 400)), 400, 400
    train = torch.cat([frame_rays(Ht, Wt, Kt, 360.0 * i / a.views + 7.0, -15.0 - 30.0 * (i % 3), dev) for i in range(a.views)]).contiguous()
    target = scene.render(train, 2.0, 6.0, want_all=False)
    held = [frame_rays(H, W, K, az, el, dev) for az, el in ((30.0, -30.0), (200.0, -50.0))]
    held_truth = [scene.render(r, 2.0, 6.0, want_all=False) for r in held]
    lines = [f"lattice-regulariser probe: scenes.SolidScene.default() baked on the box +-{BOX:g} (shell='neighbours'); medians of {a.reps} interleaved "
             f"repetitions after a warm-up, device time by events; byte model 12 B per float of the array over the points of the standing workgroups, "
             f"at the copy rate {COPY_RATE / 1e12:.2f} TB/s"]

    # ---- kernels -----------------------------------------------------------------------------------
    lines.append("  res   B  entry                     array        mask    standing points   model MB   model us   measured us   model / measured")
    for res in a.res:
        for B in (1, 9):
            g = baked.bake_field(scene.field, -BOX, BOX, res, B=B, D=32, device=dev, shell="neighbours")
            g.sigma.grad, g.coef.grad = torch.zeros_like(g.sigma), torch.zeros_like(g.coef)
            R = g.record_floats
            calls, points = [], {}
            for mname, m in (("NULL", None), ("skip", True)):
                mask = None if m is None else g.skip
                calls += [("tv gradient", "sigma", 1, mname, True, lambda m=m: baked_train._lattice(g, "tv", "sigma", 1e-8, m, 1e-6, None, False)),
                          ("tv gradient", "coef", R, mname, True, lambda m=m: baked_train._lattice(g, "tv", "coef", 1e-8, m, 1e-6, None, False)),
                          ("tv value + gradient", "coef", R, mname, True, lambda m=m: baked_train.lattice_tv(g, "coef", mask=m, scale=1e-6)),
                          ("tv value", "coef", R, mname, False, lambda m=m: baked_train.lattice_tv(g, "coef", mask=m)),
                          ("sparsity gradient", "sigma", 1, mname, False, lambda m=m: baked_train._lattice(g, "sparsity", "sigma", 0.0, m, 1e-6, None, False)),
                          ("sparsity value + gradient", "sigma", 1, mname, False, lambda m=m: baked_train.lattice_sparsity(g, mask=m, scale=1e-6))]
                points.update({(mname, back): standing_points(g, mask, back) for back in (False, True)})
            times = [[] for _ in calls]
            for rep in range(a.reps + 1):                             # the first pass warms up
                for i, c in enumerate(calls):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    c[5]()
                    e1.record()
                    e1.synchronize()
                    if rep:
                        times[i].append(e0.elapsed_time(e1) * 1e3)
            for c, t in zip(calls, times):
                pts = points[(c[3], c[4])]
                per_float = 4 if c[0] == "tv value" else 12
                model = pts * c[2] * per_float
                us = float(np.median(t))
                lines.append(f"  {res:3d}   {B}  {c[0]:25s} {c[1]:5s} R={c[2]:<2d}   {c[3]:4s}   {pts:15d}   {model / 1e6:8.1f}   {model / COPY_RATE * 1e6:8.1f}   {us:11.1f}   {model / COPY_RATE * 1e6 / us:8.3f}")
            # one step of finetune as it was (all weights 0), same process
            g.sigma.grad = g.coef.grad = None
            baked_train.finetune(g, train, target, 3, batch=a.batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            baked_train.finetune(g, train, target, 20, batch=a.batch)
            torch.cuda.synchronize()
            lines.append(f"  {res:3d}   {B}  one finetune step without regularisers, batch {a.batch} (optimiser included, wall over 20 steps): {(time.perf_counter() - t0) / 20 * 1e3:.2f} ms")
            del g, calls
            torch.cuda.empty_cache()

    # ---- training ----------------------------------------------------------------------------------
    tv_s, tv_c, sp = a.weights
    reg = dict(tv_sigma=tv_s, tv_coef=tv_c, sparsity=sp)
    lines.append(f"training, B = 9, batch {a.batch}, {a.steps} steps, {a.views} views of {Ht} x {Wt}; regularised: tv_sigma {tv_s:g}, tv_coef {tv_c:g}, sparsity {sp:g}; "
                 f"PSNR to scene.render of two held-out {H} x {W} views (azimuth 30 / 200)")
    for res in a.res:
        for start in ("nothing", "bake"):
            for name, kw in (("plain", {}), ("regularised", reg)):
                if start == "nothing":
                    g = baked.RadianceGrid(-BOX, BOX, res, B=9).allocate(dev)
                    extra = dict(skip=False, lr_sigma=a.lr_sigma_nothing)
                else:
                    g = baked.bake_field(scene.field, -BOX, BOX, res, B=9, D=32, device=dev, shell="neighbours")
                    extra = {}
                with torch.no_grad():
                    before = [psnr(g.render(r, want_all=False), t) for r, t in zip(held, held_truth)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                losses = baked_train.finetune(g, train, target, a.steps, batch=a.batch, **extra, **kw)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                with torch.no_grad():
                    after = [psnr(g.render(r, want_all=False), t) for r, t in zip(held, held_truth)]
                tenth = max(a.steps // 10, 1)
                lines.append(f"  res {res}^3 from {start:7s} {name:11s}: held-out PSNR {before[0]:.2f} / {before[1]:.2f} -> {after[0]:.2f} / {after[1]:.2f} dB; "
                             f"{1e3 * wall / max(a.steps, 1):.2f} ms per step; data loss first / last tenth {float(losses[:tenth].mean()):.5f} / {float(losses[-tenth:].mean()):.5f}; "
                             f"TV(sigma) {float(baked_train.lattice_tv(g)):.4g}, TV(coef) {float(baked_train.lattice_tv(g, 'coef')):.4g}, SP {float(baked_train.lattice_sparsity(g)):.4g}, "
                             f"occupied blocks {int((g.skip != 0).sum())} of {g.skip.numel()}")
                del g
                torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
