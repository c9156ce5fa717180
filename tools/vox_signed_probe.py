"""A signed radiance grid, measured (docs/design/29_signed_density.md): the signed renderer next to the unsigned one on the same grid, the
backward pass next to another build of it, and what the signed plane does to the quality of a baked and a fine-tuned grid -- one process,
interleaved, device time by HIP events, as medians.

    python tools/vox_signed_probe.py [--res 128 256] [--reps 7] [--steps 300] [--other-voxgrad LIB.so] [--out profiles/r29_vox_signed.txt]

The scene is scenes.SolidScene.default() baked on the box +-1.2 with shell="neighbours", as tools/voxgrad_probe.py bakes it.
Frame time: per (res, B = 1 / 9) the 800 x 800 frame of tools/vox_probe.py through mi_vox_render and mi_vox_render_signed on the SAME arrays
(a baked plane is >= 0: the outputs are equal bit for bit, which the probe checks), skip plane on, T_min = 0, rgb alone.  Every repetition
runs unsigned, signed, unsigned: the second unsigned run against the first is the spread of one kernel against itself.
Backward time: tools/voxgrad_probe.py's twelve cases (res x B x 4 096 / 65 536 random rays / the frame).  With --other-voxgrad the same
entry of another build of libmi_nerf_voxgrad.so (the parent commit's, say) is loaded beside this one and timed on the same arrays in the
same repetitions, this build twice, so that the ratio stands next to this build's own spread.
Quality: held-out PSNR (two 800 x 800 views) of the unsigned bake, of its to_signed(), and of each after --steps finetune steps at batch
32 768 on 20 training views of 400 x 400; for the signed grid a sweep of lr_sigma in units of the plane's amplitude (its largest |sigma|),
and how far the density moved: the number of lattice points whose sign of sigma changed, and the mean |change| of sigma where a ray reached.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pytorch_paeng_amd import _voxgrad, baked, baked_train, ops, scenes, synthetic      # noqa: E402
from nerf_pytorch_paeng_amd._lib import dev_ptr, stream_ptr                                  # noqa: E402
from nerf_pytorch_paeng_amd.rays import make_o_d                                               # noqa: E402

BOX = 1.2


def frame_rays(H, W, K, az, el, dev, radius=4.0):
    pose = torch.from_numpy(np.asarray(synthetic.pose_spherical(az, el, radius), dtype=np.float32)).to(dev)
    o, d = make_o_d(W, H, K, pose[:3, :4])
    return torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1).contiguous()


def psnr(a, b):
    return -10.0 * float(torch.log10(torch.mean((a - b) ** 2)))


def med(x):
    return float(np.median(x))


def spread(x):
    return (max(x) - min(x)) / med(x)


def as_signed(g):
    """A signed grid on the arrays of ``g`` (a plane that is >= 0), with a skip plane of its own from the signed builder."""
    s = baked.RadianceGrid(g.lo, g.hi, g.res, g.B, signed=True)
    s.sigma, s.coef, s.skip = g.sigma, g.coef, torch.empty_like(g.skip)
    return s.build_skip()


def other_backward(path):
    """mi_voxgrad_render_backward of another build of the library, with this build's argument types."""
    lib = C.CDLL(path)
    fn = lib.mi_voxgrad_render_backward
    fn.restype, fn.argtypes = _voxgrad.SIGNATURES["mi_voxgrad_render_backward"]
    return fn


def call_backward(fn, grid, rays, g_rgb, d_sigma, d_coef):
    dev = rays.device
    cfg = _voxgrad.RenderCfg(float(0.5 * grid.cell_edge()), 0.0, float("inf"), 0.0, (C.c_float * 3)(1.0, 1.0, 1.0), 1)
    g = _voxgrad.Grid((C.c_float * 3)(*grid.lo), (C.c_float * 3)(*grid.hi), (C.c_int32 * 3)(*grid.res))
    with ops._guard(dev):
        rc = fn(C.byref(g), grid.B, dev_ptr(grid.sigma, "sigma"), dev_ptr(grid.coef, "coef", torch.float32, 16), dev_ptr(grid.skip, "skip", torch.uint8, 1),
                dev_ptr(rays, "rays"), rays.shape[0], C.byref(cfg), dev_ptr(g_rgb, "g_rgb"), None, None, dev_ptr(d_sigma, "d_sigma"),
                dev_ptr(d_coef, "d_coef", torch.float32, 16), None, None, None, stream_ptr(dev))
    if rc:
        raise RuntimeError(f"mi_voxgrad_render_backward: status {rc}")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--rates", type=float, nargs="+", default=[0.0003, 0.001, 0.003, 0.01], help="lr_sigma of the signed runs, in units of the plane's amplitude")
    ap.add_argument("--other-voxgrad", default=None, metavar="LIB.so", help="another build of libmi_nerf_voxgrad.so to time beside this one")
    ap.add_argument("--out", default=os.path.join("profiles", "r29_vox_signed.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    scene = scenes.SolidScene.default()
    K, H, W = synthetic.lego_camera()
    frame = frame_rays(H, W, K, 30.0, -30.0, dev)
    n_frame = frame.shape[0]
    lines = [f"signed radiance-grid probe: scenes.SolidScene.default() baked on the box +-{BOX:g} (shell='neighbours'), frame {H} x {W}, azimuth 30, elevation -30, "
             f"radius 4; step = half a cell, skip plane on, T_min = 0; medians of {a.reps} interleaved repetitions after a warm-up; spread = (max - min) / median"]
    grids = {(res, B): baked.bake_field(scene.field, -BOX, BOX, res, B=B, D=32, device=dev, shell="neighbours") for res in a.res for B in (1, 9)}

    # ---- frame time: mi_vox_render_signed against mi_vox_render on the same arrays ---------------------------
    lines.append("frame time, ms:  res   B   unsigned   unsigned again   signed   signed / unsigned   unsigned again / unsigned   spread unsigned   spread signed   equal bits")
    with torch.no_grad():
        for (res, B), g in grids.items():
            s = as_signed(g)
            same = torch.equal(g.skip, s.skip) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(g.render(frame), s.render(frame)))
            t = {"u": [], "s": [], "v": []}
            for rep in range(a.reps + 1):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                ev[0].record()
                g.render(frame, want_all=False)
                ev[1].record()
                s.render(frame, want_all=False)
                ev[2].record()
                g.render(frame, want_all=False)
                ev[3].record()
                ev[3].synchronize()
                if rep:
                    for k, i in (("u", 0), ("s", 1), ("v", 2)):
                        t[k].append(ev[i].elapsed_time(ev[i + 1]))
            lines.append(f"                 {res:3d}   {B}   {med(t['u']):8.3f}   {med(t['v']):14.3f}   {med(t['s']):6.3f}   {med(t['s']) / med(t['u']):17.4f}   "
                         f"{med(t['v']) / med(t['u']):25.4f}   {spread(t['u']):15.4f}   {spread(t['s']):13.4f}   {same}")

    # ---- backward time: this build, this build again, and another build ---------------------------------------
    perm = torch.randperm(n_frame, generator=torch.Generator().manual_seed(0)).to(dev)
    sets = {"4096 random": frame[perm[:4096]].contiguous(), "65536 random": frame[perm[:65536]].contiguous(), f"{n_frame} frame": frame}
    truth = {k: scene.render(v, 2.0, 6.0, want_all=False) for k, v in sets.items()}
    mine = _voxgrad.lib().mi_voxgrad_render_backward
    other = other_backward(a.other_voxgrad) if a.other_voxgrad else None
    lines.append("backward time, ms (unsigned baked planes, the twelve cases of tools/voxgrad_probe.py)" + ("" if other else "; no other build given"))
    lines.append("  res   B  rays               this build   this build again   other build   this / other   again / this   spread this   spread other")
    with torch.no_grad():
        for (res, B), g in grids.items():
            d_sigma, d_coef = torch.zeros_like(g.sigma), torch.zeros_like(g.coef)
            for name, rays in sets.items():
                rgb = g.render(rays, want_all=False)
                up = (2.0 * (rgb - truth[name]) / rgb.shape[0]).contiguous()
                t = {"a": [], "b": [], "o": []}
                for rep in range(a.reps + 1):
                    order = [("a", mine), ("o", other), ("b", mine)] if other else [("a", mine), ("b", mine)]
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(order) + 1)]
                    ev[0].record()
                    for i, (_, fn) in enumerate(order):
                        call_backward(fn, g, rays, up, d_sigma, d_coef)
                        ev[i + 1].record()
                    ev[-1].synchronize()
                    if rep:
                        for i, (k, _) in enumerate(order):
                            t[k].append(ev[i].elapsed_time(ev[i + 1]))
                o_ms = f"{med(t['o']):11.3f}   {med(t['a']) / med(t['o']):12.4f}" if other else f"{'-':>11s}   {'-':>12s}"
                lines.append(f"  {res:3d}   {B}  {name:16s}  {med(t['a']):10.3f}   {med(t['b']):16.3f}   {o_ms}   {med(t['b']) / med(t['a']):12.4f}   {spread(t['a']):11.4f}   "
                             + (f"{spread(t['o']):12.4f}" if other else f"{'-':>12s}"))
            del d_sigma, d_coef

    # ---- quality ---------------------------------------------------------------------------------------------
    Kt, Ht, Wt = scenes.scaled_camera((400, 400)), 400, 400
    train = torch.cat([frame_rays(Ht, Wt, Kt, 360.0 * i / a.views + 7.0, -15.0 - 30.0 * (i % 3), dev) for i in range(a.views)]).contiguous()
    target = scene.render(train, 2.0, 6.0, want_all=False)
    held = [frame_rays(H, W, K, az, el, dev) for az, el in ((30.0, -30.0), (200.0, -50.0))]
    held_truth = [scene.render(r, 2.0, 6.0, want_all=False) for r in held]

    def quality(g):
        with torch.no_grad():
            return " / ".join(f"{psnr(g.render(r, want_all=False), t):.2f}" for r, t in zip(held, held_truth))

    lines.append(f"quality: B = 9; {a.views} training views of {Ht} x {Wt} ({train.shape[0]} rays), baked_train.finetune (Adam, lr_coef 0.005, skip plane rebuilt every step), "
                 f"batch {a.batch}, {a.steps} steps from the same bake; PSNR in dB to scene.render of two held-out {H} x {W} views (azimuth 30 / 200)")
    for res in a.res:
        g = grids.pop((res, 9))
        grids.pop((res, 1), None)
        torch.cuda.empty_cache()
        s = g.to_signed()
        amp = float(s.sigma.abs().max())
        lines.append(f"  res {res}^3: unsigned bake {quality(g)};  to_signed() of it {quality(s)};  amplitude (largest |sigma|) {amp:.1f}, "
                     f"{int((s.sigma < 0).sum())} negative points, {int((s.sigma > 0).sum())} positive")
        sigma0, coef0, signed0 = g.sigma.clone(), g.coef.clone(), s.sigma.clone()
        t0 = time.perf_counter()
        baked_train.finetune(g, train, target, a.steps, batch=a.batch)
        torch.cuda.synchronize()
        reached = g.sigma != sigma0
        lines.append(f"    unsigned, lr_sigma 0.05 (the default): {quality(g)};  {time.perf_counter() - t0:.2f} s;  sigma changed at {int(reached.sum())} points, mean |change| there "
                     f"{float((g.sigma - sigma0).abs()[reached].mean()) if bool(reached.any()) else 0.0:.4f}, {int(((g.sigma > 0) != (sigma0 > 0)).sum())} points opened or closed")
        del g, sigma0, reached
        for rate in [None] + list(a.rates):
            s.sigma.copy_(signed0)
            s.coef.copy_(coef0)
            lr = 0.05 if rate is None else rate * amp
            t0 = time.perf_counter()
            baked_train.finetune(s, train, target, a.steps, batch=a.batch, lr_sigma=lr)
            torch.cuda.synchronize()
            reached = s.sigma != signed0
            lines.append(f"    signed, lr_sigma {lr:.4g} ({'the default' if rate is None else '%g x amplitude' % rate}): {quality(s)};  {time.perf_counter() - t0:.2f} s;  sigma changed at "
                         f"{int(reached.sum())} points, mean |change| there {float((s.sigma - signed0).abs()[reached].mean()) if bool(reached.any()) else 0.0:.4f}, "
                         f"{int(((s.sigma > 0) != (signed0 > 0)).sum())} points opened or closed")
        del s, signed0, coef0
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
