"""The lazy optimiser of a radiance grid, measured: mi_optim_adam_step_lazy against a byte model and against the dense step, what one
``baked_train.finetune`` step costs under torch.optim.Adam, FusedAdam and LazyAdam, and the equal-time schedules of
docs/design/25_coarse_to_fine.md under Adam and LazyAdam -- one process, interleaved, as medians.

    python tools/lazy_adam_probe.py [--reps 9] [--steps 300] [--skip-kernel] [--skip-steps] [--skip-training] [--out profiles/r24_lazy_adam.txt]

The kernel alone.  The record array of a 256^3, B = 9 bake of scenes.SolidScene.default() (257^3 points x 32 floats) is the parameter; the
gradient is (a) what one real backward of 32 768 training rays adds into a zero array, (b) all zero, (c) all non-zero.  The byte model is
the gradient read once plus 7 x 4 bytes per float of a touched 16-byte piece (p, m, v read and written, the gradient's zero written:
``consume = 1``; 6 x 4 with ``consume = 0``); beside every case the same repetition times a device copy that moves the model's bytes (a copy
of half of them: each byte read and written) and mi_optim_adam_step on the same arrays.  Device time by HIP events; every repetition runs
every variant once; the first pass warms up.  Under ``consume = 1`` the gradient is restored before every call, outside the timing.

One step.  ``finetune`` at 128^3 and 256^3, B = 9, batch 32 768, from the bake and from nothing (``allocate()``, skip=False): per optimiser the
wall time of an 11-step call minus that of a 3-step call, over 8 (what a call pays once cancels), as medians of interleaved repetitions;
and the Adam path's step taken apart by events (render, zero_grad, backward node, optimiser, clamp) in a loop that restates it.

Training.  128^3 and 256^3 alone and the equal-time 3-level schedules, from nothing, as tools/vox_refine_probe.py runs them (the level's steps
from the Adam path's measured rates), each under Adam and under LazyAdam: wall time, held-out PSNR, occupied skip blocks.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nerf_pytorch_paeng_amd import _optim, baked, baked_train, scenes, synthetic              # noqa: E402
from nerf_pytorch_paeng_amd._lib import stream_ptr                                             # noqa: E402
from nerf_pytorch_paeng_amd.optim import FusedAdam, LazyAdam                                   # noqa: E402
from vox_refine_probe import BOX, finish, frame_rays, psnr                                     # noqa: E402


def timed(calls, reps):
    """Median device time in us of each (before, call), interleaved: every repetition runs every pair once, ``before`` outside the timing;
    the first pass warms up."""
    times = [[] for _ in calls]
    for rep in range(reps + 1):
        for i, (before, c) in enumerate(calls):
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c()
            e1.record()
            e1.synchronize()
            if rep:
                times[i].append(e0.elapsed_time(e1) * 1e3)
    return [float(np.median(t)) for t in times]


def fresh(src, res, dev):
    """A grid of its own with the values of ``src`` (None: an empty one)."""
    g = baked.RadianceGrid(-BOX, BOX, res, B=9).allocate(dev)
    if src is not None:
        g.sigma.copy_(src.sigma)
        g.coef.copy_(src.coef)
        g.build_skip()
    return g


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=300, help="total steps of every training schedule")
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--lr-sigma", type=float, default=0.5, help="from nothing; from the bake finetune's defaults are used")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-training", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "r24_lazy_adam.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    scene = scenes.SolidScene.default()
    lines = [f"lazy optimiser probe: scenes.SolidScene.default() on the box +-{BOX:g}, B = 9, batch {a.batch}; medians of {a.reps} interleaved repetitions "
             f"after a warm-up"]

    def out(line):
        lines.append(line)
        print(line, flush=True)
        finish(lines, a.out)                                         # the file is whole after every line

    K, H, W = synthetic.lego_camera()
    Kt, Ht, Wt = scenes.scaled_camera((400, 400)), 400, 400
    train = torch.cat([frame_rays(Ht, Wt, Kt, 360.0 * i / a.views + 7.0, -15.0 - 30.0 * (i % 3), dev) for i in range(a.views)]).contiguous()
    target = scene.render(train, 2.0, 6.0, want_all=False)
    bakes = {}

    def bake(res):
        if res not in bakes:
            bakes[res] = baked.bake_field(scene.field, -BOX, BOX, res, B=9, D=32, device=dev, shell="neighbours")
        return bakes[res]

    # ---- the kernel alone --------------------------------------------------------------------------
    if not a.skip_kernel:
        g0 = bake(256)
        p = g0.coef.detach().clone()
        N = p.numel()
        idx = torch.randint(train.shape[0], (a.batch,), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
        with torch.no_grad():
            r = train[idx]
            rgb = g0.render(r)[0]
            g_real = baked_train.backward(g0, r, ((rgb - target[idx]) * (2.0 / (3 * a.batch))).contiguous())[1]
        m, v, g = torch.zeros_like(p), torch.zeros_like(p), torch.empty_like(p)
        cfg = _optim.AdamCfg(size=C.sizeof(_optim.AdamCfg), decoupled=0, lr=5e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0)
        cfgs = (_optim.AdamCfg * 1)(cfg)
        one = lambda ctype, x: (ctype * 1)(x)                        # noqa: E731
        a_p, a_g, a_n, a_off, a_step = one(C.c_void_p, p.data_ptr()), one(C.c_void_p, g.data_ptr()), one(C.c_int64, N), one(C.c_int64, 0), one(C.c_int64, 10)
        L = _optim.lib()

        def lazy(consume):
            _optim.check(L.mi_optim_adam_step_lazy(1, a_p, a_g, a_n, a_off, a_step, m.data_ptr(), v.data_ptr(), N, cfgs, 1, None, None, consume, stream_ptr(dev)),
                         "mi_optim_adam_step_lazy")

        def plain():
            _optim.check(L.mi_optim_adam_step(1, a_p, a_g, a_n, a_off, a_step, m.data_ptr(), v.data_ptr(), N, cfgs, 1, None, stream_ptr(dev)), "mi_optim_adam_step")

        out(f"kernel alone: the records of a 256^3 bake, {tuple(p.shape)} = {N} floats = {4 * N / 1e6:.0f} MB per array; model = g read once + 7 x 4 bytes per float "
            f"of a touched 16-byte piece (6 x 4 with consume = 0); the copy moves the consume = 1 model's bytes")
        out("  gradient                 touched floats   touched pieces   touched chunks   model MB   copy us   copy GB/s   lazy consume=1 us   copy / lazy   "
            "lazy consume=0 us   mi_optim_adam_step us   dense / lazy")
        for name, src in (("one 32 768-ray backward", g_real), ("all zero", torch.zeros_like(p)), ("all non-zero", torch.full_like(p, 1e-3))):
            flat = src.view(-1)
            nz = int(flat.count_nonzero())
            pieces = int(flat.view(-1, 4).ne(0).any(1).sum())
            whole = N // _optim.CHUNK * _optim.CHUNK
            chunks = int(flat[:whole].view(-1, _optim.CHUNK).ne(0).any(1).sum()) + int(bool(flat[whole:].any()))
            n_chunks = -(-N // _optim.CHUNK)
            model = 4 * N + 7 * 16 * pieces
            half = model // 8
            a_buf, b_buf = torch.empty(half, dtype=torch.float32, device=dev).normal_(), torch.empty(half, dtype=torch.float32, device=dev)
            restore = lambda: g.copy_(src)                           # noqa: E731
            restore()
            t_copy, t_c1, t_c0, t_dense = timed([(None, lambda: b_buf.copy_(a_buf)), (restore, lambda: lazy(1)), (restore, lambda: lazy(0)), (restore, plain)], a.reps)
            out(f"  {name:24s} {nz / N:14.5f}   {pieces / (N // 4):14.5f}   {chunks / n_chunks:14.5f}   {model / 1e6:8.0f}   {t_copy:7.1f}   {model / t_copy / 1e3:9.0f}   "
                f"{t_c1:17.1f}   {t_copy / t_c1:11.3f}   {t_c0:17.1f}   {t_dense:21.1f}   {t_dense / t_c1:12.2f}")
            del a_buf, b_buf, src
            torch.cuda.empty_cache()
        del p, m, v, g, g_real
        torch.cuda.empty_cache()

    # ---- one finetune step -------------------------------------------------------------------------
    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    if not a.skip_steps:
        out("one finetune step, ms: wall of an 11-step call minus a 3-step call, over 8; Adam is the parent's path (torch.optim.Adam), FusedAdam the same path with "
            "the fused dense step, LazyAdam the direct path")
        out("  grid    start          Adam   FusedAdam   LazyAdam   Adam / LazyAdam")
        parts_rows = []
        for res in (128, 256):
            for start in ("the bake", "nothing"):
                src = bake(res) if start == "the bake" else None
                kw = dict(batch=a.batch) if src is not None else dict(batch=a.batch, lr_sigma=a.lr_sigma, skip=False)
                opts = (torch.optim.Adam, FusedAdam, LazyAdam)
                per = [[] for _ in opts]
                for rep in range(a.reps + 1):
                    for i, o in enumerate(opts):
                        t = []
                        for steps in (3, 11):
                            g = fresh(src, res, dev)
                            t.append(wall(lambda: baked_train.finetune(g, train, target, steps=steps, optimizer=o, **kw)))
                            del g
                        if rep:
                            per[i].append((t[1] - t[0]) / 8.0 * 1e3)
                ms = [float(np.median(x)) for x in per]
                out(f"  {res:3d}^3   {start:10s} {ms[0]:8.2f}   {ms[1]:9.2f}   {ms[2]:8.2f}   {ms[0] / ms[2]:15.2f}")
                # the Adam path taken apart: finetune's loop restated, an event between its parts
                g = fresh(src, res, dev)
                g.sigma.requires_grad_(True)
                g.coef.requires_grad_(True)
                opt = torch.optim.Adam([dict(params=[g.sigma], lr=kw.get("lr_sigma", 0.05)), dict(params=[g.coef], lr=0.005)])
                gen = torch.Generator(device=dev).manual_seed(0)
                names = ("build_skip + draw + render", "loss + zero_grad", "backward (node, zeros_like, accumulate)", "optimiser", "clamp_")
                rows = []
                for it in range(a.reps + 2):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
                    ev[0].record()
                    if src is not None:
                        g.build_skip()
                    idx = torch.randint(train.shape[0], (a.batch,), generator=gen, device=dev)
                    rgb = baked_train.render(g, train[idx], skip=src is not None)[0]
                    ev[1].record()
                    loss = torch.mean((rgb - target[idx]) ** 2)
                    opt.zero_grad(set_to_none=False)
                    ev[2].record()
                    loss.backward()
                    ev[3].record()
                    opt.step()
                    ev[4].record()
                    with torch.no_grad():
                        g.sigma.clamp_(min=0.0)
                    ev[5].record()
                    ev[5].synchronize()
                    if it >= 2:
                        rows.append([ev[k].elapsed_time(ev[k + 1]) for k in range(len(names))])
                med = np.median(np.asarray(rows), axis=0)
                parts_rows.append(f"  {res:3d}^3   {start:10s} " + "   ".join(f"{n} {x:.2f}" for n, x in zip(names, med)) + f"   sum {med.sum():.2f}")
                del g, opt
                torch.cuda.empty_cache()
        out("the Adam path's step taken apart, ms by events (the first step has no .grad yet: zero_grad starts at the second; two steps warm up):")
        for row in parts_rows:
            out(row)
    bakes.clear()
    torch.cuda.empty_cache()
    if a.skip_training:
        return

    # ---- training: docs/design/25_coarse_to_fine.md's schedules under both optimisers ---------------
    held = [frame_rays(H, W, K, az, el, dev) for az, el in ((30.0, -30.0), (200.0, -50.0))]
    held_truth = [scene.render(r, 2.0, 6.0, want_all=False) for r in held]
    out(f"training from nothing, {a.views} views of {Ht} x {Wt}, lr_sigma {a.lr_sigma:g}, no pruning; held-out PSNR to scene.render of two {H} x {W} views; "
        f"skip=False on the first level, the plane from the second on; the equal-time levels' steps come from the Adam path's measured rates, and both "
        f"optimisers run the same steps")

    def run(name, levels, optimizer):
        g = baked.RadianceGrid(-BOX, BOX, levels[0][0], B=9).allocate(dev)
        walls = []
        for i, (res, steps) in enumerate(levels):
            def level():
                nonlocal g
                g, _ = baked_train.coarse_to_fine(g, train, target, [(res, steps)], batch=a.batch, lr_sigma=a.lr_sigma, skip=(i > 0), optimizer=optimizer)
            walls.append(wall(level))
        with torch.no_grad():
            p = [psnr(g.render(r, want_all=False), t_) for r, t_ in zip(held, held_truth)]
        out(f"  {name:44s} " + " + ".join(f"{res}^3 x {steps} ({1e3 * w / max(steps, 1):.2f} ms/step)" for (res, steps), w in zip(levels, walls))
            + f": {sum(walls):.2f} s, held-out PSNR {p[0]:.2f} / {p[1]:.2f} dB, occupied blocks {int((g.skip != 0).sum())} of {g.skip.numel()}")
        del g
        torch.cuda.empty_cache()
        return walls

    for o in (torch.optim.Adam, LazyAdam):                           # a warm-up outside every timing
        warm = baked.RadianceGrid(-BOX, BOX, 64, B=9).allocate(dev)
        baked_train.coarse_to_fine(warm, train, target, [(64, 10), (128, 10)], batch=a.batch, lr_sigma=a.lr_sigma, skip=(False, True), optimizer=o)
        torch.cuda.synchronize()
        del warm
    torch.cuda.empty_cache()
    third = a.steps // 3
    for top in (128, 256):
        alone = [(top, a.steps)]
        c2f = [(top // 4, third), (top // 2, third), (top, a.steps - 2 * third)]
        w_alone = run(f"{top}^3 alone, Adam", alone, torch.optim.Adam)
        run(f"{top}^3 alone, LazyAdam", alone, LazyAdam)
        w = run(f"{top // 4}->{top // 2}->{top}, equal steps, Adam", c2f, torch.optim.Adam)
        run(f"{top // 4}->{top // 2}->{top}, equal steps, LazyAdam", c2f, LazyAdam)
        per = [wi / max(s, 1) for wi, (_, s) in zip(w, c2f)]
        timed_levels = [(r, max(int(w_alone[0] / 3.0 / p), 1)) for (r, _), p in zip(c2f, per)]
        run(f"{top // 4}->{top // 2}->{top}, equal time, Adam", timed_levels, torch.optim.Adam)
        run(f"{top // 4}->{top // 2}->{top}, equal time, LazyAdam", timed_levels, LazyAdam)


if __name__ == "__main__":
    main()
