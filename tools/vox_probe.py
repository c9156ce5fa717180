"""The radiance grid, measured: bake time, and an 800 x 800 frame marched through the grid next to the fp32 network's frame of the same
pose, in one process, interleaved, as medians.

    python tools/vox_probe.py [--res 128 256] [--reps 7] [--out profiles/r17_vox.txt]

The scene is scenes.SolidScene.default() (opaque solids in empty space, box +-1.2): ``baked.bake_field(scene.field, ...)`` per resolution
and per B in (1, 9) -- wall time around a device synchronise, median of ``--bake-reps``.  The frame is the lego camera at azimuth 30,
elevation -30, radius 4.  Per (res, B, skip, T_min) the device time of mi_vox_render (HIP events; every repetition runs every variant
once, so drift hits all alike), the `visited` total, and the byte model the design file reads the time against:
    requested bytes = visited x 8 x 4 (sigma)  +  hits x 8 x 4 R (records),   hits = samples with sigma_s > 0,
`hits` counted in numpy (fp32, the header's position rule) on every 8th pixel of every 8th row and scaled by 64 for T_min = 0; with
T_min > 0 a ray stops within a few samples of a solid's surface, so hits are bounded by visited and reported as such.  Next to these, the
fp32 network frame (nerf_process.batchify_rays_and_render_by_chunk on a synthetic 8 x 256 network: its time does not depend on the
weights), host clock around a synchronise, the same repetitions.
"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pytorch_paeng_amd import baked, scenes, synthetic, weights                           # noqa: E402
from nerf_pytorch_paeng_amd import nerf_process as NP                                          # noqa: E402
from nerf_pytorch_paeng_amd.rays import make_o_d                                               # noqa: E402

BOX = 1.2


def count_hits(grid, rays, step, near=0.0, far=np.inf):
    """(samples, hits) over rays [n,6] (numpy fp32) with T_min = 0: the header's slab, interval and cell rule in fp32; a hit is a sample
    whose eight corners hold some density where the sample's weight is positive."""
    f32 = np.float32
    sigma = grid.sigma.cpu().numpy()
    lo, hi = np.asarray(grid.lo, f32), np.asarray(grid.hi, f32)
    res = np.asarray(grid.res)
    inv = res.astype(f32) / (hi - lo)
    o, d = rays[:, :3], rays[:, 3:]
    with np.errstate(all="ignore"):
        L = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        ta, tb = (lo - o) / d, (hi - o) / d
        t0 = np.fmax(f32(near), np.where(d != 0, np.fmin(ta, tb), -np.inf).max(1)).astype(f32)
        t1 = np.fmin(f32(far), np.where(d != 0, np.fmax(ta, tb), np.inf).min(1)).astype(f32)
        live = (t1 > t0) & (((o >= lo) & (o <= hi)) | (d != 0)).all(1)
        dt = f32(step) / L
    samples = hits = 0
    for k in range(int(grid_max_steps(grid, step))):
        ak = t0 + f32(k) * dt
        live &= ak < t1
        r = np.nonzero(live)[0]
        if r.size == 0:
            break
        mk = f32(0.5) * (ak[r] + np.fmin(t0[r] + f32(k + 1) * dt[r], t1[r]))
        c, f = [], []
        for i in range(3):
            g = ((o[r, i] + mk * d[r, i]) - lo[i]) * inv[i]
            ci = np.clip(np.floor(g).astype(np.int64), 0, res[i] - 1)
            c.append(ci)
            f.append(np.clip(g - ci.astype(f32), 0, 1))
        s = np.zeros(r.size, f32)
        for e in range(8):
            ex, ey, ez = e & 1, (e >> 1) & 1, e >> 2
            w = (f[0] if ex else 1 - f[0]) * (f[1] if ey else 1 - f[1]) * (f[2] if ez else 1 - f[2])
            s += w * sigma[c[2] + ez, c[1] + ey, c[0] + ex]
        samples += r.size
        hits += int((s > 0).sum())
    return samples, hits


def grid_max_steps(grid, step):
    import ctypes as C
    from nerf_pytorch_paeng_amd import _vox
    return _vox.lib().mi_vox_max_steps(C.byref(grid.c_grid()), float(step))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bake-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r17_vox.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    scene = scenes.SolidScene.default()
    K, H, W = synthetic.lego_camera()
    pose = torch.from_numpy(np.asarray(synthetic.pose_spherical(30.0, -30.0, 4.0), dtype=np.float32)).to(dev)
    o, d = make_o_d(W, H, K, pose[:3, :4])
    rays = torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1).contiguous()
    n = rays.shape[0]
    truth = scene.render(rays, 2.0, 6.0, want_all=False)
    lines = [f"radiance-grid probe: scenes.SolidScene.default() baked on the box +-{BOX:g}, D = 32 directions; frame {H} x {W}, azimuth 30, elevation -30, radius 4; "
             f"step = half a cell; medians of {a.reps} interleaved repetitions after a warm-up (bake: {a.bake_reps})"]

    # ---- bake ------------------------------------------------------------------------------------
    grids, shell_psnr = {}, {}
    for res in a.res:
        for B in (1, 9):
            times = []
            for _ in range(a.bake_reps + 1):                          # the first pass warms up
                grids.pop((res, B), None)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                g = baked.bake_field(scene.field, -BOX, BOX, res, B=B, D=32, device=dev)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
                grids[(res, B)] = g
            filled = baked.bake_field(scene.field, -BOX, BOX, res, B=B, D=32, device=dev, shell="neighbours")
            shell_psnr[(res, B)] = float(-10.0 * torch.log10(torch.mean((filled.render(rays, want_all=False) - truth) ** 2)))
            del filled
            active = int((g.coef[..., :3].abs().sum(-1) > 0).sum())
            lines.append(f"bake res {res}^3 B={B}: {float(np.median(times[1:])):9.1f} ms   {g.nbytes / 2 ** 20:8.1f} MiB; sigma > 0 at {float((g.sigma > 0).float().mean()):.4f} of the "
                         f"points, {active} records written ({active / g.sigma.numel():.4f}), skip bytes set {float(g.skip.float().mean()):.4f}")

    # ---- frames ----------------------------------------------------------------------------------
    variants = [(res, B, skip, T_min) for res in a.res for B in (1, 9) for skip in (True, False) for T_min in (0.0, 1e-3)]
    sd = synthetic.make_state_dict(0, 8, 256)
    packed = weights.PackedNeRF.from_state_dict(sd, dev)
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=64, N_samples_f=128, perturb=1.0, chunk_rays=4096, chunk_pts=524288, data_type="blender", gpu_ids=[0],
                           rank=0, precision="fp32")
    times = {v: [] for v in variants}
    times["network"] = []
    seen, psnr = {}, {}
    with torch.no_grad():
        for rep in range(a.reps + 1):                                 # the first pass warms up
            for v in variants:
                res, B, skip, T_min = v
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                rgb, _, _, _, vis = grids[(res, B)].render(rays, T_min=T_min, skip=skip, visited=True)
                t1.record()
                t1.synchronize()
                if rep:
                    times[v].append(t0.elapsed_time(t1))
                else:
                    seen[v] = int(vis.sum(dtype=torch.int64))
                    psnr[v] = float(-10.0 * torch.log10(torch.mean((rgb - truth) ** 2)))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            NP.batchify_rays_and_render_by_chunk(o, d, packed, None, H, W, K, opts, seed=5)
            torch.cuda.synchronize()
            if rep:
                times["network"].append((time.perf_counter() - t0) * 1e3)
    net_ms = float(np.median(times["network"]))
    lines.append(f"network frame (fp32, 8 x 256, 64 + 128 samples, host clock around a synchronise): {net_ms:9.1f} ms")
    sub = rays.reshape(H, W, 6)[::8, ::8].reshape(-1, 6).cpu().numpy()
    hits = {}
    for res in a.res:
        g = grids[(res, 1)]
        s, h = count_hits(g, sub, 0.5 * g.cell_edge())
        hits[res] = (64 * s, 64 * h)
        lines.append(f"res {res}^3: every 8th pixel of every 8th row counted in numpy, x 64: {64 * s} samples, {64 * h} with sigma_s > 0 ({h / max(s, 1):.4f})")
    lines.append("PSNR to the truth of the same frame from a grid baked with shell='neighbours' (same time: the kernel reads the same table): "
                 + ", ".join(f"res {r}^3 B={B} {p:.3f} dB" for (r, B), p in sorted(shell_psnr.items())))
    lines.append("  res   B  skip  T_min    frame ms   x network   visited      per ray   PSNR to truth   requested MB (sigma + records)   GB/s of requests")
    for v in variants:
        res, B, skip, T_min = v
        ms = float(np.median(times[v]))
        R = grids[(res, B)].record_floats
        if T_min == 0.0:
            rec = hits[res][1] * 8 * 4 * R
            note = ""
        else:
            rec = min(seen[v], hits[res][1]) * 8 * 4 * R
            note = " (records: upper bound)"
        req = seen[v] * 32 + rec
        lines.append(f"  {res:3d}   {B}  {'on ' if skip else 'off'}   {T_min:5.0e}  {ms:9.3f}   {net_ms / ms:9.1f}   {seen[v]:11d}  {seen[v] / n:7.1f}   {psnr[v]:8.3f} dB     "
                     f"{seen[v] * 32 / 1e6:9.1f} + {rec / 1e6:9.1f}   {req / ms / 1e6:9.1f}{note}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
