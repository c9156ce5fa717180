"""The compact radiance grid, measured against the dense one: an 800 x 800 frame from the dense table (mi_vox_render), from the sparse
fp32 table and from the sparse f16 table (mi_vox_render_sparse), in one process, interleaved, as medians.

    python tools/vox_sparse_probe.py [--res 128 256] [--reps 7] [--out profiles/r18_vox_sparse.txt]

The scene is scenes.SolidScene.default() (box +-1.2, shell "field"): ``baked.bake_field(scene.field, ...)`` per resolution and per B in
(1, 9), then ``compact("fp32")`` and ``compact("f16")`` of that grid (tests/test_gpu_vox_sparse.py: a sparse bake gives the same arrays).
The frame is the lego camera at azimuth 30, elevation -30, radius 4, skipping on, T_min in (0, 1e-3).  Every repetition runs every variant
once (HIP events around the launch), so drift hits all alike; the first repetition warms up and is dropped.  The comparator of every
sparse time is the dense time of the same loop.  Per case: M / P, the table's bytes against the dense record array's, the frame time, and
the PSNR of the f16 frame to the fp32 frame.  Last, the increment of B = 9 over B = 1 per storage: the byte model of
docs/design/22_radiance_grid.md (record bytes dominate the B = 9 frame) expects the f16 increment near half the fp32 one.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pytorch_paeng_amd import baked, scenes, synthetic                                    # noqa: E402
from nerf_pytorch_paeng_amd.rays import make_o_d                                               # noqa: E402

BOX = 1.2
STORAGES = ("dense", "sparse fp32", "sparse f16")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "r18_vox_sparse.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    scene = scenes.SolidScene.default()
    K, H, W = synthetic.lego_camera()
    pose = torch.from_numpy(np.asarray(synthetic.pose_spherical(30.0, -30.0, 4.0), dtype=np.float32)).to(dev)
    o, d = make_o_d(W, H, K, pose[:3, :4])
    rays = torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1).contiguous()
    lines = [f"compact radiance-grid probe: scenes.SolidScene.default() baked on the box +-{BOX:g}, D = 32 directions, shell 'field'; frame {H} x {W}, azimuth 30, "
             f"elevation -30, radius 4; step = half a cell; skipping on; medians of {a.reps} interleaved repetitions after a warm-up"]

    grids = {}
    for res in a.res:
        for B in (1, 9):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dense = baked.bake_field(scene.field, -BOX, BOX, res, B=B, D=32, device=dev)
            torch.cuda.synchronize()
            t_dense = (time.perf_counter() - t0) * 1e3
            grids[(res, B)] = (dense, dense.compact("fp32"), dense.compact("f16"))
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            t0 = time.perf_counter()
            again = baked.bake_field(scene.field, -BOX, BOX, res, B=B, D=32, device=dev, storage="sparse16")
            torch.cuda.synchronize()
            t_sparse = (time.perf_counter() - t0) * 1e3
            peak = torch.cuda.max_memory_allocated(dev) - base
            s16 = grids[(res, B)][2]
            same = all(torch.equal(getattr(again, k).view(torch.uint8), getattr(s16, k).view(torch.uint8)) for k in ("sigma", "slot", "table", "skip"))
            del again
            P = dense.sigma.numel()
            coef_bytes = P * 4 * dense.record_floats
            lines.append(f"res {res}^3 B={B}: M / P = {s16.count} / {P} = {s16.count / P:.4f}; record bytes: dense {coef_bytes / 2 ** 20:9.1f} MiB, sparse fp32 "
                         f"{grids[(res, B)][1].table.numel() * 4 / 2 ** 20:8.1f} MiB, sparse f16 {s16.table.numel() * 2 / 2 ** 20:8.1f} MiB; whole grid: dense {dense.nbytes / 2 ** 20:9.1f} MiB, "
                         f"sparse fp32 {grids[(res, B)][1].nbytes / 2 ** 20:8.1f} MiB, sparse f16 {s16.nbytes / 2 ** 20:8.1f} MiB; one bake (not warmed, host clock): dense "
                         f"{t_dense:8.1f} ms, storage='sparse16' {t_sparse:8.1f} ms with a peak of {peak / 2 ** 20:8.1f} MiB above its start, "
                         f"{'equal to' if same else 'DIFFERENT FROM'} compact('f16')")

    variants = [(res, B, T_min, st) for res in a.res for B in (1, 9) for T_min in (0.0, 1e-3) for st in range(3)]
    times = {v: [] for v in variants}
    frames, seen = {}, {}
    with torch.no_grad():
        for rep in range(a.reps + 1):                                 # the first pass warms up
            for v in variants:
                res, B, T_min, st = v
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                rgb, _, _, _, vis = grids[(res, B)][st].render(rays, T_min=T_min, skip=True, visited=True)
                t1.record()
                t1.synchronize()
                if rep:
                    times[v].append(t0.elapsed_time(t1))
                else:
                    frames[v], seen[v] = rgb, int(vis.sum(dtype=torch.int64))
    lines.append("  res   B  T_min   storage        frame ms   x dense    visited      sparse fp32 = dense bit for bit   PSNR of the f16 frame to the fp32 frame")
    med = {v: float(np.median(times[v])) for v in variants}
    for v in variants:
        res, B, T_min, st = v
        dense_v = (res, B, T_min, 0)
        note = ""
        if st == 1:
            note = "yes" if torch.equal(frames[v].view(torch.int32), frames[dense_v].view(torch.int32)) and seen[v] == seen[dense_v] else "NO"
        psnr = ""
        if st == 2:
            mse = float(torch.mean((frames[v].double() - frames[dense_v].double()) ** 2))
            psnr = f"{-10.0 * np.log10(mse):8.2f} dB (max |diff| {float((frames[v] - frames[dense_v]).abs().max()):.2e})" if mse > 0 else "identical"
        lines.append(f"  {res:3d}   {B}  {T_min:5.0e}   {STORAGES[st]:12s} {med[v]:9.3f}   {med[v] / med[dense_v]:7.3f}   {seen[v]:11d}   {note:32s}   {psnr}")
    lines.append("the increment of B = 9 over B = 1 (frame ms), per storage:")
    for res in a.res:
        for T_min in (0.0, 1e-3):
            inc = [med[(res, 9, T_min, st)] - med[(res, 1, T_min, st)] for st in range(3)]
            lines.append(f"  res {res:3d}  T_min {T_min:5.0e}:  dense {inc[0]:7.3f}   sparse fp32 {inc[1]:7.3f}   sparse f16 {inc[2]:7.3f}   f16 / fp32 (sparse) {inc[2] / inc[1]:6.3f}   "
                         f"f16 / dense {inc[2] / inc[0]:6.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
