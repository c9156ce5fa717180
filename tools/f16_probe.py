"""BASELINE config #5's render modes side by side (one process, one box, interleaved rounds): fp32, bf16, f16s+bf16 (coarse network in split
precision), f16+bf16 (coarse network on the f16 kernel) and f16 (both networks on it) -- the whole render_rays step and its coarse / fine
MLP launches, at 512, 1024 and 4096 rays.
    python tools/f16_probe.py [rays ...]
Step time: hipEvent-bracketed (torch.cuda.Event on the launch stream) runs of 20 back-to-back render_rays calls; launches: mi_nerf_time_mlp_rays
(10 back-to-back, on the fine / coarse depths of one fp32 step).  Medians of 5 interleaved rounds; the spread (max / min - 1) beside them."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nerf_pytorch_paeng_amd import ops, synthetic, weights

dev = torch.device("cuda:0")
SC, NF = 64, 128
packed = weights.PackedNeRF.from_state_dict(synthetic.make_state_dict(0, 8, 256), dev)
K, H, W = synthetic.lego_camera()
pose = synthetic.pose_spherical(0.0, -30.0, 4.0)
bf, fs = packed.bf16(), packed.f16s()
# mode -> (render_cfg keywords, (coarse blob, fine blob), time_mlp_rays keywords of the coarse / fine network)
modes = {
    "fp32": (dict(), (packed.coarse, packed.fine), dict(), dict()),
    "bf16": (dict(bf16=True), bf, dict(bf16=True), dict(bf16=True)),
    "f16s+bf16": (dict(bf16=True, coarse_f16s=True), (fs[0], bf[1]), dict(f16s=True), dict(bf16=True)),
    "f16+bf16": (dict(bf16=True, coarse_f16=True), (fs[0], bf[1]), dict(f16=True), dict(bf16=True)),
    "f16": (dict(f16=True), fs, dict(f16=True), dict(f16=True)),
}


def step_ms(cfg, bc, bfine, rays, ws, out, reps=20):
    for _ in range(3):
        ops.render_rays(packed.net, bc, bfine, cfg, rays, None, None, workspace=ws, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ops.render_rays(packed.net, bc, bfine, cfg, rays, None, None, workspace=ws, out=out)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


for n in [int(a) for a in sys.argv[1:]] or [512, 1024, 4096]:
    pix = torch.from_numpy(synthetic.pixel_batch(H, W, n, 0)).to(dev)
    o, d = ops.make_o_d_pixels(W, H, K, pose, pix)
    rays = torch.cat([o, d], -1).contiguous()
    out = (torch.empty(n, 3, device=dev), torch.empty(n, device=dev), torch.empty(n, 3, device=dev), torch.empty(n, device=dev))
    cfg0 = ops.render_cfg(2.0, 6.0, SC, NF, False)
    ws = torch.empty(ops.workspace_layout(cfg0, n).total, dtype=torch.uint8, device=dev)
    ops.render_rays(packed.net, packed.coarse, packed.fine, cfg0, rays, None, None, workspace=ws, out=out)
    v = ops.workspace_views(cfg0, n, ws)
    z_c, z_f = v["z_c"].clone(), v["z_f"].clone()
    raw_c, raw_f = torch.empty(n, SC, 4, device=dev), torch.empty(n, SC + NF, 4, device=dev)
    res = {m: {"coarse": [], "fine": [], "step": []} for m in modes}
    for _ in range(5):
        for m, (kw, (bc, bfine), kc, kf) in modes.items():
            cfg = ops.render_cfg(2.0, 6.0, SC, NF, False, **kw)
            ops.time_mlp_rays(packed.net, bc, rays, z_c, raw_c, 2, **kc)
            res[m]["coarse"].append(ops.time_mlp_rays(packed.net, bc, rays, z_c, raw_c, 10, **kc))
            ops.time_mlp_rays(packed.net, bfine, rays, z_f, raw_f, 2, **kf)
            res[m]["fine"].append(ops.time_mlp_rays(packed.net, bfine, rays, z_f, raw_f, 10, **kf))
            res[m]["step"].append(step_ms(cfg, bc, bfine, rays, ws, out))
    med = {m: {k: float(np.median(res[m][k])) for k in ("coarse", "fine", "step")} for m in modes}
    for m in modes:
        c, f, st = med[m]["coarse"], med[m]["fine"], med[m]["step"]
        spread = max(res[m]["step"]) / min(res[m]["step"]) - 1
        print(f"{n:5d} rays  {m:9s}: coarse launch {c:8.4f} ms  fine launch {f:8.4f} ms  step {st:8.4f} ms (spread {100 * spread:4.1f} %) "
              f"= {n / st / 1e3:6.3f} M rays/s   step / bf16 step {st / med['bf16']['step']:5.3f}", flush=True)
