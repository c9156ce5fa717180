"""Ray / pose gradients, measured (docs/design/19_pose_gradients.md).

    python tools/pose_probe.py [--rays 4096] [--reps 20] [--limit 120] [--out profiles/r14_pose.txt]

Two parts, each in a child process of its own under a time limit of its own (``--limit`` seconds); a part that fails, or runs out of time,
ends the probe: nothing further is started on the device.  Each part's lines go to ``--out`` as soon as it is done.

input_grad  device time (events on the launch stream) of ``pose.input_grad`` alone on the bench's batch, ``--rays`` rays x 64 samples (coarse)
            and x 192 (fine: 64 + 128 sorted) on an 8 x 256 network, against the bound from its delta reads alone: (2 W + W / 2) floats per point
            = 2.5 KB at W = 256.
step        one training step (forward, loss, backward; no optimizer step) of that batch with ``ray_grad`` off and on, alternating in one
            process; host clock around work that ends in a device synchronise.
Nothing here is asserted.
"""
import argparse
import os
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 6.3          # HBM rate an MI355X sustains on a streaming copy (8.0 TB/s is the specification); the bound is stated against it


def setup(n):
    import torch
    from nerf_pytorch_paeng_amd import ops, synthetic
    from nerf_pytorch_paeng_amd.model import NeRF
    dev = torch.device("cuda:0")
    model = NeRF(8, 256, 63, 27, skips=[4]).to(dev)
    sd = synthetic.make_state_dict(0, 8, 256)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    K, H, W = synthetic.lego_camera()
    pix = torch.from_numpy(synthetic.pixel_batch(H, W, n, 0)).to(dev)
    o, d = ops.make_o_d_pixels(W, H, K, synthetic.pose_spherical(0.0, -30.0, 4.0), pix)
    return dev, model, sd, torch.cat([o, d], -1).contiguous()


def spread(v):
    import numpy as np
    return f"{float(np.median(v)):.3f} ms [{min(v):.3f} .. {max(v):.3f}]"


def part_input_grad(a):
    import torch
    from nerf_pytorch_paeng_amd import ops, pose
    dev, _, sd, rays = setup(a.rays)
    net = ops.make_net(8, 256, 4, 10, 4)
    packed = ops.pack_module(sd, "model_fine.", net).to(dev)
    packed_bwd = ops.pack_module(sd, "model_fine.", net, backward=True).to(dev)
    flat = ops.flatten_params(sd, "model_fine.", net, dev)
    lines = [f"input_grad: {a.rays} rays, 8 x 256 network, device time per launch from events on the stream, {a.reps} launches each"]
    for S in (64, 192):
        g = torch.Generator().manual_seed(S)
        z = torch.sort(2.0 + 4.0 * torch.rand(a.rays, S, generator=g), -1).values.to(dev)
        raw, stash = ops.mlp_rays_train(net, packed, rays, z)
        d_raw = torch.randn(a.rays, S, 4, generator=g).to(dev) * 1e-3
        _, work = ops.mlp_backward(net, packed, packed_bwd, rays, z, d_raw, stash, stage=1)
        for _ in range(3):
            pose.input_grad(net, flat, rays, z, raw, d_raw, work)
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pose.input_grad(net, flat, rays, z, raw, d_raw, work)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        nbytes = a.rays * S * (2 * 256 + 128) * 4
        bound = nbytes / (HBM_TBS * 1e12) * 1e3
        med = sorted(ms)[len(ms) // 2]
        lines.append(f"  S = {S}: {spread(ms)}; delta reads {nbytes / 1e6:.0f} MB -> {nbytes / med / 1e9:.2f} TB/s; bound at {HBM_TBS:.1f} TB/s {bound:.3f} ms "
                     f"({med / bound:.1f} x the bound)")
    return lines


def part_step(a):
    import torch
    from nerf_pytorch_paeng_amd import train_path
    dev, model, _, rays = setup(a.rays)
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=64, N_samples_f=128, perturb=1.0)
    tgt = torch.rand(a.rays, 3, generator=torch.Generator().manual_seed(1)).to(dev)

    def one(ray_grad, seed):
        model.zero_grad(set_to_none=True)
        r = rays.clone().requires_grad_(ray_grad)
        out = train_path.render_train(r, model, opts, seed=seed, **({"ray_grad": True} if ray_grad else {}))
        (torch.mean((out["rgb_c"] - tgt) ** 2) + torch.mean((out["rgb_f"] - tgt) ** 2)).backward()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for w in range(3):
        one(False, w)
        one(True, w)
    off, on = [], []
    for i in range(a.reps):
        off.append(timed(lambda: one(False, 10 + i)))
        on.append(timed(lambda: one(True, 10 + i)))
    return [f"step: {a.rays} rays x (64 + 128) samples, 8 x 256, fp32, forward + loss + backward, host clock, {a.reps} steps each, alternating",
            f"  ray_grad off: {spread(off)}", f"  ray_grad on:  {spread(on)}"]


PARTS = {"input_grad": part_input_grad, "step": part_step}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_pose.txt"))
    ap.add_argument("--part", choices=sorted(PARTS))
    a = ap.parse_args()
    if a.part:                                                       # the child: one part, its lines on stdout
        print("\n".join(PARTS[a.part](a)))
        return 0
    lines = ["pose gradients (tools/pose_probe.py): " + " ".join(sys.argv[1:])]
    for name in ("input_grad", "step"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", name, "--rays", str(a.rays), "--reps", str(a.reps)],
                               capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{name}: not measured (no result within {a.limit} s); the probe ends here")
            break
        if r.returncode != 0:
            lines.append(f"{name}: not measured (exit status {r.returncode}); the probe ends here\n{r.stderr[-2000:]}")
            break
        lines.append(r.stdout.rstrip())
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
