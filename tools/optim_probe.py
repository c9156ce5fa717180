"""The optimiser step, measured (docs/design/20_optimizer.md).

    python tools/optim_probe.py [--reps 200] [--step-reps 30] [--out profiles/r15_optim.txt]

One process, four variants, each on a copy of its own of the two 8 x 256 networks (48 tensors, 1.19 M parameters):
torch.optim.Adam as it defaults (multi-tensor), torch.optim.Adam(fused=True), optim.FusedAdam plain, optim.FusedAdam guarded (clipping by
global norm and skipping non-finite steps).  The variants take turns inside every repetition, so a drift of the box hits all of them alike.

optimizer   ``opt.step()`` alone on fixed gradients: host clock around the call and a device synchronise (launch overhead is what is being
            measured, so the host's share belongs in the figure), and beside it the time the call itself takes to return (enqueue).
step        the whole training step -- zero_grad, forward, loss, backward, opt.step() -- at 512, 1024 and 4096 rays x (64 + 128) samples,
            host clock around work that ends in a device synchronise.
Nothing here is asserted.
"""
import argparse
import copy
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANTS = ("torch Adam (default)", "torch Adam (fused=True)", "FusedAdam plain", "FusedAdam guarded")


def make_optimizer(name, params):
    import torch
    from nerf_pytorch_paeng_amd.optim import FusedAdam
    if name == VARIANTS[0]:
        return torch.optim.Adam(params, lr=5e-4)
    if name == VARIANTS[1]:
        return torch.optim.Adam(params, lr=5e-4, fused=True)
    if name == VARIANTS[2]:
        return FusedAdam(params, lr=5e-4)
    return FusedAdam(params, lr=5e-4, max_grad_norm=1.0, skip_nonfinite=True)


def spread(v):
    import numpy as np
    return f"{float(np.median(v)) * 1e3:8.1f} us [{min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step-reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_optim.txt"))
    a = ap.parse_args()
    import torch
    from nerf_pytorch_paeng_amd import ops, synthetic, train_path
    from nerf_pytorch_paeng_amd.model import NeRF
    dev = torch.device("cuda:0")
    base = NeRF(8, 256, 63, 27, skips=[4]).to(dev)
    base.load_state_dict({k: torch.as_tensor(v) for k, v in synthetic.make_state_dict(0, 8, 256).items()})
    models = {name: copy.deepcopy(base) for name in VARIANTS}
    opts_ = {name: make_optimizer(name, list(models[name].parameters())) for name in VARIANTS}
    n_param = sum(p.numel() for p in base.parameters())
    lines = ["optimizer step (tools/optim_probe.py): " + " ".join(sys.argv[1:]),
             f"{len(list(base.parameters()))} tensors, {n_param} parameters; {torch.cuda.get_device_name(0)}; torch {torch.__version__}"]

    # ---- the optimiser alone -----------------------------------------------------------------------
    g = torch.Generator().manual_seed(0)
    for m in models.values():
        for p in m.parameters():
            p.grad = (torch.randn(p.shape, generator=g) * 1e-3).to(dev)
    for _ in range(10):
        for name in VARIANTS:
            opts_[name].step()
    torch.cuda.synchronize()
    wall, enq = {n: [] for n in VARIANTS}, {n: [] for n in VARIANTS}
    for _ in range(a.reps):
        for name in VARIANTS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            opts_[name].step()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            enq[name].append((t1 - t0) * 1e3)
            wall[name].append((t2 - t0) * 1e3)
    lines.append(f"optimizer: opt.step() alone, host clock, {a.reps} calls each, taking turns; median [min .. max]")
    for name in VARIANTS:
        lines.append(f"  {name:24s} call + synchronise {spread(wall[name])}   call returns after {spread(enq[name])}")
    nbytes = 28 * n_param
    lines.append(f"  (the update reads 16 and writes 12 bytes per parameter: {nbytes / 1e6:.1f} MB, {nbytes / 6.0e12 * 1e6:.1f} us at 6.0 TB/s)")

    # ---- the whole training step -------------------------------------------------------------------
    for m in models.values():                                        # the steps above moved the weights: every variant starts over from the same ones
        m.load_state_dict(base.state_dict())
    K, H, W = synthetic.lego_camera()
    topts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=64, N_samples_f=128, perturb=1.0)
    for n in (512, 1024, 4096):
        pix = torch.from_numpy(synthetic.pixel_batch(H, W, n, 0)).to(dev)
        o, d = ops.make_o_d_pixels(W, H, K, synthetic.pose_spherical(0.0, -30.0, 4.0), pix)
        rays = torch.cat([o, d], -1).contiguous()
        tgt = torch.rand(n, 3, generator=torch.Generator().manual_seed(1)).to(dev)

        def one(name, seed):
            opts_[name].zero_grad(set_to_none=True)
            out = train_path.render_train(rays, models[name], topts, seed=seed)
            (torch.mean((out["rgb_c"] - tgt) ** 2) + torch.mean((out["rgb_f"] - tgt) ** 2)).backward()
            opts_[name].step()
        for w in range(3):
            for name in VARIANTS:
                one(name, w)
        ms = {name: [] for name in VARIANTS}
        for i in range(a.step_reps):
            for name in VARIANTS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                one(name, 10 + i)
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3)
        lines.append(f"step: {n} rays x (64 + 128) samples, fp32, zero_grad + forward + loss + backward + opt.step(), host clock, {a.step_reps} steps each, taking turns")
        for name in VARIANTS:
            lines.append(f"  {name:24s} {spread(ms[name])}")
    skipped = int(opts_[VARIANTS[3]].skipped_steps)
    lines.append(f"guarded variant: {skipped} steps skipped, last gradient norm {float(opts_[VARIANTS[3]].last_grad_norm):.3e}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
