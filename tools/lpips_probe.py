"""The LPIPS engine, measured (docs/design/21_lpips.md).

    python tools/lpips_probe.py [--reps 12] [--torch] [--out profiles/r16_lpips.txt]

One process, seeded random VGG-16 weights, hipEvent medians after two warm-up rounds; the items take turns inside every repetition, so a
drift of the box hits all of them alike.

distance    mi_lpips_distance for one pair at 800 x 800 and at 378 x 504.
layers      at 800 x 800, one image: mi_lpips_features of the plan cut after convolution k (its pools kept), k = 1..13.  A layer's time is the
            difference of two neighbouring prefixes, so it includes the max-pool in front of it; its rate is 2 * 9 * cin * cout * H * W over
            that time, against the 157.3 TFLOP/s fp32-MFMA peak.
--torch     for context only: the same 13 layers as torch.nn.functional.conv2d calls (MIOpen, which may pick Winograd: not like for like).
Nothing here is asserted.
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHANNELS = [64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512]
POOL_AFTER = (2, 4, 7, 10)
TAP_AFTER = (2, 4, 7, 10, 13)
PEAK = 157.3e12


def plan_ops(n_conv, taps):
    ops = []
    for k in range(1, n_conv + 1):
        ops.append(("conv", CHANNELS[k - 1]))
        if k in taps:
            ops.append("tap")
        if k in POOL_AFTER and k < n_conv:
            ops.append("pool")
    return ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_lpips.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from nerf_pytorch_paeng_amd.perceptual import Lpips
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    conv_w, conv_b, c = [], [], 3
    for co in CHANNELS:
        conv_w.append(torch.randn(co, c, 3, 3, generator=g) * math.sqrt(2.0 / (9 * c)))
        conv_b.append(torch.randn(co, generator=g) * 0.1)
        c = co
    tap_w = [torch.rand(CHANNELS[k - 1], generator=g) for k in TAP_AFTER]
    ab = ([4.4, 4.5, 4.4], [-2.1, -2.0, -1.8])
    full = Lpips.from_arrays((3, plan_ops(13, TAP_AFTER)), conv_w, conv_b, tap_w, *ab, device=dev)
    prefixes = [Lpips.from_arrays((3, plan_ops(k, (k,))), conv_w[:k], conv_b[:k], [tap_w[0][:1].repeat(CHANNELS[k - 1])], *ab, device=dev)
                for k in range(1, 14)]
    full_b = Lpips(full.net, full.blob_host, dev)              # a second object: a scratch of its own for the second frame size
    imgs = {hw: (torch.rand(1, *hw, 3, generator=g).to(dev), torch.rand(1, *hw, 3, generator=g).to(dev)) for hw in ((800, 800), (378, 504))}
    items = {"distance 800x800": lambda: full(*imgs[(800, 800)]), "distance 378x504": lambda: full_b(*imgs[(378, 504)])}
    for k, m in enumerate(prefixes, 1):
        items[f"prefix {k}"] = (lambda m=m: m.features(imgs[(800, 800)][0], 0))
    if a.torch:
        wd, bd = [w.to(dev) for w in conv_w], [b.to(dev) for b in conv_b]
        x_nchw = imgs[(800, 800)][0].permute(0, 3, 1, 2).contiguous()

        def torch_layers(upto):
            x = x_nchw
            for k in range(1, upto + 1):
                x = torch.relu(F.conv2d(x, wd[k - 1], bd[k - 1], padding=1))
                if k in POOL_AFTER and k < upto:
                    x = F.max_pool2d(x, 2, 2)
            return x
        for k in range(1, 14):
            items[f"torch prefix {k}"] = (lambda k=k: torch_layers(k))
    times = {name: [] for name in items}
    for rep in range(a.reps + 2):
        for name, fn in items.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= 2:
                times[name].append(e0.elapsed_time(e1))
    med = {name: float(np.median(v)) for name, v in times.items()}
    lines = ["LPIPS engine (tools/lpips_probe.py): " + " ".join(sys.argv[1:]),
             f"{torch.cuda.get_device_name(0)}; torch {torch.__version__}; {a.reps} repetitions after 2 warm-up rounds, hipEvent medians [min .. max], ms"]
    for name in ("distance 800x800", "distance 378x504"):
        lines.append(f"{name:18s} {med[name]:9.3f} [{min(times[name]):.3f} .. {max(times[name]):.3f}]")
    lines.append("layer (800x800 input, one image; includes the pool in front of it)      ms      GFLOP   TFLOP/s  of peak" + ("   torch ms" if a.torch else ""))
    h, w, c, total = 800, 800, 3, 0.0
    for k in range(1, 14):
        t = med[f"prefix {k}"] - (med[f"prefix {k - 1}"] if k > 1 else 0.0)
        flop = 2.0 * 9 * c * CHANNELS[k - 1] * h * w
        total += flop
        extra = ""
        if a.torch:
            extra = f"  {med[f'torch prefix {k}'] - (med[f'torch prefix {k - 1}'] if k > 1 else 0.0):9.3f}"
        lines.append(f"conv {k:2d}  {c:3d} -> {CHANNELS[k - 1]:3d}  {h:3d} x {w:3d}  prefix {med[f'prefix {k}']:9.3f}   {t:9.3f}  {flop / 1e9:9.2f}  {flop / t / 1e9:8.2f}  "
                     f"{100 * flop / t / 1e-3 / PEAK:6.1f} %" + extra)
        c = CHANNELS[k - 1]
        if k in POOL_AFTER:
            h, w = h // 2, w // 2
    lines.append(f"13 layers, one image: {med['prefix 13']:.3f} ms for {total / 1e9:.1f} GFLOP = {total / med['prefix 13'] / 1e9:.2f} TFLOP/s "
                 f"({100 * total / med['prefix 13'] / 1e-3 / PEAK:.1f} % of peak)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
