"""A restatement of the LPIPS definition of include/mi_nerf_lpips.h for the tests, with torch CPU conv2d / max_pool2d, runnable in float64
and in float32.  Written from the header, not from any package.  Also the seeded weights and images the LPIPS tests share.

A plan is (cin0, ops) with ops a list of ("conv", cout) / "pool" / "tap" entries, the form ``_lpips.make_net`` takes.
"""
import math

import torch
import torch.nn.functional as F

VGG16 = (3, [("conv", 64), ("conv", 64), "tap", "pool", ("conv", 128), ("conv", 128), "tap", "pool",
             ("conv", 256), ("conv", 256), ("conv", 256), "tap", "pool", ("conv", 512), ("conv", 512), ("conv", 512), "tap", "pool",
             ("conv", 512), ("conv", 512), ("conv", 512), "tap"])
NARROW = (3, [("conv", 32), ("conv", 32), "tap", "pool", ("conv", 64), ("conv", 64), "tap", "pool", ("conv", 32), "tap"])


def random_weights(plan, seed=0):
    """conv weights N(0, 2 / (9 cin)), biases N(0, 0.01) (standard deviation 0.1), tap weights uniform in [0, 1], a mild input affine."""
    cin0, ops = plan
    g = torch.Generator().manual_seed(seed)
    conv_w, conv_b, tap_w = [], [], []
    c = cin0
    for op in ops:
        if isinstance(op, tuple):
            conv_w.append(torch.randn(op[1], c, 3, 3, generator=g) * math.sqrt(2.0 / (9 * c)))
            conv_b.append(torch.randn(op[1], generator=g) * 0.1)
            c = op[1]
        elif op == "tap":
            tap_w.append(torch.rand(c, generator=g))
    a = 4.0 + torch.rand(cin0, generator=g)
    b = -2.0 - 0.2 * torch.rand(cin0, generator=g)
    return {"conv_w": conv_w, "conv_b": conv_b, "tap_w": tap_w, "a": a, "b": b}


def smooth_images(n, H, W, c=3, seed=0, noise=0.03):
    """(pred, target) [n, H, W, c] fp32: smooth random fields in [0, 1]; the target is the prediction plus noise of a few per cent."""
    g = torch.Generator().manual_seed(1000 + seed)
    low = torch.rand(n, c, max(2, H // 4 + 1), max(2, W // 4 + 1), generator=g)
    pred = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).contiguous()
    target = (pred + noise * torch.randn(pred.shape, generator=g)).clamp(0.0, 1.0)
    return pred.float().contiguous(), target.float().contiguous()


def features(plan, wts, img, dtype=torch.float64):
    """The un-normalised features at every tap of img [n, H, W, cin0]: a list of [n, H_t, W_t, C_t] tensors of `dtype`."""
    cin0, ops = plan
    a, b = wts["a"].to(dtype), wts["b"].to(dtype)
    x = (img.to(dtype) * a + b).permute(0, 3, 1, 2)             # the affine first: the zero padding is applied to x'
    out, k = [], 0
    for op in ops:
        if isinstance(op, tuple):
            x = torch.relu(F.conv2d(x, wts["conv_w"][k].to(dtype), wts["conv_b"][k].to(dtype), stride=1, padding=1))
            k += 1
        elif op == "pool":
            x = F.max_pool2d(x, 2, 2)                           # floor: the remainder row / column is dropped
        else:
            out.append(x.permute(0, 2, 3, 1).contiguous())
    return out


def tap_term(fx, fy, w):
    """d_t [n] of two [n, H_t, W_t, C_t] feature maps, in their dtype."""
    nx = fx / (torch.sqrt((fx * fx).sum(-1, keepdim=True)) + 1e-10)
    ny = fy / (torch.sqrt((fy * fy).sum(-1, keepdim=True)) + 1e-10)
    return (w.to(fx.dtype).reshape(-1) * (nx - ny) ** 2).sum(-1).mean((1, 2))


def distance(plan, wts, pred, target, dtype=torch.float64):
    """(LPIPS [n], per-tap terms [n, n_taps]) in `dtype`."""
    fx, fy = features(plan, wts, pred, dtype), features(plan, wts, target, dtype)
    terms = torch.stack([tap_term(x, y, w) for x, y, w in zip(fx, fy, wts["tap_w"])], -1)
    return terms.sum(-1), terms
