"""THE SHADOW RULE, THE VISIBILITY RULE and THE SEEN PRUNING RULE of include/mi_nerf_vox.h restated in numpy, written from the header's
comment and not from the kernels.  The cell's corners, their weights and the pairwise sum are tests/vox_restate.py's (step 3 of the render
rule); the stencil is tests/vox_refine_restate.py's kept set.

``dtype=np.float32`` evaluates the library's own operations in its order -- there is no exponential in the three rules, so the GPU tests
hold the library to it bit for bit; ``dtype=np.float64`` is the same rule in exact-enough arithmetic, for the properties of the rule
itself.  Inputs are fp32 values in both.  Pixels and lattice points are vectorised, the slice counter k is the one Python loop.
"""
from __future__ import annotations

import numpy as np

from tests.vox_refine_restate import kept_set
from tests.vox_restate import _interp, corners

f32 = np.float32


class View:
    """mi_vox_view on the host: H, W, fx, fy, cx, cy, c2w [3,4] (R | t), depth_near, depth_step, K slices -- fp32 values."""

    def __init__(self, H, W, fx, fy, cx, cy, c2w, depth_near, depth_step, K):
        self.H, self.W, self.K = int(H), int(W), int(K)
        self.fx, self.fy, self.cx, self.cy, self.depth_near, self.depth_step = (f32(v) for v in (fx, fy, cx, cy, depth_near, depth_step))
        self.c2w = np.asarray(c2w, f32).reshape(-1)[:12].reshape(3, 4).copy()

    @classmethod
    def from_c(cls, v):
        """From the ctypes struct (nerf_pytorch_paeng_amd._vox.View)."""
        return cls(v.H, v.W, v.fx, v.fy, v.cx, v.cy, list(v.c2w), v.depth_near, v.depth_step, v.slices)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """c2w [3,4] fp32 of the make_o_d camera (it looks along its -z, y up, x right) at `eye` looking at `target`."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    true_up = np.cross(right, fwd)
    return np.concatenate([np.stack([right, true_up, -fwd], 1), eye[:, None]], 1).astype(f32)


def _box(lo, hi, res, dtype):
    lo, hi = np.asarray(lo, f32).astype(dtype), np.asarray(hi, f32).astype(dtype)
    return lo, hi, [int(r) for r in res]


def pixel_rays(view, dtype=np.float32):
    """(o [3], d [3][H * W], L [H * W]) of the view's pixels, row-major (element j W + i), by THE SHADOW RULE."""
    fx, fy, cx, cy = (dtype(v) for v in (view.fx, view.fy, view.cx, view.cy))
    R, t = view.c2w[:, :3].astype(dtype), view.c2w[:, 3].astype(dtype)
    i = np.broadcast_to(np.arange(view.W).astype(dtype)[None, :], (view.H, view.W)).reshape(-1)
    j = np.broadcast_to(np.arange(view.H).astype(dtype)[:, None], (view.H, view.W)).reshape(-1)
    a, b, c = (i - cx) / fx, -((j - cy) / fy), dtype(-1)
    d = [(R[r, 0] * a + R[r, 1] * b) + R[r, 2] * c for r in range(3)]
    L = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return t, d, L


def shadow(lo, hi, res, sigma, view, dtype=np.float32):
    """tvol [H, W, K] in `dtype`: the optical depth before each slice along each pixel's ray.  (The skip plane changes no value and is
    not modelled.)"""
    lo, hi, res = _box(lo, hi, res, dtype)
    inv = [dtype(res[i]) / (hi[i] - lo[i]) for i in range(3)]
    sigma = np.asarray(sigma, f32).astype(dtype)
    near, step = dtype(view.depth_near), dtype(view.depth_step)
    with np.errstate(all="ignore"):
        o, d, L = pixel_rays(view, dtype)
        delta = step * L
        n = L.shape[0]
        od = np.zeros(n, dtype)
        tvol = np.empty((n, view.K), dtype)
        for k in range(view.K):
            tvol[:, k] = od
            m = near + (dtype(k) + dtype(0.5)) * step
            p = [o[i] + m * d[i] for i in range(3)]
            inside = np.ones(n, bool)
            for i in range(3):
                inside &= (lo[i] <= p[i]) & (p[i] <= hi[i])
            r = np.nonzero(inside)[0]
            if r.size == 0:
                continue
            c, f = [], []
            for i in range(3):
                g = (p[i][r] - lo[i]) * inv[i]
                ci = np.clip(np.floor(g).astype(np.int64), 0, res[i] - 1)
                c.append(ci)
                f.append(np.fmin(np.fmax(g - ci.astype(dtype), dtype(0)), dtype(1)))
            w, at = corners(c, f)
            sigma_s = _interp(w, [sigma[a] for a in at])
            od[r] = od[r] + sigma_s * delta[r]
    return tvol.reshape(view.H, view.W, view.K)


def looked_at(lo, hi, res, view, dtype=np.float32):
    """(look bool, fi, fj int64, k0 int64), each [P_z, P_y, P_x]: whether the view looks at the lattice point, its nearest pixel, and its
    slice floorf((z - depth_near) / depth_step) before the bias (the last three are meaningful where look is set)."""
    lo, hi, res = _box(lo, hi, res, dtype)
    fx, fy, cx, cy = (dtype(v) for v in (view.fx, view.fy, view.cx, view.cy))
    R, t = view.c2w[:, :3].astype(dtype), view.c2w[:, 3].astype(dtype)
    near, step = dtype(view.depth_near), dtype(view.depth_step)
    shape = (res[2] + 1, res[1] + 1, res[0] + 1)
    x = [lo[i] + np.arange(res[i] + 1).astype(dtype) * ((hi[i] - lo[i]) / dtype(res[i])) for i in range(3)]
    X = [np.broadcast_to(x[0][None, None, :], shape), np.broadcast_to(x[1][None, :, None], shape), np.broadcast_to(x[2][:, None, None], shape)]
    with np.errstate(all="ignore"):
        e = [X[k] - t[k] for k in range(3)]
        q = [(R[0, i] * e[0] + R[1, i] * e[1]) + R[2, i] * e[2] for i in range(3)]
        z = -q[2]
        sx, sy = cx + (fx * q[0]) / z, cy - (fy * q[1]) / z
        fi, fj = np.rint(sx), np.rint(sy)
        look = (z > 0) & np.isfinite(z) & (fi >= 0) & (fi <= dtype(view.W - 1)) & (fj >= 0) & (fj <= dtype(view.H - 1))
        kf = np.fmin(np.fmax(np.floor((z - near) / step), dtype(-2.0 ** 40)), dtype(2.0 ** 40))
    zero = np.zeros(shape, np.int64)
    return (look, np.where(look, fi, 0).astype(np.int64), np.where(look, fj, 0).astype(np.int64),
            np.where(look, np.where(np.isnan(kf), 0, kf), 0).astype(np.int64) + zero)


def seen(lo, hi, res, view, tvol, bias, od, dtype=np.float32):
    """The od plane [P_z, P_y, P_x] after this view: fmin(od, tvol at the point's pixel and slice) where the view looks."""
    look, fi, fj, k0 = looked_at(lo, hi, res, view, dtype)
    tvol = np.asarray(tvol).astype(dtype)
    out = np.array(od, dtype)
    k = k0 - int(bias)
    hit = look & (k < view.K)
    val = np.where(k >= 0, tvol[fj, fi, np.clip(k, 0, view.K - 1)], dtype(0))
    out[hit] = np.fmin(out[hit], val[hit])
    return out


def seen_all(lo, hi, res, sigma, views, bias, dtype=np.float32):
    """The od plane after every view, from +inf."""
    od = np.full((int(res[2]) + 1, int(res[1]) + 1, int(res[0]) + 1), np.inf, dtype)
    for v in views:
        od = seen(lo, hi, res, v, shadow(lo, hi, res, sigma, v, dtype), bias, od, dtype)
    return od


def kept_seen_set(sigma, tau, od_max, od):
    """bool [P_z, P_y, P_x]: the point or one of its 26 neighbours is a seed (sigma > tau and od <= od_max; a NaN od fails).  tau >= 0,
    so a point whose sigma is replaced by 0 is no seed: the stencil is vox_refine_restate.kept_set's."""
    with np.errstate(invalid="ignore"):
        ok = np.asarray(od, f32) <= f32(od_max)
    return kept_set(np.where(ok, np.asarray(sigma, f32), f32(0)), tau)


def prune_seen(sigma, coef, tau, od_max, od):
    """(sigma_out, coef_out): THE PRUNING RULE's writes under the seen seed."""
    sigma, coef = np.asarray(sigma, f32), np.asarray(coef, f32)
    keep = kept_seen_set(sigma, tau, od_max, od)
    return np.where(keep, sigma, f32(0)), np.where(keep[..., None], coef, f32(0))
