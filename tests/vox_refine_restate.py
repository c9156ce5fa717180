"""THE RESAMPLING RULE and THE PRUNING RULE of include/mi_nerf_vox.h restated in numpy, written from the header's comment and not from the
kernels.  The cell's corners, their weights and the pairwise sum are tests/vox_restate.py's (step 3 of the render rule); the stencil of the
pruning rule is tests/vox_sparse_restate.py's active set with a threshold.

``dtype=np.float32`` evaluates the library's own operations in its order -- the GPU tests hold the library to it bit for bit;
``dtype=np.float64`` is the same rule in exact-enough arithmetic, for the properties of the rule itself.  Inputs are fp32 values in both.
"""
from __future__ import annotations

import numpy as np

from tests.vox_restate import RECORD, _interp, corners


def resample(lo_s, hi_s, res_s, lo_d, hi_d, res_d, B, sigma, coef, dtype=np.float32):
    """(sigma_d [P_z, P_y, P_x], coef_d [P_z, P_y, P_x, R]) on the destination lattice, in `dtype`.  The padding of the result is zero and
    the source's padding is never read."""
    f32 = np.float32
    lo_s, hi_s = np.asarray(lo_s, f32).astype(dtype), np.asarray(hi_s, f32).astype(dtype)
    lo_d, hi_d = np.asarray(lo_d, f32).astype(dtype), np.asarray(hi_d, f32).astype(dtype)
    res_s, res_d = [int(r) for r in res_s], [int(r) for r in res_d]
    sigma = np.asarray(sigma, f32).astype(dtype)
    coef = np.asarray(coef, f32)[..., :3 * B].astype(dtype)                  # the counted floats alone
    c, f = [], []
    for i in range(3):                                                       # x, y, z: one axis at a time, the rule is separable up to the weights
        step = (hi_d[i] - lo_d[i]) / dtype(res_d[i])
        inv = dtype(res_s[i]) / (hi_s[i] - lo_s[i])
        x = lo_d[i] + np.arange(res_d[i] + 1).astype(dtype) * step
        g = (x - lo_s[i]) * inv
        ci = np.clip(np.floor(g).astype(np.int64), 0, res_s[i] - 1)
        c.append(ci)
        f.append(np.fmin(np.fmax(g - ci.astype(dtype), dtype(0)), dtype(1)))
    # every destination point, as arrays [P_z, P_y, P_x]
    shape = (res_d[2] + 1, res_d[1] + 1, res_d[0] + 1)
    cc = [np.broadcast_to(c[0][None, None, :], shape), np.broadcast_to(c[1][None, :, None], shape), np.broadcast_to(c[2][:, None, None], shape)]
    ff = [np.broadcast_to(f[0][None, None, :], shape), np.broadcast_to(f[1][None, :, None], shape), np.broadcast_to(f[2][:, None, None], shape)]
    w, at = corners(cc, ff)
    sigma_d = _interp(w, [sigma[a] for a in at])
    out = np.zeros(shape + (RECORD[B],), dtype)
    out[..., :3 * B] = _interp([we[..., None] for we in w], [coef[a] for a in at])
    return sigma_d.astype(dtype), out


def rays_into_box(lo, hi, n, seed):
    """rays [n, 6] fp32 from a sphere around the box, aimed at random points inside it, with |d| of 1, 0.5 or 2: what a restatement test
    needs of rays without a GPU test module."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    o = c + v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(2.5, 3.5, (n, 1))
    d = c + rng.uniform(-0.9, 0.9, (n, 3)) * h - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.choice([1.0, 0.5, 2.0], (n, 1))
    return np.concatenate([o, d], 1).astype(np.float32)


def kept_set(sigma, tau):
    """bool [P_z, P_y, P_x]: the point or one of its 26 neighbours, clipped to the lattice, has sigma > tau."""
    dense = np.asarray(sigma, np.float32) > np.float32(tau)
    P = dense.shape
    pad = np.pad(dense, 1)                                                   # False outside the lattice
    out = np.zeros(P, bool)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                out |= pad[dz:dz + P[0], dy:dy + P[1], dx:dx + P[2]]
    return out


def prune(sigma, coef, tau):
    """(sigma_out, coef_out): sigma and the whole record (padding included) become zero where the point is not kept; a kept point keeps
    every bit of both."""
    sigma, coef = np.asarray(sigma, np.float32), np.asarray(coef, np.float32)
    keep = kept_set(sigma, tau)
    return np.where(keep, sigma, np.float32(0)), np.where(keep[..., None], coef, np.float32(0))
