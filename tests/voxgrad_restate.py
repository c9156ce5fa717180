"""THE BACKWARD RULE of include/mi_nerf_voxgrad.h restated in numpy, written from the header's comment and not from the kernel; the
forward pieces (basis, interpolation order, step bound) are those of tests/vox_restate.py.

``dtype=np.float64`` is the comparator; ``dtype=np.float32`` evaluates the same operations in the library's own number format and sums
every gradient element's contributions in ray order, then sample order, then corner order.  Per gradient array the result holds
    g   the gradient,
    A   the sum of the absolute values of the contributions to each element (float64),
    c   their count (contributions that are exactly 0 are not counted: they are not added),
so that a sum of the same contributions in any order lies within c * 2^-24 * A of the exact one.  Inputs are fp32 values in both modes.
Rays are vectorised, the interval counter k is the one Python loop.
"""
from __future__ import annotations

import numpy as np

from tests import vox_restate as VR


def _flat(at, P):
    """flat(j) = (j_z * P_y + j_y) * P_x + j_x of an index triple (z, y, x); P = (P_z, P_y, P_x)."""
    return (at[0] * P[1] + at[1]) * P[2] + at[2]


def backward(lo, hi, res, B, sigma, coef, rays, step, t_near, t_far, G, ga=None, gd=None, T_min=0.0, bg=(1.0, 1.0, 1.0), skip=None,
             dtype=np.float64, prefixes=()):
    """The gradients of sum over rays of (G . rgb) + ga acc + gd depth.  ``skip`` [B_z, B_y, B_x] or None (use_skip = 0).
    Returns a dict: d_sigma / d_coef -> dict(g, A, c) in the shapes of sigma / coef; rgb, acc, depth (the forward, as the backward
    recomputes it); qdist_w / qdist_all, the smallest distance of a pre-clamp colour from 0 or 1 over the samples with w_k > 0 / over all
    visited samples (inf if there is none); samples [n]; prefix -> {m: the d_sigma / d_coef of the first m rays alone} for m in ``prefixes``."""
    f32 = np.float32
    lo, hi = np.asarray(lo, f32).astype(dtype), np.asarray(hi, f32).astype(dtype)
    res = [int(r) for r in res]
    inv = [dtype(res[i]) / (hi[i] - lo[i]) for i in range(3)]
    sigma = np.asarray(sigma, f32).astype(dtype)
    coef = np.asarray(coef, f32).astype(dtype)
    P = sigma.shape
    R = VR.RECORD[B]
    assert coef.shape == P + (R,)
    rays = np.asarray(rays, f32).astype(dtype).reshape(-1, 6)
    n = rays.shape[0]
    bg = np.asarray(bg, f32).astype(dtype)
    G = np.asarray(G, f32).astype(dtype).reshape(n, 3)
    ga = np.zeros(n, dtype) if ga is None else np.asarray(ga, f32).astype(dtype)
    gd = np.zeros(n, dtype) if gd is None else np.asarray(gd, f32).astype(dtype)
    step, t_near, t_far, T_min = dtype(f32(step)), dtype(f32(t_near)), dtype(f32(t_far)), dtype(f32(T_min))
    cap = VR.max_steps(lo, hi, step)
    o, d = rays[:, :3], rays[:, 3:]
    L, t0, t1, miss = VR.slab(lo, hi, o, d, t_near, t_far)
    with np.errstate(all="ignore"):
        dt = step / L
        Y = VR.sh_basis(d / L[:, None], B, dtype)
    gap = ga - ((G[:, 0] * bg[0] + G[:, 1] * bg[1]) + G[:, 2] * bg[2])            # the effective gradient of acc
    rgb, acc, depth = np.zeros((n, 3), dtype), np.zeros(n, dtype), np.zeros(n, dtype)
    T = np.ones(n, dtype)
    S = np.zeros(n, dtype)
    samples = np.zeros(n, np.int64)
    live = ~miss
    one, zero = dtype(1), dtype(0)
    qdist_w = qdist_all = np.inf
    kept = []                                                                    # what the second pass needs of every sample
    # ---- the forward, and S ---------------------------------------------------------------------------
    for k in range(cap):
        live, r, ak, bk, mk, c, f = VR.samples(k, live, lo, inv, res, o, d, t0, t1, dt)
        if r.size == 0:
            break
        if skip is not None:                                                     # a sample whose cell's block byte is 0 contributes nothing
            keep = np.asarray(skip)[c[2] >> 3, c[1] >> 3, c[0] >> 3] != 0
            r, ak, bk, mk = r[keep], ak[keep], bk[keep], mk[keep]
            c, f = [ci[keep] for ci in c], [fi[keep] for fi in f]
            if r.size == 0:
                continue
        delta = (bk - ak) * L[r]
        w, at = VR.corners(c, f)
        sigma_s = VR._interp(w, [sigma[a] for a in at])
        alpha = one - np.exp(-(sigma_s * delta))
        wt = T[r] * alpha
        # the colour at EVERY visited sample
        Yr = Y[r]
        qe = []
        for e in range(8):
            kc = coef[at[e]]
            v = kc[:, 0:3] * Yr[:, 0:1]
            for b in range(1, B):
                v = v + kc[:, 3 * b:3 * b + 3] * Yr[:, b:b + 1]
            qe.append(v)
        q = VR._interp([we[:, None] for we in w], qe)                            # pre-clamp [m, 3]
        col = np.fmin(np.fmax(q, zero), one)
        Gr = G[r]
        sk = (((Gr[:, 0] * col[:, 0] + Gr[:, 1] * col[:, 1]) + Gr[:, 2] * col[:, 2]) + gap[r]) + gd[r] * mk
        pos = sigma_s > 0
        rgb[r] = rgb[r] + np.where(pos[:, None], wt[:, None] * col, zero)        # the forward adds colour only when sigma_s > 0
        acc[r] = acc[r] + wt
        depth[r] = depth[r] + wt * mk
        S[r] = S[r] + wt * sk
        dist = np.minimum(np.abs(q), np.abs(q - one)).min(1)
        if dist.size:
            qdist_all = min(qdist_all, float(dist.min()))
        if (wt > 0).any():
            qdist_w = min(qdist_w, float(dist[wt > 0].min()))
        kept.append((r, T[r].copy(), wt, sk, delta, w, at, q))
        T[r] = T[r] * (one - alpha)
        samples[r] += 1
        live[r] = ~(T[r] < T_min)
    rgb = rgb + (one - acc)[:, None] * bg[None, :]
    # ---- the second pass: prefix, density and colour gradients, contribution by contribution ----------------
    Pfx = np.zeros(n, dtype)
    s_ray, s_idx, s_val, c_ray, c_idx, c_val = [], [], [], [], [], []
    for r, Tb, wt, sk, delta, w, at, q in kept:
        dsig = delta * (Tb * sk - (S[r] - Pfx[r]))
        inside = (q >= zero) & (q <= one)
        gq = np.where(inside, wt[:, None] * G[r], zero)                          # [m, 3]
        Yr = Y[r]
        for e in range(8):
            flat = _flat(at[e], P)
            s_ray.append(r); s_idx.append(flat); s_val.append(w[e] * dsig)
            wy = w[e][:, None] * Yr                                              # (w_e Y_b) [m, B]
            val = wy[:, :, None] * gq[:, None, :]                                # [m, B, 3]: element 3 b + c
            idx = flat[:, None] * R + np.arange(3 * B)[None, :]
            c_ray.append(np.repeat(r, 3 * B)); c_idx.append(idx.reshape(-1)); c_val.append(val.reshape(-1))
        Pfx[r] = Pfx[r] + wt * sk

    def ordered(ray, idx, val):
        if not ray:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, dtype)
        ray, idx, val = np.concatenate(ray), np.concatenate(idx), np.concatenate(val)
        order = np.argsort(ray, kind="stable")                                   # ray order; within a ray the samples are in k order already
        ray, idx, val = ray[order], idx[order], val[order]
        nzv = val != 0                                                           # a contribution that is exactly 0 is not added
        return ray[nzv], idx[nzv], val[nzv]

    def total(ray, idx, val, shape, first):
        size = int(np.prod(shape))
        m = ray < first
        idx, val = idx[m], val[m]
        g, A = np.zeros(size, dtype), np.zeros(size, np.float64)
        np.add.at(g, idx, val)                                                   # unbuffered: one rounded add per contribution, in this order
        np.add.at(A, idx, np.abs(val.astype(np.float64)))
        cnt = np.bincount(idx, minlength=size).astype(np.int64)
        return dict(g=g.reshape(shape), A=A.reshape(shape), c=cnt.reshape(shape))

    s_all, c_all = ordered(s_ray, s_idx, s_val), ordered(c_ray, c_idx, c_val)
    out = {"d_sigma": total(*s_all, P, n), "d_coef": total(*c_all, P + (R,), n),
           "rgb": rgb, "acc": acc, "depth": depth, "qdist_w": qdist_w, "qdist_all": qdist_all, "samples": samples}
    # the gradients of the first m rays alone, for every m asked for: the same contributions, cut off
    out["prefix"] = {int(m): {"d_sigma": total(*s_all, P, m), "d_coef": total(*c_all, P + (R,), m)} for m in prefixes}
    return out


def error(x, ref):
    """e(x) = max over the elements with A > 0 of |x - g64| / A, for a gradient array x against the float64 result ``ref``."""
    m = ref["A"] > 0
    if not m.any():
        return 0.0
    return float((np.abs(np.asarray(x, np.float64)[m] - ref["g"][m]) / ref["A"][m]).max())
