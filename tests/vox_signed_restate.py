"""A SIGNED GRID of include/mi_nerf_vox.h and the Signed paragraph of THE BACKWARD RULE of include/mi_nerf_voxgrad.h restated in numpy,
written from the headers' comments and not from the kernels: the signed render, the signed skip plane, the widened backward, and the
rule by which ``RadianceGrid.to_signed`` makes a signed plane of one that only knows inside and outside.  The slab, the intervals, the
cells, the corner weights, the pairwise sum and the basis are those of tests/vox_restate.py, imported and not respelled.

``dtype=np.float64`` is the comparator; ``dtype=np.float32`` evaluates the same operations in the library's own number format.  Inputs are
fp32 values in both modes.  The one change against the unsigned rule is where the ReLU sits: ``sigma_s = fmax(interpolation, 0)``.
"""
from __future__ import annotations

import numpy as np

from tests import vox_restate as VR
from tests.voxgrad_restate import _flat, error  # noqa: F401  (error: the measure of tests/test_gpu_voxgrad.py, for the signed GPU tests)


def build_skip(sigma, res):
    """The signed skip plane [B_z, B_y, B_x]: 0 iff sigma <= 0 on the block's cells extended by one cell, clipped -- the points of
    vox_restate.build_skip, the test > 0 in the place of != 0."""
    return VR.build_skip(np.asarray(sigma) > 0, res)


def to_signed(sigma):
    """sigma[j] where it is > 0; elsewhere minus the largest sigma of the 26 neighbours (clipped to the lattice).  The largest of the
    3 x 3 x 3 window serves: the centre of a point that is not > 0 never exceeds a neighbour that is, and a window without density gives
    -max(., 0) = 0.  Exact in any arithmetic: a maximum and a negation."""
    s = np.asarray(sigma)
    p = np.pad(np.maximum(s, 0), 1, mode="constant", constant_values=0)
    best = np.zeros_like(s)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                best = np.maximum(best, p[dz:dz + s.shape[0], dy:dy + s.shape[1], dx:dx + s.shape[2]])
    return np.where(s > 0, s, -best).astype(s.dtype)


def render(lo, hi, res, B, sigma, coef, rays, step, t_near, t_far, T_min=0.0, bg=(1.0, 1.0, 1.0), dtype=np.float64, skip=None):
    """THE RENDER RULE with A SIGNED GRID's step 3.  ``skip`` None: every sample is fetched (use_skip = 0).  With a plane, a sample whose
    cell's block byte is 0 is not fetched -- the rule per sample, without the jump, which only ever leaves out more of the same samples;
    ``samples`` then bounds ``visited`` from above.  Returns the dict of vox_restate.render and ``min_abs``, the smallest |interpolation|
    over all fetched samples, and ``min_abs_nz``, the smallest that is not exactly 0 (inf if there is none)."""
    f32 = np.float32
    lo, hi = np.asarray(lo, f32).astype(dtype), np.asarray(hi, f32).astype(dtype)
    res = [int(r) for r in res]
    inv = [dtype(res[i]) / (hi[i] - lo[i]) for i in range(3)]
    sigma = np.asarray(sigma, f32).astype(dtype)
    coef = np.asarray(coef, f32).astype(dtype)
    rays = np.asarray(rays, f32).astype(dtype).reshape(-1, 6)
    bg = np.asarray(bg, f32).astype(dtype)
    step, t_near, t_far, T_min = dtype(f32(step)), dtype(f32(t_near)), dtype(f32(t_far)), dtype(f32(T_min))
    cap = VR.max_steps(lo, hi, step)
    n = rays.shape[0]
    o, d = rays[:, :3], rays[:, 3:]
    L, t0, t1, miss = VR.slab(lo, hi, o, d, t_near, t_far)
    with np.errstate(all="ignore"):
        dt = step / L
        Y = VR.sh_basis(d / L[:, None], B, dtype)
    rgb, acc, depth = np.zeros((n, 3), dtype), np.zeros(n, dtype), np.zeros(n, dtype)
    T = np.ones(n, dtype)
    visited = np.zeros(n, np.int64)
    live = ~miss
    one, zero = dtype(1), dtype(0)
    min_abs = min_abs_nz = np.inf
    for k in range(cap):
        live, r, ak, bk, mk, c, f = VR.samples(k, live, lo, inv, res, o, d, t0, t1, dt)
        if r.size == 0:
            break
        if skip is not None:
            keep = np.asarray(skip)[c[2] >> 3, c[1] >> 3, c[0] >> 3] != 0
            r, ak, bk, mk = r[keep], ak[keep], bk[keep], mk[keep]
            c, f = [ci[keep] for ci in c], [fi[keep] for fi in f]
            if r.size == 0:
                continue
        delta = (bk - ak) * L[r]
        w, at = VR.corners(c, f)
        raw = VR._interp(w, [sigma[a] for a in at])
        min_abs = min(min_abs, float(np.abs(raw).min()))
        if (raw != 0).any():
            min_abs_nz = min(min_abs_nz, float(np.abs(raw[raw != 0]).min()))
        sigma_s = np.fmax(raw, zero)                                             # the ReLU AFTER the interpolation
        alpha = one - np.exp(-(sigma_s * delta))
        wt = T[r] * alpha
        pos = sigma_s > 0
        if pos.any():
            col = np.zeros((r.size, 3), dtype)
            Yp = Y[r][pos]
            q = []
            for e in range(8):
                kc = coef[at[e][0][pos], at[e][1][pos], at[e][2][pos]]
                qe = kc[:, 0:3] * Yp[:, 0:1]
                for b in range(1, B):
                    qe = qe + kc[:, 3 * b:3 * b + 3] * Yp[:, b:b + 1]
                q.append(qe)
            wp = [we[pos][:, None] for we in w]
            col[pos] = np.fmin(np.fmax(VR._interp(wp, q), zero), one)
            rgb[r] = rgb[r] + wt[:, None] * col
        acc[r] = acc[r] + wt
        depth[r] = depth[r] + wt * mk
        T[r] = T[r] * (one - alpha)
        visited[r] += 1
        live[r] = ~(T[r] < T_min)
    rgb = rgb + (one - acc)[:, None] * bg[None, :]
    with np.errstate(all="ignore"):
        q = depth / acc
        m = np.where(np.isnan(q), q, np.fmax(dtype(1e-10) if dtype == np.float64 else dtype(np.float32(1e-10)), q))
        disp = one / m
        disp = np.where(np.isnan(disp), zero, disp)
        disp = np.where(disp > dtype(5), dtype(5), disp)
    return {"rgb": rgb, "disp": disp, "acc": acc, "depth": depth, "samples": visited, "min_abs": min_abs, "min_abs_nz": min_abs_nz}


def backward(lo, hi, res, B, sigma, coef, rays, step, t_near, t_far, G, ga=None, gd=None, T_min=0.0, bg=(1.0, 1.0, 1.0), skip=None,
             dtype=np.float64):
    """THE BACKWARD RULE on a signed plane: sigma_s = fmax(interpolation, 0) in both marches, and d_sigma receives w_e dL/d sigma_s only
    from the samples whose interpolation is >= 0.  Returns what voxgrad_restate.backward returns (without ``prefix``), ``min_abs`` as
    ``render`` and ``neg_only``, a mask of the sigma elements that some sample touches and all of whose samples interpolate below 0."""
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
    gap = ga - ((G[:, 0] * bg[0] + G[:, 1] * bg[1]) + G[:, 2] * bg[2])
    rgb, acc, depth = np.zeros((n, 3), dtype), np.zeros(n, dtype), np.zeros(n, dtype)
    T = np.ones(n, dtype)
    S = np.zeros(n, dtype)
    samples = np.zeros(n, np.int64)
    live = ~miss
    one, zero = dtype(1), dtype(0)
    qdist_w = qdist_all = min_abs = min_abs_nz = np.inf
    kept = []
    size = int(np.prod(P))
    touched, open_ = np.zeros(size, bool), np.zeros(size, bool)                  # touched by a sample | by one that interpolates >= 0
    for k in range(cap):
        live, r, ak, bk, mk, c, f = VR.samples(k, live, lo, inv, res, o, d, t0, t1, dt)
        if r.size == 0:
            break
        if skip is not None:
            keep = np.asarray(skip)[c[2] >> 3, c[1] >> 3, c[0] >> 3] != 0
            r, ak, bk, mk = r[keep], ak[keep], bk[keep], mk[keep]
            c, f = [ci[keep] for ci in c], [fi[keep] for fi in f]
            if r.size == 0:
                continue
        delta = (bk - ak) * L[r]
        w, at = VR.corners(c, f)
        raw = VR._interp(w, [sigma[a] for a in at])
        min_abs = min(min_abs, float(np.abs(raw).min()))
        if (raw != 0).any():
            min_abs_nz = min(min_abs_nz, float(np.abs(raw[raw != 0]).min()))
        sigma_s = np.fmax(raw, zero)
        alpha = one - np.exp(-(sigma_s * delta))
        wt = T[r] * alpha
        Yr = Y[r]
        qe = []
        for e in range(8):
            kc = coef[at[e]]
            v = kc[:, 0:3] * Yr[:, 0:1]
            for b in range(1, B):
                v = v + kc[:, 3 * b:3 * b + 3] * Yr[:, b:b + 1]
            qe.append(v)
        q = VR._interp([we[:, None] for we in w], qe)
        col = np.fmin(np.fmax(q, zero), one)
        Gr = G[r]
        sk = (((Gr[:, 0] * col[:, 0] + Gr[:, 1] * col[:, 1]) + Gr[:, 2] * col[:, 2]) + gap[r]) + gd[r] * mk
        pos = sigma_s > 0
        rgb[r] = rgb[r] + np.where(pos[:, None], wt[:, None] * col, zero)
        acc[r] = acc[r] + wt
        depth[r] = depth[r] + wt * mk
        S[r] = S[r] + wt * sk
        dist = np.minimum(np.abs(q), np.abs(q - one)).min(1)
        if dist.size:
            qdist_all = min(qdist_all, float(dist.min()))
        if (wt > 0).any():
            qdist_w = min(qdist_w, float(dist[wt > 0].min()))
        kept.append((r, T[r].copy(), wt, sk, delta, w, at, q, raw >= zero))
        for e in range(8):
            flat = _flat(at[e], P)
            touched[flat] = True
            open_[flat[raw >= zero]] = True
        T[r] = T[r] * (one - alpha)
        samples[r] += 1
        live[r] = ~(T[r] < T_min)
    rgb = rgb + (one - acc)[:, None] * bg[None, :]
    Pfx = np.zeros(n, dtype)
    s_ray, s_idx, s_val, c_ray, c_idx, c_val = [], [], [], [], [], []
    for r, Tb, wt, sk, delta, w, at, q, through in kept:
        dsig = np.where(through, delta * (Tb * sk - (S[r] - Pfx[r])), zero)      # nothing where the interpolation is negative
        inside = (q >= zero) & (q <= one)
        gq = np.where(inside, wt[:, None] * G[r], zero)
        Yr = Y[r]
        for e in range(8):
            flat = _flat(at[e], P)
            s_ray.append(r[through]); s_idx.append(flat[through]); s_val.append((w[e] * dsig)[through])
            wy = w[e][:, None] * Yr
            val = wy[:, :, None] * gq[:, None, :]
            idx = flat[:, None] * R + np.arange(3 * B)[None, :]
            c_ray.append(np.repeat(r, 3 * B)); c_idx.append(idx.reshape(-1)); c_val.append(val.reshape(-1))
        Pfx[r] = Pfx[r] + wt * sk

    def total(ray, idx, val, shape):
        size = int(np.prod(shape))
        g, A = np.zeros(size, dtype), np.zeros(size, np.float64)
        cnt = np.zeros(size, np.int64)
        if ray:
            ray, idx, val = np.concatenate(ray), np.concatenate(idx), np.concatenate(val)
            order = np.argsort(ray, kind="stable")
            idx, val = idx[order], val[order]
            nzv = val != 0
            idx, val = idx[nzv], val[nzv]
            np.add.at(g, idx, val)
            np.add.at(A, idx, np.abs(val.astype(np.float64)))
            cnt = np.bincount(idx, minlength=size).astype(np.int64)
        return dict(g=g.reshape(shape), A=A.reshape(shape), c=cnt.reshape(shape))

    return {"d_sigma": total(s_ray, s_idx, s_val, P), "d_coef": total(c_ray, c_idx, c_val, P + (R,)), "rgb": rgb, "acc": acc, "depth": depth,
            "qdist_w": qdist_w, "qdist_all": qdist_all, "samples": samples, "min_abs": min_abs, "min_abs_nz": min_abs_nz, "neg_only": (touched & ~open_).reshape(P)}
