"""The rule of include/mi_nerf_vox.h restated in numpy, written from the header's comment and not from the kernel.

``dtype=np.float64`` is the comparator the GPU tests hold the library against; ``dtype=np.float32`` evaluates the same operations in the
same order in the library's own number format, and its distance from the float64 result is the measure of what fp32 arithmetic allows on
a given case (tests/test_gpu_vox.py: e_hip <= max(4 e_ref, one ulp)).  Inputs are fp32 values in both modes; only the arithmetic differs.
Rays are vectorised, the interval counter k is the one Python loop.
"""
from __future__ import annotations

import math

import numpy as np

BLOCK = 8
MAX_STEPS = 65536
RECORD = {1: 4, 4: 16, 9: 32}
# the header's constants, as written there
C0, C1, C2, C20, C22 = 0.28209479, 0.48860251, 1.0925484, 0.31539157, 0.54627422


def _c(v, dtype):
    """A constant of the header in the arithmetic of `dtype`: the fp32 library holds its fp32 rounding."""
    return dtype(np.float32(v)) if dtype == np.float32 else dtype(v)


def points(res):
    return tuple(int(r) + 1 for r in res)              # (P_x, P_y, P_z)


def record_floats(B):
    return RECORD.get(B, 0)


def skip_shape(res):
    return tuple(-(-int(r) // BLOCK) for r in reversed(res))        # [B_z, B_y, B_x]


def max_steps(lo, hi, step):
    lo, hi = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    return int(math.ceil(float(np.sqrt(((hi - lo) ** 2).sum())) / float(np.float32(step)))) + 1


def sh_basis(u, B, dtype=np.float64):
    """Y [n, B] at unit vectors u [n, 3], with the header's constants and its order of operations."""
    u = np.asarray(u).astype(dtype)
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    Y = np.empty((u.shape[0], B), dtype)
    Y[:, 0] = _c(C0, dtype)
    if B >= 4:
        Y[:, 1] = -_c(C1, dtype) * y
        Y[:, 2] = _c(C1, dtype) * z
        Y[:, 3] = -_c(C1, dtype) * x
    if B >= 9:
        Y[:, 4] = _c(C2, dtype) * (x * y)
        Y[:, 5] = -_c(C2, dtype) * (y * z)
        Y[:, 6] = _c(C20, dtype) * (((dtype(2) * z) * z - x * x) - y * y)
        Y[:, 7] = -_c(C2, dtype) * (x * z)
        Y[:, 8] = _c(C22, dtype) * (x * x - y * y)
    return Y


def build_skip(sigma, res):
    """skip [B_z, B_y, B_x] of a sigma plane [P_z, P_y, P_x]: 0 iff sigma == 0 on the block's cells extended by one cell, clipped."""
    sigma = np.asarray(sigma)
    out = np.zeros(skip_shape(res), np.uint8)
    rng = []
    for axis in range(3):                                # x, y, z
        r = int(res[axis])
        rng.append([(max(BLOCK * b - 1, 0), min(min(BLOCK * b + BLOCK, r) + 1, r)) for b in range(-(-r // BLOCK))])
    for bz, (z0, z1) in enumerate(rng[2]):
        for by, (y0, y1) in enumerate(rng[1]):
            for bx, (x0, x1) in enumerate(rng[0]):
                out[bz, by, bx] = 1 if np.any(sigma[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] != 0) else 0
    return out


def project(raw, proj, B, dtype=np.float64):
    """(sigma [M], records [M, R]) of raw [M, D, 4] under proj [B, D]: THE PROJECTION of the header."""
    raw32 = np.asarray(raw, np.float32)
    raw, proj = raw32.astype(dtype), np.asarray(proj, np.float32).astype(dtype)
    M, D = raw.shape[:2]
    with np.errstate(all="ignore"):
        dens = raw32[:, 0, 3]
        sigma = np.where(dens > 0, dens, np.float32(0)).astype(np.float32)       # fmaxf(x, 0): a NaN becomes 0; exact in any arithmetic
        s = dtype(1) / (dtype(1) + np.exp(-raw[:, :, :3]))                        # [M, D, 3]
        rec = np.zeros((M, RECORD[B]), dtype)
        for b in range(B):
            acc = proj[b, 0] * s[:, 0, :]
            for j in range(1, D):
                acc = acc + proj[b, j] * s[:, j, :]
            rec[:, 3 * b:3 * b + 3] = acc
    return sigma, rec


def _interp(w, q):
    """The header's order: v_e = w_e q_e, x neighbours first, then y, then z."""
    v = [w[e] * q[e] for e in range(8)]
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))


def slab(lo, hi, o, d, t_near, t_far):
    """Step 1 of the rule for a ray set, in the arithmetic of the arrays passed: (L, t0, t1, miss), each [n]."""
    dtype = o.dtype.type
    n = o.shape[0]
    with np.errstate(all="ignore"):
        L = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        miss = ~(np.isfinite(o).all(1) & np.isfinite(L)) | (L == 0)
        entry, exit_ = np.full(n, -np.inf, dtype), np.full(n, np.inf, dtype)
        for i in range(3):
            nz = d[:, i] != 0
            ta, tb = (lo[i] - o[:, i]) / d[:, i], (hi[i] - o[:, i]) / d[:, i]
            entry = np.where(nz, np.fmax(entry, np.fmin(ta, tb)), entry)
            exit_ = np.where(nz, np.fmin(exit_, np.fmax(ta, tb)), exit_)
            miss |= ~nz & ~((lo[i] <= o[:, i]) & (o[:, i] <= hi[i]))
        t0, t1 = np.fmax(t_near, entry), np.fmin(t_far, exit_)
        miss |= ~(t1 > t0)
    return L, t0, t1, miss


def samples(k, live, lo, inv, res, o, d, t0, t1, dt):
    """Interval k of the rays still live: (live, r, ak, bk, mk, c, f) -- the rays whose interval k exists (a_k < t1) as a mask and as
    indices r, and per such ray the interval's ends and midpoint, the cell c = [c_x, c_y, c_z] and the fractions f of the midpoint."""
    dtype = o.dtype.type
    with np.errstate(all="ignore"):
        ak_all = t0 + dtype(k) * dt
        live = live & (ak_all < t1)
    r = np.nonzero(live)[0]
    ak = ak_all[r]
    bk = np.fmin(t0[r] + dtype(k + 1) * dt[r], t1[r])
    mk = dtype(0.5) * (ak + bk)
    c, f = [], []
    for i in range(3):
        p = o[r, i] + mk * d[r, i]
        g = (p - lo[i]) * inv[i]
        ci = np.clip(np.floor(g).astype(np.int64), 0, res[i] - 1)
        c.append(ci)
        f.append(np.fmin(np.fmax(g - ci.astype(dtype), dtype(0)), dtype(1)))
    return live, r, ak, bk, mk, c, f


def corners(c, f):
    """The eight corners of the samples' cells, e = e_x + 2 e_y + 4 e_z: weights w[e] and index triples at[e] = (z, y, x)."""
    one = f[0].dtype.type(1)
    w, at = [], []
    for e in range(8):
        ex, ey, ez = e & 1, (e >> 1) & 1, e >> 2
        wx, wy, wz = (f[0] if ex else one - f[0]), (f[1] if ey else one - f[1]), (f[2] if ez else one - f[2])
        w.append((wx * wy) * wz)
        at.append((c[2] + ez, c[1] + ey, c[0] + ex))
    return w, at


def render(lo, hi, res, B, sigma, coef, rays, step, t_near, t_far, T_min=0.0, bg=(1.0, 1.0, 1.0), dtype=np.float64):
    """THE RENDER RULE of the header without skipping (skipping changes no output but `visited`).  Returns a dict: rgb [n,3], disp, acc,
    depth [n], and samples [n], the number of samples the ray evaluated (`visited` with use_skip = 0)."""
    f32 = np.float32
    lo, hi = np.asarray(lo, f32).astype(dtype), np.asarray(hi, f32).astype(dtype)
    res = [int(r) for r in res]
    inv = [dtype(res[i]) / (hi[i] - lo[i]) for i in range(3)]
    sigma = np.asarray(sigma, f32).astype(dtype)
    coef = np.asarray(coef, f32).astype(dtype)
    rays = np.asarray(rays, f32).astype(dtype).reshape(-1, 6)
    bg = np.asarray(bg, f32).astype(dtype)
    step, t_near, t_far, T_min = dtype(f32(step)), dtype(f32(t_near)), dtype(f32(t_far)), dtype(f32(T_min))
    cap = max_steps(lo, hi, step)
    n = rays.shape[0]
    o, d = rays[:, :3], rays[:, 3:]
    L, t0, t1, miss = slab(lo, hi, o, d, t_near, t_far)
    with np.errstate(all="ignore"):
        dt = step / L
        Y = sh_basis(d / L[:, None], B, dtype)
    rgb, acc, depth = np.zeros((n, 3), dtype), np.zeros(n, dtype), np.zeros(n, dtype)
    T = np.ones(n, dtype)
    visited = np.zeros(n, np.int64)
    live = ~miss
    one, zero = dtype(1), dtype(0)
    for k in range(cap):
        live, r, ak, bk, mk, c, f = samples(k, live, lo, inv, res, o, d, t0, t1, dt)
        if r.size == 0:
            break
        delta = (bk - ak) * L[r]
        w, at = corners(c, f)
        s_e = [sigma[a] for a in at]
        sigma_s = _interp(w, s_e)
        alpha = one - np.exp(-(sigma_s * delta))
        wt = T[r] * alpha
        pos = sigma_s > 0
        if pos.any():
            col = np.zeros((r.size, 3), dtype)
            Yp = Y[r][pos]
            q = []
            for e in range(8):
                kc = coef[at[e][0][pos], at[e][1][pos], at[e][2][pos]]                   # [m, R]
                qe = kc[:, 0:3] * Yp[:, 0:1]
                for b in range(1, B):
                    qe = qe + kc[:, 3 * b:3 * b + 3] * Yp[:, b:b + 1]
                q.append(qe)
            wp = [we[pos][:, None] for we in w]
            col[pos] = np.fmin(np.fmax(_interp(wp, q), zero), one)
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
    return {"rgb": rgb, "disp": disp, "acc": acc, "depth": depth, "samples": visited}
