"""THE RAY GRADIENT RULE of include/mi_nerf_vox.h restated in numpy, written from the header's comment and not from the kernel; the forward
pieces (slab, intervals, corners, basis, interpolation order, step bound) are those of tests/vox_restate.py.

``dtype=np.float64`` is the comparator; ``dtype=np.float32`` evaluates the same operations in the same order in the library's own number
format.  Per component of d_rays [n, 6] the result holds
    g   the gradient,
    A   the sum of the absolute values of the contributions to it: the rule evaluated a second time with every term replaced by its
        absolute value (float64), so that A bounds the magnitude of everything that was added or subtracted on the way to g,
    c   the number of terms summed into the component along the ray (8 corners x 4 quantities per evaluated sample, plus the end),
so that the rounding of an fp32 evaluation lies within a small multiple of c * 2^-24 * A.  ``sig`` is per ray a tuple that names the
branch of every kink the ray took (slab axes, interval count, cell sequence, clamp states): two rays with equal ``sig`` lie on one smooth
piece of the rendered function.  Inputs are fp32 values in both modes.  Rays are vectorised, the interval counter k is the one Python loop.
"""
from __future__ import annotations

import numpy as np

from tests import vox_restate as VR


def slab_axes(lo, hi, o, d, t_near, t_far):
    """(ie, ix) [n]: the first axis that attains entry / exit, -1 where t0 = t_near / t1 = t_far (or no axis bounds)."""
    dtype = o.dtype.type
    n = o.shape[0]
    entry, exit_ = np.full(n, -np.inf, dtype), np.full(n, np.inf, dtype)
    ie, ix = np.full(n, -1), np.full(n, -1)
    with np.errstate(all="ignore"):
        for i in range(3):
            nz = d[:, i] != 0
            ta, tb = (lo[i] - o[:, i]) / d[:, i], (hi[i] - o[:, i]) / d[:, i]
            tn, tf = np.fmin(ta, tb), np.fmax(ta, tb)
            ie = np.where(nz & (tn > entry), i, ie)
            ix = np.where(nz & (tf < exit_), i, ix)
            entry = np.where(nz, np.fmax(entry, tn), entry)
            exit_ = np.where(nz, np.fmin(exit_, tf), exit_)
        ie = np.where(entry > t_near, ie, -1)
        ix = np.where(exit_ < t_far, ix, -1)
    return ie, ix


def ray_grad(lo, hi, res, B, sigma, coef, rays, step, t_near, t_far, G, ga=None, gd=None, T_min=0.0, bg=(1.0, 1.0, 1.0), dtype=np.float64,
             want_sig=True):
    """d_rays of sum over rays of (G . rgb) + ga acc + gd depth, without skipping (skipping changes nothing).  Returns a dict: g, A, c
    [n, 6]; rgb, acc, depth (the forward); samples [n]; sig (a list of n tuples; only (ie, ix, miss, ()) each without ``want_sig``)."""
    f32 = np.float32
    lo, hi = np.asarray(lo, f32).astype(dtype), np.asarray(hi, f32).astype(dtype)
    res = [int(r) for r in res]
    inv = [dtype(res[i]) / (hi[i] - lo[i]) for i in range(3)]
    sigma = np.asarray(sigma, f32).astype(dtype)
    coef = np.asarray(coef, f32).astype(dtype)
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
    ie, ix = slab_axes(lo, hi, o, d, t_near, t_far)
    with np.errstate(all="ignore"):
        dt = step / L
        u = d / L[:, None]
        Y = VR.sh_basis(u, B, dtype)
    gap = ga - ((G[:, 0] * bg[0] + G[:, 1] * bg[1]) + G[:, 2] * bg[2])
    gap_abs = np.abs(ga) + np.abs(G) @ np.abs(bg)
    one, zero, half = dtype(1), dtype(0), dtype(0.5)
    f64 = np.float64
    rgb, acc, depth = np.zeros((n, 3), dtype), np.zeros(n, dtype), np.zeros(n, dtype)
    T = np.ones(n, dtype)
    S, S_abs = np.zeros(n, dtype), np.zeros(n, f64)
    samples = np.zeros(n, np.int64)
    live = ~miss
    kept = []
    sig = [[] for _ in range(n)]
    # ---- the forward, and S ---------------------------------------------------------------------------
    for k in range(cap):
        live, r, ak, bk, mk, c, f = VR.samples(k, live, lo, inv, res, o, d, t0, t1, dt)
        if r.size == 0:
            break
        cut = t1[r] < t0[r] + dtype(k + 1) * dt[r]
        moves = []
        for i in range(3):
            p = o[r, i] + mk * d[r, i]
            gi = (p - lo[i]) * inv[i]
            rr = gi - c[i].astype(dtype)
            moves.append((rr >= zero) & (rr <= one))
        delta = (bk - ak) * L[r]
        w, at = VR.corners(c, f)
        s_e = [sigma[a] for a in at]
        sigma_s = VR._interp(w, s_e)
        alpha = one - np.exp(-(sigma_s * delta))
        wt = T[r] * alpha
        pos = sigma_s > 0
        Yr = Y[r]
        kcs, qe = [], []
        for e in range(8):
            kc = np.where(pos[:, None], coef[at[e]], zero)                       # the colour is evaluated only where sigma_s > 0
            v = kc[:, 0:3] * Yr[:, 0:1]
            for b in range(1, B):
                v = v + kc[:, 3 * b:3 * b + 3] * Yr[:, b:b + 1]
            kcs.append(kc)
            qe.append(v)
        q = VR._interp([we[:, None] for we in w], qe)                            # pre-clamp [m, 3]
        col = np.fmin(np.fmax(q, zero), one)
        Gr = G[r]
        sk = (((Gr[:, 0] * col[:, 0] + Gr[:, 1] * col[:, 1]) + Gr[:, 2] * col[:, 2]) + gap[r]) + gd[r] * mk
        sk_abs = (np.abs(Gr).astype(f64) * np.abs(col)).sum(1) + gap_abs[r] + np.abs(gd[r] * mk).astype(f64)
        rgb[r] = rgb[r] + np.where(pos[:, None], wt[:, None] * col, zero)
        acc[r] = acc[r] + wt
        depth[r] = depth[r] + wt * mk
        S[r] = S[r] + wt * sk
        S_abs[r] += np.abs(wt).astype(f64) * sk_abs
        inside = pos[:, None] & (q >= zero) & (q <= one)
        kept.append((k, r, T[r].copy(), wt, sk, sk_abs, delta, ak, mk, cut, moves, w, f, s_e, sigma_s, kcs, qe, inside))
        for j, ray in enumerate(r if want_sig else ()):
            sig[ray].append((int(c[0][j]), int(c[1][j]), int(c[2][j]), bool(cut[j]), bool(pos[j]), tuple(bool(m[j]) for m in moves),
                             tuple(bool(x) for x in inside[j])))
        T[r] = T[r] * (one - alpha)
        samples[r] += 1
        live[r] = ~(T[r] < T_min)
    rgb = rgb + (one - acc)[:, None] * bg[None, :]
    # ---- the second pass: every quantity beside its absolute twin (float64) -------------------------------------
    Pfx, P_abs = np.zeros(n, dtype), np.zeros(n, f64)
    gpo, gpd = np.zeros((n, 3), dtype), np.zeros((n, 3), dtype)
    gpo_a, gpd_a = np.zeros((n, 3), f64), np.zeros((n, 3), f64)
    gt0, gdt, gt1, gL = (np.zeros(n, dtype) for _ in range(4))
    gt0_a, gdt_a, gt1_a, gL_a = (np.zeros(n, f64) for _ in range(4))
    gy = [np.zeros((n, B), dtype) for _ in range(8)]
    gy_a = np.zeros((n, B), f64)
    terms = np.zeros(n, np.int64)
    A64 = lambda x: np.abs(x).astype(f64)                                         # noqa: E731
    for k, r, Tb, wt, sk, sk_abs, delta, ak, mk, cut, moves, w, f, s_e, sigma_s, kcs, qe, inside in kept:
        E = Tb * sk - (S[r] - Pfx[r])
        E_abs = A64(Tb) * sk_abs + S_abs[r] + P_abs[r]
        Dk, Zk = delta * E, sigma_s * E
        Dk_a, Zk_a = A64(delta) * E_abs, A64(sigma_s) * E_abs
        Q = np.where(inside, wt[:, None] * G[r], zero)                           # [m, 3]
        h, h_a = [], []
        for e in range(8):
            h.append(Dk * s_e[e] + ((Q[:, 0] * qe[e][:, 0] + Q[:, 1] * qe[e][:, 1]) + Q[:, 2] * qe[e][:, 2]))
            h_a.append(Dk_a * A64(s_e[e]) + (A64(Q) * A64(qe[e])).sum(1))
        wxyz = [[(f[i] if (e >> i) & 1 else one - f[i]) for i in range(3)] for e in range(8)]
        gp, gp_a = [], []
        for i in range(3):
            j1, j2 = [j for j in range(3) if j != i]
            v = []
            for e in range(8):
                prod = wxyz[e][j1] * wxyz[e][j2]
                v.append(np.where(moves[i], prod if (e >> i) & 1 else -prod, zero))
            gp.append(inv[i] * VR._interp(v, h))
            gp_a.append(f64(abs(inv[i])) * sum(A64(v[e]) * h_a[e] for e in range(8)))
        for i in range(3):
            gpo[r, i] = gpo[r, i] + gp[i]
            gpd[r, i] = gpd[r, i] + mk * gp[i]
            gpo_a[r, i] += gp_a[i]
            gpd_a[r, i] += A64(mk) * gp_a[i]
        dr = d[r]
        gw = gd[r] * wt
        Mk = ((dr[:, 0] * gp[0] + dr[:, 1] * gp[1]) + dr[:, 2] * gp[2]) + gw
        Mk_a = A64(dr[:, 0]) * gp_a[0] + A64(dr[:, 1]) * gp_a[1] + A64(dr[:, 2]) * gp_a[2] + A64(gw)
        kf = dtype(k)
        ld, ld_a = L[r] * Zk, A64(L[r]) * Zk_a
        lower = half * Mk - ld
        lower_a = 0.5 * Mk_a + ld_a
        gt0[r] = gt0[r] + np.where(cut, lower, Mk)
        gdt[r] = gdt[r] + np.where(cut, kf * lower, (kf + half) * Mk)
        gt1[r] = gt1[r] + np.where(cut, half * Mk + ld, zero)
        gL[r] = gL[r] + np.where(cut, (t1[r] - ak) * Zk, zero)
        gt0_a[r] += np.where(cut, lower_a, Mk_a)
        gdt_a[r] += np.where(cut, k * lower_a, (k + 0.5) * Mk_a)
        gt1_a[r] += np.where(cut, lower_a, 0.0)
        gL_a[r] += np.where(cut, A64(t1[r] - ak) * Zk_a, 0.0)
        for e in range(8):
            for b in range(B):
                wk = [w[e] * kcs[e][:, 3 * b + ch] for ch in range(3)]
                gy[e][r, b] = gy[e][r, b] + ((Q[:, 0] * wk[0] + Q[:, 1] * wk[1]) + Q[:, 2] * wk[2])
                gy_a[r, b] += sum(A64(Q[:, ch]) * A64(wk[ch]) for ch in range(3))
        Pfx[r] = Pfx[r] + wt * sk
        P_abs[r] += A64(wt) * sk_abs
        terms[r] += 32
    # ---- the ray's end ------------------------------------------------------------------------------------
    gY = VR._interp([one] * 8, gy) if B > 1 else np.zeros((n, B), dtype)          # 1 * y_e,b is exact: the pairwise sum over the corners
    c1, c2, c20, c22 = (VR._c(v, dtype) for v in (VR.C1, VR.C2, VR.C20, VR.C22))
    two, four = dtype(2), dtype(4)
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    du = np.zeros((n, 3), dtype)
    du_a = np.zeros((n, 3), f64)

    def add(i, coeff, b, first=False):
        t = coeff * gY[:, b]
        du[:, i] = t if first else du[:, i] + t
        du_a[:, i] += A64(coeff) * gy_a[:, b]

    with np.errstate(all="ignore"):
        if B >= 4:
            add(1, -c1, 1, True); add(2, c1, 2, True); add(0, -c1, 3, True)
        if B >= 9:
            add(0, c2 * uy, 4); add(1, c2 * ux, 4)
            add(1, -c2 * uz, 5); add(2, -c2 * uy, 5)
            add(0, -(two * c20) * ux, 6); add(1, -(two * c20) * uy, 6); add(2, (four * c20) * uz, 6)
            add(0, -c2 * uz, 7); add(2, -c2 * ux, 7)
            add(0, (two * c22) * ux, 8); add(1, -(two * c22) * uy, 8)
        udu = (ux * du[:, 0] + uy * du[:, 1]) + uz * du[:, 2]
        udu_a = (A64(u) * du_a).sum(1)
        cdt = gdt * -(step / ((L * L) * L))
        cdt_a = gdt_a * A64(step / ((L * L) * L))
        cl, cl_a = gL / L, gL_a / A64(L)
        go, gdir = gpo.copy(), np.zeros((n, 3), dtype)
        go_a, gdir_a = gpo_a.copy(), np.zeros((n, 3), f64)
        for i in range(3):
            gdir[:, i] = ((gpd[:, i] + (du[:, i] - u[:, i] * udu) / L) + cdt * d[:, i]) + cl * d[:, i]
            gdir_a[:, i] = gpd_a[:, i] + (du_a[:, i] + A64(u[:, i]) * udu_a) / A64(L) + cdt_a * A64(d[:, i]) + cl_a * A64(d[:, i])
        rows = np.arange(n)
        for axis, gt, gt_a, tt in ((ie, gt0, gt0_a, t0), (ix, gt1, gt1_a, t1)):
            m = (axis >= 0) & ~miss
            a = np.where(m, axis, 0)
            qq = np.where(m, gt / d[rows, a], zero)
            qq_a = np.where(m, gt_a / A64(d[rows, a]), 0.0)
            go[rows, a] = go[rows, a] - qq
            gdir[rows, a] = gdir[rows, a] - qq * np.where(m, tt, zero)
            go_a[rows, a] += qq_a
            gdir_a[rows, a] += qq_a * np.where(m, A64(tt), 0.0)
    g = np.concatenate([go, gdir], 1)
    A = np.concatenate([go_a, gdir_a], 1)
    g[miss], A[miss] = zero, 0.0
    cnt = np.where(miss, 0, terms + 3 * B + 8)[:, None].repeat(6, 1)
    for ray in range(n):
        sig[ray] = (int(ie[ray]), int(ix[ray]), bool(miss[ray]), tuple(sig[ray]))
    return {"g": g, "A": A, "c": cnt, "rgb": rgb, "acc": acc, "depth": depth, "samples": samples, "sig": sig}


def error(x, ref):
    """e(x) = max over the components with A > 0 of |x - g64| / A."""
    m = ref["A"] > 0
    if not m.any():
        return 0.0
    return float((np.abs(np.asarray(x, np.float64)[m] - ref["g"][m]) / ref["A"][m]).max())
