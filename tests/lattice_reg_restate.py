"""THE LATTICE REGULARISERS of include/mi_nerf_geo.h restated in numpy, operation by operation in the header's order, written from the header
and not from the kernel.  ``dtype=np.float32`` is what the library must equal bit for bit (numpy's float32 +, -, *, / and sqrt are single
correctly rounded operations and nothing is contracted); ``dtype=np.float64`` is the same rule in double, which the CPU tests hold against
central differences of its own value.

Every function returns a dict: ``d`` (the array d_v after the add), ``g`` (the gradient per counted channel), ``written`` (which points
are written at all), ``terms`` (the per-term values in ``dtype``, 0 where a term is not counted), ``value`` (their float64 sum by
math.fsum, i.e. exactly rounded) and ``count`` (the number of counted terms)."""
import math

import numpy as np


def mask_shape(P):
    return tuple(-(-(int(p) - 1) // 8) for p in P)


def counted(P, mask):
    """bool [P_z, P_y, P_x]: mask is None or mask[block(p)] != 0, block(p)_a = min(p_a, P_a - 2) >> 3."""
    P = tuple(int(p) for p in P)
    if mask is None:
        return np.ones(P, bool)
    mask = np.asarray(mask)
    assert mask.shape == mask_shape(P) and mask.dtype == np.uint8, (mask.shape, mask_shape(P))
    b = [np.minimum(np.arange(p), p - 2) >> 3 for p in P]
    return mask[b[0][:, None, None], b[1][None, :, None], b[2][None, None, :]] != 0


def _shift(a, axis):
    """a at p - e_axis (zeros where p_axis == 0)."""
    out = np.zeros_like(a)
    dst = [slice(None)] * a.ndim
    src = [slice(None)] * a.ndim
    dst[axis], src[axis] = slice(1, None), slice(None, -1)
    out[tuple(dst)] = a[tuple(src)]
    return out


def tv(v, C, eps, mask=None, scale=None, d_v=None, dtype=np.float32):
    """v [P_z, P_y, P_x, R] (or [P_z, P_y, P_x] for the plane); C counted channels."""
    v = np.asarray(v)
    plane = v.ndim == 3
    if plane:
        v = v[..., None]
        d_v = None if d_v is None else np.asarray(d_v)[..., None]
    P = v.shape[:3]
    w = v[..., :C].astype(dtype)
    eps = dtype(eps)
    d = []
    for axis in (2, 1, 0):                                           # d_x, d_y, d_z: forward differences, exactly 0 at the last point
        da = np.zeros_like(w)
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[axis], hi[axis] = slice(None, -1), slice(1, None)
        da[tuple(lo)] = w[tuple(hi)] - w[tuple(lo)]
        d.append(da)
    dx, dy, dz = d
    t = np.sqrt(((eps + dx * dx) + dy * dy) + dz * dz)
    cnt = counted(P, mask)
    cnt4 = cnt[..., None]
    zero = dtype(0.0)
    own = np.where(cnt4, -(((dx + dy) + dz) / t), zero)
    b = []
    for da, axis in ((dx, 2), (dy, 1), (dz, 0)):                      # b_a = d_a(p - e_a) / t(p - e_a) where p_a >= 1 and p - e_a is counted
        b.append(_shift(np.where(cnt4, da / t, zero), axis))
    g = ((own + b[0]) + b[1]) + b[2]
    written = cnt | _shift(cnt, 2) | _shift(cnt, 1) | _shift(cnt, 0)
    out = None
    if scale is not None:
        out = np.array(d_v, dtype=dtype, copy=True)
        new = out[..., :C] + dtype(scale) * g
        out[..., :C] = np.where(written[..., None], new, out[..., :C])
        if plane:
            out = out[..., 0]
    terms = np.where(cnt4, t, zero)
    return dict(d=out, g=g, written=written, terms=terms, value=math.fsum(terms.astype(np.float64).ravel().tolist()), count=int(cnt.sum()) * C)


def sparsity(sigma, mask=None, scale=None, d_sigma=None, dtype=np.float32):
    """sigma [P_z, P_y, P_x]."""
    s = np.asarray(sigma).astype(dtype)
    cnt = counted(s.shape, mask)
    g = (dtype(4.0) * s) / (dtype(1.0) + (dtype(2.0) * s) * s)
    out = None
    if scale is not None:
        out = np.array(d_sigma, dtype=dtype, copy=True)
        out = np.where(cnt, out + dtype(scale) * g, out)
    sd = s.astype(np.float64)                                         # the term: sigma widened, 2 sigma^2 formed in double, log1p in double
    terms = np.where(cnt, np.log1p((2.0 * sd) * sd), 0.0)
    return dict(d=out, g=g, written=cnt, terms=terms, value=math.fsum(terms.ravel().tolist()), count=int(cnt.sum()))
