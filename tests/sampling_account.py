"""Accounting for hierarchical (inverse-CDF) samples without a discontinuity.  TEST INFRASTRUCTURE ONLY: float64 torch on the CPU.

``sample_pdf`` (nerf_process.py:144-182) is discontinuous in its cdf: a sample whose uniform sits on a ``searchsorted`` edge, or whose
bin sits on the ``denom < 1e-5`` threshold, lands somewhere else in the bin when the cdf is summed in another order.  Comparing sample
with sample therefore needs an allowance for "flips", and an allowance hides a kernel that misplaces a small share of samples.

The forward map, sample -> cdf value, is continuous and monotone.  For one ray take ``bins[B]``, ``weights[B-1]`` and the uniforms
``u[N]`` the implementation consumed, and compute in float64

    p = (w + 1e-5) / sum(w + 1e-5)          c = [0, cumsum(p)]
    F(s) = the piecewise-linear interpolation of (bins_k, c_k), clamped to 0 / 1 outside the hull.

A returned sample ``s`` is ACCOUNTED FOR when

  * it is finite and lies in [bins[0] - eps_s, bins[-1] + eps_s], and
  * the interval [F(s - eps_s) - delta, F(s + eps_s) + delta] contains its ``u``.

``eps_s`` is ``EPS_ULPS`` = 2 fp32 ulps of the row's largest |bin|: the rounding of the final ``b0 + t * (b1 - b0)``.  (In a narrow,
heavy bin one ulp of ``s`` is worth 1e-3 of cdf, so the check is two-sided in ``s`` and not a residual in cdf space.  The oracle needed no
more than 2 ulps in any weight family of this module, at any shape of tests/test_sampling_account_cpu.py.)

``delta = delta_u + flat``:

  * ``delta_u = (B + 3) * 2^-24``.  An fp32 sum of B - 1 non-negative terms whose total is <= 1 is, in ANY order, within
    (B - 1) * 2^-25 of the exact sum (each add rounds by at most half an ulp of a partial sum <= 1, 2^-25); twice that, (B - 1) * 2^-24,
    bounds the reference's order and the kernel's alike.  The other 4 * 2^-24 cover the per-sample arithmetic: the pdf division,
    ``u - c0``, the division by ``denom`` and the product.  3.9e-6 at B = 63, 3.6e-7 at B = 3.  Derived, not measured.
  * ``flat`` is the float64 mass of the bin holding ``s`` when that mass is below 1e-5 + delta_u, else 0.  In such a bin the reference
    either interpolates or, through ``denom = 1``, returns ``b0 + (u - c0) * (b1 - b0)``: both are the reference's answers, and both lie
    within one bin mass of ``u``.

Where two bins coincide (a zero-width bin) F jumps; the lower end of the interval takes F's left limit and the upper end its right limit.

A row whose weights hold a NaN is outside the check; its samples must all be NaN (include/mi_nerf.h, mi_nerf_fine_z), and any that is
not is reported.  Nothing else is exempt: a test tolerates ZERO unaccounted samples.

What the check cannot see: ``searchsorted(right=False)`` against ``right=True`` (a uniform exactly on a cdf entry maps to the same depth
either way), and where inside a flat bin a sample was placed (the reference's own answer is ambiguous there to within ``delta``).
"""
from typing import Callable, Dict, NamedTuple, Optional

import numpy as np
import torch

F64 = torch.float64
EPS_ULPS = 2
FLOOR = 1e-5                   # nerf_process.py:150 and :179


def delta_u(B: int) -> float:
    return (B + 3) * 2.0 ** -24


class Account(NamedTuple):
    bad: torch.Tensor          # bool [n, N]: unaccounted samples
    residual: torch.Tensor     # float64 [n, N]: distance of u from [F(s - eps_s), F(s + eps_s)] (0 inside; inf where s is not finite)
    flat: torch.Tensor         # float64 [n, N]: the flat-bin allowance that applied (0 in steep bins)
    nan_rows: torch.Tensor     # bool [n]: rows outside the check (NaN weights)

    def worst(self) -> str:
        """One line for a test to print: the count, the largest residual in steep bins, the largest in flat bins as a share of the bin mass."""
        ok = ~self.nan_rows[:, None].expand_as(self.bad) & torch.isfinite(self.residual)
        steep = self.residual[ok & (self.flat == 0)]
        fl = ok & (self.flat > 0)
        r_flat = (self.residual[fl] / self.flat[fl]) if bool(fl.any()) else self.residual.new_zeros(0)
        return (f"unaccounted {int(self.bad.sum())}/{self.bad.numel()}, steep-bin residual max {float(steep.max()) if steep.numel() else 0.0:.2e}, "
                f"flat-bin residual / bin mass max {float(r_flat.max()) if r_flat.numel() else 0.0:.2f}")


def _f64(x) -> torch.Tensor:
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.detach().cpu().to(F64)


def _F(bins: torch.Tensor, c: torch.Tensor, x: torch.Tensor, right: bool) -> torch.Tensor:
    """F at x; where bins coincide, the right limit (``right``) or the left limit."""
    B = bins.shape[-1]
    if right:
        k = torch.searchsorted(bins, x, right=True) - 1          # last k with bins_k <= x
        below, above = k < 0, k >= B - 1
    else:
        k = torch.searchsorted(bins, x, right=False) - 1         # bins_k < x <= bins_{k+1}
        below, above = k < 0, k >= B - 1
    k = k.clamp(0, B - 2)
    b0, b1 = torch.gather(bins, -1, k), torch.gather(bins, -1, k + 1)
    c0, c1 = torch.gather(c, -1, k), torch.gather(c, -1, k + 1)
    w = b1 - b0
    t = ((x - b0) / torch.where(w > 0, w, torch.ones_like(w))).clamp(0.0, 1.0)
    f = c0 + t * (c1 - c0)
    f = torch.where(below, torch.zeros_like(f), f)
    return torch.where(above, torch.ones_like(f), f)


def account(bins, weights, u, samples, eps_ulps: int = EPS_ULPS) -> Account:
    """bins [n, B] (sorted, fp32 values), weights [n, B-1], u [n, N] or [N], samples [n, N]."""
    bins32 = bins.detach().cpu().float() if isinstance(bins, torch.Tensor) else torch.from_numpy(np.asarray(bins, np.float32))
    bins, w, s = bins32.to(F64).contiguous(), _f64(weights), _f64(samples)
    n, B = bins.shape
    u = _f64(u).expand(n, s.shape[1]).contiguous()
    assert w.shape == (n, B - 1) and s.shape == u.shape and B >= 2, (bins.shape, w.shape, u.shape, s.shape)
    nan_rows = torch.isnan(w).any(-1)
    w = torch.where(nan_rows[:, None], torch.zeros_like(w), w) + FLOOR
    p = w / w.sum(-1, keepdim=True)
    c = torch.cat([torch.zeros(n, 1, dtype=F64), torch.cumsum(p, -1)], -1)
    c[:, -1] = 1.0
    top = torch.from_numpy(np.spacing(bins32.abs().amax(-1).numpy())).to(F64)
    eps = (eps_ulps * top)[:, None]
    finite = torch.isfinite(s)
    s0 = torch.where(finite, s, bins[:, :1].expand_as(s))
    in_hull = finite & (s0 >= bins[:, :1] - eps) & (s0 <= bins[:, -1:] + eps)
    lo = _F(bins, c, (s0 - eps).contiguous(), right=False)
    hi = _F(bins, c, (s0 + eps).contiguous(), right=True)
    k = (torch.searchsorted(bins, s0.contiguous(), right=True) - 1).clamp(0, B - 2)        # the bin holding s
    mass = torch.gather(p, -1, k)
    du = delta_u(B)
    flat = torch.where(mass < FLOOR + du, mass, torch.zeros_like(mass))
    residual = torch.maximum(torch.maximum(lo - u, u - hi), torch.zeros_like(u))
    residual = torch.where(finite, residual, torch.full_like(residual, float("inf")))
    bad = ~in_hull | (residual > du + flat)
    bad = torch.where(nan_rows[:, None], ~torch.isnan(s), bad)
    return Account(bad, residual, flat, nan_rows)


def unaccounted(bins, weights, u, samples) -> torch.Tensor:
    """bool [n, N]: True where a sample is NOT accounted for (module docstring).  A test asserts that none is."""
    return account(bins, weights, u, samples).bad


# ------------------------------------------------------------------------------------------------------------------------
# the flip counts of the parity tests (sample against sample, with an allowance): what they count
# ------------------------------------------------------------------------------------------------------------------------
def beyond(got, want, tol: float) -> torch.Tensor:
    """bool, elementwise: |got - want| > tol, or either side is not finite (``nan > tol`` is False: a plain comparison counts a NaN as agreeing)."""
    d = (_f64(got) - _f64(want)).abs()
    return ~(d <= tol)


def rays_beyond(got_rgb, want_rgb, tol: float = 1e-4) -> torch.Tensor:
    """bool [n]: rays with a colour channel beyond ``tol`` of the oracle's (or not finite)."""
    return beyond(got_rgb, want_rgb, tol).any(-1)


def bad_rays_without_a_flip(got_rgb, want_rgb, got_z, want_z, rgb_tol: float = 1e-4, z_tol: float = 5e-6) -> torch.Tensor:
    """bool [n]: rays beyond ``rgb_tol`` of the un-pinned oracle whose fine depths all agree with the oracle's to ``z_tol``.  With the depths
    pinned the colour error is bounded far below ``rgb_tol``, so such a ray is a failure and not a sampling outlier: a test asserts there is none."""
    return rays_beyond(got_rgb, want_rgb, rgb_tol) & ~beyond(got_z, want_z, z_tol).any(-1)


# ------------------------------------------------------------------------------------------------------------------------
# weight families: (n, B, seed) -> fp32 [n, B - 1]
# ------------------------------------------------------------------------------------------------------------------------
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def w_soft(n: int, B: int, seed: int) -> torch.Tensor:
    return torch.rand(n, B - 1, generator=_gen(seed))


def w_zero(n: int, B: int, seed: int) -> torch.Tensor:
    return torch.zeros(n, B - 1)


def w_tiny(n: int, B: int, seed: int) -> torch.Tensor:
    return torch.rand(n, B - 1, generator=_gen(seed)) * 1e-7


def w_one_hot(n: int, B: int, seed: int) -> torch.Tensor:
    g = _gen(seed)
    w = torch.zeros(n, B - 1)
    at = torch.randint(0, B - 1, (n, 1), generator=g)
    return w.scatter_(-1, at, 0.2 + 0.8 * torch.rand(n, 1, generator=g))


def w_peak(n: int, B: int, seed: int) -> torch.Tensor:
    """A Gaussian peak 1.5 bins wide (what a trained surface produces): every bin away from it is on the ``denom < 1e-5`` threshold."""
    g = _gen(seed)
    at = torch.rand(n, 1, generator=g) * (B - 1)
    k = torch.arange(B - 1, dtype=torch.float32)[None] + 0.5
    return (0.2 + 0.8 * torch.rand(n, 1, generator=g)) * torch.exp(-0.5 * ((k - at) / 1.5) ** 2)


def w_ends(n: int, B: int, seed: int) -> torch.Tensor:
    g = _gen(seed)
    w = torch.zeros(n, B - 1)
    w[:, 0] = torch.rand(n, generator=g)
    w[:, -1] = torch.rand(n, generator=g)
    return w


FAMILIES: Dict[str, Callable[[int, int, int], torch.Tensor]] = {"soft": w_soft, "zero": w_zero, "tiny": w_tiny, "one_hot": w_one_hot,
                                                                "peak": w_peak, "ends": w_ends}


# ------------------------------------------------------------------------------------------------------------------------
# inputs: depths with one tied pair per row, uniforms that hold the edge values
# ------------------------------------------------------------------------------------------------------------------------
def sorted_depths(n: int, S: int, seed: int, near: float = 2.0, far: float = 6.0, tie: bool = True) -> torch.Tensor:
    """fp32 [n, S], ascending in [near, far]; with ``tie`` the middle pair of every row coincides (S >= 3)."""
    z = torch.sort(near + (far - near) * torch.rand(n, S, generator=_gen(seed)), -1)[0]
    if tie and S >= 3:
        z[:, S // 2] = z[:, S // 2 - 1]
    return z


def edge_uniforms(n: int, N: int, seed: int) -> torch.Tensor:
    """U[0, 1) fp32 [n, N] holding exactly 0 and nextafter(1, 0) in every row (N = 1: in alternate rows)."""
    u = torch.rand(n, N, generator=_gen(seed))
    last = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    if N >= 2:
        u[:, 0], u[:, -1] = 0.0, last
    else:
        u[0::2, 0] = 0.0
        u[1::2, 0] = last
    return u


def det_uniforms(N: int) -> torch.Tensor:
    """The deterministic draw, torch.linspace(0, 1, N) (nerf_process.py:158): holds 0 and, for N >= 2, exactly 1."""
    return torch.linspace(0.0, 1.0, steps=N, dtype=torch.float32)


def mids(z_c: torch.Tensor) -> torch.Tensor:
    """The fine branch's bins (nerf_process.py:63), in fp32 as the kernel computes them."""
    z_c = _f64(z_c).float()
    return 0.5 * (z_c[..., 1:] + z_c[..., :-1])


def fine_account(z_c, weights_c, u: Optional[torch.Tensor], samples) -> Account:
    """The check for the fine branch: bins = mids(z_c), weights = weights_c[1:-1] (B = Sc - 1); ``u`` None = the deterministic draw."""
    s = _f64(samples)
    uu = det_uniforms(s.shape[1]) if u is None else u
    return account(mids(z_c), _f64(weights_c)[..., 1:-1], uu, s)
