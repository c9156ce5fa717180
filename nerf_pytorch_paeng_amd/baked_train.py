"""Training a radiance grid against images: the backward pass of the grid renderer (include/mi_nerf_voxgrad.h, libmi_nerf_voxgrad.so).

    grid = baked.RadianceGrid(-1.2, 1.2, 128, B=9).bake(model)           # or .allocate(dev): an empty grid, trained from nothing (skip=False)
    losses = baked_train.finetune(grid, rays, target, steps=300)         # Adam on sigma and coef against the images' rgb
    rgb, disp, acc, depth = baked_train.render(grid, rays)               # one autograd node, for a loss of one's own
    tv = baked_train.lattice_tv(grid, "sigma", mask=True, scale=1e-4)    # the priors a grid trained from nothing wants: total variation and
    sp = baked_train.lattice_sparsity(grid, scale=1e-4)                  # Cauchy sparsity, value returned, gradient ADDED into .grad
    grid, losses = baked_train.coarse_to_fine(grid, rays, target, [(64, 200), (128, 200)], prune=1.0, skip=(False, True))   # train coarse, resample, prune, go on

The forward is ``grid.render`` (libmi_nerf_vox.so); the backward is mi_voxgrad_render_backward, which recomputes the march and ADDS
dL/d sigma and dL/d coef by THE BACKWARD RULE of the header.  Its sums are fp32 hardware atomic adds: unlike every other entry of the
package, the gradient is not bit-identical from run to run (docs/design/23_radiance_grid_training.md).  The regularisers are THE LATTICE
REGULARISERS of include/mi_nerf_geo.h (libmi_nerf_geo.so): gathers without an atomic, bit-identical from run to run
(docs/design/24_lattice_regularisers.md).  Dense fp32 grids only; there is no
fallback: a missing library or a failed call raises ``MiNerfError``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _geo, _voxgrad, ops
from .optim import LazyAdam
from ._lib import MiNerfError, dev_ptr, stream_ptr
from .baked import RadianceGrid, SparseRadianceGrid, Views


def _check_grid(grid) -> torch.device:
    if isinstance(grid, SparseRadianceGrid):
        raise MiNerfError("a SparseRadianceGrid has no dense record array to differentiate: fine-tune the dense grid, then compact()")
    if not isinstance(grid, RadianceGrid):
        raise MiNerfError(f"a baked.RadianceGrid expected, got {type(grid).__name__}")
    grid._need()
    dev = grid.sigma.device
    if dev.type != "cuda":
        raise MiNerfError(f"the grid must live on a HIP device (got {dev}); this path has no CPU fallback")
    return dev


def _check(grid, rays) -> torch.device:
    dev = _check_grid(grid)
    if not isinstance(rays, torch.Tensor) or rays.dim() != 2 or rays.shape[1] != 6:
        raise MiNerfError(f"rays [n,6] expected, got {tuple(rays.shape) if isinstance(rays, torch.Tensor) else type(rays).__name__}")
    if rays.device != dev:
        raise MiNerfError(f"rays live on {rays.device}, the grid on {dev}")
    return dev


def backward(grid: RadianceGrid, rays: torch.Tensor, g_rgb: torch.Tensor, g_acc: Optional[torch.Tensor] = None, g_depth: Optional[torch.Tensor] = None,
             d_sigma: Optional[torch.Tensor] = None, d_coef: Optional[torch.Tensor] = None, step: Optional[float] = None, near: float = 0.0,
             far: float = math.inf, T_min: float = 0.0, bg=(1.0, 1.0, 1.0), skip: bool = True, check: bool = False):
    """mi_voxgrad_render_backward: ADDS the gradients of rays [n,6] under g_rgb [n,3] (and g_acc, g_depth [n]) into ``d_sigma`` / ``d_coef``
    (zeros of the grid's shapes when not given) and returns them; ``check=True`` appends the forward the backward recomputed,
    (rgb [n,3], acc [n], depth [n])."""
    dev = _check(grid, rays)
    n = rays.shape[0]
    if tuple(g_rgb.shape) != (n, 3) or any(t is not None and tuple(t.shape) != (n,) for t in (g_acc, g_depth)):
        raise MiNerfError(f"g_rgb [{n},3] and g_acc, g_depth [{n}] expected")
    d_sigma = torch.zeros_like(grid.sigma) if d_sigma is None else d_sigma
    d_coef = torch.zeros_like(grid.coef) if d_coef is None else d_coef
    if d_sigma.shape != grid.sigma.shape or d_coef.shape != grid.coef.shape:
        raise MiNerfError(f"d_sigma {tuple(grid.sigma.shape)} and d_coef {tuple(grid.coef.shape)} expected")
    cfg = _voxgrad.RenderCfg(float(0.5 * grid.cell_edge() if step is None else step), float(near), float(far), float(T_min),
                             (C.c_float * 3)(*(float(v) for v in bg)), int(bool(skip)))
    g = _voxgrad.Grid((C.c_float * 3)(*grid.lo), (C.c_float * 3)(*grid.hi), (C.c_int32 * 3)(*grid.res))
    rgb = torch.empty(n, 3, dtype=torch.float32, device=dev) if check else None
    acc, depth = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2)) if check else (None, None)
    with ops._guard(dev):
        _voxgrad.check(_voxgrad.lib().mi_voxgrad_render_backward(
            C.byref(g), grid.B, dev_ptr(grid.sigma.detach(), "sigma"), dev_ptr(grid.coef.detach(), "coef", torch.float32, 16),
            dev_ptr(grid.skip, "skip", torch.uint8, 1), dev_ptr(rays, "rays"), n, C.byref(cfg), dev_ptr(g_rgb, "g_rgb"), dev_ptr(g_acc, "g_acc"),
            dev_ptr(g_depth, "g_depth"), dev_ptr(d_sigma, "d_sigma"), dev_ptr(d_coef, "d_coef", torch.float32, 16), dev_ptr(rgb, "rgb_check"),
            dev_ptr(acc, "acc_check"), dev_ptr(depth, "depth_check"), stream_ptr(dev)), "mi_voxgrad_render_backward")
    return (d_sigma, d_coef, rgb, acc, depth) if check else (d_sigma, d_coef)


class _Render(torch.autograd.Function):
    """sigma and coef are the grid's own tensors, passed so that the node hangs on them."""

    @staticmethod
    def forward(ctx, sigma, coef, grid, rays, kw):
        ctx.grid, ctx.rays, ctx.kw = grid, rays, kw
        rgb, disp, acc, depth = grid.render(rays, **kw)
        ctx.mark_non_differentiable(disp)
        return rgb, disp, acc, depth

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rgb, _g_disp, g_acc, g_depth):
        grid = ctx.grid
        n = ctx.rays.shape[0]
        g_rgb = torch.zeros(n, 3, dtype=torch.float32, device=ctx.rays.device) if g_rgb is None else g_rgb.contiguous()
        g_acc, g_depth = (None if t is None else t.contiguous() for t in (g_acc, g_depth))
        d_sigma, d_coef = backward(grid, ctx.rays, g_rgb, g_acc, g_depth, **ctx.kw)
        return d_sigma, d_coef, None, None, None


def render(grid: RadianceGrid, rays: torch.Tensor, step: Optional[float] = None, near: float = 0.0, far: float = math.inf, T_min: float = 0.0,
           bg=(1.0, 1.0, 1.0), skip: bool = True):
    """(rgb [n,3], disp [n], acc [n], depth [n]) as ``grid.render`` gives them, differentiable with respect to ``grid.sigma`` and
    ``grid.coef`` where those require a gradient: one autograd node whose backward fills ``grid.sigma.grad`` / ``grid.coef.grad``.  ``disp``
    is detached and the rays carry no gradient.  Without ``requires_grad`` on either tensor, or under ``no_grad``, it is ``grid.render``.
    The node differentiates once: a second differentiation raises."""
    _check(grid, rays)
    kw = dict(step=step, near=near, far=far, T_min=T_min, bg=tuple(float(v) for v in bg), skip=bool(skip))
    if not (torch.is_grad_enabled() and (grid.sigma.requires_grad or grid.coef.requires_grad)):
        return grid.render(rays, **kw)
    return _Render.apply(grid.sigma, grid.coef, grid, rays.detach().contiguous(), kw)


# ---------------------------------------------------------------------------------------------------
# THE LATTICE REGULARISERS (include/mi_nerf_geo.h)
# ---------------------------------------------------------------------------------------------------
def _lattice(grid: RadianceGrid, kind: str, which: str, eps: float, mask, scale: Optional[float], out: Optional[torch.Tensor], value: bool):
    """One call of mi_geo_lattice_tv / mi_geo_lattice_sparsity on ``grid.sigma`` or ``grid.coef``: the gradient is added when ``scale`` is
    given, the value is formed (and returned) when ``value``."""
    dev = _check_grid(grid)
    if which not in ("sigma", "coef") or (kind == "sparsity" and which != "sigma"):
        raise MiNerfError(f"which={which!r}: 'sigma' or 'coef' expected (the sparsity prior is on sigma alone)")
    v = (grid.sigma if which == "sigma" else grid.coef).detach()
    R, Cn = (1, 1) if which == "sigma" else (grid.record_floats, 3 * grid.B)
    align = 4 if R == 1 else 16
    if mask is True:
        mask = grid.skip
    elif mask is False:
        mask = None
    if mask is not None and (not isinstance(mask, torch.Tensor) or tuple(mask.shape) != tuple(grid.skip_shape) or mask.device != dev):
        raise MiNerfError(f"mask: None, True (the grid's skip plane) or a uint8 tensor {tuple(grid.skip_shape)} on {dev} expected")
    grad = None
    if scale is not None:
        owner = grid.sigma if which == "sigma" else grid.coef
        if out is None:
            if owner.grad is None:
                owner.grad = torch.zeros_like(owner)
            out = owner.grad
        if not isinstance(out, torch.Tensor) or out.shape != v.shape:
            raise MiNerfError(f"out {tuple(v.shape)} expected, got {tuple(out.shape) if isinstance(out, torch.Tensor) else type(out).__name__}")
        grad = out
    elif out is not None:
        raise MiNerfError("out is given without a scale: nothing would be added to it")
    P = (C.c_int32 * 3)(*grid.points)
    L = _geo.lib()
    val = scratch = None
    nbytes = 0
    if value:
        nbytes = int(L.mi_geo_lattice_scratch_bytes(P, R, Cn))
        if nbytes == 0:
            raise MiNerfError(f"the lattice {grid.points} x {R} is refused by mi_geo_lattice_scratch_bytes")
        val = torch.empty((), dtype=torch.float64, device=dev)
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    sc = 0.0 if scale is None else float(scale)
    with ops._guard(dev):
        if kind == "tv":
            _geo.check(L.mi_geo_lattice_tv(P, R, Cn, dev_ptr(v, which, torch.float32, align), dev_ptr(mask, "mask", torch.uint8, 1), float(eps), sc,
                                           dev_ptr(grad, "out", torch.float32, align), dev_ptr(val, "value", torch.float64, 8),
                                           dev_ptr(scratch, "scratch", torch.float64, 8), nbytes, stream_ptr(dev)), "mi_geo_lattice_tv")
        else:
            _geo.check(L.mi_geo_lattice_sparsity(P, dev_ptr(v, which), dev_ptr(mask, "mask", torch.uint8, 1), sc, dev_ptr(grad, "out"),
                                                 dev_ptr(val, "value", torch.float64, 8), dev_ptr(scratch, "scratch", torch.float64, 8), nbytes,
                                                 stream_ptr(dev)), "mi_geo_lattice_sparsity")
    return val


def lattice_tv(grid: RadianceGrid, which: str = "sigma", eps: float = 1e-8, mask=None, scale: Optional[float] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mi_geo_lattice_tv on ``grid.sigma`` (``which="sigma"``) or on the 3 B counted floats of ``grid.coef`` (``"coef"``): the total
    variation as a 0-dim float64 device tensor.  With ``scale`` the gradient times ``scale`` is ADDED into ``out`` (default: the tensor's
    ``.grad``, created as zeros if absent).  ``mask``: None (every point counts), True (``grid.skip``) or a uint8 tensor of its shape."""
    return _lattice(grid, "tv", which, eps, mask, scale, out, True)


def lattice_sparsity(grid: RadianceGrid, mask=None, scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mi_geo_lattice_sparsity on ``grid.sigma``: sum of log1p(2 sigma^2) over the counted points, as a 0-dim float64 device tensor; with
    ``scale`` the gradient times ``scale`` is ADDED into ``out`` (default ``grid.sigma.grad``).  ``mask`` as for ``lattice_tv``."""
    return _lattice(grid, "sparsity", "sigma", 0.0, mask, scale, out, True)


def _regularise(grid: RadianceGrid, masked: bool, n_points: int, tv_sigma: float, tv_coef: float, sparsity: float, tv_eps: float) -> None:
    """finetune's regularisers: their gradients are ADDED into ``grid.sigma.grad`` / ``grid.coef.grad``; a weight of 0 makes no call."""
    plane = True if masked else None
    if tv_sigma:
        _lattice(grid, "tv", "sigma", tv_eps, plane, tv_sigma / n_points, None, False)
    if tv_coef:
        _lattice(grid, "tv", "coef", tv_eps, plane, tv_coef / (n_points * 3 * grid.B), None, False)
    if sparsity:
        _lattice(grid, "sparsity", "sigma", 0.0, plane, sparsity / n_points, None, False)


def finetune(grid: RadianceGrid, rays: torch.Tensor, target: torch.Tensor, steps: int, batch: int = 4096, lr_sigma: float = 0.05, lr_coef: float = 0.005,
             optimizer=torch.optim.Adam, rebuild_skip_every: int = 1, seed: int = 0, step: Optional[float] = None, near: float = 0.0,
             far: float = math.inf, T_min: float = 0.0, bg=(1.0, 1.0, 1.0), skip: bool = True, tv_sigma: float = 0.0, tv_coef: float = 0.0,
             sparsity: float = 0.0, tv_eps: float = 1e-8, sigma_floor: Optional[float] = None) -> torch.Tensor:
    """``steps`` optimiser steps on ``grid.sigma`` (lr_sigma) and ``grid.coef`` (lr_coef) against target [N,3], the rgb of rays [N,6]: a
    seeded batch of ``batch`` rays drawn on the device per step, the mean squared error on rgb, and ``sigma.clamp_(min=0)`` after every
    step.  Returns the per-step losses [steps] as a device tensor: nothing synchronises with the host.

    The skip plane describes the sigma that is rendered at every step: ``grid.build_skip()`` runs every ``rebuild_skip_every`` steps and at
    the end, a step that follows a rebuild renders with the plane (``skip=True``), and the steps between two rebuilds render without it
    (exact, slower).  With the plane, a sample in an empty block contributes no gradient (the header's rule per sample): density grows
    outwards from where there is some, block margin by block margin.  ``skip=False`` never uses the plane -- the setting for a grid that
    starts empty (``allocate()``), where the plane would hide every sample.

    The default rates suit a baked grid: the colours move, the density barely does.  Adam steps every touched element by about its rate
    whatever the gradient's size, so a large ``lr_sigma`` on small batches fills the empty space next to surfaces with noise (measured in
    docs/design/23_radiance_grid_training.md, with the gain from larger batches); a grid trained from nothing wants a larger one.

    ``tv_sigma``, ``tv_coef``, ``sparsity`` (>= 0) weigh THE LATTICE REGULARISERS: between ``loss.backward()`` and the optimiser's step the
    gradients of ``tv_sigma TV(sigma) / N``, ``tv_coef TV(coef) / (N 3 B)`` and ``sparsity SP / N`` are added, N the number of lattice
    points (known on the host: nothing synchronises), ``tv_eps`` the eps of the total variation.  Their mask is ``grid.skip`` on the steps that
    render with the plane and none otherwise.  The returned losses stay the data loss; with all three weights 0 no regulariser is
    called.

    ``optimizer=optim.LazyAdam`` takes THE DIRECT PATH (docs/design/26_lazy_optimizer.md): ``.grad`` of both tensors becomes a zero buffer
    once; a step renders under ``no_grad``, forms ``g_rgb = 2 (rgb - target) / (3 n)`` itself, has ``backward`` and the regularisers add
    straight into those buffers, and ends in ``LazyAdam.step`` with ``clamp_min=0`` on sigma and ``consume=True``, which updates the touched
    elements and leaves the buffers zero.  No ``zero_grad``, no ``clamp_``, no autograd node, no ``zeros_like``: nothing sweeps the grid
    but the optimiser's read of the gradients.  An element no ray reaches stays what it is, moments included.

    A SIGNED GRID (``grid.signed``; include/mi_nerf_vox.h) is trained by the same steps with the ReLU after the interpolation in the
    forward and in the backward (the Signed paragraph of THE BACKWARD RULE), and WITHOUT the clamp at 0: sigma keeps its sign, the
    autograd path runs no ``clamp_`` and LazyAdam's ``clamp_min`` is None -- or ``sigma_floor`` (<= 0, signed grids only), an optional
    lower bound on sigma that keeps a point the optimiser pushes away from being pushed out of reach.  The skip plane is rebuilt by the
    signed builder.  There is no gain factor between the stored plane and the density: Adam's step is in parameter units, so a plane of
    amplitude c trained with ``lr_sigma = c r`` follows the same trajectory as one of amplitude 1 with ``lr_sigma = r`` -- choose
    ``lr_sigma`` in units of the plane's amplitude."""
    if not all(isinstance(w, (int, float)) and math.isfinite(w) and w >= 0 for w in (tv_sigma, tv_coef, sparsity)):
        raise MiNerfError(f"tv_sigma={tv_sigma}, tv_coef={tv_coef} and sparsity={sparsity} must be finite numbers >= 0")
    dev = _check(grid, rays)
    if sigma_floor is not None and not (grid.signed and isinstance(sigma_floor, (int, float)) and math.isfinite(sigma_floor) and sigma_floor <= 0):
        raise MiNerfError(f"sigma_floor={sigma_floor!r}: a finite number <= 0, for a signed grid only")
    floor = (None if sigma_floor is None else float(sigma_floor)) if grid.signed else 0.0      # the lower bound on sigma after a step
    N = rays.shape[0]
    if not isinstance(target, torch.Tensor) or tuple(target.shape) != (N, 3) or target.device != dev:
        raise MiNerfError(f"target [{N},3] on {dev} expected")
    if steps < 0 or batch < 1 or rebuild_skip_every < 1:
        raise MiNerfError(f"steps={steps} >= 0, batch={batch} >= 1 and rebuild_skip_every={rebuild_skip_every} >= 1 expected")
    n_points = grid.points[0] * grid.points[1] * grid.points[2]
    rays, target = rays.detach().float().contiguous(), target.detach().float()
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    was = (grid.sigma.requires_grad, grid.coef.requires_grad)
    grid.sigma.requires_grad_(True)
    grid.coef.requires_grad_(True)
    opt = optimizer([dict(params=[grid.sigma], lr=lr_sigma), dict(params=[grid.coef], lr=lr_coef)])
    lazy = isinstance(opt, LazyAdam)
    losses = []
    try:
        if lazy:                                                             # the direct path: no dense sweep of the grid per step
            opt.param_groups[0]["clamp_min"] = floor                         # sigma >= 0 (a signed grid: no bound, or sigma_floor), applied where the step lands
            opt.consume = True                                               # the step leaves the gradients zero: no zero_grad
            grid.sigma.grad, grid.coef.grad = torch.zeros_like(grid.sigma), torch.zeros_like(grid.coef)
            kw = dict(step=step, near=near, far=far, T_min=T_min, bg=tuple(float(v) for v in bg))
        for it in range(steps):
            fresh = it % rebuild_skip_every == 0
            if fresh and skip:
                grid.build_skip()
            idx = torch.randint(N, (min(batch, N),), generator=gen, device=dev)
            if lazy:
                with torch.no_grad():
                    r = rays[idx]
                    rgb = grid.render(r, skip=skip and fresh, **kw)[0]
                    diff = rgb - target[idx]
                    loss = torch.mean(diff ** 2)
                    backward(grid, r, (diff * (2.0 / (3 * r.shape[0]))).contiguous(), d_sigma=grid.sigma.grad, d_coef=grid.coef.grad,
                             skip=skip and fresh, **kw)
                    _regularise(grid, skip and fresh, n_points, tv_sigma, tv_coef, sparsity, tv_eps)
                    opt.step()
                losses.append(loss)
                continue
            rgb = render(grid, rays[idx], step=step, near=near, far=far, T_min=T_min, bg=bg, skip=skip and fresh)[0]
            loss = torch.mean((rgb - target[idx]) ** 2)
            opt.zero_grad(set_to_none=False)
            loss.backward()
            _regularise(grid, skip and fresh, n_points, tv_sigma, tv_coef, sparsity, tv_eps)
            opt.step()
            if floor is not None:
                with torch.no_grad():
                    grid.sigma.clamp_(min=floor)
            losses.append(loss.detach())
    finally:
        grid.sigma.requires_grad_(was[0])
        grid.coef.requires_grad_(was[1])
        grid.sigma.grad = grid.coef.grad = None
    grid.build_skip()
    return torch.stack(losses) if losses else torch.zeros(0, dtype=torch.float32, device=dev)


# ---------------------------------------------------------------------------------------------------
# coarse to fine: THE RESAMPLING RULE and THE PRUNING RULE of include/mi_nerf_vox.h between runs of finetune
# ---------------------------------------------------------------------------------------------------
PER_LEVEL = ("lr_sigma", "lr_coef", "batch", "skip")


def _per_level(name: str, v, n: int) -> list:
    """One value for every level, or one per level."""
    if isinstance(v, (list, tuple)):
        if len(v) != n:
            raise MiNerfError(f"{name}: one value or one per level ({n}) expected, got {len(v)}")
        return list(v)
    return [v] * n


def coarse_to_fine(grid: RadianceGrid, rays: torch.Tensor, target: torch.Tensor, levels, prune=None, prune_views=None, prune_T: float = 1e-3,
                   **finetune_kw):
    """Train through ``levels``, a sequence of (res, steps): per level the grid is resampled to ``res`` (``grid.resample``; not when it has
    that resolution already), ``finetune`` runs ``steps`` steps with a fresh optimiser, and with ``prune`` the level ends in
    ``grid.prune(tau)`` -- ``prune`` one tau or one per level (None: that level is not pruned).  ``lr_sigma``, ``lr_coef``, ``batch`` and
    ``skip`` may each be one value or one per level (a grid that starts empty wants ``skip=False`` on its first level only: after it the
    skip plane describes what was learnt); every other keyword goes to ``finetune`` as it is.  Returns (the final grid, the levels' losses
    concatenated as one device tensor).  The grid handed in is trained in place on the levels before the first resample and untouched
    afterwards.  Nothing synchronises with the host.
    With ``prune_views`` (a ``baked.Views``: the training cameras) every level that is pruned is pruned by visibility as well:
    ``grid.prune(tau, seen=grid.seen(prune_views), T_vis=prune_T)``, THE SEEN PRUNING RULE (``prune=None`` then stands for tau = 0 at
    every level).  Without it nothing changes."""
    dev = _check(grid, rays)
    levels = [tuple(lv) if isinstance(lv, (list, tuple)) else lv for lv in levels]
    if not levels or any(not isinstance(lv, tuple) or len(lv) != 2 for lv in levels):
        raise MiNerfError(f"levels: a sequence of (res, steps) pairs expected, got {levels!r}")
    n = len(levels)
    if "steps" in finetune_kw:
        raise MiNerfError("steps are given per level, in levels")
    if prune_views is not None and not isinstance(prune_views, Views):
        raise MiNerfError(f"prune_views: a baked.Views expected, got {type(prune_views).__name__}")
    taus = _per_level("prune", 0.0 if prune is None and prune_views is not None else prune, n)
    for tau in taus:
        if tau is not None and not (isinstance(tau, (int, float)) and math.isfinite(tau) and tau >= 0):
            raise MiNerfError(f"prune={prune!r}: each tau must be a finite number >= 0 (or None)")
    each = {k: _per_level(k, finetune_kw.pop(k), n) for k in PER_LEVEL if k in finetune_kw}
    losses = []
    for i, (res, steps) in enumerate(levels):
        res3 = tuple(int(r) for r in res) if isinstance(res, (list, tuple)) else (int(res),) * 3
        if res3 != tuple(grid.res):
            grid = grid.resample(res3)
        losses.append(finetune(grid, rays, target, steps=int(steps), **{k: v[i] for k, v in each.items()}, **finetune_kw))
        if taus[i] is not None:
            if prune_views is None:
                grid.prune(taus[i])
            else:
                grid.prune(taus[i], seen=grid.seen(prune_views), T_vis=prune_T)
    return grid, (torch.cat(losses) if losses else torch.zeros(0, dtype=torch.float32, device=dev))
