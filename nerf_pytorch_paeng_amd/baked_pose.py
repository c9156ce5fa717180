"""Gradients of a radiance-grid render with respect to its rays, and a camera fitted to a grid (THE RAY GRADIENT RULE of
include/mi_nerf_vox.h, libmi_nerf_vox.so).

    rgb, disp, acc, depth = baked_pose.render(grid, rays)                 # grid.render as one autograd node: rays.grad by the rule
    pose, losses = baked_pose.locate(grid, H, W, K, pose0, target)        # the camera of a picture, recovered against the grid

The forward is ``grid.render`` (the same bits); the backward is ``grid.render_backward_rays`` -- mi_vox_render_backward_rays for a dense grid,
mi_vox_render_sparse_backward_rays for a compact one (fp32 or f16 records): one launch, no atomic, bit-identical from run to run.  With
``pose.make_o_d`` upstream the gradient reaches a camera's pose and intrinsics.  A dense grid whose ``sigma`` / ``coef`` require a gradient is
differentiated as well, by ``baked_train.backward`` (a second launch).  There is no fallback: a missing library or a failed call raises
``MiNerfError``.  docs/design/28_grid_ray_gradients.md.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import pose as _pose_mod
from ._lib import MiNerfError
from .baked import RadianceGrid, SparseRadianceGrid


def _check(grid, rays) -> torch.device:
    if not isinstance(grid, RadianceGrid):
        raise MiNerfError(f"a baked.RadianceGrid or baked.SparseRadianceGrid expected, got {type(grid).__name__}")
    grid._need()
    grid._need_unsigned("baked_pose (THE RAY GRADIENT RULE)")
    dev = grid.sigma.device
    if dev.type != "cuda":
        raise MiNerfError(f"the grid must live on a HIP device (got {dev}); this path has no CPU fallback")
    if not isinstance(rays, torch.Tensor) or rays.dim() != 2 or rays.shape[1] != 6:
        raise MiNerfError(f"rays [n,6] expected, got {tuple(rays.shape) if isinstance(rays, torch.Tensor) else type(rays).__name__}")
    if rays.device != dev:
        raise MiNerfError(f"rays live on {rays.device}, the grid on {dev}")
    return dev


def _trains(grid) -> bool:
    """A dense grid whose arrays ask for a gradient."""
    return not isinstance(grid, SparseRadianceGrid) and (grid.sigma.requires_grad or grid.coef.requires_grad)


class _Render(torch.autograd.Function):
    """rays -> (rgb, disp, acc, depth); sigma and coef are the dense grid's own tensors (or None), passed so that the node hangs on them."""

    @staticmethod
    def forward(ctx, rays, sigma, coef, grid, kw):
        rays = rays.detach().contiguous()
        ctx.grid, ctx.rays, ctx.kw = grid, rays, kw
        rgb, disp, acc, depth = grid.render(rays, **kw)
        ctx.mark_non_differentiable(disp)
        return rgb, disp, acc, depth

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rgb, _g_disp, g_acc, g_depth):
        grid, rays = ctx.grid, ctx.rays
        n = rays.shape[0]
        g_rgb = torch.zeros(n, 3, dtype=torch.float32, device=rays.device) if g_rgb is None else g_rgb.contiguous()
        g_acc, g_depth = (None if t is None else t.contiguous() for t in (g_acc, g_depth))
        d_rays = grid.render_backward_rays(rays, g_rgb, g_acc, g_depth, **ctx.kw) if ctx.needs_input_grad[0] else None
        d_sigma = d_coef = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            from . import baked_train
            d_sigma, d_coef = baked_train.backward(grid, rays, g_rgb, g_acc, g_depth, **ctx.kw)
        return d_rays, d_sigma, d_coef, None, None


def render(grid: RadianceGrid, rays: torch.Tensor, step: Optional[float] = None, near: float = 0.0, far: float = math.inf, T_min: float = 0.0,
           bg=(1.0, 1.0, 1.0), skip: bool = True):
    """(rgb [n,3], disp [n], acc [n], depth [n]) as ``grid.render`` gives them, differentiable with respect to ``rays`` [n,6] where they
    require a gradient: one autograd node whose backward is ``grid.render_backward_rays``.  ``grid`` is a RadianceGrid or a
    SparseRadianceGrid of either storage.  For a dense grid whose ``sigma`` / ``coef`` require a gradient the node also fills theirs
    (``baked_train.backward``, a second launch).  ``disp`` is detached.  Without ``requires_grad`` on the rays (and on a dense grid's arrays),
    or under ``no_grad``, it is ``grid.render``.  The node differentiates once: a second differentiation raises."""
    _check(grid, rays)
    kw = dict(step=step, near=near, far=far, T_min=T_min, bg=tuple(float(v) for v in bg), skip=bool(skip))
    trains = _trains(grid)
    if not (torch.is_grad_enabled() and (rays.requires_grad or trains)):
        return grid.render(rays, **kw)
    return _Render.apply(rays, grid.sigma if trains else None, grid.coef if trains else None, grid, kw)


def locate(grid: RadianceGrid, H: int, W: int, K, pose0, target: torch.Tensor, steps: int = 200, batch: int = 1024, lr_rot: float = 2e-3,
           lr_trans: float = 5e-3, pixels: Optional[torch.Tensor] = None, seed: int = 0, step: Optional[float] = None, near: float = 0.0,
           far: float = math.inf, T_min: float = 0.0, bg=(1.0, 1.0, 1.0), skip: bool = True):
    """The camera of a picture, fitted to the grid: ``steps`` Adam steps on a ``pose.CameraRefiner(1)`` (axis-angle ``lr_rot``, translation
    ``lr_trans``) from ``pose0`` [3,4] or [4,4], each on a seeded batch of ``batch`` pixels drawn on the device from ``pixels`` (int64 indices
    y * W + x; None: the whole image): ``pose.make_o_d`` -> ``baked_pose.render`` -> the mean squared error against ``target`` [H,W,3] or
    [H*W,3].  Returns (pose [3,4], losses [steps]), both device tensors: no loss is read back, and
    the one host read of a step is ``pose.make_o_d``'s own, which takes the pose's twelve floats by value as it does on the network path.
    The grid is not changed."""
    if not isinstance(grid, RadianceGrid):
        raise MiNerfError(f"a baked.RadianceGrid or baked.SparseRadianceGrid expected, got {type(grid).__name__}")
    grid._need()
    grid._need_unsigned("baked_pose (THE RAY GRADIENT RULE)")
    dev = grid.sigma.device
    if dev.type != "cuda":
        raise MiNerfError(f"the grid must live on a HIP device (got {dev}); this path has no CPU fallback")
    H, W = int(H), int(W)
    if not isinstance(target, torch.Tensor) or target.numel() != H * W * 3 or target.device != dev:
        raise MiNerfError(f"target [{H},{W},3] on {dev} expected")
    if steps < 0 or batch < 1:
        raise MiNerfError(f"steps={steps} >= 0 and batch={batch} >= 1 expected")
    target = target.detach().float().reshape(H * W, 3)
    if pixels is None:
        pixels = torch.arange(H * W, dtype=torch.int64, device=dev)
    elif not isinstance(pixels, torch.Tensor) or pixels.dtype != torch.int64 or pixels.dim() != 1 or pixels.numel() < 1 or pixels.device != dev:
        raise MiNerfError(f"pixels: a non-empty int64 vector of indices y * W + x on {dev} expected")
    base = torch.as_tensor(pose0).detach().to(device=dev, dtype=torch.float32)[:3, :4].contiguous()
    refiner = _pose_mod.CameraRefiner(1).to(dev)
    opt = torch.optim.Adam([dict(params=[refiner.rot], lr=lr_rot), dict(params=[refiner.trans], lr=lr_trans)])
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    kw = dict(step=step, near=near, far=far, T_min=T_min, bg=bg, skip=skip)
    P = pixels.numel()
    losses = []
    for _ in range(int(steps)):
        pix = pixels[torch.randint(P, (min(int(batch), P),), generator=gen, device=dev)].contiguous()
        o, d = _pose_mod.make_o_d(W, H, K, refiner(0, base), pixels=pix)
        rgb = render(grid, torch.cat([o, d], -1), **kw)[0]
        loss = torch.mean((rgb - target[pix]) ** 2)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    with torch.no_grad():
        found = refiner(0, base).detach()
    return found, (torch.stack(losses) if losses else torch.zeros(0, dtype=torch.float32, device=dev))
