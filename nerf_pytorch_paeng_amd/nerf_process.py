"""Volume-rendering hot path -- drop-in for the reference's nerf_process.py (252 lines).

Same function names, positional arguments and return structures as the reference
(``batchify_rays_and_render_by_chunk``, ``render_rays``, ``pre_process``, ``post_process``,
``sample_pdf``, ``ndc_rays``), executed by hand-written HIP kernels through ``libmi_nerf.so``.
Keyword-only extras (``t_rand=``, ``u=``, ``seed=``, ``ray_offset=``) make the randomness explicit;
``occupancy=`` (an ``occupancy.OccupancyGrid``) skips the networks at samples the grid marks empty (inference only;
``train_occupancy=`` is the same grid for the training path, the node's route of occupancy_train.py):
the reference draws unseeded ``torch.rand`` (nerf_process.py:58-60,162-163); here the default is a
counter-based generator keyed on (seed, global ray index, sample index), so a frame renders
identically however its rays are chunked or sharded across GPUs.

Under ``torch.no_grad()`` (test.py:36,140) this is the forward-only inference path.  With gradients enabled
and a model whose parameters require them (train.py:53-70) the same entry points run the training path
(train_path.py): same kernels plus an activation stash, hand-written backward behind one autograd node.
Inputs are borrowed, outputs are fresh fp32 tensors on the inputs' device.
``opts`` fields read: near, far, N_samples_c, N_samples_f, perturb, chunk_rays, data_type
(gpu_ids / rank / chunk_pts are accepted and unused: the device comes from the tensors and the fused
kernel never materialises the [n_pts, 90] network input that chunk_pts exists to bound).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import ops
from ._lib import MiNerfError, as_f32_dev
from .weights import PackedNeRF, packed_for
from . import train_path
from . import occupancy as occ
from . import occupancy_train
from . import geometry as geo

# rays handed to one mi_nerf_render_rays call (workspace: 5.4 KB/ray at 64+128 samples -> ~5.6 GB)
MAX_RAYS_PER_LAUNCH = 1 << 20

_rng = {"seed": 0, "calls": 0}


def manual_seed(seed: int) -> None:
    """Seed the default jitter generator (the reference is unseeded and irreproducible)."""
    _rng["seed"], _rng["calls"] = int(seed), 0


def _next_seed(seed: Optional[int]) -> int:
    if seed is not None:
        return int(seed)
    s = (_rng["seed"] * 0x9E3779B1 + _rng["calls"]) & 0xFFFFFFFF
    _rng["calls"] += 1
    return s


_det = ops.deterministic


# --------------------------------------------------------------------------------------------------
def ndc_rays(H, W, focal, near, rays_o, rays_d):
    """NDC warp for forward-facing scenes (nerf_process.py:8-28)."""
    lead = rays_d.shape[:-1]
    d = as_f32_dev(rays_d).reshape(-1, 3)
    o = rays_o.to(torch.float32) if rays_o.dtype != torch.float32 else rays_o
    o = o.expand(rays_d.shape).reshape(-1, 3) if o.shape != rays_d.shape else o.reshape(-1, 3)
    if isinstance(focal, torch.Tensor):
        focal = float(focal.item())
    oo, dd = ops.ndc_rays(int(H), int(W), float(focal), float(near), o, d)
    return oo.reshape(*lead, 3), dd.reshape(*lead, 3)


def sample_pdf(bins, weights, N_samples, det=False, opts=None, *, u=None):
    """Hierarchical inverse-CDF sampling (nerf_process.py:144-182).  ``u`` [n, N_samples] injects the
    uniforms; by default they come from the counter-based generator."""
    assert opts is not None                                         # nerf_process.py:147
    bins, weights = as_f32_dev(bins), as_f32_dev(weights, bins.device)
    lead = bins.shape[:-1]
    b2, w2 = bins.reshape(-1, bins.shape[-1]), weights.reshape(-1, weights.shape[-1])
    if not det:
        u = (ops.fill_uniform(_next_seed(None), 1, 0, b2.shape[0], int(N_samples), bins.device) if u is None
             else as_f32_dev(u, bins.device).reshape(-1, int(N_samples)))
    out = ops.sample_pdf(b2, w2, int(N_samples), bool(det), u)
    return out.reshape(*lead, int(N_samples))


def pre_process(rays, posenc, opts, z_vals=None, weights=None, isFine=False, *, t_rand=None, u=None):
    """Sample depths and build the network input (nerf_process.py:32-85).
    Returns ``(embedded [n*S, 90], z_vals [n, S], rays_d [n, 3])``."""
    rays = as_f32_dev(rays)
    n = rays.shape[0]
    L_x, L_d = int(getattr(posenc[0], "L", 10)), int(getattr(posenc[1], "L", 4))
    if not isFine:
        if t_rand is None:
            t_rand = ops.fill_uniform(_next_seed(None), 0, 0, n, int(opts.N_samples_c), rays.device)
        z = ops.stratified_z(float(opts.near), float(opts.far), as_f32_dev(t_rand, rays.device))
    else:
        det = _det(opts)
        if not det and u is None:
            u = ops.fill_uniform(_next_seed(None), 1, 0, n, int(opts.N_samples_f), rays.device)
        z = ops.fine_z(as_f32_dev(z_vals, rays.device), as_f32_dev(weights, rays.device), int(opts.N_samples_f), det,
                       None if det else as_f32_dev(u, rays.device))
    embedded = ops.embed(rays, z, L_x, L_d)
    return embedded, z, rays[:, 3:]


class _Composite(torch.autograd.Function):
    """post_process, differentiable in rgb_map, acc_map and depth_map, and in weights when ``weights_grad``.  A loss that reads the colours
    alone (train.py:60-66) gets d rgb_map -> d raw from mi_nerf_composite_backward; one that reads the others too, from
    mi_geo_composite_backward (geometry.py).  disp is returned without a graph (it passes through a max, a NaN filter and a clamp)."""

    @staticmethod
    def forward(ctx, raw, z, d, weights_grad=False):
        rgb, disp, acc, wts, depth = ops.composite(raw, z, d, want_all=True)
        ctx.save_for_backward(raw, z, d)
        ctx.mark_non_differentiable(*((disp,) if weights_grad else (disp, wts)))
        ctx.set_materialize_grads(False)
        return rgb, disp, acc, wts, depth

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_acc, g_wts, g_depth):
        if g_rgb is None and g_acc is None and g_wts is None and g_depth is None:
            return None, None, None, None
        raw, z, d = ctx.saved_tensors
        if g_acc is None and g_wts is None and g_depth is None:
            return ops.composite_backward(raw, z, d, g_rgb.contiguous().float()), None, None, None
        g_rgb, g_acc, g_wts, g_depth = (None if g is None else g.contiguous().float() for g in (g_rgb, g_acc, g_wts, g_depth))
        # no distortion term here: the normalising bounds are not read
        return geo.composite_geo_backward(raw, z, d, 0.0, 1.0, g_rgb, g_acc, g_depth, None, g_wts), None, None, None


def post_process(outputs, z_vals, rays_d, *, weights_grad: bool = False):
    """Alpha compositing (nerf_process.py:89-140) -> (rgb_map, disp_map, acc_map, weights, depth_map).
    Differentiable in ``rgb_map``, ``acc_map`` and ``depth_map`` w.r.t. ``outputs`` when they carry a graph; ``weights_grad=True`` makes the
    per-sample ``weights`` differentiable too (without the keyword they are returned without a graph, as they always were)."""
    z = as_f32_dev(z_vals)
    raw = as_f32_dev(outputs, z.device)
    d = as_f32_dev(rays_d, z.device)
    if torch.is_grad_enabled() and raw.requires_grad:
        return _Composite.apply(raw, z.detach(), d.detach(), bool(weights_grad))
    return ops.composite(raw, z, d, want_all=True)


raw2outputs = post_process          # north-star alias (original NeRF naming)


def run_network(model, embedded, is_fine: bool = False):
    """north-star alias: the chunked ``model(embedded)`` loop of nerf_process.py:190-192,206-207 as one launch."""
    if train_path.wants_grad(model):
        return model(embedded, is_fine)                          # differentiable route of the model mirror (model/NeRF.py)
    packed = packed_for(model)
    return ops.mlp_embedded(packed.net, packed.blob(is_fine), as_f32_dev(embedded, packed.device))


# --------------------------------------------------------------------------------------------------
def _render(rays: torch.Tensor, packed: PackedNeRF, opts, t_rand, u, seed: int, ray_offset: int, prec: ops.Precision,
            intermediates: bool, occupancy=None, geometry: bool = False) -> Dict[str, torch.Tensor]:
    n = rays.shape[0]
    dev = rays.device
    Sc, Nf = int(opts.N_samples_c), int(opts.N_samples_f)
    det = _det(opts)
    # jitter: explicit tensors when the caller injects them (or wants them back); otherwise the kernels draw it themselves from the
    # same counter-based generator, keyed on (seed, ray_offset + ray, sample) -- identical values, no tensors, no extra launches
    cfg = ops.render_cfg(float(opts.near), float(opts.far), Sc, Nf, det, seed=seed, ray_offset=ray_offset)
    cfg.mode = prec.mode
    if t_rand is not None:
        t_rand = as_f32_dev(t_rand, dev)
    elif intermediates:
        t_rand = ops.fill_uniform(seed, 0, ray_offset, n, Sc, dev)
    if Nf > 0 and not det:
        if u is not None:
            u = as_f32_dev(u, dev)
        elif intermediates:
            u = ops.fill_uniform(seed, 1, ray_offset, n, Nf, dev)
    else:
        u = None
    net, blob_c, blob_f = packed.kernel_blobs(prec)
    stats = None
    if occupancy is None:
        rgb_c, disp_c, rgb_f, disp_f, ws = ops.render_rays(net, blob_c, blob_f if Nf > 0 else None, cfg, rays, t_rand, u)
        views = ops.workspace_views
    else:
        rgb_c, disp_c, rgb_f, disp_f, ws, stats = occ.render_rays(net, blob_c, blob_f if Nf > 0 else None, cfg, occupancy, rays, t_rand, u)
        occupancy.last_stats = occ.add_stats(occupancy.last_stats, stats)
        views = occ.workspace_views
    out = {"rgb_c": rgb_c, "disp_c": disp_c}                        # nerf_process.py:215-216
    if Nf > 0:
        out["rgb_f"], out["disp_f"] = rgb_f, disp_f
    if geometry:                                                    # the six geometry outputs from the raw / z the pass left in its workspace
        v = views(cfg, n, ws)
        for key in ("c", "f") if Nf > 0 else ("c",):
            extra = geo.composite_geo(v["raw_" + key], v["z_" + key], rays, float(opts.near), float(opts.far))
            out.update({name + "_" + key: t for name, t in zip(geo.EXTRA_KEYS, (extra[2], extra[4], extra[5]))})
    if intermediates:
        for k, v in views(cfg, n, ws).items():
            out["_" + k] = v
        out["_t_rand"], out["_u"] = t_rand, u
        if stats is not None:
            out["_occ_stats"] = stats
    return out


def _occupancy_arg(occupancy, training: bool, prec: ops.Precision):
    """``occupancy=``: None (today's path), or an OccupancyGrid -- inference only, one kernel family (fp32 / f16s / bf16) for both networks."""
    if occupancy is None:
        return None
    if training:
        raise MiNerfError("occupancy= is an inference feature (call under torch.no_grad(), or freeze the model); to train with a grid pass it as "
                          "train_occupancy=")
    if not isinstance(occupancy, occ.OccupancyGrid):
        raise MiNerfError(f"occupancy must be an occupancy.OccupancyGrid, got {type(occupancy).__name__}")
    occ.check_precision(prec)
    occupancy.last_stats = None
    return occupancy


def _train_occupancy_arg(grid, training: bool, prec: ops.Precision):
    """``train_occupancy=``: None, or an OccupancyGrid for the training path (occupancy_train.py) -- gradients enabled, fp32 or f16s."""
    if grid is None:
        return None
    occupancy_train.check_grid(grid)
    if not training:
        raise MiNerfError("train_occupancy= is a training feature: gradients are disabled or no parameter of the model requires them "
                          "(under torch.no_grad() render with occupancy=)")
    if prec.coarse != prec.fine or prec.fine not in ("fp32", "f16s"):
        raise MiNerfError(f"training with a grid runs fp32 or f16s for both networks (got coarse {prec.coarse}, fine {prec.fine})")
    grid.last_stats = None
    return grid


def _train_f16s(prec: ops.Precision, intermediates: bool = False) -> bool:
    """The training path's precision: True = split precision (f16s forward, fp32 backward), False = fp32.  It has no other mode."""
    if prec.fine not in ("fp32", "f16s") or intermediates:
        raise MiNerfError("the training path has no bf16 / f16 mode (fp32, or f16s=True: split-precision forward, fp32 backward) and returns no intermediates")
    return prec.fine == "f16s"


def _geometry_kw(geometry, ray_grad=False) -> Dict[str, bool]:
    """No keyword means today's call, argument for argument."""
    return {**({"geometry": True} if geometry else {}), **({"ray_grad": True} if ray_grad else {})}


def _render_train(rays, model, opts, train_occupancy, t_rand, u, seed: int, ray_offset: int, f16s: bool, geometry, ray_grad):
    """The training call of ``render_rays`` and of every slab: one node, its route through the grid when ``train_occupancy`` is one
    (what occupancy_train.render_train calls)."""
    grid = {} if train_occupancy is None else {"grid": train_occupancy}
    return train_path.render_train(rays, model, opts, t_rand=t_rand, u=u, seed=seed, ray_offset=ray_offset, f16s=f16s,
                                   **_geometry_kw(geometry, ray_grad), **grid)


def _ray_grad_arg(ray_grad, train_occupancy) -> bool:
    if ray_grad and train_occupancy is not None:
        raise MiNerfError(train_path.RAY_GRAD_WITH_GRID)
    return bool(ray_grad)


def render_rays(rays, model, posenc, opts, *, t_rand=None, u=None, seed=None, ray_offset: int = 0, bf16: bool = False,
                return_intermediates: bool = False, f16s: bool = False, coarse_f16s: bool = False, f16: bool = False, coarse_f16: bool = False,
                occupancy=None, train_occupancy=None, geometry: bool = False, ray_grad: bool = False):
    """Coarse pass -> composite -> resample -> fine pass (nerf_process.py:185-216) as one fused launch
    sequence.  Returns ``{'rgb_c','disp_c'[,'rgb_f','disp_f']}``; ``geometry=True`` adds ``acc_*``, ``depth_*`` and ``distortion_*`` [n] per
    network (geometry.py), differentiable outputs of the training node when gradients are enabled.  ``bf16`` / ``f16s`` / ``coarse_f16s`` / ``f16`` / ``coarse_f16`` select
    the networks' precision mode (ops.precision(); fp32 MFMA by default).  With gradients: fp32 or f16s.  ``occupancy``: an OccupancyGrid
    (occupancy.py) -- the networks skip the samples it marks empty; ``return_intermediates`` then also returns ``_occ_stats``.
    ``train_occupancy``: the same for the training path (gradients enabled; fp32 or f16s); the counts are in the grid's ``last_stats``.
    ``ray_grad``: rays that require grad receive their gradient from the training node (pose.py), also when the model is frozen."""
    prec = ops.precision(bf16, f16s, coarse_f16s, f16, coarse_f16)
    ray_grad = _ray_grad_arg(ray_grad, train_occupancy)
    training = train_path.wants_grad(model) or train_path.wants_ray_grad(model, ray_grad, rays)
    occupancy = _occupancy_arg(occupancy, training, prec)
    train_occupancy = _train_occupancy_arg(train_occupancy, training, prec)
    if training:
        train_f16s = _train_f16s(prec, return_intermediates)
        if rays.dim() != 2 or rays.shape[1] != 6:
            raise MiNerfError(f"rays must be [n, 6] (o, d), got {tuple(rays.shape)}")
        return _render_train(rays, model, opts, train_occupancy, t_rand, u, _next_seed(seed), int(ray_offset), train_f16s, geometry, ray_grad)
    packed = packed_for(model)
    rays = as_f32_dev(rays, packed.device)
    if rays.dim() != 2 or rays.shape[1] != 6:
        raise MiNerfError(f"rays must be [n, 6] (o, d), got {tuple(rays.shape)}")
    if occupancy is not None and rays.shape[0] > occ.MAX_RAYS_PER_LAUNCH:
        raise MiNerfError(f"render_rays with a grid takes at most {occ.MAX_RAYS_PER_LAUNCH} rays per call (batchify_rays_and_render_by_chunk slabs them)")
    return _render(rays, packed, opts, t_rand, u, _next_seed(seed), int(ray_offset), prec, return_intermediates, occupancy, **_geometry_kw(geometry))


def batchify_rays_and_render_by_chunk(ray_o, ray_d, model, posenc, H, W, K, opts, *, t_rand=None, u=None, seed=None,
                                      ray_offset: int = 0, bf16: bool = False, f16s: bool = False, coarse_f16s: bool = False, f16: bool = False,
                                      coarse_f16: bool = False, occupancy=None, train_occupancy=None, geometry: bool = False,
                                      ray_grad: bool = False):
    """Drop-in entry point (nerf_process.py:220-252): flatten, optional NDC warp for llff, render.
    Returns ``(rgb_c [N,3], disp_c [N], rgb_f [N,3] | None, disp_f [N] | None)``; with ``geometry=True`` a fifth element, the dict of
    ``acc_*`` / ``depth_*`` / ``distortion_*`` [N] that ``render_rays(..., geometry=True)`` adds, concatenated over the slabs.

    ``opts.chunk_rays`` bounded the reference's activation memory; the fused kernels keep activations in
    registers, so rays are launched in slabs of up to MAX_RAYS_PER_LAUNCH.  The result does not depend on
    the slab size because the jitter is keyed on the global ray index (``ray_offset`` + position).
    ``occupancy``: an OccupancyGrid (occupancy.py); its ``last_stats`` then holds the sample counts of this call.  ``train_occupancy``: the
    same for the training path (occupancy_train.py).  ``ray_grad``: ``ray_o`` / ``ray_d`` that require grad receive their gradient (through
    the NDC warp too, for llff), also when the model is frozen."""
    prec = ops.precision(bf16, f16s, coarse_f16s, f16, coarse_f16)
    ray_grad = _ray_grad_arg(ray_grad, train_occupancy)
    training = train_path.wants_grad(model) or train_path.wants_ray_grad(model, ray_grad, ray_o, ray_d)
    occupancy = _occupancy_arg(occupancy, training, prec)
    train_occupancy = _train_occupancy_arg(train_occupancy, training, prec)
    train_f16s = _train_f16s(prec) if training else False
    packed = None if training else packed_for(model)
    dev = next(model.parameters()).device if training else packed.device
    ray_d = as_f32_dev(ray_d, dev)
    flat_d = ray_d.reshape(-1, 3)
    ray_o = ray_o.to(dev) if ray_o.device != dev else ray_o
    flat_o = ray_o.to(torch.float32).expand(ray_d.shape).reshape(-1, 3)     # nerf_process.py:221 (accepts the stride-0 view)
    if getattr(opts, "data_type", None) == "llff":                  # nerf_process.py:224-226
        k00 = K[0][0]
        focal = float(k00.item()) if isinstance(k00, torch.Tensor) else float(k00)
        if ray_grad:
            from . import pose
            flat_o, flat_d = pose.ndc_rays(H, W, focal, 1.0, flat_o, flat_d)
        else:
            flat_o, flat_d = ndc_rays(H, W, focal, 1.0, flat_o, flat_d)
    rays = torch.cat((flat_o, flat_d), dim=-1)                      # nerf_process.py:229
    N = rays.shape[0]
    seed = _next_seed(seed)
    Nf = int(opts.N_samples_f)
    parts = []
    train_stats = None
    slab = train_path.MAX_TRAIN_RAYS if training else (MAX_RAYS_PER_LAUNCH if occupancy is None else occ.MAX_RAYS_PER_LAUNCH)
    for i in range(0, N, slab):
        j = min(N, i + slab)
        tr, uu = (None if t_rand is None else t_rand[i:j]), (None if u is None else u[i:j])
        if training:                                                # train.py:53-54: one autograd node per slab
            parts.append(_render_train(rays[i:j].contiguous(), model, opts, train_occupancy, tr, uu, seed, int(ray_offset) + i, train_f16s, geometry,
                                       ray_grad))
            if train_occupancy is not None:
                train_stats = occ.add_stats(train_stats, train_occupancy.last_stats)
        else:
            parts.append(_render(rays[i:j], packed, opts, tr, uu, seed, int(ray_offset) + i, prec, False, occupancy, **_geometry_kw(geometry)))
    if train_occupancy is not None:
        train_occupancy.last_stats = train_stats
    def cat(key):
        return parts[0][key] if len(parts) == 1 else torch.cat([p[key] for p in parts], dim=0)
    res = (cat("rgb_c"), cat("disp_c"), cat("rgb_f"), cat("disp_f")) if Nf > 0 else (cat("rgb_c"), cat("disp_c"), None, None)
    if geometry:
        return (*res, {name + "_" + key: cat(name + "_" + key) for key in (("c", "f") if Nf > 0 else ("c",)) for name in geo.EXTRA_KEYS})
    return res
