"""Training with an occupancy grid: ``train_path._RenderTrain`` with the grid in it (docs/design/17_occupancy_training.md).

Per network the forward is  compact | ops.mlp_rays_train on the (n', 32) pseudo-rays | scatter_raw | ops.composite  (ops.fine_z after the
coarse pass, unchanged), the backward  ops.composite_backward on the scattered raw | gather_raw | ops.mlp_backward on the tiles with the
stash of the forward.  A skipped sample's raw is (0, 0, 0, 0) as in the inference path, so the step is the full staged step with raw zeroed
where ``grid.mark`` answers 0 and d_raw dropped there; a padding lane evaluates a real point with d_raw = 0 and adds exactly zero to every
weight-gradient and bias sum.  The networks are driven from here through the public staged entries: libmi_nerf_occ.so calls none of the
training entries of libmi_nerf.so.  One 8-byte device -> host read per network pass (the tile count sizes the network launch).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import geometry as geo
from . import occupancy as occ
from . import ops
from ._lib import MiNerfError, as_f32_dev
from .train_path import _state_for, _TrainState, node_outputs

TILE = 32


def check_grid(grid) -> "occ.OccupancyGrid":
    if not isinstance(grid, occ.OccupancyGrid):
        raise MiNerfError(f"train_occupancy must be an occupancy.OccupancyGrid, got {type(grid).__name__}")
    return grid


class _RenderTrainOcc(torch.autograd.Function):
    """rays (+ explicit randomness), the grid and the two networks' parameters -> rgb_c, disp_c, rgb_f, disp_f (+ the six geometry outputs
    with ``cfg["geometry"]``, as train_path._RenderTrain)."""

    @staticmethod
    def forward(ctx, st: _TrainState, grid, rays, cfg: Dict, t_rand, u, z_override, stats: Dict, *params):
        n_each = len(st.names)
        net = st.net
        Nf, det = cfg["Nf"], cfg["det"]
        f16s = bool(cfg.get("f16s", False))

        def forward_net(which, flat, blob, z):
            c = grid.compact(rays, z, which)                         # the one host read of the pass
            n_t = c["tiles"]
            key = "c" if which == "coarse" else "f"
            stats["total_" + key] += z.numel()
            stats["evaluated_" + key] += c["survivors"]
            stats["padded_" + key] += n_t * TILE - c["survivors"]
            if n_t == 0:                                             # nothing survived: no network launch, raw is all zeros
                empty = torch.empty(0, TILE, 4, dtype=torch.float32, device=rays.device)
                return occ.scatter_raw(empty, c["slot"]), c, torch.empty(0, dtype=torch.uint8, device=rays.device)
            ops.train_layout(net, n_t, TILE)                         # asked before anything is sized: a shape the kernels refuse raises here
            if f16s:
                blob_fwd = ops.pack_apply_f16s(net, st.map_f16s(), flat, st.f16s_out_of_range)
                raw_t, stash = ops.mlp_rays_train(net, blob_fwd, c["tile_rays"], c["tile_z"], f16s=True)
            else:
                raw_t, stash = ops.mlp_rays_train(net, blob, c["tile_rays"], c["tile_z"])
            return occ.scatter_raw(raw_t, c["slot"]), c, stash

        flat_c = st.flat(params[:n_each])
        blob_c = ops.pack_apply(st.map_fwd, flat_c)
        z_c = ops.stratified_z(cfg["near"], cfg["far"], t_rand) if z_override is None else z_override[0]
        raw_c, cc, stash_c = forward_net("coarse", flat_c, blob_c, z_c)
        rgb_c, disp_c, w_c, extra_c = geo.node_forward(cfg, raw_c, z_c, rays, True)
        ctx.st, ctx.Nf, ctx.f16s, ctx.cfg = st, Nf, f16s, cfg
        saved = [rays, flat_c, blob_c, z_c, raw_c, stash_c, cc["tile_rays"], cc["tile_z"], cc["tile_src"]]
        if Nf > 0:
            flat_f = st.flat(params[n_each:])
            blob_f = ops.pack_apply(st.map_fwd, flat_f)
            z_f = ops.fine_z(z_c, w_c, Nf, det, None if det else u) if (z_override is None or z_override[1] is None) else z_override[1]
            raw_f, cf, stash_f = forward_net("fine", flat_f, blob_f, z_f)
            rgb_f, disp_f, _, extra_f = geo.node_forward(cfg, raw_f, z_f, rays, False)
            saved += [flat_f, blob_f, z_f, raw_f, stash_f, cf["tile_rays"], cf["tile_z"], cf["tile_src"]]
        else:
            rgb_f = torch.empty(0, 3, device=rays.device)
            disp_f = torch.empty(0, device=rays.device)
            extra_f = tuple(torch.empty(0, device=rays.device) for _ in extra_c)
        ctx.save_for_backward(*saved)
        ctx.mark_non_differentiable(disp_c, disp_f)
        ctx.set_materialize_grads(False)
        return (rgb_c, disp_c, rgb_f, disp_f, *extra_c, *extra_f)

    @staticmethod
    def backward(ctx, g_rgb_c, g_disp_c, g_rgb_f, g_disp_f, *g_extra):
        st: _TrainState = ctx.st
        net = st.net
        saved = ctx.saved_tensors
        rays = saved[0]
        f16s = ctx.f16s and net.W == 256
        launched = False
        g_extra_c, g_extra_f = g_extra[:len(g_extra) // 2], g_extra[len(g_extra) // 2:]

        def one(flat, blob, z, raw, stash, tile_rays, tile_z, tile_src, g_rgb, g_ext) -> List[Optional[torch.Tensor]]:
            nonlocal launched
            if g_rgb is None and all(g is None for g in g_ext):
                return [None] * len(st.names)
            n_t = tile_src.shape[0]
            if n_t == 0:                                             # no sample was evaluated: the parameters did not reach the colours
                return st.split_grads(torch.zeros(st.n_flat, dtype=torch.float32, device=rays.device))
            f16s_dgrad = f16s and ops.f16s_dgrad_fits(net)
            blob_b = ops.pack_apply_f16s(net, st.map_bwd_f16s(), flat, st.f16s_out_of_range, backward=True) if f16s_dgrad else ops.pack_apply(st.map_bwd, flat)
            d_raw = geo.node_backward(ctx.cfg, raw, z, rays, g_rgb, g_ext)
            d_tiles = occ.gather_raw(d_raw, tile_src)
            grads, work = ops.mlp_backward(net, blob, blob_b, tile_rays, tile_z, d_tiles, stash, f16s_wgrad=f16s, f16s_dgrad=f16s_dgrad)
            if f16s:
                st.note_f16s_backward(work, n_t, TILE)
                launched = True
            return st.split_grads(grads)

        gc = one(*saved[1:9], g_rgb_c, g_extra_c)
        gf = one(*saved[9:17], g_rgb_f, g_extra_f) if ctx.Nf > 0 else [None] * len(st.names)
        if launched:
            st.end_f16s_step()                                       # both nets' range words are folded: read them at the cadence
        return (None, None, None, None, None, None, None, None, *gc, *gf)


def new_stats() -> Dict[str, int]:
    return {k: 0 for k in ("total_c", "evaluated_c", "padded_c", "total_f", "evaluated_f", "padded_f")}


def render_train(rays: torch.Tensor, model: torch.nn.Module, opts, grid, *, t_rand=None, u=None, seed: int = 0, ray_offset: int = 0,
                 z_override=None, det: Optional[bool] = None, f16s: bool = False, geometry: bool = False) -> Dict[str, torch.Tensor]:
    """``train_path.render_train`` with an occupancy grid: same arguments, same defaults for drawn jitter, same outputs.  The sample counts
    of the call go into ``grid.last_stats`` (the keys of mi_occ_stats)."""
    check_grid(grid)
    st = _state_for(model, f16s)
    dev = st.device
    if isinstance(rays, torch.Tensor) and rays.requires_grad:
        raise MiNerfError("rays require grad: the training path differentiates w.r.t. the MLP parameters only (the reference trains "
                          "nothing else, main.py:79-80); detach the rays, or a gradient would be dropped silently")
    bits = grid._need_bits()
    if bits.device != dev:
        raise MiNerfError(f"the occupancy grid lives on {bits.device}, the model on {dev}")
    rays = as_f32_dev(rays, dev)
    n = rays.shape[0]
    Sc, Nf = int(opts.N_samples_c), int(opts.N_samples_f)
    if det is None:
        p = getattr(opts, "perturb", 1.0)
        det = isinstance(p, (int, float)) and p == 0.0
    t_rand = ops.fill_uniform(seed, 0, ray_offset, n, Sc, dev) if t_rand is None else as_f32_dev(t_rand, dev)
    if Nf > 0 and not det:
        u = ops.fill_uniform(seed, 1, ray_offset, n, Nf, dev) if u is None else as_f32_dev(u, dev)
    else:
        u = None
    cfg = {"near": float(opts.near), "far": float(opts.far), "Sc": Sc, "Nf": Nf, "det": bool(det), "f16s": bool(f16s), "geometry": bool(geometry)}
    params = st.params(model.model_coarse) + st.params(model.model_fine)
    stats = new_stats()
    rgb_c, disp_c, rgb_f, disp_f, *extra = _RenderTrainOcc.apply(st, grid, rays, cfg, t_rand, u, z_override, stats, *params)
    grid.last_stats = stats
    return node_outputs(rgb_c, disp_c, rgb_f, disp_f, extra, Nf)
