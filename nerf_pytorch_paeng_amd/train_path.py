"""Training step of the hot path -- what the reference gets from autograd for train.py:53-70.

``batchify_rays_and_render_by_chunk`` routes here when gradients are enabled and the model's parameters
require them.  The forward runs the same kernels as inference (the MLP in its STASH variant, which also
keeps every layer's activations), wrapped in ONE ``torch.autograd.Function`` whose inputs are the model's
parameters; the backward is hand-written HIP (composite backward, backward-data chain, backward-weights)
and returns one gradient per parameter, so ``loss.backward(); optimizer.step()`` work unchanged
(train.py:69-70).  PyTorch does the bookkeeping (graph node, parameter ``.grad`` accumulation, the
optimizer); no PyTorch kernel touches the activations.

Semantics copied from the reference: only ``rgb_c`` / ``rgb_f`` carry gradient; the fine depths are
detached (nerf_process.py:66), so the fine loss does not reach the coarse network; disparity outputs are
not differentiable here (the reference's loss never reads them, train.py:60-66).

The node, ``_RenderTrain``, owns everything around the two networks once: parameters -> blobs, depths, compositing, what is saved, which
gradients arrived, the split-precision bookkeeping.  How one network's samples reach the kernels is a route handed to it: ``Dense``
evaluates every sample, occupancy_train.Compacted only those an occupancy grid keeps (``render_train(..., grid=)``).
"""
from __future__ import annotations

import weakref
from typing import Dict, List, Optional

import torch

from . import geometry as geo
from . import ops
from ._lib import MiNerfError, Net, as_f32_dev
from .weights import _param_shape, infer_net, pad_index_map, padded_train_net

# rays per autograd node: the activation stash is ~9.9 KB per sample point (W = 256, D = 8)
MAX_TRAIN_RAYS = 16384

# The split-precision backward runs on d_raw * s with ~256x of f16 headroom (FP16_OVFL: conversions clip at 65504, never inf), and the
# split-precision packers cannot represent a weight beyond the f16 range: both failure modes are silent on the device.  Every f16s backward
# folds what it saw into three device words of the model's state (no host synchronisation); they are READ -- one device -> host copy -- on
# after the LAST backward launch of the first F16S_CHECK_FIRST training steps (a step = one _RenderTrain.backward: the coarse and the fine net's
# launches together, so the fine net's words are in the first read) and then every F16S_CHECK_EVERY-th step, and a saturated chain or an
# unrepresentable weight then raises (or warns, by F16S_ON_SATURATION).  By the time a later read raises, up to F16S_CHECK_EVERY - 1
# optimizer.step() calls have already applied clipped gradients: the message says so.  f16s_status(model) reads the words on demand (without
# resetting them unless asked); harness.train() returns them in its dict.
F16S_CHECK_EVERY = 50
F16S_CHECK_FIRST = 3
F16S_ON_SATURATION = "raise"          # or "warn"
F16_MAX = 65504.0


class _TrainState:
    """Per-model constants of the training path: network shape and the device-side pack maps."""

    def __init__(self, model: torch.nn.Module, device: torch.device, f16s: bool = False):
        sd = model.state_dict()
        # net_model: the module's own shape (model/NeRF.py:24-30); net: what the training kernels run -- the same, or for a width without
        # training kernels (--netWidth 64, config.py:57) the next wider one, parameters scattered into zeros (weights.pad_index_map)
        self.net_model: Net = infer_net(sd)
        # ... which depends on the precision: the split-precision kernels exist for W = 256 only (one state per kernel width, _state_for)
        self.net: Net = padded_train_net(self.net_model, f16s)
        self.pad_idx = None if self.net is self.net_model else pad_index_map(self.net_model, self.net).to(device)
        self.n_flat = ops.param_count(self.net)
        self.device = device
        self.names = ops.param_names(self.net)
        self.map_fwd = ops.pack_map(self.net, False).to(device)
        self.map_bwd = ops.pack_map(self.net, True).to(device)
        self._map_f16s = None
        self.f16s_out_of_range = None          # device counter: weights the split-precision packer could not represent (NaN / beyond f16)
        self.f16s_range = None                 # device [2]: running max of (max |d_raw|, max |delta * s|) over the f16s backwards since the last read
        self.f16s_steps = 0                    # f16s training steps (backward passes) so far (host count; sets the read cadence)
        self.f16s_steps_since_read = 0

    def map_f16s(self) -> torch.Tensor:
        """Gather map of the split-precision blob, built on first use (f16s=True training forward)."""
        if self._map_f16s is None:
            self._map_f16s = ops.pack_map_f16s(self.net).to(self.device)
            self._map_bwd_f16s = ops.pack_map_f16s(self.net, backward=True).to(self.device)
            self.f16s_out_of_range = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.f16s_range = torch.zeros(2, dtype=torch.float32, device=self.device)
        return self._map_f16s

    def note_f16s_backward(self, work: torch.Tensor, n_rays: int, S: int) -> None:
        """Fold the range words the split-precision backward left in ``work`` into the running maximum (device side; no host sync)."""
        if n_rays == 0:
            return                                 # an empty slab launches nothing: there are no words to fold
        torch.maximum(self.f16s_range, ops.backward_range_words(self.net, n_rays, S, work), out=self.f16s_range)

    def end_f16s_step(self) -> None:
        """After the last backward launch of a training step: at the cadence, read the words and complain."""
        self.f16s_steps += 1
        self.f16s_steps_since_read += 1
        if self.f16s_steps <= int(F16S_CHECK_FIRST) or self.f16s_steps % max(1, int(F16S_CHECK_EVERY)) == 0:
            self.check_f16s()

    def read_f16s(self, reset: bool = True) -> Dict[str, float]:
        """One device -> host read of the three words: {"max_abs_d_raw", "max_abs_delta_scaled", "weights_out_of_range", "saturated"}."""
        if self.f16s_range is None:
            return {"max_abs_d_raw": 0.0, "max_abs_delta_scaled": 0.0, "weights_out_of_range": 0, "saturated": False}
        both = torch.cat([self.f16s_range, self.f16s_out_of_range.float()]).cpu()
        if reset:
            self.f16s_range.zero_()
            self.f16s_out_of_range.zero_()
            self.f16s_steps_since_read = 0
        d, ds, oor = float(both[0]), float(both[1]), int(both[2])
        return {"max_abs_d_raw": d, "max_abs_delta_scaled": ds, "weights_out_of_range": oor, "saturated": bool(ds >= F16_MAX or ds != ds or oor > 0)}

    def check_f16s(self) -> Dict[str, float]:
        steps = self.f16s_steps_since_read
        r = self.read_f16s()
        if r["saturated"]:
            msg = (f"split-precision training step out of range: max |delta * s| = {r['max_abs_delta_scaled']:.4g} (f16 max {F16_MAX:.0f}; max |d_raw| = "
                   f"{r['max_abs_d_raw']:.4g}), {r['weights_out_of_range']} weight(s) beyond the f16 range, within the last {steps} training step(s) "
                   f"(this one included): their gradients were clipped, and the optimizer has already applied up to {max(0, steps - 1)} of them.  "
                   f"Train with the fp32 backward (precision 'fp32') or scale the loss down.")
            if F16S_ON_SATURATION == "warn":
                import warnings
                warnings.warn(msg, RuntimeWarning, stacklevel=3)
            else:
                raise MiNerfError(msg)
        return r

    def map_bwd_f16s(self) -> torch.Tensor:
        self.map_f16s()
        return self._map_bwd_f16s

    def forward_blob(self, flat: torch.Tensor, f16s: bool = False) -> torch.Tensor:
        """The weight stream a forward launch reads, re-packed on the device from the flat vector: the fp32 one, or the split-precision one."""
        if f16s:
            return ops.pack_apply_f16s(self.net, self.map_f16s(), flat, self.f16s_out_of_range)
        return ops.pack_apply(self.map_fwd, flat)

    def backward_blob(self, flat: torch.Tensor, f16s_dgrad: bool = False) -> torch.Tensor:
        """The transposed stream of the backward-data chain: the fp32 one, or the one of the split-precision chain."""
        if f16s_dgrad:
            return ops.pack_apply_f16s(self.net, self.map_bwd_f16s(), flat, self.f16s_out_of_range, backward=True)
        return ops.pack_apply(self.map_bwd, flat)

    def flat(self, params) -> torch.Tensor:
        """Flat fp32 parameter vector of the network the kernels run (zero-padded to its width when the module's is narrower)."""
        f = _flat(params)
        if self.pad_idx is None:
            return f
        wide = torch.zeros(self.n_flat, dtype=torch.float32, device=f.device)
        wide[self.pad_idx] = f
        return wide

    def split_grads(self, grads: torch.Tensor) -> List[torch.Tensor]:
        """The kernels' flat gradient -> one tensor per parameter of the MODULE, in st.names order."""
        if self.pad_idx is not None:
            grads = grads[self.pad_idx]
        out, off = [], 0
        for k in self.names:
            shape = _param_shape(self.net_model, k)
            cnt = 1
            for s in shape:
                cnt *= s
            out.append(grads[off:off + cnt].view(shape))
            off += cnt
        return out

    def params(self, module: torch.nn.Module) -> List[torch.Tensor]:
        named = dict(module.named_parameters())
        try:
            return [named[k] for k in self.names]
        except KeyError as e:
            raise MiNerfError(f"module lacks parameter {e} (expected the layout of model/NeRF.py:24-30)") from e


# model -> {kernel width: state}: a netWidth below 128 trains 128 wide in fp32 and 256 wide in split precision
_states: "weakref.WeakKeyDictionary[torch.nn.Module, Dict[int, _TrainState]]" = weakref.WeakKeyDictionary()


def _state_for(model: torch.nn.Module, f16s: bool = False) -> _TrainState:
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise MiNerfError(f"model lives on {dev}: the MI355X path needs a HIP device (no CPU fallback)")
    per_width = _states.get(model)
    if per_width is None:
        per_width = _states[model] = {}
    known = next(iter(per_width.values()), None)
    st = None
    if known is not None:                                  # the module's own shape is on record: which kernel width does this precision train at?
        st = per_width.get(padded_train_net(known.net_model, f16s).W)
    if st is None or st.device != dev:
        st = _TrainState(model, dev, f16s)
        per_width[st.net.W] = st
    if f16s:                                               # a depth the split-precision forward has no LDS for: refused here, before the step starts
        ops.check_f16s_forward_depth(st.net)
    return st


def wants_grad(model) -> bool:
    return (torch.is_grad_enabled() and isinstance(model, torch.nn.Module)
            and any(p.requires_grad for p in model.parameters()))


def wants_ray_grad(model, ray_grad: bool, *rays) -> bool:
    """``ray_grad=True`` and one of the ray tensors carries a graph: the call goes to the training node even when no parameter requires
    grad (a frozen model: pose estimation), and the node then runs the backward-data chain alone."""
    return (bool(ray_grad) and torch.is_grad_enabled() and isinstance(model, torch.nn.Module)
            and any(isinstance(r, torch.Tensor) and r.requires_grad for r in rays))


def _flat(params) -> torch.Tensor:
    return torch.cat([p.detach().reshape(-1) for p in params]).float()


class Dense:
    """The route of ``_RenderTrain`` that evaluates every sample.  A route says how one network's samples reach the kernels and how d_raw gets
    back, in these four members; the other one, occupancy_train.Compacted, is this one run on the tiles of the samples a grid keeps."""
    saves = 0                                      # tensors per network the route adds to the node's (flat, blob, z, raw, stash)

    def forward(self, st, f16s, which, flat, blob, rays, z):
        """-> raw [n, S, 4], the stash, the ``saves`` tensors.  f16s: the launch runs in split precision (fp32-grade outputs and stash; blob
        re-packed on the device like the fp32 one); the backward keeps reading the fp32 ``blob``'s side tables either way."""
        if f16s:
            return (*ops.mlp_rays_train(st.net, st.forward_blob(flat, True), rays, z, f16s=True), ())
        return (*ops.mlp_rays_train(st.net, blob, rays, z), ())

    def skipped(self, saved) -> bool:
        """The forward launched nothing, so the parameters did not reach the outputs: their gradient is zero."""
        return False

    def backward(self, st, f16s, f16s_dgrad, blob, blob_b, rays, z, d_raw, stash, saved, stage):
        grads, work = ops.mlp_backward(st.net, blob, blob_b, rays, z, d_raw, stash, stage=stage, f16s_wgrad=f16s, f16s_dgrad=f16s_dgrad)
        if f16s:
            st.note_f16s_backward(work, z.shape[0], z.shape[1])
        return grads, work


# what _RenderTrain.forward takes before the parameters and saves per network after the rays: every index of needs_input_grad and of
# saved_tensors comes from these two
_INPUTS = ("st", "route", "rays", "cfg", "t_rand", "u", "z_override")
_KEPT = ("flat", "blob", "z", "raw", "stash")


class _RenderTrain(torch.autograd.Function):
    """rays (+ explicit randomness) and the two networks' parameters -> rgb_c, disp_c, rgb_f, disp_f; with ``cfg["geometry"]`` also
    acc_c, depth_c, distortion_c, acc_f, depth_f, distortion_f, differentiable like the colours (geometry.node_forward / node_backward).
    ``route`` (``Dense``, or with an occupancy grid occupancy_train.Compacted) runs the networks; everything around them is here once.
    With ``cfg["ray_grad"]`` the backward also returns the gradient of ``rays`` (pose.input_grad on the deltas the backward-data chain left
    in its workspace: no second backward pass), and a network none of whose parameters requires grad runs that chain alone (stage 1)."""

    @staticmethod
    def forward(ctx, st: _TrainState, route, rays, cfg: Dict, t_rand, u, z_override, *params):
        n_each = len(st.names)
        Nf, det = cfg["Nf"], cfg["det"]
        f16s = bool(cfg.get("f16s", False))
        saved = [rays]

        def network(k, depths):
            flat = st.flat(params[k * n_each:(k + 1) * n_each])
            blob = st.forward_blob(flat)
            z = depths()
            raw, stash, more = route.forward(st, f16s, ("coarse", "fine")[k], flat, blob, rays, z)
            rgb, disp, weights, extra = geo.node_forward(cfg, raw, z, rays, k == 0)
            saved.extend((flat, blob, z, raw, stash, *more))
            return rgb, disp, extra, z, weights

        rgb_c, disp_c, extra_c, z_c, w_c = network(0, lambda: ops.stratified_z(cfg["near"], cfg["far"], t_rand) if z_override is None else z_override[0])
        if Nf > 0:
            rgb_f, disp_f, extra_f, _, _ = network(1, lambda: ops.fine_z(z_c, w_c, Nf, det, None if det else u)
                                                   if (z_override is None or z_override[1] is None) else z_override[1])
        else:
            rgb_f = torch.empty(0, 3, device=rays.device)
            disp_f = torch.empty(0, device=rays.device)
            extra_f = tuple(torch.empty(0, device=rays.device) for _ in extra_c)
        ctx.st, ctx.route, ctx.Nf, ctx.f16s, ctx.cfg = st, route, Nf, f16s, cfg
        ctx.save_for_backward(*saved)
        ctx.mark_non_differentiable(disp_c, disp_f)
        ctx.set_materialize_grads(False)
        return (rgb_c, disp_c, rgb_f, disp_f, *extra_c, *extra_f)

    @staticmethod
    def backward(ctx, g_rgb_c, g_disp_c, g_rgb_f, g_disp_f, *g_extra):
        st: _TrainState = ctx.st
        route, cfg, net = ctx.route, ctx.cfg, st.net
        rays, *kept = ctx.saved_tensors
        per_net = len(_KEPT) + route.saves
        n_each = len(st.names)
        g_extra_c, g_extra_f = g_extra[:len(g_extra) // 2], g_extra[len(g_extra) // 2:]
        f16s = ctx.f16s and net.W == 256
        ray_grad = bool(cfg.get("ray_grad", False))
        need_rays = ray_grad and ctx.needs_input_grad[_INPUTS.index("rays")]
        g_rays: List[torch.Tensor] = []
        launched = False

        def one(k, g_rgb, g_ext) -> List[Optional[torch.Tensor]]:
            nonlocal launched
            if g_rgb is None and all(g is None for g in g_ext):
                return [None] * n_each
            flat, blob, z, raw, stash, *more = kept[k * per_net:(k + 1) * per_net]
            if route.skipped(more):
                return st.split_grads(torch.zeros(st.n_flat, dtype=torch.float32, device=rays.device))
            # without ray_grad every call is what it was (stage 0); with it a network whose parameters are all frozen skips the weight gradients
            first = len(_INPUTS) + k * n_each
            need_params = not ray_grad or any(ctx.needs_input_grad[first:first + n_each])
            f16s_dgrad = f16s and ops.f16s_dgrad_fits(net)   # the split-precision chain keeps a tile's ReLU' words of all layers in LDS
            blob_b = st.backward_blob(flat, f16s_dgrad)
            d_raw = geo.node_backward(cfg, raw, z, rays, g_rgb, g_ext)
            grads, work = route.backward(st, f16s, f16s_dgrad, blob, blob_b, rays, z, d_raw, stash, more, 0 if need_params else 1)
            launched = True
            if need_rays:
                from . import pose
                g_rays.append(pose.input_grad(net, flat, rays, z, raw, d_raw, work))
            return st.split_grads(grads) if need_params else [None] * n_each

        gc = one(0, g_rgb_c, g_extra_c)
        gf = one(1, g_rgb_f, g_extra_f) if ctx.Nf > 0 else [None] * n_each
        if f16s and launched:                                  # dense: a gradient arrived; compacted: and a sample had survived
            st.end_f16s_step()                                 # both nets' range words are folded: read them at the cadence
        g_in: List[Optional[torch.Tensor]] = [None] * len(_INPUTS)
        if g_rays:
            g_in[_INPUTS.index("rays")] = g_rays[0] if len(g_rays) == 1 else g_rays[0] + g_rays[1]
        return (*g_in, *gc, *gf)


class _EmbeddedTrain(torch.autograd.Function):
    """model(embedded, is_fine) with gradients: pre-embedded rows [n, 90] and ONE network's parameters -> [n, 4]."""

    @staticmethod
    def forward(ctx, st: _TrainState, x, *params):
        flat = st.flat(params)
        blob = ops.pack_apply(st.map_fwd, flat)
        out, stash = ops.mlp_embedded_train(st.net, blob, x)
        ctx.st = st
        ctx.save_for_backward(x, flat, blob, stash)
        return out

    @staticmethod
    def backward(ctx, g_out):
        st: _TrainState = ctx.st
        x, flat, blob, stash = ctx.saved_tensors
        blob_b = ops.pack_apply(st.map_bwd, flat)
        grads = ops.mlp_embedded_backward(st.net, blob, blob_b, x, g_out.contiguous().float(), stash)
        return (None, None, *st.split_grads(grads))


RAY_GRAD_WITH_GRID = "ray_grad=True with train_occupancy= is not built: with a grid the training node differentiates the parameters only"


def node_inputs(rays, model, opts, t_rand, u, seed: int, ray_offset: int, det: Optional[bool], f16s: bool, geometry: bool, ray_grad: bool, grid):
    """What ``_RenderTrain.apply`` takes for one slab, but for ``z_override``: st, route, rays, cfg, t_rand, u and the parameter list."""
    if ray_grad and grid is not None:
        raise MiNerfError(RAY_GRAD_WITH_GRID)
    st = _state_for(model, f16s)                 # f16s: the 256-wide state (any netWidth <= 256 is scattered into it)
    dev = st.device
    if isinstance(rays, torch.Tensor) and rays.requires_grad and not ray_grad:
        raise MiNerfError("rays require grad: the training path differentiates w.r.t. the MLP parameters only (the reference trains "
                          "nothing else, main.py:79-80); detach the rays, or a gradient would be dropped silently")
    if grid is None:
        route = Dense()
    else:
        from . import occupancy_train                                # at call time: that module imports this one
        route = occupancy_train.Compacted(grid, dev)
    rays = as_f32_dev(rays, dev)
    n = rays.shape[0]
    Sc, Nf = int(opts.N_samples_c), int(opts.N_samples_f)
    if det is None:
        det = ops.deterministic(opts)
    t_rand = ops.fill_uniform(seed, 0, ray_offset, n, Sc, dev) if t_rand is None else as_f32_dev(t_rand, dev)
    if Nf > 0 and not det:
        u = ops.fill_uniform(seed, 1, ray_offset, n, Nf, dev) if u is None else as_f32_dev(u, dev)
    else:
        u = None
    cfg = {"near": float(opts.near), "far": float(opts.far), "Sc": Sc, "Nf": Nf, "det": bool(det), "f16s": bool(f16s), "geometry": bool(geometry)}
    if ray_grad:
        cfg["ray_grad"] = True
    return st, route, rays, cfg, t_rand, u, st.params(model.model_coarse) + st.params(model.model_fine)


def render_train(rays: torch.Tensor, model: torch.nn.Module, opts, *, t_rand=None, u=None, seed: int = 0, ray_offset: int = 0,
                 z_override=None, det: Optional[bool] = None, f16s: bool = False, geometry: bool = False,
                 ray_grad: bool = False, grid=None) -> Dict[str, torch.Tensor]:
    """Differentiable ``render_rays`` (nerf_process.py:185-216) for one slab of rays [n, 6].  ``f16s``: the two forward launches run in
    split precision (fp32-grade results, ~3x faster); the backward kernels are the fp32 ones.  ``geometry``: the dict also carries
    ``acc_*``, ``depth_*`` and ``distortion_*`` per network, differentiable like the colours (geometry.py).  ``ray_grad``: rays that require
    grad are accepted and receive their gradient (pose.py: d rays, from there d pose); the depths stay constants, as in the reference.
    Without it such rays are refused, so that a gradient is never dropped silently.  ``grid``: an occupancy.OccupancyGrid -- the networks
    skip the samples it marks empty, forward and backward (occupancy_train.py; not with ``ray_grad``)."""
    st, route, rays, cfg, t_rand, u, params = node_inputs(rays, model, opts, t_rand, u, seed, ray_offset, det, f16s, geometry, ray_grad, grid)
    rgb_c, disp_c, rgb_f, disp_f, *extra = _RenderTrain.apply(st, route, rays, cfg, t_rand, u, z_override, *params)
    if grid is not None:
        grid.last_stats = route.stats                               # the sample counts of the call
    return node_outputs(rgb_c, disp_c, rgb_f, disp_f, extra, cfg["Nf"])


def node_outputs(rgb_c, disp_c, rgb_f, disp_f, extra, Nf: int) -> Dict[str, torch.Tensor]:
    """The dict of ``render_rays`` from a training node's outputs (``extra``: empty, or the six geometry outputs)."""
    out = {"rgb_c": rgb_c, "disp_c": disp_c}
    if Nf > 0:
        out["rgb_f"], out["disp_f"] = rgb_f, disp_f
    if extra:
        k = len(geo.EXTRA_KEYS)
        out.update({name + "_c": v for name, v in zip(geo.EXTRA_KEYS, extra[:k])})
        if Nf > 0:
            out.update({name + "_f": v for name, v in zip(geo.EXTRA_KEYS, extra[k:])})
    return out


def f16s_status(model: torch.nn.Module, reset: bool = True) -> Dict[str, float]:
    """What the split-precision training steps of ``model`` saw since the last read (one device -> host copy): max |d_raw|, max |delta * s|
    (how much of the f16 range the scaled backward chain used; >= 65504 means a conversion saturated and gradients were clipped), the number
    of weights the split-precision packers could not represent, and ``saturated``.  The training path itself reads these after each of the first
    F16S_CHECK_FIRST f16s steps and every F16S_CHECK_EVERY-th after them, and raises / warns; this is the on-demand read."""
    st = next((s for s in (_states.get(model) or {}).values() if s.f16s_range is not None), None)
    if st is None:
        return {"max_abs_d_raw": 0.0, "max_abs_delta_scaled": 0.0, "weights_out_of_range": 0, "saturated": False}
    return st.read_f16s(reset)


def rank_seed(seed: int, rank: int) -> int:
    """Per-rank jitter seed: ``seed`` mixed with a hash of the rank (distinct for every rank below 2^32, rank 0 included)."""
    h = ((rank + 1) * 0x9E3779B1) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x85EBCA77) & 0xFFFFFFFF
    h ^= h >> 13
    return (seed ^ h) & 0xFFFFFFFF


class RenderModule(torch.nn.Module):
    """``forward(rays_o, rays_d, H, W, K)`` = ``batchify_rays_and_render_by_chunk`` on the wrapped model.

    The reference trains on one GPU (main.py:166-170).  For data-parallel training wrap THIS module, not the NeRF, in
    ``torch.nn.parallel.DistributedDataParallel``: DDP needs the forward to go through the wrapper, and the NeRF's own
    ``forward(x, is_fine)`` is the embedded-input call of model/NeRF.py:70-78.  The hand-written backward returns ordinary
    parameter gradients and DDP all-reduces them in buckets (RCCL over xGMI with backend "nccl").  Both networks' gradients
    come out of ONE autograd node, so they become ready together at the end of the backward: the all-reduce of the 4.8 MB of
    gradients (~0.1 ms on xGMI) follows the 20 ms backward, it does not overlap with it.

    Jitter: without explicit ``t_rand`` / ``u`` / ``ray_offset`` / ``seed`` the generator is keyed on (seed, local ray index);
    every rank would then draw the SAME jitter for its local ray i.  ``forward`` therefore folds the rank into the SEED
    (not into the 32-bit ray counter, which would wrap for large rank x batch products) whenever one of the two random
    tensors is generated internally and the caller pins neither ``ray_offset`` nor ``seed``."""

    def __init__(self, model: torch.nn.Module, posenc, opts):
        super().__init__()
        self.model, self.posenc, self.opts = model, posenc, opts

    def forward(self, rays_o, rays_d, H, W, K, **kw):
        from . import nerf_process as NP
        generates = kw.get("t_rand") is None or (kw.get("u") is None and int(self.opts.N_samples_f) > 0)
        if generates and "ray_offset" not in kw and "seed" not in kw:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                kw["seed"] = rank_seed(NP._next_seed(None), dist.get_rank())
        return NP.batchify_rays_and_render_by_chunk(rays_o, rays_d, self.model, self.posenc, H, W, K, self.opts, **kw)
