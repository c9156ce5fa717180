"""Geometry losses: opacity, depth and the mip-NeRF 360 distortion regulariser (docs/design/18_geometry_losses.md).

Tensor-level wrappers over libmi_nerf_geo.so (include/mi_nerf_geo.h) in the style of ``ops.composite`` / ``ops.composite_backward``, the
compositing pair the two training nodes share (``node_forward`` / ``node_backward``: with ``geometry`` off they are ``ops.composite`` and
``ops.composite_backward``, call for call), and the ``opts.geometry`` mapping of ``harness.train``.
"""
from __future__ import annotations

from typing import Dict, Mapping, Optional, Tuple

import torch

from . import _geo, ops
from ._lib import MiNerfError, dev_ptr, stream_ptr

EXTRA_KEYS = ("acc", "depth", "distortion")           # what geometry=True adds per network, in the order the nodes return them


def _shapes(raw, z, rays_or_d) -> Tuple[int, int, int]:
    if z.dim() != 2:
        raise MiNerfError(f"z must be [n,S], got {tuple(z.shape)}")
    n, S = z.shape
    if tuple(raw.shape) != (n, S, 4):
        raise MiNerfError(f"raw must be [n,S,4] = {(n, S, 4)}, got {tuple(raw.shape)}")
    stride = rays_or_d.shape[-1]
    if tuple(rays_or_d.shape) != (n, stride) or stride not in (3, 6):
        raise MiNerfError("rays must be [n,6] or rays_d [n,3]")
    return n, S, stride


def composite_geo(raw: torch.Tensor, z: torch.Tensor, rays_or_d: torch.Tensor, near: float, far: float):
    """(rgb [n,3], disp [n], acc [n], weights [n,S], depth [n], distortion [n]): ``ops.composite`` bit for bit, plus the distortion loss per
    ray with the depths normalised by ``near`` / ``far`` (mi_geo_composite)."""
    n, S, stride = _shapes(raw, z, rays_or_d)
    dev = z.device
    rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
    disp, acc, depth, dist = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4))
    wts = torch.empty(n, S, dtype=torch.float32, device=dev)
    with ops._guard(dev):
        _geo.check(_geo.lib().mi_geo_composite(dev_ptr(raw, "raw", align=16), dev_ptr(z, "z"), dev_ptr(rays_or_d, "rays"), stride, n, S, float(near),
                                               float(far), dev_ptr(rgb), dev_ptr(disp), dev_ptr(acc), dev_ptr(wts), dev_ptr(depth), dev_ptr(dist),
                                               stream_ptr(dev)), "mi_geo_composite")
    return rgb, disp, acc, wts, depth, dist


def composite_geo_backward(raw: torch.Tensor, z: torch.Tensor, rays_or_d: torch.Tensor, near: float, far: float, g_rgb: Optional[torch.Tensor] = None,
                           g_acc: Optional[torch.Tensor] = None, g_depth: Optional[torch.Tensor] = None, g_distortion: Optional[torch.Tensor] = None,
                           g_weights: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradients w.r.t. rgb [n,3], acc [n], depth [n], distortion [n], weights [n,S] (each optional: None is zero) -> d raw [n,S,4]
    (mi_geo_composite_backward; every element is written, into ``out`` when given).  With ``g_rgb`` alone the result is
    ``ops.composite_backward``'s."""
    n, S, stride = _shapes(raw, z, rays_or_d)
    for name, g, shape in (("g_rgb", g_rgb, (n, 3)), ("g_acc", g_acc, (n,)), ("g_depth", g_depth, (n,)), ("g_distortion", g_distortion, (n,)),
                           ("g_weights", g_weights, (n, S))):
        if g is not None and tuple(g.shape) != shape:
            raise MiNerfError(f"{name} must be {shape}, got {tuple(g.shape)}")
    dev = z.device
    if out is not None and tuple(out.shape) != (n, S, 4):
        raise MiNerfError(f"out must be {(n, S, 4)}, got {tuple(out.shape)}")
    d_raw = torch.empty(n, S, 4, dtype=torch.float32, device=dev) if out is None else out
    with ops._guard(dev):
        _geo.check(_geo.lib().mi_geo_composite_backward(dev_ptr(raw, "raw", align=16), dev_ptr(z, "z"), dev_ptr(rays_or_d, "rays"), stride, n, S,
                                                        float(near), float(far), dev_ptr(g_rgb, "g_rgb"), dev_ptr(g_acc, "g_acc"),
                                                        dev_ptr(g_depth, "g_depth"), dev_ptr(g_distortion, "g_distortion"),
                                                        dev_ptr(g_weights, "g_weights"), dev_ptr(d_raw, "d_raw", align=16), stream_ptr(dev)),
                   "mi_geo_composite_backward")
    return d_raw


# ---------------------------------------------------------------------------------------------------
# the compositing pair of the training node (train_path._RenderTrain, whichever route runs its networks)
# ---------------------------------------------------------------------------------------------------
def _grad(g: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if g is None else g.contiguous().float()


def node_forward(cfg: Dict, raw, z, rays, want_weights: bool):
    """-> (rgb, disp, weights | None, extras): extras is () with ``cfg["geometry"]`` off and (acc, depth, distortion) with it on."""
    if not cfg.get("geometry", False):
        rgb, disp, _, wts, _ = ops.composite(raw, z, rays, want_all=want_weights)
        return rgb, disp, wts, ()
    rgb, disp, acc, wts, depth, dist = composite_geo(raw, z, rays, cfg["near"], cfg["far"])
    return rgb, disp, wts, (acc, depth, dist)


def node_backward(cfg: Dict, raw, z, rays, g_rgb, g_extras=()) -> torch.Tensor:
    """d_raw of one network from the gradients that arrived (at least one is not None)."""
    if not cfg.get("geometry", False):
        return ops.composite_backward(raw, z, rays, _grad(g_rgb))
    g_acc, g_depth, g_dist = g_extras
    return composite_geo_backward(raw, z, rays, cfg["near"], cfg["far"], _grad(g_rgb), _grad(g_acc), _grad(g_depth), _grad(g_dist))


# ---------------------------------------------------------------------------------------------------
# opts.geometry of harness.train
# ---------------------------------------------------------------------------------------------------
_OPTION_KEYS = ("acc_weight", "depth_weight", "distortion_weight", "targets")


def parse_options(geometry, near: float, far: float) -> Optional[Dict]:
    """``opts.geometry`` (absent / None: no geometry terms) -> {"acc_weight", "depth_weight", "distortion_weight", "targets"}.  ``targets`` is
    a callable rays [B,6] -> (acc [B], depth [B]), or an object with the ``render`` of scenes.SolidScene (its ground truth between
    ``near`` and ``far``); it is required when ``acc_weight`` or ``depth_weight`` is not zero."""
    if geometry is None:
        return None
    if not isinstance(geometry, Mapping):
        raise MiNerfError(f"opts.geometry must be a mapping with the keys {', '.join(_OPTION_KEYS)}, got {type(geometry).__name__}")
    unknown = sorted(set(geometry) - set(_OPTION_KEYS))
    if unknown:
        raise MiNerfError(f"opts.geometry: unknown key(s) {', '.join(map(repr, unknown))} (known: {', '.join(_OPTION_KEYS)})")
    out = {}
    for k in _OPTION_KEYS[:3]:
        v = geometry.get(k, 0.0)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v < 0:
            raise MiNerfError(f"opts.geometry[{k!r}] must be a number >= 0, got {v!r}")
        out[k] = float(v)
    targets = geometry.get("targets")
    if targets is not None and not callable(targets):
        if not callable(getattr(targets, "render", None)):
            raise MiNerfError("opts.geometry['targets'] must be a callable rays [B,6] -> (acc [B], depth [B]) or a scenes.SolidScene")
        scene = targets
        targets = lambda r: scene.render(r, near, far)[2:4]                 # noqa: E731
    if targets is None and (out["acc_weight"] != 0.0 or out["depth_weight"] != 0.0):
        raise MiNerfError("opts.geometry: acc_weight / depth_weight need 'targets', a callable rays [B,6] -> (acc [B], depth [B])")
    out["targets"] = targets
    return out


def loss_terms(g: Dict, extras: Mapping[str, torch.Tensor], suffix: str, acc_t, depth_t) -> Dict[str, torch.Tensor]:
    """The three geometry terms of one network (``suffix`` "c" or "f"), unweighted: mse(acc, acc*), mean(acc* (depth - depth*)^2),
    mean(distortion).  A term whose weight is zero is left out."""
    terms = {}
    if g["acc_weight"] != 0.0:
        terms["acc"] = torch.mean((extras["acc_" + suffix] - acc_t) ** 2)
    if g["depth_weight"] != 0.0:
        terms["depth"] = torch.mean(acc_t * (extras["depth_" + suffix] - depth_t) ** 2)
    if g["distortion_weight"] != 0.0:
        terms["distortion"] = torch.mean(extras["distortion_" + suffix])
    return terms
