"""Gradients with respect to rays and camera poses (docs/design/19_pose_gradients.md).

Tensor-level wrappers over libmi_nerf_pose.so (include/mi_nerf_pose.h) in the style of ``geometry.py``, the autograd nodes that put them
behind the existing ray generators (``make_o_d``, ``ndc_rays``: forward is the existing kernel, bit for bit), and ``CameraRefiner``, the
per-image pose correction a caller optimises.  The training node asks ``input_grad`` for the gradient of its rays when it is called with
``ray_grad=True`` (train_path.py); nothing here runs without that keyword.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _pose, ops
from ._lib import MiNerfError, Net, as_f32_dev, dev_ptr, stream_ptr


# ---------------------------------------------------------------------------------------------------
# where the three narrow weight blocks sit in the flat parameter vector (ops.param_names order, [out, in] row-major)
# ---------------------------------------------------------------------------------------------------
def weight_blocks(net: Net) -> Dict[str, Optional[Tuple[int, int]]]:
    """{"x0", "skip", "d"} -> (offset in floats, leading dimension) of linear_x[0].weight, linear_x[skip+1].weight and linear_d.weight
    inside the flat vector; "skip" is None when no layer concatenates gamma(x) (``skip < 0`` or ``skip + 1 >= D``, model/NeRF.py:25)."""
    in_x, in_d, W, D = 3 + 6 * net.L_x, 3 + 6 * net.L_d, net.W, net.D
    has_skip = 0 <= net.skip and net.skip + 1 < D
    off, out = 0, {"x0": None, "skip": None, "d": None}
    for l in range(D):
        fan_in = in_x if l == 0 else (W + in_x if (has_skip and l == net.skip + 1) else W)
        if l == 0:
            out["x0"] = (off, fan_in)
        elif fan_in != W:
            out["skip"] = (off, fan_in)
        off += W * fan_in + W
    out["d"] = (off, W + in_d)
    return out


def input_grad(net: Net, flat: torch.Tensor, rays: torch.Tensor, z: torch.Tensor, raw: torch.Tensor, d_raw: torch.Tensor, work: torch.Tensor,
               want_staged: bool = False):
    """d rays [n,6] of one network from what ``ops.mlp_backward`` left in ``work`` (stage 0 or 1) -- THE INPUT-GRADIENT RULE of
    include/mi_nerf_pose.h.  ``flat``: the flat fp32 parameter vector the kernels ran (train_path._TrainState.flat).
    ``want_staged``: also return (d_pts [P,3], d_view [n,3], d_emb [P, in_x + in_d])."""
    n, S = z.shape
    if tuple(rays.shape) != (n, 6) or tuple(raw.shape) != (n, S, 4) or tuple(d_raw.shape) != (n, S, 4):
        raise MiNerfError(f"rays / raw / d_raw must be {(n, 6)} / {(n, S, 4)} / {(n, S, 4)}, got {tuple(rays.shape)} / {tuple(raw.shape)} / {tuple(d_raw.shape)}")
    if flat.numel() != ops.param_count(net):
        raise MiNerfError(f"flat parameter vector has {flat.numel()} entries, expected {ops.param_count(net)}")
    dev = z.device
    views = ops.train_views(net, n, S, work=work)
    blocks = weight_blocks(net)
    wp = dev_ptr(flat, "flat")
    x0, sk, dd = blocks["x0"], blocks["skip"], blocks["d"]
    delta_skip = views["delta_h"][net.skip + 1] if sk is not None else None
    in_all = 6 + 6 * net.L_x + 6 * net.L_d
    d_rays = torch.empty(n, 6, dtype=torch.float32, device=dev)
    d_pts = torch.empty(n * S, 3, dtype=torch.float32, device=dev) if want_staged else None
    d_view = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_staged else None
    d_emb = torch.empty(n * S, in_all, dtype=torch.float32, device=dev) if want_staged else None
    with ops._guard(dev):
        _pose.check(_pose.lib().mi_pose_input_grad(
            dev_ptr(rays, "rays"), dev_ptr(z, "z"), dev_ptr(raw, "raw", align=16), dev_ptr(d_raw, "d_raw", align=16), n, S,
            dev_ptr(views["delta_h"][0], "delta_x0", align=16), dev_ptr(delta_skip, "delta_skip", align=16), dev_ptr(views["delta_d"], "delta_d", align=16),
            wp + 4 * x0[0], x0[1], None if sk is None else wp + 4 * sk[0], 0 if sk is None else sk[1], wp + 4 * dd[0], dd[1],
            net.W, net.L_x, net.L_d, dev_ptr(d_rays), dev_ptr(d_pts), dev_ptr(d_view), dev_ptr(d_emb), stream_ptr(dev)), "mi_pose_input_grad")
    return (d_rays, d_pts, d_view, d_emb) if want_staged else d_rays


# ---------------------------------------------------------------------------------------------------
# NDC warp
# ---------------------------------------------------------------------------------------------------
def _strided(t: torch.Tensor, name: str, n: int):
    """What ops.ndc_rays accepts: [n,3] fp32 on the device, rows contiguous or one broadcast row (stride 0)."""
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32 or not t.is_cuda:
        raise MiNerfError(f"{name} must be a [n,3] fp32 device tensor")
    if t.stride(1) != 1 or (t.stride(0) not in (0, 3) and n > 1):
        t = t.contiguous()
    return t, (t.stride(0) if n > 1 else 3)


def ndc_rays_backward(H: int, W: int, focal: float, near: float, rays_o: torch.Tensor, rays_d: torch.Tensor, g_o_ndc: Optional[torch.Tensor],
                      g_d_ndc: Optional[torch.Tensor]):
    """(g_o [n,3], g_d [n,3]) from the gradients of ``ops.ndc_rays``'s outputs (None is zero); a broadcast origin still gets one row per ray."""
    n = rays_d.shape[0]
    dev = rays_d.device
    o, os_ = _strided(rays_o, "rays_o", n)
    d, ds_ = _strided(rays_d, "rays_d", n)
    for name, g in (("g_o_ndc", g_o_ndc), ("g_d_ndc", g_d_ndc)):
        if g is not None and tuple(g.shape) != (n, 3):
            raise MiNerfError(f"{name} must be {(n, 3)}, got {tuple(g.shape)}")
    g_o = torch.empty(n, 3, dtype=torch.float32, device=dev)
    g_d = torch.empty(n, 3, dtype=torch.float32, device=dev)
    with ops._guard(dev):
        _pose.check(_pose.lib().mi_pose_ndc_rays_backward(int(H), int(W), float(focal), float(near), o.data_ptr(), os_, d.data_ptr(), ds_, n,
                                                          dev_ptr(g_o_ndc, "g_o_ndc"), dev_ptr(g_d_ndc, "g_d_ndc"), dev_ptr(g_o), dev_ptr(g_d),
                                                          stream_ptr(dev)), "mi_pose_ndc_rays_backward")
    return g_o, g_d


def _grad(g: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if g is None else g.contiguous().float()


class _NdcRays(torch.autograd.Function):
    @staticmethod
    def forward(ctx, H, W, focal, near, rays_o, rays_d):
        ctx.args = (H, W, focal, near)
        ctx.save_for_backward(rays_o, rays_d)
        ctx.set_materialize_grads(False)
        return ops.ndc_rays(H, W, focal, near, rays_o, rays_d)

    @staticmethod
    def backward(ctx, g_oo, g_dd):
        if g_oo is None and g_dd is None:
            return (None,) * 6
        rays_o, rays_d = ctx.saved_tensors
        g_o, g_d = ndc_rays_backward(*ctx.args, rays_o, rays_d, _grad(g_oo), _grad(g_dd))
        return None, None, None, None, (g_o if ctx.needs_input_grad[4] else None), (g_d if ctx.needs_input_grad[5] else None)


def ndc_rays(H: int, W: int, focal: float, near: float, rays_o: torch.Tensor, rays_d: torch.Tensor):
    """``ops.ndc_rays`` (the same kernel, the same bits) as an autograd node: differentiable in the origins and the directions.  A
    broadcast origin (the stride-0 view ``make_o_d`` returns) is accepted as it is; autograd sums its per-ray gradient rows."""
    return _NdcRays.apply(int(H), int(W), float(focal), float(near), rays_o, rays_d)


# ---------------------------------------------------------------------------------------------------
# ray generation
# ---------------------------------------------------------------------------------------------------
def make_o_d_backward(img_w: int, img_h: int, img_k, pose, g_o: Optional[torch.Tensor], g_d: torch.Tensor, pixels: Optional[torch.Tensor] = None,
                      row0: int = 0):
    """(d_pose [3,4], d_k4 [4] = d(fx, fy, cx, cy)) on the device from the gradients of the rays ``make_o_d`` made: ``g_d`` [n,3], ``g_o`` [n,3]
    or None (zero).  ``pixels``: the int64 indices y * W + x of the forward, or None for whole rows from ``row0``."""
    dev = g_d.device
    n = g_d.shape[0]
    k4, p12 = ops._cam(img_k, pose)
    d_pose = torch.empty(3, 4, dtype=torch.float32, device=dev)
    d_k4 = torch.empty(4, dtype=torch.float32, device=dev)
    nbytes = int(_pose.lib().mi_pose_reduce_scratch_bytes())
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if tuple(g_d.shape) != (n, 3) or (g_o is not None and tuple(g_o.shape) != (n, 3)) or (pixels is not None and pixels.numel() != n):
        raise MiNerfError(f"g_d / g_o must be [n,3] and pixels [n]; got {tuple(g_d.shape)} / {None if g_o is None else tuple(g_o.shape)}")
    with ops._guard(dev):
        _pose.check(_pose.lib().mi_pose_make_o_d_backward(int(img_w), int(img_h), k4, p12, dev_ptr(pixels, "pixels", torch.int64, 8), int(row0), n,
                                                          dev_ptr(g_o, "g_o"), dev_ptr(g_d, "g_d"), dev_ptr(d_pose), dev_ptr(d_k4),
                                                          dev_ptr(scratch, "scratch", torch.uint8, 16), nbytes, stream_ptr(dev)),
                    "mi_pose_make_o_d_backward")
    return d_pose, d_k4


class _MakeOD(torch.autograd.Function):
    """pose [3,4] (and the intrinsics as a [4] tensor (fx, fy, cx, cy), or None) -> (rays_o [n,3], rays_d [n,3])."""

    @staticmethod
    def forward(ctx, img_w, img_h, img_k, pose, k_vec, pixels, device):
        if pixels is None:
            o, d = ops.make_o_d(img_w, img_h, img_k, pose, device)
            o, d = o.reshape(-1, 3), d.reshape(-1, 3)
        else:
            o, d = ops.make_o_d_pixels(img_w, img_h, img_k, pose, pixels)
        ctx.args = (img_w, img_h, img_k, pose.detach(), pixels)
        ctx.set_materialize_grads(False)
        return o, d

    @staticmethod
    def backward(ctx, g_o, g_d):
        if g_o is None and g_d is None:
            return (None,) * 7
        img_w, img_h, img_k, pose, pixels = ctx.args
        g_o, g_d = _grad(g_o), _grad(g_d)
        if g_d is None:
            g_d = torch.zeros_like(g_o)
        d_pose, d_k4 = make_o_d_backward(img_w, img_h, img_k, pose, g_o, g_d, pixels)
        return (None, None, None, d_pose.to(pose.dtype) if ctx.needs_input_grad[3] else None, d_k4 if ctx.needs_input_grad[4] else None, None, None)


def _k_parts(img_k):
    """(K as ops._cam reads it, the [4] vector (fx, fy, cx, cy) that carries K's graph or None)."""
    if isinstance(img_k, torch.Tensor) and img_k.requires_grad:
        return img_k.detach(), torch.stack([img_k[0][0], img_k[1][1], img_k[0][2], img_k[1][2]]).float()
    return img_k, None


def make_o_d(img_w: int, img_h: int, img_k, pose: torch.Tensor, pixels: Optional[torch.Tensor] = None, device=None):
    """(rays_o [n,3], rays_d [n,3]): ``ops.make_o_d_pixels`` for the int64 pixel indices ``pixels`` (y * W + x), or ``ops.make_o_d`` for the
    whole image flattened (``pixels`` None) -- the same kernels, the same bits -- differentiable in ``pose`` [3,4] (a device tensor) and in
    ``img_k`` when that is a tensor requiring grad."""
    if not isinstance(pose, torch.Tensor):
        raise MiNerfError("pose.make_o_d takes the pose as a tensor (use ops.make_o_d for plain arrays)")
    if tuple(pose.shape[-2:]) not in ((3, 4), (4, 4)) or pose.dim() != 2:
        raise MiNerfError(f"pose must be [3,4] or [4,4], got {tuple(pose.shape)}")
    dev = pixels.device if pixels is not None else torch.device(device if device is not None else pose.device)
    if dev.type != "cuda":
        raise MiNerfError(f"rays are made on a HIP device (got {dev}); this path has no CPU fallback")
    k_plain, k_vec = _k_parts(img_k)
    pose34 = pose[:3, :4]
    if pose34.device != dev:
        pose34 = pose34.to(dev)
    return _MakeOD.apply(int(img_w), int(img_h), k_plain, pose34, k_vec, pixels, dev)


# ---------------------------------------------------------------------------------------------------
# the pose correction a caller optimises
# ---------------------------------------------------------------------------------------------------
def _skew(w: torch.Tensor) -> torch.Tensor:
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


class CameraRefiner(torch.nn.Module):
    """Per-image pose corrections, zero-initialised: ``rot`` [n,3] (axis-angle) and ``trans`` [n,3].

    ``forward(i, base_pose)`` -> [3,4] with R = exp([rot_i]x) R_base and t = t_base + trans_i (a dozen scalars: torch ops on the device;
    nothing per ray goes through torch).  Put ``parameters()`` into the optimizer; ``poses(base_poses)`` gives all corrected poses."""

    def __init__(self, n_images: int):
        super().__init__()
        if int(n_images) < 1:
            raise MiNerfError(f"CameraRefiner needs at least one image, got {n_images}")
        self.rot = torch.nn.Parameter(torch.zeros(int(n_images), 3))
        self.trans = torch.nn.Parameter(torch.zeros(int(n_images), 3))

    def forward(self, i: int, base_pose) -> torch.Tensor:
        base = torch.as_tensor(base_pose).to(device=self.rot.device, dtype=torch.float32)[:3, :4]
        R = torch.matrix_exp(_skew(self.rot[int(i)])) @ base[:, :3]
        t = base[:, 3] + self.trans[int(i)]
        return torch.cat([R, t[:, None]], dim=1)

    def poses(self, base_poses) -> torch.Tensor:
        """[n,3,4]: every image's corrected pose, without a graph (evaluation)."""
        with torch.no_grad():
            return torch.stack([self.forward(i, base_poses[i]) for i in range(self.rot.shape[0])])
