"""Procedural solid-object scenes (include/mi_nerf_scene.h, libmi_nerf_scene.so): opaque spheres, boxes and cylinders in empty space, rendered
on the device through the reference's own image-formation model -- something object-like to train on and to measure against where no
dataset is at hand.

    scene = SolidScene.default()
    images, poses, K = scene.dataset(14, (64, 64))              # [V,H,W,3] on the device, [V,4,4], [3,3]: what harness.global_batch / test take
    rgb, disp, acc, depth = scene.render(rays, 2.0, 6.0)        # the fused ground-truth renderer (mi_scene_render)
    raw = scene.field(rays, z)                                  # [n,S,4]: the scene as a stand-in network (mi_scene_field_rays)

Colours are given in (0, 1) and stored as the raw logits ``sigmoid`` in post_process consumes (float64 logit, rounded to fp32 once).
There is no fallback: constructing and validating a scene needs the library but no GPU, everything else runs on one.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _scene, ops
from ._lib import MiNerfError, as_f32_dev, dev_ptr, stream_ptr
from ._scene import BOX, CYLINDER, SPHERE, Prim


def _logits(rgb) -> Tuple[float, float, float]:
    v = tuple(float(x) for x in rgb)
    if len(v) != 3 or not all(0.0 < x < 1.0 for x in v):
        raise MiNerfError(f"a colour is three values inside (0, 1), got {rgb!r}")
    return tuple(float(np.float32(math.log(x / (1.0 - x)))) for x in v)


def _vec3(v, what: str) -> Tuple[float, float, float]:
    t = tuple(float(x) for x in v)
    if len(t) != 3:
        raise MiNerfError(f"{what} takes three values, got {v!r}")
    return t


def _prim(kind: int, axis: int, centre, h, sigma: float, rgb, rgb2, freq: float) -> Prim:
    c0 = _logits(rgb)
    c1 = _logits(rgb if rgb2 is None else rgb2)
    if freq > 0 and rgb2 is None:
        raise MiNerfError("a checker (freq > 0) takes a second colour")
    return Prim(kind, int(axis), (C.c_float * 3)(*_vec3(centre, "centre")), (C.c_float * 3)(*h), float(sigma),
                ((C.c_float * 3) * 2)((C.c_float * 3)(*c0), (C.c_float * 3)(*c1)), float(freq))


def sphere(centre, radius: float, rgb, *, sigma: float = 4096.0, rgb2=None, freq: float = 0.0) -> Prim:
    return _prim(SPHERE, 0, centre, (float(radius), 0.0, 0.0), sigma, rgb, rgb2, freq)


def box(centre, half, rgb, *, sigma: float = 4096.0, rgb2=None, freq: float = 0.0) -> Prim:
    return _prim(BOX, 0, centre, _vec3(half, "half"), sigma, rgb, rgb2, freq)


def cylinder(centre, radius: float, half_height: float, rgb, *, axis: int = 2, sigma: float = 4096.0, rgb2=None, freq: float = 0.0) -> Prim:
    return _prim(CYLINDER, axis, centre, (float(radius), float(half_height), 0.0), sigma, rgb, rgb2, freq)


def scaled_camera(hw) -> np.ndarray:
    """The lego camera (synthetic.lego_camera: 800 x 800) scaled to ``hw``."""
    from . import synthetic
    H, W = hw
    K800, _, _ = synthetic.lego_camera()
    return np.array([[K800[0][0] * W / 800.0, 0, W / 2], [0, K800[1][1] * H / 800.0, H / 2], [0, 0, 1]])


class SolidScene:
    """1 .. 16 primitives; the first one in list order that contains a point owns it.  Validated on construction (mi_scene_check)."""

    def __init__(self, prims: Sequence[Prim]):
        prims = list(prims)
        if not prims or len(prims) > _scene.MAX_PRIMS or not all(isinstance(p, Prim) for p in prims):
            raise MiNerfError(f"a scene takes 1..{_scene.MAX_PRIMS} primitives made by sphere() / box() / cylinder(), got {len(prims)}")
        self.prims: List[Prim] = prims
        self._arr = (Prim * len(prims))(*prims)
        _scene.check(_scene.lib().mi_scene_check(self._arr, len(prims)), "mi_scene_check")

    def __len__(self) -> int:
        return len(self.prims)

    @classmethod
    def default(cls) -> "SolidScene":
        """A table-top: three boxes (one checkered, one carrying a small cube), a sphere and a standing cylinder on a thin slab, all inside
        the box +-1.2 -- inside near / far = 2 / 6 of cameras at radius 4 -- and dense enough (sigma 4096) that one sample inside is opaque."""
        return cls([
            box((-0.55, -0.45, -0.20), (0.30, 0.30, 0.30), (0.85, 0.15, 0.12)),
            box((-0.55, -0.45, 0.25), (0.15, 0.15, 0.15), (0.92, 0.92, 0.88)),
            box((0.50, -0.50, -0.10), (0.25, 0.35, 0.40), (0.10, 0.25, 0.85), rgb2=(0.95, 0.85, 0.15), freq=5.0),
            box((-0.25, 0.75, -0.35), (0.35, 0.12, 0.15), (0.15, 0.70, 0.25)),
            sphere((0.55, 0.45, -0.10), 0.40, (0.95, 0.55, 0.10)),
            cylinder((-0.65, 0.30, 0.00), 0.22, 0.50, (0.55, 0.20, 0.75), axis=2),
            box((0.0, 0.0, -0.55), (1.10, 1.10, 0.05), (0.60, 0.60, 0.62)),
        ])

    # ---- the scene as a network ----------------------------------------------------------------------
    def field(self, rays: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
        """raw [n,S,4] at the samples (rays [n,6], z [n,S]): THE FIELD RULE of the header (mi_scene_field_rays)."""
        rays = as_f32_dev(rays)
        z = as_f32_dev(z, rays.device)
        if z.dim() != 2 or tuple(rays.shape) != (z.shape[0], 6):
            raise MiNerfError(f"rays [n,6] and z [n,S] expected, got {tuple(rays.shape)} / {tuple(z.shape)}")
        n, S = z.shape
        raw = torch.empty(n, S, 4, dtype=torch.float32, device=rays.device)
        with ops._guard(rays.device):
            _scene.check(_scene.lib().mi_scene_field_rays(self._arr, len(self), dev_ptr(rays, "rays"), dev_ptr(z, "z"), n, S,
                                                          dev_ptr(raw, "raw", torch.float32, 16), stream_ptr(rays.device)), "mi_scene_field_rays")
        return raw

    # ---- the ground truth ----------------------------------------------------------------------------
    def render(self, rays: torch.Tensor, near: float, far: float, S: int = 1024, want_all: bool = True):
        """(rgb [n,3], disp [n], acc [n], depth [n]) of rays [n,6] at the S bin centres of [near, far] (mi_scene_render); ``want_all=False``:
        rgb alone, the other outputs are not written."""
        rays = as_f32_dev(rays)
        if rays.dim() != 2 or rays.shape[1] != 6:
            raise MiNerfError(f"rays [n,6] expected, got {tuple(rays.shape)}")
        n, dev = rays.shape[0], rays.device
        rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
        disp, acc, depth = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3)) if want_all else (None, None, None)
        with ops._guard(dev):
            _scene.check(_scene.lib().mi_scene_render(self._arr, len(self), dev_ptr(rays, "rays"), n, float(near), float(far), int(S), dev_ptr(rgb),
                                                      dev_ptr(disp), dev_ptr(acc), dev_ptr(depth), stream_ptr(dev)), "mi_scene_render")
        return (rgb, disp, acc, depth) if want_all else rgb

    def render_views(self, poses, K, hw, near: float, far: float, S: int = 1024, device="cuda:0") -> torch.Tensor:
        """images [V,H,W,3] on ``device``: per pose [4,4] (or [3,4]) the rays of ops.make_o_d, rendered by mi_scene_render."""
        H, W = hw
        device = torch.device(device)
        images = []
        for pose in poses:
            o, d = ops.make_o_d(W, H, K, pose, device)
            rays = torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1).contiguous()
            images.append(self.render(rays, near, far, S, want_all=False).reshape(H, W, 3))
        return torch.stack(images, 0)

    def dataset(self, n_views: int, hw, radius: float = 4.0, phi: float = -30.0, near: float = 2.0, far: float = 6.0, S: int = 1024,
                device="cuda:0", K: Optional[np.ndarray] = None):
        """(images [V,H,W,3] on the device, poses [V,4,4], K [3,3]): ``n_views`` cameras evenly on the circle of harness.get_render_pose at
        ``radius`` and elevation ``phi``, looking at the origin, with the lego camera scaled to ``hw``.  Deterministic: no jitter anywhere."""
        from . import harness
        if int(n_views) < 1:
            raise MiNerfError(f"n_views={n_views}: at least one view")
        K = scaled_camera(hw) if K is None else np.asarray(K)
        poses = torch.from_numpy(harness.spherical_poses(np.linspace(-180, 180, int(n_views) + 1)[:-1], phi, radius))
        return self.render_views(poses, K, hw, near, far, S, device), poses, K
