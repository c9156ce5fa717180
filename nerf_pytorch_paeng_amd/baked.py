"""A trained NeRF baked into a radiance grid, and frames rendered from the grid alone (include/mi_nerf_vox.h, libmi_nerf_vox.so).

    grid = baked.RadianceGrid(-1.2, 1.2, 256, B=9).bake(model)          # density + 9 spherical-harmonic colour coefficients per lattice point
    rgb, disp, acc, depth = grid.render(rays)                            # marching through the table: no network
    opts.baked = grid                                                    # harness.test / harness.render then render every pose from it
    small = grid.compact("f16")                                          # records of the active points only (THE COMPACT GRID), fp32 or f16
    small = baked.SparseRadianceGrid(-1.2, 1.2, 512, B=9, storage="f16").bake(model)    # ... baked without the dense record array
    fine = grid.resample(512)                                            # the same field on another lattice (THE RESAMPLING RULE)
    grid.prune(0.5)                                                      # sigma and records cleared away from density > 0.5 (THE PRUNING RULE)
    od = grid.seen(baked.Views(H, W, K, poses))                          # the least optical depth under which a camera sees each point
    grid.prune(0.0, seen=od, T_vis=1e-3)                                 # ... and what no camera sees with transmittance 1e-3 goes too
    signed = grid.to_signed()                                            # A SIGNED GRID: the density before its ReLU, the ReLU after the interpolation
    signed = baked.RadianceGrid(-1.2, 1.2, 256, B=9, signed=True).bake(model)           # ... baked from the network's own signed density

The lattice is the one of mesh.density_lattice (include/mi_nerf_mesh.h): the grid's sigma plane is that lattice after a ReLU.  Colour is
the network's post-sigmoid colour at the lattice point, seen from D fixed directions, projected by least squares onto B real spherical
harmonics (``projection_matrix``); the renderer interpolates trilinearly and composites front to back by THE RENDER RULE of the header.
Baking is not the hot path (torch ops build the active-point list); rendering is one launch.  There is no fallback: a missing library or a
failed call raises ``MiNerfError``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Optional, Tuple

import numpy as np
import torch

from . import _vox, ops
from ._lib import MiNerfError, as_f32_dev, dev_ptr, stream_ptr
from ._vox import Grid, RenderCfg

BASES = (1, 4, 9)
# lattice points handed to the field per slab by bake_field (D one-sample rays each)
SLAB_POINTS = 1 << 16
# the header's constants
_C0, _C1, _C2, _C20, _C22 = 0.28209479, 0.48860251, 1.0925484, 0.31539157, 0.54627422


def _triple(v, cast) -> Tuple:
    if isinstance(v, (int, float)):
        return (cast(v),) * 3
    t = tuple(cast(x) for x in v)
    if len(t) != 3:
        raise MiNerfError(f"expected a scalar or three values (x, y, z), got {v!r}")
    return t


def _check_basis(B: int) -> int:
    if B not in BASES:
        raise MiNerfError(f"B={B!r}: 1, 4 or 9 basis functions (degree 0, 1, 2)")
    return int(B)


# ---------------------------------------------------------------------------------------------------
# the basis and the projection: host, float64
# ---------------------------------------------------------------------------------------------------
def sh_basis(dirs, B: int) -> np.ndarray:
    """Y [n, B] (float64) of the header's real spherical harmonics at unit vectors dirs [n, 3]."""
    B = _check_basis(B)
    u = np.asarray(dirs, np.float64).reshape(-1, 3)
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    Y = [np.full_like(x, _C0), -_C1 * y, _C1 * z, -_C1 * x, _C2 * (x * y), -_C2 * (y * z), _C20 * (((2.0 * z) * z - x * x) - y * y), -_C2 * (x * z),
         _C22 * (x * x - y * y)]
    return np.stack(Y[:B], 1)


def fibonacci_directions(D: int) -> np.ndarray:
    """D unit vectors [D, 3] (float64) on the spherical Fibonacci spiral: near-uniform for any D, no randomness."""
    if D < 1:
        raise MiNerfError(f"D={D}: at least one direction")
    i = np.arange(D, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / D
    phi = 2.0 * math.pi * i / ((1.0 + math.sqrt(5.0)) / 2.0)
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def projection_matrix(D: int = 32, B: int = 9) -> np.ndarray:
    """pinv(Y) [B, D] (float64) of the basis at fibonacci_directions(D): the least-squares coefficients of D colour samples.  For
    D = 9 .. 64 the condition number of Y runs from 2.1 to 1.01 and pinv(Y) Y = I to 4e-15."""
    B = _check_basis(B)
    if not B <= D <= _vox.MAX_DIRS:
        raise MiNerfError(f"D={D}: B={B} .. {_vox.MAX_DIRS} directions")
    return np.linalg.pinv(sh_basis(fibonacci_directions(D), B))


# ---------------------------------------------------------------------------------------------------
# the grid
# ---------------------------------------------------------------------------------------------------
class Views:
    """The training cameras for ``RadianceGrid.seen``: ``H`` rows, ``W`` columns, the harness's ``K`` ([[fx, 0, cx], [0, fy, cy], ...]) and
    camera-to-world ``poses`` [V,3,4] or [V,4,4] (a tensor on any device, or host numbers).  The values are read to the host once, here, as
    mesh.Camera does; ``poses`` is kept as float32 [V,3,4]."""

    def __init__(self, H: int, W: int, K, poses):
        k = K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)
        p = np.asarray(poses.detach().cpu().numpy() if isinstance(poses, torch.Tensor) else poses, dtype=np.float32)
        if p.ndim != 3 or p.shape[1:] not in ((3, 4), (4, 4)):
            raise MiNerfError(f"poses must be [V,3,4] or [V,4,4], got {list(p.shape)}")
        self.H, self.W = int(H), int(W)
        self.fx, self.fy, self.cx, self.cy = (float(np.float32(v)) for v in (k[0][0], k[1][1], k[0][2], k[1][2]))
        self.poses = np.ascontiguousarray(p[:, :3, :4])

    def __len__(self) -> int:
        return int(self.poses.shape[0])


class RadianceGrid:
    """``sigma`` float [P_z, P_y, P_x], ``coef`` float [P_z, P_y, P_x, R], ``skip`` uint8 [B_z, B_y, B_x] on ``device`` (THE GRID of the
    header); None until ``allocate`` / ``bake`` / ``load``.  ``signed=True``: A SIGNED GRID of the header -- ``sigma`` holds the density
    before its ReLU, of any sign, and ``render``, ``build_skip`` and ``compact`` go through the signed entries; ``resample`` and
    ``prune(tau)`` keep the flag.  What reads sigma without the ReLU (``seen``, ``prune(seen=)``, ``render_backward_rays``, baked_pose)
    refuses a signed grid."""

    def __init__(self, lo, hi, res, B: int = 9, signed: bool = False):
        # the box is fp32, as the library reads it: what save() writes is what load() reads
        self.lo, self.hi, self.res = _triple(lo, lambda v: float(np.float32(v))), _triple(hi, lambda v: float(np.float32(v))), _triple(res, int)
        self.B = _check_basis(B)
        self.signed = bool(signed)
        self.sigma: Optional[torch.Tensor] = None
        self.coef: Optional[torch.Tensor] = None
        self.skip: Optional[torch.Tensor] = None
        g = self.c_grid()
        if int(_vox.lib().mi_vox_skip_bytes(C.byref(g))) == 0:
            raise MiNerfError(f"the grid is refused: {_vox.last_error()}")

    # ---- shape ---------------------------------------------------------------------------------------
    def c_grid(self) -> Grid:
        return Grid((C.c_float * 3)(*self.lo), (C.c_float * 3)(*self.hi), (C.c_int32 * 3)(*self.res))

    @property
    def points(self) -> Tuple[int, int, int]:
        """(P_z, P_y, P_x)"""
        return tuple(r + 1 for r in reversed(self.res))

    @property
    def record_floats(self) -> int:
        return int(_vox.lib().mi_vox_record_floats(self.B))

    @property
    def skip_shape(self) -> Tuple[int, int, int]:
        return tuple(-(-r // _vox.BLOCK) for r in reversed(self.res))

    @property
    def device(self):
        return None if self.sigma is None else self.sigma.device

    @property
    def nbytes(self) -> int:
        """Bytes of the three arrays (whether or not they are allocated)."""
        n = self.points[0] * self.points[1] * self.points[2]
        return 4 * n * (1 + self.record_floats) + self.skip_shape[0] * self.skip_shape[1] * self.skip_shape[2]

    def cell_edge(self) -> float:
        """The smallest cell edge."""
        return min((np.float32(self.hi[i]) - np.float32(self.lo[i])) / np.float32(self.res[i]) for i in range(3)).item()

    def allocate(self, device) -> "RadianceGrid":
        """Zero arrays on ``device``: an empty scene."""
        device = torch.device(device)
        self.sigma = torch.zeros(self.points, dtype=torch.float32, device=device)
        self.coef = torch.zeros(*self.points, self.record_floats, dtype=torch.float32, device=device)
        self.skip = torch.zeros(self.skip_shape, dtype=torch.uint8, device=device)
        return self

    def to(self, device) -> "RadianceGrid":
        self._need()
        self.sigma, self.coef, self.skip = (t.to(device) for t in (self.sigma, self.coef, self.skip))
        return self

    def _need(self) -> None:
        if self.sigma is None or self.coef is None or self.skip is None:
            raise MiNerfError("the grid holds nothing yet: bake(), bake_field(), allocate() or load() first")

    def _need_unsigned(self, what: str) -> None:
        if self.signed:
            raise MiNerfError(f"{what} is not defined on a signed grid: its rule reads sigma without the ReLU (include/mi_nerf_vox.h, A SIGNED GRID)")

    # ---- the library's entries -----------------------------------------------------------------------
    def project(self, raw: torch.Tensor, proj: torch.Tensor, index: torch.Tensor, write_sigma: bool = True) -> "RadianceGrid":
        """mi_vox_project: raw [M, D, 4], proj [B, D], index [M] (int64 flat lattice indices, distinct) -> records (and sigma)."""
        self._need()
        dev = self.sigma.device
        if raw.dim() != 3 or raw.shape[2] != 4 or tuple(proj.shape) != (self.B, raw.shape[1]) or tuple(index.shape) != (raw.shape[0],):
            raise MiNerfError(f"raw [M,D,4], proj [{self.B},D] and index [M] expected, got {tuple(raw.shape)} / {tuple(proj.shape)} / {tuple(index.shape)}")
        g = self.c_grid()
        with ops._guard(dev):
            _vox.check(_vox.lib().mi_vox_project(C.byref(g), self.B, int(raw.shape[1]), dev_ptr(raw, "raw", torch.float32, 16), dev_ptr(proj, "proj"),
                                                 dev_ptr(index, "index", torch.int64, 8), int(raw.shape[0]),
                                                 dev_ptr(self.sigma, "sigma") if write_sigma else None, dev_ptr(self.coef, "coef", torch.float32, 16),
                                                 stream_ptr(dev)), "mi_vox_project")
        return self

    def build_skip(self) -> "RadianceGrid":
        """mi_vox_build_skip (a signed grid: mi_vox_build_skip_signed): the empty-space plane from sigma."""
        self._need()
        dev = self.sigma.device
        g = self.c_grid()
        name = "mi_vox_build_skip_signed" if self.signed else "mi_vox_build_skip"
        with ops._guard(dev):
            _vox.check(getattr(_vox.lib(), name)(C.byref(g), dev_ptr(self.sigma.detach(), "sigma"), dev_ptr(self.skip, "skip", torch.uint8, 1), stream_ptr(dev)),
                       name)
        return self

    def render(self, rays: torch.Tensor, step: Optional[float] = None, near: float = 0.0, far: float = math.inf, T_min: float = 0.0,
               bg=(1.0, 1.0, 1.0), skip: bool = True, want_all: bool = True, visited: bool = False):
        """(rgb [n,3], disp [n], acc [n], depth [n]) of rays [n,6] by THE RENDER RULE (mi_vox_render); ``want_all=False``: rgb alone, the
        other outputs are not written; ``visited=True`` appends the per-ray count of fetched samples (int32).  ``step=None``: half the
        smallest cell edge.  The default background is white, as the path's compositing always uses."""
        self._need()
        dev = self.sigma.device
        if not isinstance(rays, torch.Tensor) or rays.dim() != 2 or rays.shape[1] != 6:
            raise MiNerfError(f"rays [n,6] expected, got {tuple(rays.shape) if isinstance(rays, torch.Tensor) else type(rays).__name__}")
        if rays.device != dev:
            raise MiNerfError(f"rays live on {rays.device}, the grid on {dev}")
        n = rays.shape[0]
        cfg = RenderCfg(float(0.5 * self.cell_edge() if step is None else step), float(near), float(far), float(T_min),
                        (C.c_float * 3)(*(float(v) for v in bg)), int(bool(skip)))
        rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
        disp, acc, depth = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3)) if want_all else (None, None, None)
        seen = torch.empty(n, dtype=torch.int32, device=dev) if visited else None
        with ops._guard(dev):
            self._launch_render(rays, n, cfg, rgb, disp, acc, depth, seen, dev)
        out = (rgb, disp, acc, depth) if want_all else (rgb,)
        out = out + (seen,) if visited else out
        return out if len(out) > 1 else out[0]

    def _launch_render(self, rays, n, cfg, rgb, disp, acc, depth, seen, dev) -> None:
        g = self.c_grid()
        name = "mi_vox_render_signed" if self.signed else "mi_vox_render"
        _vox.check(getattr(_vox.lib(), name)(C.byref(g), self.B, dev_ptr(self.sigma, "sigma"), dev_ptr(self.coef, "coef", torch.float32, 16),
                                             dev_ptr(self.skip, "skip", torch.uint8, 1), dev_ptr(rays, "rays"), n, C.byref(cfg), dev_ptr(rgb, "rgb"),
                                             dev_ptr(disp, "disp"), dev_ptr(acc, "acc"), dev_ptr(depth, "depth"),
                                             dev_ptr(seen, "visited", torch.int32), stream_ptr(dev)), name)

    def render_backward_rays(self, rays: torch.Tensor, g_rgb: torch.Tensor, g_acc: Optional[torch.Tensor] = None,
                             g_depth: Optional[torch.Tensor] = None, step: Optional[float] = None, near: float = 0.0, far: float = math.inf,
                             T_min: float = 0.0, bg=(1.0, 1.0, 1.0), skip: bool = True, check: bool = False):
        """d_rays [n,6], the gradient of a loss on ``render``'s rgb, acc and depth with respect to rays [n,6] under g_rgb [n,3] (and g_acc,
        g_depth [n]; None: zeros) by THE RAY GRADIENT RULE (mi_vox_render_backward_rays): written, not added, bit-identical from run to run
        and equal with and without the skip plane.  ``check=True`` returns (d_rays, rgb [n,3], acc [n], depth [n]): the forward the entry
        recomputed, ``render``'s own bits.  The other arguments are ``render``'s."""
        self._need()
        self._need_unsigned("render_backward_rays (THE RAY GRADIENT RULE)")
        dev = self.sigma.device
        if not isinstance(rays, torch.Tensor) or rays.dim() != 2 or rays.shape[1] != 6:
            raise MiNerfError(f"rays [n,6] expected, got {tuple(rays.shape) if isinstance(rays, torch.Tensor) else type(rays).__name__}")
        if rays.device != dev:
            raise MiNerfError(f"rays live on {rays.device}, the grid on {dev}")
        n = rays.shape[0]
        if not isinstance(g_rgb, torch.Tensor) or tuple(g_rgb.shape) != (n, 3) or any(t is not None and tuple(t.shape) != (n,) for t in (g_acc, g_depth)):
            raise MiNerfError(f"g_rgb [{n},3] and g_acc, g_depth [{n}] expected")
        cfg = RenderCfg(float(0.5 * self.cell_edge() if step is None else step), float(near), float(far), float(T_min),
                        (C.c_float * 3)(*(float(v) for v in bg)), int(bool(skip)))
        d_rays = torch.empty(n, 6, dtype=torch.float32, device=dev)
        rgb = torch.empty(n, 3, dtype=torch.float32, device=dev) if check else None
        acc, depth = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2)) if check else (None, None)
        with ops._guard(dev):
            self._launch_ray_grad(rays, n, cfg, (dev_ptr(g_rgb, "g_rgb"), dev_ptr(g_acc, "g_acc"), dev_ptr(g_depth, "g_depth"), dev_ptr(d_rays, "d_rays"),
                                                 dev_ptr(rgb, "rgb_check"), dev_ptr(acc, "acc_check"), dev_ptr(depth, "depth_check"), stream_ptr(dev)))
        return (d_rays, rgb, acc, depth) if check else d_rays

    def _launch_ray_grad(self, rays, n, cfg, tail) -> None:
        g = self.c_grid()
        _vox.check(_vox.lib().mi_vox_render_backward_rays(C.byref(g), self.B, dev_ptr(self.sigma.detach(), "sigma"),
                                                          dev_ptr(self.coef.detach(), "coef", torch.float32, 16), dev_ptr(self.skip, "skip", torch.uint8, 1),
                                                          dev_ptr(rays, "rays"), n, C.byref(cfg), *tail), "mi_vox_render_backward_rays")

    def compact(self, storage: str = "fp32") -> "SparseRadianceGrid":
        """The same grid as a SparseRadianceGrid: mi_vox_index, one read-back of the count, mi_vox_pack.  sigma and skip are copies."""
        self._need()
        out = SparseRadianceGrid(self.lo, self.hi, self.res, self.B, storage, signed=self.signed)
        out.sigma, out.skip = self.sigma.clone(), self.skip.clone()
        out.index()
        out.table = out.empty_table(out.count)
        out.pack(self.coef, out.table, out.count, slot=out.slot)
        return out

    def to_signed(self) -> "RadianceGrid":
        """A signed grid (``signed=True``) for a plane that only knows inside and outside: sigma stays where it is > 0 and becomes minus the
        largest sigma of the 26 neighbours (clipped to the lattice) elsewhere, so that the zero crossing of the interpolation lies half way
        between a dense point and an empty neighbour and not at the empty one.  Away from density the plane stays 0.  The records are
        copies, and the skip plane has the same blocks: a point that turns negative has a neighbour with density in every block that holds
        it.  Torch ops on the dense plane (as ``fill_shell``): not the hot path."""
        self._need()
        if self.signed:
            raise MiNerfError("the grid is signed already")
        out = RadianceGrid(self.lo, self.hi, self.res, self.B, signed=True)
        with torch.no_grad():
            s = self.sigma.detach()
            best = torch.nn.functional.max_pool3d(s.clamp_min(0.0)[None, None], 3, stride=1, padding=1)[0, 0]      # -inf padding: clipped
            out.sigma = torch.where(s > 0, s, -best).contiguous()
            out.coef = self.coef.detach().clone()
            out.skip = torch.empty_like(self.skip)
        return out.build_skip()

    # ---- coarse to fine ------------------------------------------------------------------------------
    def resample(self, res, lo=None, hi=None) -> "RadianceGrid":
        """mi_vox_resample: a new dense grid of resolution ``res`` on the box (lo, hi) -- this grid's own by default -- that holds this
        grid's content by THE RESAMPLING RULE, with its skip plane built.  A multiple of the resolution on the same box represents the
        identical field; a smaller box crops, a larger one extends the faces.  This grid is left as it is."""
        self._need()
        dev = self.sigma.device
        out = RadianceGrid(self.lo if lo is None else lo, self.hi if hi is None else hi, res, self.B, signed=self.signed)
        out.sigma = torch.empty(out.points, dtype=torch.float32, device=dev)
        out.coef = torch.empty(*out.points, out.record_floats, dtype=torch.float32, device=dev)
        out.skip = torch.empty(out.skip_shape, dtype=torch.uint8, device=dev)
        gs, gd = self.c_grid(), out.c_grid()
        with ops._guard(dev):
            _vox.check(_vox.lib().mi_vox_resample(C.byref(gs), C.byref(gd), self.B, dev_ptr(self.sigma.detach(), "sigma"),
                                                  dev_ptr(self.coef.detach(), "coef", torch.float32, 16), dev_ptr(out.sigma, "sigma_dst"),
                                                  dev_ptr(out.coef, "coef_dst", torch.float32, 16), stream_ptr(dev)), "mi_vox_resample")
        return out.build_skip()

    def prune(self, tau: float, seen: Optional[torch.Tensor] = None, T_vis: float = 1e-3) -> "RadianceGrid":
        """mi_vox_prune: a point stays when it or one of its 26 neighbours has sigma > tau; everywhere else sigma becomes 0 and the record
        zero (THE PRUNING RULE).  The new sigma plane replaces the old one and the skip plane is rebuilt.
        With ``seen`` (the plane ``self.seen(views)`` returns) a neighbour counts only if some view sees it with transmittance at least
        ``T_vis`` as well: mi_vox_prune_seen with od_max = -log(T_vis) (THE SEEN PRUNING RULE)."""
        self._need()
        dev = self.sigma.device
        if seen is not None:
            self._need_unsigned("prune(seen=) (THE SEEN PRUNING RULE)")
            if not isinstance(seen, torch.Tensor) or tuple(seen.shape) != self.points or seen.device != dev:
                raise MiNerfError(f"seen must be the grid's od plane {self.points} on {dev}: what seen(views) returns")
            if not (isinstance(T_vis, (int, float)) and 0.0 <= T_vis <= 1.0):
                raise MiNerfError(f"T_vis={T_vis!r}: a transmittance, 0 .. 1")
            od_max = float(np.float32(-math.log(T_vis))) if T_vis > 0.0 else math.inf      # formed in double, rounded once
        kept = torch.empty_like(self.sigma)
        g = self.c_grid()
        with ops._guard(dev):
            if seen is None:
                _vox.check(_vox.lib().mi_vox_prune(C.byref(g), self.B, float(tau), dev_ptr(self.sigma.detach(), "sigma"), dev_ptr(kept, "sigma_out"),
                                                   dev_ptr(self.coef.detach(), "coef", torch.float32, 16), stream_ptr(dev)), "mi_vox_prune")
            else:
                _vox.check(_vox.lib().mi_vox_prune_seen(C.byref(g), self.B, float(tau), od_max, dev_ptr(self.sigma.detach(), "sigma"), dev_ptr(seen, "seen"),
                                                        dev_ptr(kept, "sigma_out"), dev_ptr(self.coef.detach(), "coef", torch.float32, 16), stream_ptr(dev)),
                           "mi_vox_prune_seen")
        self.sigma = kept.requires_grad_(self.sigma.requires_grad)
        return self.build_skip()

    # ---- visibility ----------------------------------------------------------------------------------
    def view_slices(self, views: "Views", step: Optional[float] = None):
        """Per view of ``views`` a mi_vox_view whose slices of depth ``step`` cover the box: depth_near is the smallest camera depth of the
        box's eight corners clamped at 0, the number of slices reaches past the largest, rounded up to a multiple of 8."""
        step = float(np.float32(0.5 * self.cell_edge() if step is None else step))
        if not (math.isfinite(step) and step > 0.0):
            raise MiNerfError(f"step={step!r} must be a positive finite number")
        corners = np.array([[(self.lo, self.hi)[(e >> i) & 1][i] for i in range(3)] for e in range(8)], np.float64)
        out = []
        for pose in views.poses.astype(np.float64):
            z = -((corners - pose[:, 3]) @ pose[:, :3])[:, 2]                               # camera depth: -(R^T (x - t))_z
            near = float(np.float32(max(float(z.min()), 0.0)))
            K = 8 * max(1, -(-(int(math.floor(max(float(z.max()) - near, 0.0) / step)) + 1) // 8))
            if K > _vox.MAX_STEPS:
                raise MiNerfError(f"step={step:g} cuts the box into {K} slices along a view, more than {_vox.MAX_STEPS}")
            out.append(_vox.View(views.H, views.W, views.fx, views.fy, views.cx, views.cy, (C.c_float * 12)(*pose.reshape(-1).tolist()), near, step, K))
        return out

    def seen(self, views: "Views", step: Optional[float] = None, bias: int = 2, skip: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The od plane, float [P_z, P_y, P_x]: the smallest optical depth under which any of ``views`` sees each lattice point, +inf where
        none looks (THE SHADOW RULE and THE VISIBILITY RULE, one mi_vox_shadow + mi_vox_seen pair per view through one scratch volume).
        exp(-od) is the best transmittance a view has to the point.  ``step`` is the depth of a slice (default: the renderer's default
        step), ``bias`` the shadow-map bias in slices, ``skip`` uses the grid's skip plane (the result is the same bit for bit),
        ``out`` a plane to reuse."""
        self._need()
        self._need_unsigned("seen (THE SHADOW RULE)")
        dev = self.sigma.device
        if not isinstance(views, Views):
            raise MiNerfError(f"views: a baked.Views expected, got {type(views).__name__}")
        if out is None:
            out = torch.empty(self.points, dtype=torch.float32, device=dev)
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != self.points or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
            raise MiNerfError(f"out must be a contiguous float32 plane {self.points} on {dev}")
        out.fill_(math.inf)
        cviews = self.view_slices(views, step)
        L = _vox.lib()
        need = 0
        for v in cviews:
            n = int(L.mi_vox_shadow_bytes(C.byref(v)))
            if n == 0:
                raise MiNerfError(f"the view is refused: {_vox.last_error()}")
            need = max(need, n)
        if not cviews:
            return out
        tvol = torch.empty(need // 4, dtype=torch.float32, device=dev)
        g = self.c_grid()
        sigma = self.sigma.detach()
        with ops._guard(dev):
            for v in cviews:
                _vox.check(L.mi_vox_shadow(C.byref(g), dev_ptr(sigma, "sigma"), dev_ptr(self.skip, "skip", torch.uint8, 1) if skip else None, C.byref(v),
                                           dev_ptr(tvol, "tvol", torch.float32, 32), stream_ptr(dev)), "mi_vox_shadow")
                _vox.check(L.mi_vox_seen(C.byref(g), C.byref(v), dev_ptr(tvol, "tvol", torch.float32, 32), int(bias), dev_ptr(out, "od"), stream_ptr(dev)),
                           "mi_vox_seen")
        return out

    # ---- baking --------------------------------------------------------------------------------------
    def bake(self, model_or_packed, network: str = "fine", D: int = 32, sigma_min: float = 0.0, precision=None,
             slab_points: int = SLAB_POINTS, shell: str = "field", signed: Optional[bool] = None, clip: Optional[float] = None) -> "RadianceGrid":
        """Bake one network: sigma from mesh.density_lattice (values <= sigma_min become 0), colour from one-sample rays through
        ops.mlp_rays (fp32) at every point within one lattice step of density.  ``signed=True`` (default: the grid's own flag) makes this a
        signed grid whose plane is the density lattice without the ReLU, clamped to [-clip, clip] when ``clip`` is given.  See
        ``bake_field``."""
        self.signed = self.signed if signed is None else bool(signed)
        from . import mesh
        from .weights import packed_for
        packed = packed_for(model_or_packed)                                # packed once for the lattice and the colour rays
        dev, net, blob = mesh._blob(packed, network, mesh.check_precision(None))
        density = mesh.density_lattice(packed, self.lo, self.hi, self.res, network=network, precision=precision)
        return bake_field(lambda rays, z: ops.mlp_rays(net, blob, rays, z), self.lo, self.hi, self.res, B=self.B, D=D, sigma_min=sigma_min,
                          slab_points=slab_points, device=dev, density=density, grid=self, shell=shell, signed=self.signed, clip=clip)

    # ---- persistence ---------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """npz: lo, hi, res, B and the three arrays; a signed grid adds the field ``signed`` (a file without it holds an unsigned grid)."""
        self._need()
        flag = dict(signed=np.asarray(1, np.int32)) if self.signed else {}
        np.savez_compressed(path, lo=np.asarray(self.lo, np.float32), hi=np.asarray(self.hi, np.float32), res=np.asarray(self.res, np.int32),
                            B=np.asarray(self.B, np.int32), **flag, sigma=self.sigma.detach().cpu().numpy(), coef=self.coef.cpu().numpy(), skip=self.skip.cpu().numpy())

    @classmethod
    def load(cls, path: str, device=None) -> "RadianceGrid":
        with np.load(path, allow_pickle=False) as f:
            grid = cls(f["lo"].tolist(), f["hi"].tolist(), f["res"].tolist(), int(f["B"]), signed=bool(int(f["signed"])) if "signed" in f.files else False)
            sigma, coef, skip = (torch.from_numpy(np.ascontiguousarray(f[k])) for k in ("sigma", "coef", "skip"))
        if tuple(sigma.shape) != grid.points or tuple(coef.shape) != grid.points + (grid.record_floats,) or tuple(skip.shape) != grid.skip_shape:
            raise MiNerfError(f"{path}: the arrays do not fit the grid ({tuple(sigma.shape)}, {tuple(coef.shape)}, {tuple(skip.shape)})")
        grid.sigma, grid.coef, grid.skip = sigma.float(), coef.float(), skip.to(torch.uint8)
        return grid.to(device) if device is not None else grid


STORAGES = {"fp32": (_vox.FMT_F32, torch.float32), "f16": (_vox.FMT_F16, torch.float16)}


class SparseRadianceGrid(RadianceGrid):
    """THE COMPACT GRID of the header: ``sigma`` and ``skip`` as in a RadianceGrid, ``slot`` int32 [P_z, P_y, P_x] (the record number of an
    active point, -1 elsewhere), ``table`` [count, R] float32 (``storage="fp32"``) or float16 (``"f16"``), ``count`` the number of active
    points.  ``coef`` stays None: there is no dense record array.  Renders bit for bit what the dense grid with the same records renders."""

    def __init__(self, lo, hi, res, B: int = 9, storage: str = "fp32", signed: bool = False):
        if storage not in STORAGES:
            raise MiNerfError(f"storage={storage!r}: 'fp32' or 'f16'")
        super().__init__(lo, hi, res, B, signed=signed)
        self.storage = storage
        self.slot: Optional[torch.Tensor] = None
        self.table: Optional[torch.Tensor] = None
        self.count = 0

    @property
    def fmt(self) -> int:
        return STORAGES[self.storage][0]

    @property
    def record_bytes(self) -> int:
        return int(_vox.lib().mi_vox_record_bytes(self.B, self.fmt))

    @property
    def nbytes(self) -> int:
        """The real bytes: sigma, slot, skip and ``count`` records."""
        n = self.points[0] * self.points[1] * self.points[2]
        return 8 * n + self.count * self.record_bytes + self.skip_shape[0] * self.skip_shape[1] * self.skip_shape[2]

    def empty_table(self, count: int, device=None) -> torch.Tensor:
        return torch.empty(count, self.record_floats, dtype=STORAGES[self.storage][1], device=self.sigma.device if device is None else device)

    def allocate(self, device) -> "SparseRadianceGrid":
        """An empty scene on ``device``: no active point, no record."""
        device = torch.device(device)
        self.sigma = torch.zeros(self.points, dtype=torch.float32, device=device)
        self.slot = torch.full(self.points, -1, dtype=torch.int32, device=device)
        self.skip = torch.zeros(self.skip_shape, dtype=torch.uint8, device=device)
        self.count, self.table = 0, self.empty_table(0, device)
        return self

    def to(self, device) -> "SparseRadianceGrid":
        self._need()
        self.sigma, self.slot, self.table, self.skip = (t.to(device) for t in (self.sigma, self.slot, self.table, self.skip))
        return self

    def _need(self) -> None:
        if self.sigma is None or self.slot is None or self.table is None or self.skip is None:
            raise MiNerfError("the grid holds nothing yet: bake(), bake_field(), RadianceGrid.compact(), allocate() or load() first")

    def project(self, *args, **kwargs):
        raise MiNerfError("a SparseRadianceGrid has no dense record array to project into: bake_field(..., storage='sparse') fills its table")

    def resample(self, *args, **kwargs):
        raise MiNerfError("a SparseRadianceGrid has no dense record array to resample: refine the dense grid, then compact()")

    def prune(self, *args, **kwargs):
        raise MiNerfError("a SparseRadianceGrid has no dense record array to prune: refine the dense grid, then compact()")

    def to_signed(self):
        raise MiNerfError("a SparseRadianceGrid is made signed on the dense grid: to_signed(), then compact()")

    # ---- the library's entries -----------------------------------------------------------------------
    def index(self) -> "SparseRadianceGrid":
        """mi_vox_index: ``slot`` and ``count`` from ``sigma`` (the count is read back once)."""
        if self.sigma is None:
            raise MiNerfError("index() needs sigma")
        dev = self.sigma.device
        g = self.c_grid()
        need = int(_vox.lib().mi_vox_index_scratch_bytes(C.byref(g)))
        self.slot = torch.empty(self.points, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        with ops._guard(dev):
            _vox.check(_vox.lib().mi_vox_index(C.byref(g), dev_ptr(self.sigma, "sigma"), dev_ptr(self.slot, "slot", torch.int32), dev_ptr(count, "count", torch.int64, 8),
                                               dev_ptr(scratch, "scratch", torch.uint8, 16), need, stream_ptr(dev)), "mi_vox_index")
        self.count = int(count.item())
        return self

    def pack(self, src: torch.Tensor, table: torch.Tensor, count: int, slot: Optional[torch.Tensor] = None) -> None:
        """mi_vox_pack into ``table`` (a view of the table's rows from an even record number on): from a dense coef array with ``slot``, or
        from ``count`` fp32 records one to one without."""
        dev = table.device
        g = self.c_grid()
        with ops._guard(dev):
            _vox.check(_vox.lib().mi_vox_pack(C.byref(g), self.B, self.fmt, dev_ptr(src, "src", torch.float32, 16) if count else None,
                                              dev_ptr(slot, "slot", torch.int32), int(count),
                                              dev_ptr(table, "table", STORAGES[self.storage][1], 16) if count else None, stream_ptr(dev)), "mi_vox_pack")

    def _launch_render(self, rays, n, cfg, rgb, disp, acc, depth, seen, dev) -> None:
        g = self.c_grid()
        name = "mi_vox_render_sparse_signed" if self.signed else "mi_vox_render_sparse"
        _vox.check(getattr(_vox.lib(), name)(C.byref(g), self.B, self.fmt, dev_ptr(self.sigma, "sigma"), dev_ptr(self.slot, "slot", torch.int32),
                                             dev_ptr(self.table, "table", STORAGES[self.storage][1], 16) if self.count else None, self.count,
                                             dev_ptr(self.skip, "skip", torch.uint8, 1), dev_ptr(rays, "rays"), n, C.byref(cfg), dev_ptr(rgb, "rgb"),
                                             dev_ptr(disp, "disp"), dev_ptr(acc, "acc"), dev_ptr(depth, "depth"),
                                             dev_ptr(seen, "visited", torch.int32), stream_ptr(dev)), name)

    def _launch_ray_grad(self, rays, n, cfg, tail) -> None:
        g = self.c_grid()
        _vox.check(_vox.lib().mi_vox_render_sparse_backward_rays(C.byref(g), self.B, self.fmt, dev_ptr(self.sigma, "sigma"),
                                                                 dev_ptr(self.slot, "slot", torch.int32),
                                                                 dev_ptr(self.table, "table", STORAGES[self.storage][1], 16) if self.count else None,
                                                                 self.count, dev_ptr(self.skip, "skip", torch.uint8, 1), dev_ptr(rays, "rays"), n,
                                                                 C.byref(cfg), *tail), "mi_vox_render_sparse_backward_rays")

    def compact(self, storage: str = "fp32") -> "SparseRadianceGrid":
        raise MiNerfError("the grid is compact already")

    def to_dense(self) -> RadianceGrid:
        """A RadianceGrid with the same records (binary16 widened exactly); inactive points hold zero records.  Torch ops: works on any device."""
        self._need()
        out = RadianceGrid(self.lo, self.hi, self.res, self.B, signed=self.signed)
        out.sigma, out.skip = self.sigma.clone(), self.skip.clone()
        out.coef = torch.zeros(*self.points, self.record_floats, dtype=torch.float32, device=self.sigma.device)
        where = (self.slot >= 0) & (self.slot < self.count)
        out.coef[where] = self.table[self.slot[where].long()].float()
        return out

    # ---- baking --------------------------------------------------------------------------------------
    def bake(self, model_or_packed, network: str = "fine", D: int = 32, sigma_min: float = 0.0, precision=None,
             slab_points: int = SLAB_POINTS, shell: str = "field", signed: Optional[bool] = None, clip: Optional[float] = None) -> "SparseRadianceGrid":
        """RadianceGrid.bake without a dense record array: see ``bake_field(..., storage=...)``."""
        self.signed = self.signed if signed is None else bool(signed)
        from . import mesh
        from .weights import packed_for
        packed = packed_for(model_or_packed)
        dev, net, blob = mesh._blob(packed, network, mesh.check_precision(None))
        density = mesh.density_lattice(packed, self.lo, self.hi, self.res, network=network, precision=precision)
        return bake_field(lambda rays, z: ops.mlp_rays(net, blob, rays, z), self.lo, self.hi, self.res, B=self.B, D=D, sigma_min=sigma_min,
                          slab_points=slab_points, device=dev, density=density, grid=self, shell=shell,
                          storage="sparse16" if self.storage == "f16" else "sparse", signed=self.signed, clip=clip)

    # ---- persistence ---------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """npz: lo, hi, res, B, storage and the four arrays; a signed grid adds the field ``signed``."""
        self._need()
        flag = dict(signed=np.asarray(1, np.int32)) if self.signed else {}
        np.savez_compressed(path, lo=np.asarray(self.lo, np.float32), hi=np.asarray(self.hi, np.float32), res=np.asarray(self.res, np.int32),
                            B=np.asarray(self.B, np.int32), storage=np.asarray(self.storage), **flag, sigma=self.sigma.cpu().numpy(), slot=self.slot.cpu().numpy(),
                            table=self.table.cpu().numpy(), skip=self.skip.cpu().numpy())

    @classmethod
    def load(cls, path: str, device=None) -> "SparseRadianceGrid":
        with np.load(path, allow_pickle=False) as f:
            grid = cls(f["lo"].tolist(), f["hi"].tolist(), f["res"].tolist(), int(f["B"]), str(f["storage"]),
                       signed=bool(int(f["signed"])) if "signed" in f.files else False)
            sigma, slot, table, skip = (torch.from_numpy(np.ascontiguousarray(f[k])) for k in ("sigma", "slot", "table", "skip"))
        if (tuple(sigma.shape) != grid.points or tuple(slot.shape) != grid.points or table.dim() != 2 or table.shape[1] != grid.record_floats
                or tuple(skip.shape) != grid.skip_shape or table.dtype != STORAGES[grid.storage][1]):
            raise MiNerfError(f"{path}: the arrays do not fit the grid ({tuple(sigma.shape)}, {tuple(slot.shape)}, {tuple(table.shape)} {table.dtype}, {tuple(skip.shape)})")
        grid.sigma, grid.slot, grid.table, grid.skip, grid.count = sigma.float(), slot.to(torch.int32), table, skip.to(torch.uint8), int(table.shape[0])
        return grid.to(device) if device is not None else grid


def fill_shell(grid: RadianceGrid) -> RadianceGrid:
    """Every point with sigma == 0 that has a neighbour (of the 26) with sigma > 0 takes the mean of those neighbours' records (torch ops:
    baking is not the hot path).  Points with density and points without such a neighbour keep their records."""
    grid._need()
    dense = (grid.sigma > 0).to(torch.float32)[None, None]
    count = torch.nn.functional.avg_pool3d(dense, 3, stride=1, padding=1)[0, 0]              # (dense neighbours) / 27, zero padding
    shell = ~(grid.sigma > 0) & (count > 0)                                                 # sigma == 0; on a signed grid sigma <= 0
    for c in range(3 * grid.B):                                                             # plane by plane: no second copy of the table
        plane = grid.coef[..., c]
        mean = torch.nn.functional.avg_pool3d((plane * dense[0, 0])[None, None], 3, stride=1, padding=1)[0, 0] / count.clamp_min(1e-9)
        grid.coef[..., c] = torch.where(shell, mean, plane)
    return grid


def lattice_positions(lo, hi, res, index: torch.Tensor) -> torch.Tensor:
    """x [M, 3] (fp32, on index's device) of the lattice points with flat indices ``index``: x_i(j) = lo_i + (float)j_i * step_i, product
    and sum rounded once each, step_i formed on the host in fp32 -- the rule of the header."""
    f32 = np.float32
    lo, hi, res = _triple(lo, float), _triple(hi, float), _triple(res, int)
    Px, Py = res[0] + 1, res[1] + 1
    j = (index % Px, (index // Px) % Py, index // (Px * Py))
    cols = []
    for i in range(3):
        step = float((f32(hi[i]) - f32(lo[i])) / f32(res[i]))
        cols.append(j[i].to(torch.float32) * step + float(f32(lo[i])))
    return torch.stack(cols, -1)


def bake_field(fn: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], lo, hi, res, B: int = 9, D: int = 32, sigma_min: float = 0.0,
               slab_points: int = SLAB_POINTS, device="cuda:0", density: Optional[torch.Tensor] = None,
               grid: Optional[RadianceGrid] = None, shell: str = "field", storage: str = "dense", signed: Optional[bool] = None,
               clip: Optional[float] = None) -> RadianceGrid:
    """Bake any field ``fn(rays [n,6], z [n,S]) -> raw [n,S,4]`` (a network's fused entry, ``SolidScene.field``) into a RadianceGrid.
      1. sigma: ``density`` [P_z, P_y, P_x] (raw, before the ReLU) when given, else fn over the lattice rows of mesh.lattice_rows; values
         <= sigma_min (and NaN) become 0.
      2. the active points: those within one lattice step (all 26 neighbours) of a point with sigma > 0.
      3. slab by slab, D one-sample rays (x, omega_j) with depth 0 per active point go through fn; mi_vox_project writes the records.
         Inactive points keep zero records.
      4. mi_vox_build_skip.
    ``shell``: what the active points WITHOUT density hold (the one-step shell around the density, which every sample that straddles a
    surface interpolates with).  "field" (default): the field's own colour there, as at every active point -- right for a network, whose
    colour branch is continuous across its surfaces.  "neighbours": the mean of the records of the point's neighbours (of the 26) that
    have density -- for a field whose colour outside its solids means nothing (``SolidScene.field``: frames come out washed with that
    colour otherwise, docs/design/22_radiance_grid.md).
    ``storage``: "dense" (default) | "sparse" | "sparse16" -- the last two give a SparseRadianceGrid (fp32 / binary16 records) and never
    allocate a dense record array: after sigma, mi_vox_index numbers the active points, the table of that many records is allocated, and
    step 3 projects slab by slab into the table with record numbers as mi_vox_project's index list (for binary16 into a slab-sized fp32
    buffer that mi_vox_pack converts into the table).  The result equals the dense bake's ``compact()`` bit for bit.  shell="neighbours"
    works on the dense table only.
    ``signed=True`` (default: the flag of ``grid``, False without one) gives A SIGNED GRID of the header: the plane is the density lattice
    WITHOUT the ReLU -- a NaN becomes 0, a value <= sigma_min that is > 0 becomes 0 as before, a negative value stays -- clamped to
    [-clip, clip] when ``clip`` (> 0) is given: a network's density before its ReLU can be far more negative than it is ever positive, and
    the size of the negative side sets how far the optimiser must walk to open a point.  Records are stored where the unsigned bake's
    active stencil puts them (it tests sigma > 0)."""
    from . import mesh
    if storage not in ("dense", "sparse", "sparse16"):
        raise MiNerfError(f"storage={storage!r}: 'dense', 'sparse' or 'sparse16'")
    sparse = storage != "dense"
    if sparse and shell == "neighbours":
        raise MiNerfError("shell='neighbours' fills the shell on the dense table: bake dense, then compact()")
    if grid is None:
        grid = (SparseRadianceGrid(lo, hi, res, B, "f16" if storage == "sparse16" else "fp32", signed=bool(signed)) if sparse else
                RadianceGrid(lo, hi, res, B, signed=bool(signed)))
    elif signed is not None:
        grid.signed = bool(signed)
    if clip is not None and not (grid.signed and isinstance(clip, (int, float)) and math.isfinite(clip) and clip > 0):
        raise MiNerfError(f"clip={clip!r}: a finite number > 0, for a signed bake only")
    if isinstance(grid, SparseRadianceGrid) != sparse or (sparse and grid.storage != ("f16" if storage == "sparse16" else "fp32")):
        raise MiNerfError(f"storage={storage!r} does not fit the grid handed in ({type(grid).__name__})")
    dev = torch.device(device)
    if slab_points < 1:
        raise MiNerfError(f"slab_points={slab_points}: at least one point per slab")
    if shell not in ("field", "neighbours"):
        raise MiNerfError(f"shell={shell!r}: 'field' or 'neighbours'")
    proj = torch.from_numpy(projection_matrix(D, grid.B).astype(np.float32)).to(dev).contiguous()
    omega = torch.from_numpy(fibonacci_directions(D).astype(np.float32)).to(dev)
    Pz, Py, Px = grid.points
    with torch.no_grad():
        if density is None:
            rows, z = mesh.lattice_rows(grid.lo, grid.hi, grid.res, dev)
            per = max(1, slab_points // Px)
            density = torch.cat([fn(rows[a:a + per].contiguous(), z[a:a + per].contiguous())[..., 3] for a in range(0, rows.shape[0], per)]).reshape(Pz, Py, Px)
        density = as_f32_dev(density, dev)
        if tuple(density.shape) != grid.points:
            raise MiNerfError(f"density must be {grid.points}, got {tuple(density.shape)}")
        big = torch.finfo(torch.float32).max
        sigma = torch.where(density > float(sigma_min), density, torch.zeros_like(density)).clamp_(min=0.0, max=big)
        if grid.signed:                                                          # the negative side as the field gives it; a NaN fails both tests
            bound = big if clip is None else float(clip)
            sigma = torch.where(density < 0, density, sigma).clamp_(min=-bound, max=bound)
        if sparse:
            return _bake_sparse(fn, grid, sigma.contiguous(), proj, omega, D, slab_points)
        grid.allocate(dev)
        grid.sigma.copy_(sigma)
        active = torch.nn.functional.max_pool3d((sigma > 0).to(torch.float32)[None, None], 3, stride=1, padding=1)[0, 0] > 0
        index = torch.nonzero(active.reshape(-1)).reshape(-1)
        for a in range(0, index.numel(), slab_points):
            idx = index[a:a + slab_points].contiguous()
            x = lattice_positions(grid.lo, grid.hi, grid.res, idx)
            m = idx.numel()
            rays = torch.cat([x[:, None, :].expand(m, D, 3), omega[None].expand(m, D, 3)], -1).reshape(m * D, 6).contiguous()
            raw = fn(rays, torch.zeros(m * D, 1, dtype=torch.float32, device=dev)).reshape(m, D, 4)
            grid.project(raw, proj, idx, write_sigma=False)
        if shell == "neighbours":
            fill_shell(grid)
        grid.build_skip()
    return grid


def _bake_sparse(fn, grid: "SparseRadianceGrid", sigma: torch.Tensor, proj: torch.Tensor, omega: torch.Tensor, D: int, slab_points: int) -> "SparseRadianceGrid":
    """Steps 2 to 4 of bake_field into a compact grid (under no_grad): sigma | mi_vox_index | the table | slabs of records | skip."""
    dev = sigma.device
    grid.sigma = sigma
    grid.skip = torch.zeros(grid.skip_shape, dtype=torch.uint8, device=dev)
    grid.index()
    grid.table = grid.empty_table(grid.count)
    index = torch.nonzero(grid.slot.reshape(-1) >= 0).reshape(-1)          # flat lattice indices in record order
    slab = slab_points + (slab_points & 1)                                   # slabs start at even record numbers: 16-byte aligned at 8 bytes a record
    half = grid.storage == "f16"
    buf = torch.empty(min(slab, grid.count), grid.record_floats, dtype=torch.float32, device=dev) if half else None
    c_grid = grid.c_grid()
    for a in range(0, grid.count, slab):
        idx = index[a:a + slab].contiguous()
        x = lattice_positions(grid.lo, grid.hi, grid.res, idx)
        m = idx.numel()
        rays = torch.cat([x[:, None, :].expand(m, D, 3), omega[None].expand(m, D, 3)], -1).reshape(m * D, 6).contiguous()
        raw = fn(rays, torch.zeros(m * D, 1, dtype=torch.float32, device=dev)).reshape(m, D, 4)
        # record numbers as the index list: straight into the fp32 table, or into the buffer from record 0
        record = torch.arange(0 if half else a, m if half else a + m, dtype=torch.int64, device=dev)
        with ops._guard(dev):
            _vox.check(_vox.lib().mi_vox_project(C.byref(c_grid), grid.B, D, dev_ptr(raw, "raw", torch.float32, 16), dev_ptr(proj, "proj"),
                                                 dev_ptr(record, "index", torch.int64, 8), m, None,
                                                 dev_ptr(buf if half else grid.table, "coef", torch.float32, 16), stream_ptr(dev)), "mi_vox_project")
        if half:
            grid.pack(buf, grid.table[a:a + m], m)
    grid.build_skip()
    return grid
