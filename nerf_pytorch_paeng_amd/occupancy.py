"""Occupancy-grid rendering (include/mi_nerf_occ.h, libmi_nerf_occ.so): skip the network at samples a baked density grid marks empty.

    grid = OccupancyGrid(lo=(-1.5,) * 3, hi=(1.5,) * 3, res=128)
    grid.bake(model)                                  # both networks' density, 2^3 points per cell, dilated by one cell
    out = nerf_process.render_rays(rays, model, posenc, opts, occupancy=grid)

A skipped sample's raw output is (0, 0, 0, 0), which ``post_process`` turns into weight 0 exactly: the render is the staged reference path
with raw zeroed where ``grid.mark(rays, z)`` is 0.  Inference only (``torch.no_grad()``); fp32, ``f16s`` and ``bf16``.  The render call
synchronises its stream once per network pass (the tile count goes to the host) and cannot be captured into a graph.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _occ, ops
from ._lib import MiNerfError, Net, RenderCfg, as_f32_dev, dev_ptr, stream_ptr
from ._occ import Grid, Stats, WorkspaceLayout

# rays handed to one mi_occ_render_rays call (workspace: ~12 KB/ray at 64+128 samples)
MAX_RAYS_PER_LAUNCH = 1 << 17
_OCC_FAMILIES = ("fp32", "f16s", "bf16")


def _triple(v, cast) -> Tuple:
    if isinstance(v, (int, float)):
        return (cast(v),) * 3
    t = tuple(cast(x) for x in v)
    if len(t) != 3:
        raise MiNerfError(f"expected a scalar or three values, got {v!r}")
    return t


def check_precision(prec: "ops.Precision") -> "ops.Precision":
    """The occupancy path runs one kernel family for both networks: fp32, f16s or bf16 with the launch shape chosen per launch."""
    if prec.coarse != prec.fine or prec.fine not in _OCC_FAMILIES or prec.points_per_wave != 0:
        raise MiNerfError(f"the occupancy path runs fp32, f16s or bf16 for both networks (got coarse {prec.coarse}, fine {prec.fine})")
    return prec


def workspace_layout(cfg: RenderCfg, n: int) -> WorkspaceLayout:
    wl = WorkspaceLayout()
    _occ.check(_occ.lib().mi_occ_render_workspace_layout(C.byref(cfg), int(n), C.byref(wl)), "mi_occ_render_workspace_layout")
    return wl


def workspace_views(cfg: RenderCfg, n: int, workspace: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Typed views of the intermediates inside an occupancy render workspace (staged parity checks)."""
    wl = workspace_layout(cfg, n)
    Sc, St = cfg.Sc, cfg.Sc + cfg.Nf

    def view(off, shape):
        cnt = int(np.prod(shape))
        return workspace[off:off + cnt * 4].view(torch.float32).view(*shape)
    v = {"z_c": view(wl.z_c, (n, Sc)), "raw_c": view(wl.raw_c, (n, Sc, 4)), "weights_c": view(wl.weights_c, (n, Sc))}
    if cfg.Nf > 0:
        v["z_f"] = view(wl.z_f, (n, St))
        v["raw_f"] = view(wl.raw_f, (n, St, 4))
    return v


def tile_views(cfg: RenderCfg, n: int, workspace: torch.Tensor, tiles: int) -> Dict[str, torch.Tensor]:
    """What the cull kernel left of the LAST network pass (the fine one when Nf > 0): ``slot`` int32 [n, S] (flat tile lane of each sample,
    -1 = skipped) and the first ``tiles`` tiles -- ``tile_rays`` [tiles, 6], ``tile_z`` [tiles, 32], ``tile_src`` int32 [tiles, 32] (ray * S +
    sample, -1 = padding), ``tile_raw`` [tiles, 32, 4]."""
    wl = workspace_layout(cfg, n)
    S = cfg.Sc + cfg.Nf

    def view(off, shape, dtype=torch.float32):
        cnt = int(np.prod(shape))
        return workspace[off:off + cnt * 4].view(dtype).view(*shape)
    return {"slot": view(wl.slot, (n, S), torch.int32), "tile_rays": view(wl.tile_rays, (tiles, 6)), "tile_z": view(wl.tile_z, (tiles, 32)),
            "tile_src": view(wl.tile_src, (tiles, 32), torch.int32), "tile_raw": view(wl.tile_raw, (tiles, 32, 4))}


class OccupancyGrid:
    """One bit per cell of an axis-aligned box, on the device.  ``res``: an int or (rx, ry, rz), each 1..512.  ``outside_occupied``: samples
    outside the box are evaluated (True, conservative) or skipped (False).  The box lives in the rays' space: NDC rays need an NDC box."""

    def __init__(self, lo, hi, res, outside_occupied: bool = True):
        self.lo, self.hi, self.res = _triple(lo, float), _triple(hi, float), _triple(res, int)
        self.outside_occupied = bool(outside_occupied)
        self.bits: Optional[torch.Tensor] = None          # int32 [words] on the device: the uint32 words of the header
        self.last_stats: Optional[Dict[str, int]] = None  # mi_occ_stats of the last render_rays / batchify call that used this grid (summed over slabs)
        self.words = int(_occ.lib().mi_occ_grid_words(C.byref(self.c_grid())))
        if self.words == 0:
            raise MiNerfError(f"mi_occ_grid_words refused the grid: {_occ.last_error()}")

    @property
    def cells(self) -> int:
        return self.res[0] * self.res[1] * self.res[2]

    def c_grid(self) -> Grid:
        return Grid((C.c_float * 3)(*self.lo), (C.c_float * 3)(*self.hi), (C.c_int32 * 3)(*self.res), int(self.outside_occupied))

    def _need_bits(self) -> torch.Tensor:
        if self.bits is None:
            raise MiNerfError("the occupancy grid has no bits yet: bake() it, load() one, or set_bits()")
        return self.bits

    def set_bits(self, bits) -> "OccupancyGrid":
        """Take a bitfield: an int32 / uint32 array or tensor of ``words`` words (bit b of the header: word b // 32, bit b % 32)."""
        if isinstance(bits, np.ndarray):
            bits = torch.from_numpy(np.ascontiguousarray(bits).view(np.int32).copy())
        if bits.dtype != torch.int32 or bits.dim() != 1 or bits.numel() != self.words:
            raise MiNerfError(f"bits must be {self.words} int32 words, got {tuple(bits.shape)} {bits.dtype}")
        self.bits = bits.contiguous()
        return self

    def to(self, device) -> "OccupancyGrid":
        if self.bits is not None:
            self.bits = self.bits.to(device)
        return self

    # ---- baking ------------------------------------------------------------------------------------
    def bake(self, model_or_packed, sub: int = 2, sigma_min: float = 0.0, dilate: int = 1, networks: Sequence[str] = ("coarse", "fine"),
             **precision) -> "OccupancyGrid":
        """Set a cell's bit iff a listed network's raw density exceeds ``sigma_min`` at any of the cell's ``sub``^3 lattice points, then OR
        every bit over its (2 ``dilate`` + 1)^3 neighbourhood.  ``precision``: bf16=True / f16s=True (default fp32)."""
        from .weights import packed_for
        prec = check_precision(ops.precision(**precision))
        if not networks or any(k not in ("coarse", "fine") for k in networks):
            raise MiNerfError(f"networks must name 'coarse' and / or 'fine', got {networks!r}")
        packed = packed_for(model_or_packed)
        net, blob_c, blob_f = packed.kernel_blobs(prec)
        dev = packed.device
        L = _occ.lib()
        g = self.c_grid()
        nbytes = int(L.mi_occ_bake_scratch_bytes(C.byref(g), int(sub)))
        if nbytes == 0:
            raise MiNerfError(f"mi_occ_bake refused: {_occ.last_error()}")
        sampled = torch.empty(self.words, dtype=torch.int32, device=dev)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with ops._guard(dev):
            for i, which in enumerate(networks):
                blob = blob_f if which == "fine" else blob_c
                _occ.check(L.mi_occ_bake(C.byref(g), dev_ptr(sampled, "bits", torch.int32), C.byref(net), dev_ptr(blob, "packed", torch.uint8, 16),
                                         prec.mode, int(sub), float(sigma_min), int(i > 0), dev_ptr(scratch, "scratch", torch.uint8, 256), nbytes,
                                         stream_ptr(dev)), "mi_occ_bake")
        self.bits = sampled
        if int(dilate) > 0:
            self.bits = self.dilated(int(dilate))
        return self

    def dilated(self, radius: int) -> torch.Tensor:
        """The bitfield ORed over each cell's (2 radius + 1)^3 neighbourhood (a new tensor; the grid's own bits stay)."""
        bits = self._need_bits()
        out = torch.empty_like(bits)
        with ops._guard(bits.device):
            _occ.check(_occ.lib().mi_occ_dilate(C.byref(self.c_grid()), dev_ptr(bits, "bits", torch.int32), dev_ptr(out, "out", torch.int32), int(radius),
                                                stream_ptr(bits.device)), "mi_occ_dilate")
        return out

    def count(self) -> int:
        """Occupied cells (one 8-byte device -> host read)."""
        bits = self._need_bits()
        out = torch.empty(1, dtype=torch.int64, device=bits.device)
        with ops._guard(bits.device):
            _occ.check(_occ.lib().mi_occ_count(C.byref(self.c_grid()), dev_ptr(bits, "bits", torch.int32), dev_ptr(out, "count", torch.int64, 8),
                                               stream_ptr(bits.device)), "mi_occ_count")
        return int(out.item())

    def fraction(self) -> float:
        """Share of the cells that are occupied."""
        return self.count() / self.cells

    def mark(self, rays: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
        """uint8 [n, S]: 1 where the sample (rays [n,6], z [n,S]) would be evaluated (mi_occ_mark: the cell rule of the header)."""
        bits = self._need_bits()
        rays, z = as_f32_dev(rays, bits.device), as_f32_dev(z, bits.device)
        n, S = z.shape
        if tuple(rays.shape) != (n, 6):
            raise MiNerfError(f"rays must be [n,6], got {tuple(rays.shape)}")
        mask = torch.empty(n, S, dtype=torch.uint8, device=bits.device)
        with ops._guard(bits.device):
            _occ.check(_occ.lib().mi_occ_mark(C.byref(self.c_grid()), dev_ptr(bits, "bits", torch.int32), dev_ptr(rays, "rays"), dev_ptr(z, "z"), n, S,
                                              dev_ptr(mask, "mask", torch.uint8, 1), stream_ptr(bits.device)), "mi_occ_mark")
        return mask

    # ---- persistence -------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """npz: lo, hi, res, outside_occupied and the uint32 words."""
        np.savez_compressed(path, lo=np.asarray(self.lo, np.float32), hi=np.asarray(self.hi, np.float32), res=np.asarray(self.res, np.int32),
                            outside_occupied=np.asarray(int(self.outside_occupied), np.int32), bits=self._need_bits().cpu().numpy().view(np.uint32))

    @classmethod
    def load(cls, path: str, device=None) -> "OccupancyGrid":
        with np.load(path, allow_pickle=False) as f:
            grid = cls(f["lo"].tolist(), f["hi"].tolist(), f["res"].tolist(), bool(int(f["outside_occupied"])))
            grid.set_bits(f["bits"])
        return grid.to(device) if device is not None else grid


# ------------------------------------------------------------------------------------------------
def render_rays(net: Net, packed_c: torch.Tensor, packed_f: Optional[torch.Tensor], cfg: RenderCfg, grid: OccupancyGrid, rays: torch.Tensor,
                t_rand: Optional[torch.Tensor], u: Optional[torch.Tensor], workspace: Optional[torch.Tensor] = None,
                bits_fine: Optional[torch.Tensor] = None):
    """One mi_occ_render_rays call.  Returns (rgb_c, disp_c, rgb_f|None, disp_f|None, workspace, stats dict).  ``bits_fine``: a bitfield of
    its own for the fine network (default: the grid's).  Synchronises the stream once per network pass."""
    n = rays.shape[0]
    dev = rays.device
    bits = grid._need_bits()
    if bits.device != dev:
        raise MiNerfError(f"the occupancy grid lives on {bits.device}, the rays on {dev}")
    if tuple(rays.shape) != (n, 6) or (t_rand is not None and tuple(t_rand.shape) != (n, cfg.Sc)):
        raise MiNerfError(f"rays [n,6] / t_rand [n,{cfg.Sc}] expected, got {tuple(rays.shape)} / {None if t_rand is None else tuple(t_rand.shape)}")
    if cfg.Nf > 0 and not cfg.det and u is not None and tuple(u.shape) != (n, cfg.Nf):
        raise MiNerfError(f"u [n,{cfg.Nf}] expected")
    wl = workspace_layout(cfg, n)
    if workspace is None or workspace.numel() < wl.total:
        workspace = torch.empty(max(wl.total, 256), dtype=torch.uint8, device=dev)
    rgb_c = torch.empty(n, 3, dtype=torch.float32, device=dev)
    disp_c = torch.empty(n, dtype=torch.float32, device=dev)
    rgb_f = torch.empty(n, 3, dtype=torch.float32, device=dev) if cfg.Nf > 0 else None
    disp_f = torch.empty(n, dtype=torch.float32, device=dev) if cfg.Nf > 0 else None
    st = Stats()
    with ops._guard(dev):
        _occ.check(_occ.lib().mi_occ_render_rays(
            C.byref(net), dev_ptr(packed_c, "packed_coarse", torch.uint8, 16), dev_ptr(packed_f, "packed_fine", torch.uint8, 16), C.byref(cfg),
            C.byref(grid.c_grid()), dev_ptr(bits, "bits", torch.int32), dev_ptr(bits if bits_fine is None else bits_fine, "bits_fine", torch.int32),
            dev_ptr(rays, "rays"), n, dev_ptr(t_rand, "t_rand"), dev_ptr(u, "u") if (cfg.Nf > 0 and not cfg.det) else None,
            dev_ptr(workspace, "workspace", torch.uint8, 256), workspace.numel(), dev_ptr(rgb_c), dev_ptr(disp_c), dev_ptr(rgb_f), dev_ptr(disp_f),
            C.byref(st), stream_ptr(dev)), "mi_occ_render_rays")
    return rgb_c, disp_c, rgb_f, disp_f, workspace, {k: int(getattr(st, k)) for k, _ in Stats._fields_}


def add_stats(a: Optional[Dict[str, int]], b: Dict[str, int]) -> Dict[str, int]:
    return dict(b) if a is None else {k: a[k] + b[k] for k in b}


def evaluated_share(stats: Dict[str, int]) -> float:
    """Surviving samples of both passes over all samples of both passes."""
    return (stats["evaluated_c"] + stats["evaluated_f"]) / max(1, stats["total_c"] + stats["total_f"])


def padded_share(stats: Dict[str, int]) -> float:
    """Padding lanes run through the networks over all samples of both passes."""
    return (stats["padded_c"] + stats["padded_f"]) / max(1, stats["total_c"] + stats["total_f"])
