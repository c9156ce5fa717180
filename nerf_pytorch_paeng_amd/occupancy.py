"""Occupancy-grid rendering (include/mi_nerf_occ.h, libmi_nerf_occ.so): skip the network at samples a baked density grid marks empty.

    grid = OccupancyGrid(lo=(-1.5,) * 3, hi=(1.5,) * 3, res=128)
    grid.bake(model)                                  # both networks' density, 2^3 points per cell, dilated by one cell
    out = nerf_process.render_rays(rays, model, posenc, opts, occupancy=grid)

A skipped sample's raw output is (0, 0, 0, 0), which ``post_process`` turns into weight 0 exactly: the render is the staged reference path
with raw zeroed where ``grid.mark(rays, z)`` is 0.  ``occupancy=`` is inference only (``torch.no_grad()``); fp32, ``f16s`` and ``bf16``.  The
render call synchronises its stream once per network pass (the tile count goes to the host) and cannot be captured into a graph.

Training with a grid (``train_occupancy=``, occupancy_train.py) is composed in Python from the deterministic compaction
(``OccupancyGrid.compact``, mi_occ_compact) and the two data movements around the networks (``scatter_raw``, ``gather_raw``).
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
        self.bits_fine: Optional[torch.Tensor] = None     # a bitfield of its own for the fine network in compact() (None: the grid's bits)
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
        if self.bits_fine is not None:
            self.bits_fine = self.bits_fine.to(device)
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

    # ---- deterministic compaction (the training path) ----------------------------------------------
    def compact(self, rays: torch.Tensor, z: torch.Tensor, network: str = "coarse") -> Dict[str, object]:
        """mi_occ_compact: the surviving samples of rays [n,6] / z [n,S] as 32-sample tiles in a reproducible order (THE COMPACTION RULE of
        the header).  ``network``: "coarse" or "fine" -- the fine network reads ``bits_fine`` when the grid has one, else the grid's bits.
        Returns {"tile_rays" [T,6], "tile_z" [T,32], "tile_src" int32 [T,32], "slot" int32 [n,S], "tiles": T, "survivors": sum k_r}; the tile
        tensors are views of the first T tiles.  ONE 8-byte device -> host read (the two counts): the only synchronisation of the pass."""
        if network not in ("coarse", "fine"):
            raise MiNerfError(f"network must be 'coarse' or 'fine', got {network!r}")
        bits = self._need_bits()
        if network == "fine" and self.bits_fine is not None:
            bits = self.bits_fine
        dev = bits.device
        rays, z = as_f32_dev(rays, dev), as_f32_dev(z, dev)
        if z.dim() != 2 or tuple(rays.shape) != (z.shape[0], 6):
            raise MiNerfError(f"rays [n,6] / z [n,S] expected, got {tuple(rays.shape)} / {tuple(z.shape)}")
        n, S = z.shape
        L = _occ.lib()
        nbytes = int(L.mi_occ_compact_scratch_bytes(n))
        if nbytes == 0:
            raise MiNerfError(f"mi_occ_compact refused: {_occ.last_error()}")
        T = n * ((S + _occ.TILE - 1) // _occ.TILE)
        tile_rays = torch.empty(T, 6, dtype=torch.float32, device=dev)
        tile_z = torch.empty(T, _occ.TILE, dtype=torch.float32, device=dev)
        tile_src = torch.empty(T, _occ.TILE, dtype=torch.int32, device=dev)
        slot = torch.empty(n, S, dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with ops._guard(dev):
            _occ.check(L.mi_occ_compact(C.byref(self.c_grid()), dev_ptr(bits, "bits", torch.int32), dev_ptr(rays, "rays"), dev_ptr(z, "z"), n, S,
                                        dev_ptr(tile_rays, "tile_rays"), dev_ptr(tile_z, "tile_z"), dev_ptr(tile_src, "tile_src", torch.int32),
                                        dev_ptr(slot, "slot", torch.int32), dev_ptr(counts, "counts", torch.int32),
                                        dev_ptr(scratch, "scratch", torch.uint8, 256), nbytes, stream_ptr(dev)), "mi_occ_compact")
        tiles, survivors = (int(v) for v in counts.cpu().tolist())
        return {"tile_rays": tile_rays[:tiles], "tile_z": tile_z[:tiles], "tile_src": tile_src[:tiles], "slot": slot, "tiles": tiles,
                "survivors": survivors}

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


def _out_buffer(out: Optional[torch.Tensor], shape, dev) -> torch.Tensor:
    if out is None:
        return torch.empty(*shape, dtype=torch.float32, device=dev)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise MiNerfError(f"out must be a contiguous float32 {tuple(shape)} tensor on {dev}, got {tuple(out.shape)} {out.dtype} on {out.device}")
    return out


def scatter_raw(tile_vals: torch.Tensor, slot: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mi_occ_scatter_raw: tile_vals [T,32,4], slot int32 [n,S] -> [n,S,4]; every element written, zeros where ``slot`` is -1.  ``out``: a
    buffer to write into (every element of it is overwritten)."""
    dev = slot.device
    if slot.dim() != 2 or slot.dtype != torch.int32 or tile_vals.dim() != 3 or tuple(tile_vals.shape[1:]) != (_occ.TILE, 4):
        raise MiNerfError(f"tile_vals [T,32,4] / slot int32 [n,S] expected, got {tuple(tile_vals.shape)} / {tuple(slot.shape)} {slot.dtype}")
    n, S = slot.shape
    if tile_vals.shape[0] == 0:
        tile_vals = torch.zeros(1, _occ.TILE, 4, dtype=torch.float32, device=dev)       # nothing survived: no lane is read, every output is zero
    tile_vals = as_f32_dev(tile_vals, dev)
    out = _out_buffer(out, (n, S, 4), dev)
    with ops._guard(dev):
        _occ.check(_occ.lib().mi_occ_scatter_raw(dev_ptr(tile_vals, "tile_vals", align=16), dev_ptr(slot.contiguous(), "slot", torch.int32), n, S,
                                                 dev_ptr(out, "out", align=16), stream_ptr(dev)), "mi_occ_scatter_raw")
    return out


def gather_raw(src: torch.Tensor, tile_src: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mi_occ_gather_raw: src [n,S,4], tile_src int32 [T,32] -> [T,32,4] = src[tile_src] per lane, exact zeros on padding lanes (-1).
    ``out``: a buffer to write into (every element of it is overwritten)."""
    dev = tile_src.device
    if tile_src.dim() != 2 or tile_src.shape[1] != _occ.TILE or tile_src.dtype != torch.int32 or src.dim() != 3 or src.shape[2] != 4:
        raise MiNerfError(f"src [n,S,4] / tile_src int32 [T,32] expected, got {tuple(src.shape)} / {tuple(tile_src.shape)} {tile_src.dtype}")
    src = as_f32_dev(src, dev)
    T = tile_src.shape[0]
    out = _out_buffer(out, (T, _occ.TILE, 4), dev)
    with ops._guard(dev):
        _occ.check(_occ.lib().mi_occ_gather_raw(dev_ptr(src, "src", align=16), dev_ptr(tile_src.contiguous(), "tile_src", torch.int32), T,
                                                dev_ptr(out, "out", align=16), stream_ptr(dev)), "mi_occ_gather_raw")
    return out


def add_stats(a: Optional[Dict[str, int]], b: Dict[str, int]) -> Dict[str, int]:
    return dict(b) if a is None else {k: a[k] + b[k] for k in b}


def evaluated_share(stats: Dict[str, int]) -> float:
    """Surviving samples of both passes over all samples of both passes."""
    return (stats["evaluated_c"] + stats["evaluated_f"]) / max(1, stats["total_c"] + stats["total_f"])


def padded_share(stats: Dict[str, int]) -> float:
    """Padding lanes run through the networks over all samples of both passes."""
    return (stats["padded_c"] + stats["padded_f"]) / max(1, stats["total_c"] + stats["total_f"])
