"""Training with an occupancy grid: the route of the training node (``train_path._RenderTrain``) that evaluates a network only where the
grid says a sample may matter (docs/design/17_occupancy_training.md).  The node, its argument preparation and everything around the two
networks are train_path's; what is specific to the grid is here.

Per network the forward is  compact | ops.mlp_rays_train on the (n', 32) pseudo-rays | scatter_raw | the node's composite  (the fine depths
after the coarse pass, unchanged), the backward  the node's composite backward on the scattered raw | gather_raw | ops.mlp_backward on the
tiles with the stash of the forward.  A skipped sample's raw is (0, 0, 0, 0) as in the inference path, so the step is the full staged step
with raw zeroed where ``grid.mark`` answers 0 and d_raw dropped there; a padding lane evaluates a real point with d_raw = 0 and adds
exactly zero to every weight-gradient and bias sum.  The networks are driven through the public staged entries: libmi_nerf_occ.so calls
none of the training entries of libmi_nerf.so.  One 8-byte device -> host read per network pass (the tile count sizes the network launch).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import occupancy as occ
from . import ops
from . import train_path
from ._lib import MiNerfError

TILE = 32


def check_grid(grid) -> "occ.OccupancyGrid":
    if not isinstance(grid, occ.OccupancyGrid):
        raise MiNerfError(f"train_occupancy must be an occupancy.OccupancyGrid, got {type(grid).__name__}")
    return grid


def new_stats() -> Dict[str, int]:
    return {k: 0 for k in ("total_c", "evaluated_c", "padded_c", "total_f", "evaluated_f", "padded_f")}


class Compacted(train_path.Dense):
    """The route of ``train_path._RenderTrain`` through a grid: the dense one run on the tiles of the samples that survive; what its
    backward needs of the compaction is saved with the node."""
    saves = 3                                                        # tile_rays, tile_z, tile_src

    def __init__(self, grid, dev: torch.device):
        bits = check_grid(grid)._need_bits()
        if bits.device != dev:
            raise MiNerfError(f"the occupancy grid lives on {bits.device}, the model on {dev}")
        self.grid, self.stats = grid, new_stats()

    def forward(self, st, f16s, which, flat, blob, rays, z):
        c = self.grid.compact(rays, z, which)                        # the one host read of the pass
        n_t = c["tiles"]
        key = "c" if which == "coarse" else "f"
        self.stats["total_" + key] += z.numel()
        self.stats["evaluated_" + key] += c["survivors"]
        self.stats["padded_" + key] += n_t * TILE - c["survivors"]
        tiles = (c["tile_rays"], c["tile_z"], c["tile_src"])
        if n_t == 0:                                                 # nothing survived: no network launch, raw is all zeros
            empty = torch.empty(0, TILE, 4, dtype=torch.float32, device=rays.device)
            return occ.scatter_raw(empty, c["slot"]), torch.empty(0, dtype=torch.uint8, device=rays.device), tiles
        ops.train_layout(st.net, n_t, TILE)                          # asked before anything is sized: a shape the kernels refuse raises here
        raw_t, stash, _ = super().forward(st, f16s, which, flat, blob, c["tile_rays"], c["tile_z"])
        return occ.scatter_raw(raw_t, c["slot"]), stash, tiles

    def skipped(self, tiles) -> bool:
        return tiles[2].shape[0] == 0                                # no sample was evaluated: the parameters did not reach the colours

    def backward(self, st, f16s, f16s_dgrad, blob, blob_b, rays, z, d_raw, stash, tiles, stage):
        tile_rays, tile_z, tile_src = tiles
        return super().backward(st, f16s, f16s_dgrad, blob, blob_b, tile_rays, tile_z, occ.gather_raw(d_raw, tile_src), stash, (), stage)


def render_train(rays: torch.Tensor, model: torch.nn.Module, opts, grid, *, t_rand=None, u=None, seed: int = 0, ray_offset: int = 0,
                 z_override=None, det: Optional[bool] = None, f16s: bool = False, geometry: bool = False) -> Dict[str, torch.Tensor]:
    """``train_path.render_train`` with an occupancy grid: same arguments, same defaults for drawn jitter, same outputs.  The sample counts
    of the call go into ``grid.last_stats`` (the keys of mi_occ_stats)."""
    return train_path.render_train(rays, model, opts, t_rand=t_rand, u=u, seed=seed, ray_offset=ray_offset, z_override=z_override, det=det,
                                   f16s=f16s, geometry=geometry, grid=check_grid(grid))
