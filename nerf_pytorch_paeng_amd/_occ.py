"""ctypes binding of libmi_nerf_occ.so (include/mi_nerf_occ.h): occupancy-grid rendering on top of the path.

A table of its own: ``_lib.SIGNATURES`` mirrors include/mi_nerf.h and does not know these entries.  The library links against
libmi_nerf.so (rpath $ORIGIN) and calls its public entries.  Like the rest of the package there is NO fallback: a missing library or a
failed call raises ``MiNerfError``.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _lib
from ._lib import Net, RenderCfg, loader

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmi_nerf_occ.so")
ABI_VERSION = 2
MAX_RES, MAX_SUB, MAX_RADIUS, TILE = 512, 4, 2, 32          # MI_OCC_MAX_RES, MI_OCC_MAX_SUB, MI_OCC_MAX_RADIUS, MI_OCC_TILE


class Grid(C.Structure):              # mi_occ_grid
    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3), ("res", C.c_int32 * 3), ("outside_occupied", C.c_int32)]


class Stats(C.Structure):             # mi_occ_stats
    _fields_ = [(n, C.c_int64) for n in ("total_c", "evaluated_c", "padded_c", "total_f", "evaluated_f", "padded_f")]


class WorkspaceLayout(C.Structure):   # mi_occ_workspace_layout
    _fields_ = [(n, C.c_size_t) for n in ("z_c", "raw_c", "weights_c", "z_f", "raw_f", "t_rand", "u", "slot", "tile_rays", "tile_z", "tile_src",
                                          "tile_raw", "counters", "total")]


_P, _I, _I64, _F, _SZ = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
_GRIDP, _NETP, _CFGP = C.POINTER(Grid), C.POINTER(Net), C.POINTER(RenderCfg)

# name -> (restype, argtypes); mirrors include/mi_nerf_occ.h declaration by declaration
SIGNATURES = {
    "mi_occ_abi_version": (_I, []),
    "mi_occ_last_error": (C.c_char_p, []),
    "mi_occ_grid_words": (_SZ, [_GRIDP]),
    "mi_occ_bake_scratch_bytes": (_SZ, [_GRIDP, _I]),
    "mi_occ_bake": (_I, [_GRIDP, _P, _NETP, _P, _I, _I, _F, _I, _P, _SZ, _P]),
    "mi_occ_dilate": (_I, [_GRIDP, _P, _P, _I, _P]),
    "mi_occ_count": (_I, [_GRIDP, _P, _P, _P]),
    "mi_occ_mark": (_I, [_GRIDP, _P, _P, _P, _I64, _I, _P, _P]),
    "mi_occ_compact_scratch_bytes": (_SZ, [_I64]),
    "mi_occ_compact": (_I, [_GRIDP, _P, _P, _P, _I64, _I, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "mi_occ_scatter_raw": (_I, [_P, _P, _I64, _I, _P, _P]),
    "mi_occ_gather_raw": (_I, [_P, _P, _I64, _P, _P]),
    "mi_occ_render_workspace_bytes": (_SZ, [_CFGP, _I64]),
    "mi_occ_render_workspace_layout": (_I, [_CFGP, _I64, C.POINTER(WorkspaceLayout)]),
    "mi_occ_render_rays": (_I, [_NETP, _P, _P, _CFGP, _GRIDP, _P, _P, _P, _I64, _P, _P, _P, _SZ, _P, _P, _P, _P, C.POINTER(Stats), _P]),
}

lib, check, last_error = loader(globals(), "mi_occ", first=_lib.lib)
