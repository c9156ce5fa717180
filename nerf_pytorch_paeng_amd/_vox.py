"""ctypes binding of libmi_nerf_vox.so (include/mi_nerf_vox.h): the radiance grid -- projection, empty-space plane, renderer.

A table of its own: ``_lib.SIGNATURES`` mirrors include/mi_nerf.h and does not know these entries.  The library stands alone (it links
against no other library of the package).  Like the rest of the package there is NO fallback: a missing library or a failed call raises
``MiNerfError``.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import loader

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmi_nerf_vox.so")
ABI_VERSION = 2
MAX_RES, BLOCK, MAX_DIRS, MAX_STEPS = 512, 8, 256, 65536          # MI_VOX_MAX_RES / _BLOCK / _MAX_DIRS / _MAX_STEPS
FMT_F32, FMT_F16 = 0, 1                                           # MI_VOX_FMT_F32 / _F16: the record formats of the compact grid


class Grid(C.Structure):              # mi_vox_grid
    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3), ("res", C.c_int32 * 3)]


class RenderCfg(C.Structure):         # mi_vox_render_cfg
    _fields_ = [("step", C.c_float), ("t_near", C.c_float), ("t_far", C.c_float), ("T_min", C.c_float), ("bg", C.c_float * 3),
                ("use_skip", C.c_int32)]


class View(C.Structure):              # mi_vox_view
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("c2w", C.c_float * 12), ("depth_near", C.c_float), ("depth_step", C.c_float), ("slices", C.c_int32)]


_P, _I, _I64, _F, _SZ = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
_GRIDP, _CFGP, _VIEWP = C.POINTER(Grid), C.POINTER(RenderCfg), C.POINTER(View)

# name -> (restype, argtypes); mirrors include/mi_nerf_vox.h declaration by declaration
SIGNATURES = {
    "mi_vox_abi_version": (_I, []),
    "mi_vox_last_error": (C.c_char_p, []),
    "mi_vox_record_floats": (_I, [_I]),
    "mi_vox_skip_bytes": (_SZ, [_GRIDP]),
    "mi_vox_max_steps": (_I64, [_GRIDP, _F]),
    "mi_vox_project": (_I, [_GRIDP, _I, _I, _P, _P, _P, _I64, _P, _P, _P]),
    "mi_vox_build_skip": (_I, [_GRIDP, _P, _P, _P]),
    "mi_vox_render": (_I, [_GRIDP, _I, _P, _P, _P, _P, _I64, _CFGP, _P, _P, _P, _P, _P, _P]),
    "mi_vox_record_bytes": (_SZ, [_I, _I]),
    "mi_vox_index_scratch_bytes": (_SZ, [_GRIDP]),
    "mi_vox_index": (_I, [_GRIDP, _P, _P, _P, _P, _SZ, _P]),
    "mi_vox_pack": (_I, [_GRIDP, _I, _I, _P, _P, _I64, _P, _P]),
    "mi_vox_render_sparse": (_I, [_GRIDP, _I, _I, _P, _P, _P, _I64, _P, _P, _I64, _CFGP, _P, _P, _P, _P, _P, _P]),
    "mi_vox_resample": (_I, [_GRIDP, _GRIDP, _I, _P, _P, _P, _P, _P]),
    "mi_vox_prune": (_I, [_GRIDP, _I, _F, _P, _P, _P, _P]),
    "mi_vox_shadow_bytes": (_SZ, [_VIEWP]),
    "mi_vox_shadow": (_I, [_GRIDP, _P, _P, _VIEWP, _P, _P]),
    "mi_vox_seen": (_I, [_GRIDP, _VIEWP, _P, C.c_int32, _P, _P]),
    "mi_vox_prune_seen": (_I, [_GRIDP, _I, _F, _F, _P, _P, _P, _P, _P]),
    "mi_vox_render_backward_rays": (_I, [_GRIDP, _I, _P, _P, _P, _P, _I64, _CFGP, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mi_vox_render_sparse_backward_rays": (_I, [_GRIDP, _I, _I, _P, _P, _P, _I64, _P, _P, _I64, _CFGP, _P, _P, _P, _P, _P, _P, _P, _P]),
    # A SIGNED GRID: the argument lists of mi_vox_build_skip, mi_vox_render and mi_vox_render_sparse
    "mi_vox_build_skip_signed": (_I, [_GRIDP, _P, _P, _P]),
    "mi_vox_render_signed": (_I, [_GRIDP, _I, _P, _P, _P, _P, _I64, _CFGP, _P, _P, _P, _P, _P, _P]),
    "mi_vox_render_sparse_signed": (_I, [_GRIDP, _I, _I, _P, _P, _P, _I64, _P, _P, _I64, _CFGP, _P, _P, _P, _P, _P, _P]),
}

lib, check, last_error = loader(globals(), "mi_vox")
