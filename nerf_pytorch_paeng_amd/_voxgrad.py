"""ctypes binding of libmi_nerf_voxgrad.so (include/mi_nerf_voxgrad.h): the backward pass of the radiance-grid renderer.

A table of its own: ``_lib.SIGNATURES`` mirrors include/mi_nerf.h and does not know these entries.  The library stands alone (it links
against no other library of the package); its grid and configuration structs have the layout of ``_vox.Grid`` / ``_vox.RenderCfg``.  Like
the rest of the package there is NO fallback: a missing library or a failed call raises ``MiNerfError``.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import loader

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmi_nerf_voxgrad.so")
ABI_VERSION = 1
MAX_RES, BLOCK, MAX_STEPS = 512, 8, 65536                         # MI_VOXGRAD_MAX_RES / _BLOCK / _MAX_STEPS


class Grid(C.Structure):              # mi_voxgrad_grid
    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3), ("res", C.c_int32 * 3)]


class RenderCfg(C.Structure):         # mi_voxgrad_render_cfg
    _fields_ = [("step", C.c_float), ("t_near", C.c_float), ("t_far", C.c_float), ("T_min", C.c_float), ("bg", C.c_float * 3),
                ("use_skip", C.c_int32)]


_P, _I, _I64 = C.c_void_p, C.c_int, C.c_int64
_GRIDP, _CFGP = C.POINTER(Grid), C.POINTER(RenderCfg)

# name -> (restype, argtypes); mirrors include/mi_nerf_voxgrad.h declaration by declaration
SIGNATURES = {
    "mi_voxgrad_abi_version": (_I, []),
    "mi_voxgrad_last_error": (C.c_char_p, []),
    "mi_voxgrad_render_backward": (_I, [_GRIDP, _I, _P, _P, _P, _P, _I64, _CFGP, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
}

lib, check, last_error = loader(globals(), "mi_voxgrad")
