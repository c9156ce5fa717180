"""ctypes binding of libmi_nerf_scene.so (include/mi_nerf_scene.h): procedural solid-object scenes.

A table of its own: ``_lib.SIGNATURES`` mirrors include/mi_nerf.h and does not know these entries.  The library stands alone (it links
against no other library of the package).  Like the rest of the package there is NO fallback: a missing library or a failed call raises
``MiNerfError``.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import loader

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmi_nerf_scene.so")
ABI_VERSION = 1
MAX_PRIMS, MAX_SAMPLES = 16, 4096                     # MI_SCENE_MAX_PRIMS, MI_SCENE_MAX_SAMPLES
SPHERE, BOX, CYLINDER = 0, 1, 2                       # MI_SCENE_SPHERE, MI_SCENE_BOX, MI_SCENE_CYLINDER


class Prim(C.Structure):              # mi_scene_prim
    _fields_ = [("kind", C.c_int32), ("axis", C.c_int32), ("c", C.c_float * 3), ("h", C.c_float * 3), ("sigma", C.c_float),
                ("rgb_raw", (C.c_float * 3) * 2), ("freq", C.c_float)]


_P, _I, _I64, _F = C.c_void_p, C.c_int, C.c_int64, C.c_float
_PRIMP = C.POINTER(Prim)

# name -> (restype, argtypes); mirrors include/mi_nerf_scene.h declaration by declaration
SIGNATURES = {
    "mi_scene_abi_version": (_I, []),
    "mi_scene_last_error": (C.c_char_p, []),
    "mi_scene_check": (_I, [_PRIMP, _I]),
    "mi_scene_field_rays": (_I, [_PRIMP, _I, _P, _P, _I64, _I, _P, _P]),
    "mi_scene_render": (_I, [_PRIMP, _I, _P, _I64, _F, _F, _I, _P, _P, _P, _P, _P]),
}

lib, check, last_error = loader(globals(), "mi_scene")
