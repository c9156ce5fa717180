"""ctypes binding of libmi_nerf_mesh.so (include/mi_nerf_mesh.h): triangle meshes from a density lattice.

A table of its own: ``_lib.SIGNATURES`` mirrors include/mi_nerf.h and does not know these entries.  The library links against
libmi_nerf.so (rpath $ORIGIN) and calls its three fused network entries.  Like the rest of the package there is NO fallback: a missing
library or a failed call raises ``MiNerfError``.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _lib
from ._lib import Net, loader

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmi_nerf_mesh.so")
ABI_VERSION = 1
MAX_RES, MIN_SLAB_POINTS, SCAN_TILE = 512, 1024, 1024          # MI_MESH_MAX_RES, MI_MESH_MIN_SLAB_POINTS, MI_MESH_SCAN_TILE


class Grid(C.Structure):              # mi_mesh_grid
    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3), ("res", C.c_int32 * 3)]


_P, _I, _U64, _F, _SZ = C.c_void_p, C.c_int, C.c_uint64, C.c_float, C.c_size_t
_GRIDP, _NETP = C.POINTER(Grid), C.POINTER(Net)

# name -> (restype, argtypes); mirrors include/mi_nerf_mesh.h declaration by declaration
SIGNATURES = {
    "mi_mesh_abi_version": (_I, []),
    "mi_mesh_last_error": (C.c_char_p, []),
    "mi_mesh_density_scratch_bytes": (_SZ, [_GRIDP]),
    "mi_mesh_density": (_I, [_GRIDP, _NETP, _P, _I, _P, _P, _SZ, _P]),
    "mi_mesh_extract_scratch_bytes": (_SZ, [_GRIDP]),
    "mi_mesh_count": (_I, [_GRIDP, _P, _F, _P, _SZ, _P, _P]),
    "mi_mesh_emit": (_I, [_GRIDP, _P, _F, _P, _SZ, _U64, _U64, _P, _P, _P, _P]),
}

lib, check, last_error = loader(globals(), "mi_mesh", first=_lib.lib)
