"""ctypes binding of libmi_nerf_mesh.so (include/mi_nerf_mesh.h): triangle meshes from a density lattice, and views of them.

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
ABI_VERSION = 2
MAX_RES, MIN_SLAB_POINTS, SCAN_TILE = 512, 1024, 1024          # MI_MESH_MAX_RES, MI_MESH_MIN_SLAB_POINTS, MI_MESH_SCAN_TILE
VIEW_MAX_DIM, VIEW_GUARD, VIEW_LARGE_BOX, VIEW_QUEUE = 16384, 1 << 22, 32, 65536      # MI_MESH_VIEW_*


class Grid(C.Structure):              # mi_mesh_grid
    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3), ("res", C.c_int32 * 3)]


class Camera(C.Structure):            # mi_mesh_camera
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("c2w", C.c_float * 12)]


_P, _I, _U64, _F, _SZ = C.c_void_p, C.c_int, C.c_uint64, C.c_float, C.c_size_t
_GRIDP, _NETP, _CAMP, _I64 = C.POINTER(Grid), C.POINTER(Net), C.POINTER(Camera), C.c_int64

# name -> (restype, argtypes); mirrors include/mi_nerf_mesh.h declaration by declaration
SIGNATURES = {
    "mi_mesh_abi_version": (_I, []),
    "mi_mesh_last_error": (C.c_char_p, []),
    "mi_mesh_density_scratch_bytes": (_SZ, [_GRIDP]),
    "mi_mesh_density": (_I, [_GRIDP, _NETP, _P, _I, _P, _P, _SZ, _P]),
    "mi_mesh_extract_scratch_bytes": (_SZ, [_GRIDP]),
    "mi_mesh_count": (_I, [_GRIDP, _P, _F, _P, _SZ, _P, _P]),
    "mi_mesh_emit": (_I, [_GRIDP, _P, _F, _P, _SZ, _U64, _U64, _P, _P, _P, _P]),
    "mi_mesh_project": (_I, [_CAMP, _F, _P, _I64, _P, _P, _P, _P]),
    "mi_mesh_raster_scratch_bytes": (_SZ, [_I, _I]),
    "mi_mesh_raster": (_I, [_I, _I, _I, _I, _P, _P, _P, _I64, _P, _I64, _P, _SZ, _P, _P, _P]),
    "mi_mesh_shade": (_I, [_I, _I, _P, _P, _P, _I64, _P, _I64, _P, _P, _P, C.POINTER(C.c_float), _P, _P, _P, _P, _P, _P]),
}

lib, check, last_error = loader(globals(), "mi_mesh", first=_lib.lib)
