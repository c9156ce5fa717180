"""ctypes binding of libmi_nerf_geo.so (include/mi_nerf_geo.h): alpha compositing with the gradients of the geometry losses, and
the lattice regularisers of a radiance grid (total variation, sparsity).

A table of its own: ``_lib.SIGNATURES`` mirrors include/mi_nerf.h and does not know these entries.  The library stands alone (it links
against no other library of the package).  Like the rest of the package there is NO fallback: a missing library or a failed call raises
``MiNerfError``.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import loader

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmi_nerf_geo.so")
ABI_VERSION = 2
MAX_SAMPLES = 1024                                    # MI_GEO_MAX_SAMPLES
LATTICE_MAX_POINTS = 513                              # MI_GEO_LATTICE_MAX_POINTS

_P, _I, _I64, _F, _SZ = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
_P3 = C.POINTER(C.c_int32)                            # const int32_t P[3]

# name -> (restype, argtypes); mirrors include/mi_nerf_geo.h declaration by declaration
SIGNATURES = {
    "mi_geo_abi_version": (_I, []),
    "mi_geo_last_error": (C.c_char_p, []),
    "mi_geo_composite": (_I, [_P, _P, _P, _I, _I64, _I, _F, _F, _P, _P, _P, _P, _P, _P, _P]),
    "mi_geo_composite_backward": (_I, [_P, _P, _P, _I, _I64, _I, _F, _F, _P, _P, _P, _P, _P, _P, _P]),
    "mi_geo_lattice_scratch_bytes": (_SZ, [_P3, _I, _I]),
    "mi_geo_lattice_tv": (_I, [_P3, _I, _I, _P, _P, _F, _F, _P, _P, _P, _SZ, _P]),
    "mi_geo_lattice_sparsity": (_I, [_P3, _P, _P, _F, _P, _P, _P, _SZ, _P]),
}

lib, check, last_error = loader(globals(), "mi_geo")
