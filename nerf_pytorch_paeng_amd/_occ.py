"""ctypes binding of libmi_nerf_occ.so (include/mi_nerf_occ.h): occupancy-grid rendering on top of the path.

A table of its own: ``_lib.SIGNATURES`` mirrors include/mi_nerf.h and does not know these entries.  The library links against
libmi_nerf.so (rpath $ORIGIN) and calls its public entries.  Like the rest of the package there is NO fallback: a missing library or a
failed call raises ``MiNerfError``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from . import _lib
from ._lib import MiNerfError, Net, RenderCfg

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

_handle: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load (once) and return the shared library; raise loudly if it is not there."""
    global _handle
    if _handle is None:
        if not os.path.exists(LIB_PATH):
            raise MiNerfError(
                f"{LIB_PATH} not found: build it with `python -m nerf_pytorch_paeng_amd.build` "
                "(hipcc --offload-arch=gfx950).  There is no CPU/PyTorch fallback for this path.")
        _lib.lib()                                  # libmi_nerf.so first: the copy this library's rpath resolves to
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                raise MiNerfError(f"{LIB_PATH} does not export {name}: stale build?") from e
            fn.restype, fn.argtypes = res, args
        v = handle.mi_occ_abi_version()
        if v != ABI_VERSION:
            raise MiNerfError(f"ABI mismatch: library {v}, binding {ABI_VERSION}")
        _handle = handle
    return _handle


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().mi_occ_last_error()
        raise MiNerfError(f"{what} failed (status {rc}): {msg.decode() if msg else '?'}")


def last_error() -> str:
    msg = lib().mi_occ_last_error()
    return msg.decode() if msg else ""
