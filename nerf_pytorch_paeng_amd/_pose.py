"""ctypes binding of libmi_nerf_pose.so (include/mi_nerf_pose.h): gradients of the training path with respect to rays and camera poses.

A table of its own: ``_lib.SIGNATURES`` mirrors include/mi_nerf.h and does not know these entries.  The library stands alone (it links
against no other library of the package).  Like the rest of the package there is NO fallback: a missing library or a failed call raises
``MiNerfError``.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import loader

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmi_nerf_pose.so")
ABI_VERSION = 1
MAX_LX, MAX_LD = 10, 4                                # MI_POSE_MAX_LX / MI_POSE_MAX_LD

_P, _I, _I64, _F = C.c_void_p, C.c_int, C.c_int64, C.c_float

# name -> (restype, argtypes); mirrors include/mi_nerf_pose.h declaration by declaration
SIGNATURES = {
    "mi_pose_abi_version": (_I, []),
    "mi_pose_last_error": (C.c_char_p, []),
    "mi_pose_input_grad": (_I, [_P, _P, _P, _P, _I64, _I, _P, _P, _P, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "mi_pose_ndc_rays_backward": (_I, [_I, _I, _F, _F, _P, _I64, _P, _I64, _I64, _P, _P, _P, _P, _P]),
    "mi_pose_reduce_scratch_bytes": (C.c_size_t, []),
    "mi_pose_make_o_d_backward": (_I, [_I, _I, _P, _P, _P, _I, _I64, _P, _P, _P, _P, _P, C.c_size_t, _P]),
}

lib, check, last_error = loader(globals(), "mi_pose")
