"""ctypes binding of libmi_nerf_iqa.so (include/mi_nerf_iqa.h): the image-quality metrics beside the path.

A table of its own: ``_lib.SIGNATURES`` mirrors include/mi_nerf.h and does not know these entries.  Like the rest of the package there
is NO fallback: a missing library or a failed call raises ``MiNerfError``.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import loader

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmi_nerf_iqa.so")
ABI_VERSION = 1
SSIM_CLAMP_CS = 1          # MI_IQA_SSIM_CLAMP_CS
SSIM_TAPS = 11             # MI_IQA_SSIM_TAPS

_P, _I, _I64, _U32, _SZ = C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_size_t

# name -> (restype, argtypes); mirrors include/mi_nerf_iqa.h declaration by declaration
SIGNATURES = {
    "mi_iqa_abi_version": (_I, []),
    "mi_iqa_last_error": (C.c_char_p, []),
    "mi_iqa_ssim_window": (_I, [C.POINTER(C.c_double)]),
    "mi_iqa_ssim_downsample_factor": (_I, [_I, _I, _I]),
    "mi_iqa_ssim_scratch_bytes": (_SZ, [_I64, _I, _I, _I]),
    "mi_iqa_ssim": (_I, [_P, _P, _I64, _I, _I, _I, _U32, _P, _P, _P, _SZ, _P]),
}

lib, check, last_error = loader(globals(), "mi_iqa")


def ssim_window():
    """The 11 normalised window taps the kernel uses (fp64, host side)."""
    taps = (C.c_double * SSIM_TAPS)()
    check(lib().mi_iqa_ssim_window(taps), "mi_iqa_ssim_window")
    return list(taps)
