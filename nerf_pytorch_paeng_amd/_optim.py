"""ctypes binding of libmi_nerf_optim.so (include/mi_nerf_optim.h): the Adam / AdamW step over many small fp32 tensors, plain and guarded.

A table of its own: ``_lib.SIGNATURES`` mirrors include/mi_nerf.h and does not know these entries.  The library stands alone (it links
against no other library of the package).  Like the rest of the package there is NO fallback: a missing library or a failed call raises
``MiNerfError``.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import loader

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmi_nerf_optim.so")
ABI_VERSION = 2
MAX_TENSORS, CHUNK = 80, 4096                         # MI_OPTIM_MAX_TENSORS / MI_OPTIM_CHUNK
CONTROL_WORDS, TSTATE_WORDS = 8, 4                    # MI_OPTIM_CONTROL_WORDS / MI_OPTIM_TSTATE_WORDS


class AdamCfg(C.Structure):      # mi_optim_adam_cfg
    _fields_ = [("size", C.c_uint32), ("decoupled", C.c_int32), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("weight_decay", C.c_double), ("reserved", C.c_uint32 * 2)]


_P, _I, _I64, _F, _SZ = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
_PP, _I64P, _I32P, _CFGP = C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(AdamCfg)
_FP = C.POINTER(C.c_float)

# name -> (restype, argtypes); mirrors include/mi_nerf_optim.h declaration by declaration
SIGNATURES = {
    "mi_optim_abi_version": (_I, []),
    "mi_optim_last_error": (C.c_char_p, []),
    "mi_optim_adam_step": (_I, [_I, _PP, _PP, _I64P, _I64P, _I64P, _P, _P, _I64, _CFGP, _I, _I32P, _P]),
    "mi_optim_adam_step_lazy": (_I, [_I, _PP, _PP, _I64P, _I64P, _I64P, _P, _P, _I64, _CFGP, _I, _I32P, _FP, _I, _P]),
    "mi_optim_grad_stats_scratch_bytes": (_SZ, [_I, _I64P]),
    "mi_optim_grad_stats": (_I, [_I, _PP, _I64P, _CFGP, _I, _I32P, _I32P, _I, _F, _I, _P, _P, _P, _SZ, _P]),
    "mi_optim_adam_step_guarded": (_I, [_I, _PP, _PP, _I64P, _I64P, _P, _P, _I64, _CFGP, _I, _I32P, _I32P, _I, _P, _P, _P]),
}

lib, check, last_error = loader(globals(), "mi_optim")
