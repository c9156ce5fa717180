"""ctypes binding of libmi_nerf_lpips.so (include/mi_nerf_lpips.h): the LPIPS perceptual distance beside the path.

A table of its own: ``_lib.SIGNATURES`` mirrors include/mi_nerf.h and does not know these entries.  Like the rest of the package there
is NO fallback: a missing library or a failed call raises ``MiNerfError``.
"""
from __future__ import annotations

import ctypes as C
import os

from ._lib import loader

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmi_nerf_lpips.so")
ABI_VERSION = 1
CONV, POOL, TAP = 1, 2, 3  # MI_LPIPS_CONV / _POOL / _TAP
MAX_OPS = 32               # MI_LPIPS_MAX_OPS
MAX_TAPS = 8               # MI_LPIPS_MAX_TAPS
MAX_COUT = 512             # MI_LPIPS_MAX_COUT
MAX_DIM = 8192             # MI_LPIPS_MAX_DIM


class Op(C.Structure):           # mi_lpips_op
    _fields_ = [("kind", C.c_int32), ("cout", C.c_int32)]


class Net(C.Structure):          # mi_lpips_net
    _fields_ = [("n_ops", C.c_int32), ("cin0", C.c_int32), ("ops", Op * MAX_OPS)]


_P, _I, _I64, _SZ = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
_NETP = C.POINTER(Net)
_FPP = C.POINTER(C.c_void_p)     # const float* const*

# name -> (restype, argtypes); mirrors include/mi_nerf_lpips.h declaration by declaration
SIGNATURES = {
    "mi_lpips_abi_version": (_I, []),
    "mi_lpips_last_error": (C.c_char_p, []),
    "mi_lpips_vgg16": (_I, [_NETP]),
    "mi_lpips_packed_bytes": (_SZ, [_NETP]),
    "mi_lpips_pack_weights": (_I, [_NETP, _FPP, _FPP, _FPP, _P, _P, _P, _SZ]),
    "mi_lpips_scratch_bytes": (_SZ, [_NETP, _I, _I]),
    "mi_lpips_distance": (_I, [_NETP, _P, _SZ, _P, _P, _I64, _I, _I, _P, _P, _P, _SZ, _P]),
    "mi_lpips_features": (_I, [_NETP, _P, _SZ, _P, _I64, _I, _I, _I, _P, _P, _SZ, _P]),
}

lib, check, last_error = loader(globals(), "mi_lpips")


def vgg16() -> Net:
    """The standard plan (mi_lpips_vgg16)."""
    net = Net()
    check(lib().mi_lpips_vgg16(C.byref(net)), "mi_lpips_vgg16")
    return net


def make_net(cin0: int, ops) -> Net:
    """A plan from a list of ("conv", cout) / "pool" / "tap" entries (or the integer kinds).  Nothing is checked here: the library refuses."""
    net = Net()
    net.cin0 = int(cin0)
    ops = list(ops)
    net.n_ops = len(ops)
    kinds = {"conv": CONV, "pool": POOL, "tap": TAP}
    for k, op in enumerate(ops[:MAX_OPS]):
        kind, cout = op if isinstance(op, (tuple, list)) else (op, 0)
        net.ops[k].kind = kinds.get(kind, kind)
        net.ops[k].cout = int(cout)
    return net


def describe(net: Net):
    """(conv (cin, cout) list, tap channel list, pools before each tap) of a plan the library accepts."""
    convs, taps, tap_pools = [], [], []
    c, pools = net.cin0, 0
    for k in range(net.n_ops):
        op = net.ops[k]
        if op.kind == CONV:
            convs.append((c, op.cout))
            c = op.cout
        elif op.kind == POOL:
            pools += 1
        elif op.kind == TAP:
            taps.append(c)
            tap_pools.append(pools)
    return convs, taps, tap_pools
