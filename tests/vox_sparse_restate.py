"""THE COMPACT GRID of include/mi_nerf_vox.h restated in numpy, written from the header's comment and not from the kernels: the active
set, the slot plane, the record table in both formats, and the dense grid a compact grid stands for.  The render rule itself is
tests/vox_restate.py's: a compact grid renders as the dense grid ``to_dense`` gives.
"""
from __future__ import annotations

import numpy as np

FMT_F32, FMT_F16 = 0, 1
RECORD = {1: 4, 4: 16, 9: 32}


def record_bytes(B, fmt):
    return RECORD.get(B, 0) * {FMT_F32: 4, FMT_F16: 2}.get(fmt, 0)


def active_set(sigma):
    """bool [P_z, P_y, P_x]: the point or one of its 26 neighbours, clipped to the lattice, has sigma > 0."""
    dense = np.asarray(sigma) > 0
    P = dense.shape
    pad = np.pad(dense, 1)                                  # False outside the lattice: a clipped neighbour adds nothing
    out = np.zeros(P, bool)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                out |= pad[dz:dz + P[0], dy:dy + P[1], dx:dx + P[2]]
    return out


def slots(sigma):
    """(slot int32 [P_z, P_y, P_x], M): at an active point the number of active points with a smaller flat index, -1 elsewhere."""
    act = active_set(sigma)
    flat = act.reshape(-1)
    before = np.cumsum(flat) - flat                         # exclusive running count in flat order
    slot = np.where(flat, before, -1).astype(np.int32).reshape(act.shape)
    return slot, int(flat.sum())


def pack(records, fmt):
    """fp32 records [M, R] in the table's format: unchanged, or IEEE binary16 by round-to-nearest-even (beyond the range: +-inf)."""
    records = np.asarray(records, np.float32)
    if fmt == FMT_F32:
        return records.copy()
    with np.errstate(over="ignore"):
        return records.astype(np.float16)                   # numpy's conversion is round-to-nearest-even, overflow to inf


def table_of(coef, slot, M, fmt):
    """The table of a dense coef array [P_z, P_y, P_x, R]: the record of every point with 0 <= slot < M at table[slot]."""
    coef = np.asarray(coef, np.float32)
    R = coef.shape[-1]
    s = np.asarray(slot).reshape(-1)
    ok = (s >= 0) & (s < M)
    table = np.zeros((M, R), np.float32)
    table[s[ok]] = coef.reshape(-1, R)[ok]
    return pack(table, fmt)


def to_dense(slot, table, M):
    """coef float32 [P_z, P_y, P_x, R] the render rule reads through the slot plane: table[slot] widened exactly; a slot < 0 or >= M is
    a zero record."""
    slot = np.asarray(slot)
    table = np.asarray(table)
    R = table.shape[1]
    s = slot.reshape(-1)
    ok = (s >= 0) & (s < M)
    coef = np.zeros((s.size, R), np.float32)
    coef[ok] = table[s[ok]].astype(np.float32)
    return coef.reshape(slot.shape + (R,))
