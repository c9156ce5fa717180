"""Training with an occupancy grid, without a GPU: ``compaction_rule`` (numpy, written from THE COMPACTION RULE of include/mi_nerf_occ.h, not
from the kernels) is the restatement tests/test_gpu_occ_train.py compares mi_occ_compact with, bit for bit; it checks itself on hand-made rays.
Every new entry answers MI_OCC_EINVAL with a message before any HIP call; ``train_occupancy=`` is refused where it cannot work and
``occupancy=`` with gradients enabled keeps raising."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_occ_cpu import cell_rule

EINVAL = 1
f32 = np.float32
TILE = 32


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------
def compaction_rule(mask, rays, z):
    """mask bool [n,S] (THE CELL RULE), rays [n,6], z [n,S] -> the outputs of mi_occ_compact: tile_rays [T,6], tile_z [T,32], tile_src int32
    [T,32], slot int32 [n,S], counts (tiles, survivors)."""
    mask, rays, z = np.asarray(mask, bool), np.asarray(rays, f32), np.asarray(z, f32)
    n, S = mask.shape
    k = mask.sum(1).astype(np.int64)                                 # survivors of ray r
    t = (k + TILE - 1) // TILE                                       # its tiles
    base = np.concatenate([[0], np.cumsum(t)[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
    T = int(t.sum())
    tile_rays = np.zeros((T, 6), f32)
    tile_z = np.zeros(T * TILE, f32)
    tile_src = np.full(T * TILE, -1, np.int32)
    slot = np.full((n, S), -1, np.int32)
    for r in range(n):
        if k[r] == 0:
            continue
        s = np.nonzero(mask[r])[0]                                   # in sample order
        first = TILE * base[r]
        lanes = first + np.arange(k[r])                              # survivor i sits in tile base_r + i // 32, lane i % 32
        tile_z[lanes] = z[r, s]
        tile_src[lanes] = r * S + s
        slot[r, s] = lanes
        tile_z[first + k[r]:first + TILE * t[r]] = z[r, s[-1]]       # padding repeats the last surviving depth, tile_src stays -1
        tile_rays[base[r]:base[r] + t[r]] = rays[r]
    return {"tile_rays": tile_rays, "tile_z": tile_z.reshape(T, TILE), "tile_src": tile_src.reshape(T, TILE), "slot": slot,
            "counts": (T, int(k.sum()))}


# ---------------------------------------------------------------------------------------------------
# hand-made rays: +x through a 64 x 1 x 1 grid whose EVEN cells are set; sample s of a ray sits at the centre of an even cell if it is to
# survive and of an odd cell if not, so the survivor count of every ray is chosen (and every coordinate is exact in fp32)
# ---------------------------------------------------------------------------------------------------
HAND_GRID = dict(lo=(0.0, 0.0, 0.0), hi=(64.0, 1.0, 1.0), res=(64, 1, 1))
HAND_BITS = np.array([0x55555555, 0x55555555], np.uint32)
HAND_COUNTS = {64: (0, 1, 31, 32, 33, 63, 64), 40: (0, 1, 32, 33, 40)}


def hand_made(n, S, seed=0):
    """n rays whose survivor counts cycle through HAND_COUNTS[S], the survivors at random sample positions: (rays, z, counts)."""
    rng = np.random.RandomState(seed)
    counts = [HAND_COUNTS[S][(r + seed) % len(HAND_COUNTS[S])] for r in range(n)]
    rays = np.zeros((n, 6), f32)
    rays[:, 1:3] = 0.5
    rays[:, 3] = 1.0
    rays[:, 0] = -2.0 * (np.arange(n) % 4)                           # origins at x = 0, -2, -4, -6: z is shifted to land on the same cells
    z = np.zeros((n, S), f32)
    for r, k in enumerate(counts):
        keep = np.zeros(S, bool)
        keep[rng.permutation(S)[:k]] = True
        cell = 2 * (np.arange(S) % 32) + np.where(keep, 0, 1)        # even: set, odd: clear
        z[r] = cell.astype(f32) + f32(0.5) - rays[r, 0]
    return rays, z, counts


def hand_mask(rays, z, outside=False):
    return cell_rule(HAND_GRID["lo"], HAND_GRID["hi"], HAND_GRID["res"], outside, HAND_BITS, rays, z)


@pytest.mark.parametrize("S", [64, 40])
def test_compaction_rule_restatement_on_hand_made_rays(S):
    n = len(HAND_COUNTS[S])
    rays, z, counts = hand_made(n, S)
    mask = hand_mask(rays, z)
    assert mask.sum(1).tolist() == list(counts) == list(HAND_COUNTS[S])
    c = compaction_rule(mask, rays, z)
    tiles = [(k + 31) // 32 for k in counts]
    assert c["counts"] == (sum(tiles), sum(counts))
    assert c["tile_z"].shape == (sum(tiles), 32) and c["tile_src"].shape == (sum(tiles), 32) and c["tile_rays"].shape == (sum(tiles), 6)
    base = 0
    for r, (k, t) in enumerate(zip(counts, tiles)):
        s = np.nonzero(mask[r])[0]
        src = c["tile_src"][base:base + t].reshape(-1)
        assert src[:k].tolist() == (r * S + s).tolist()              # the survivors in sample order, from the ray's first tile on
        assert (src[k:] == -1).all() and len(src) - k < 32           # then padding, less than a tile of it
        tz = c["tile_z"][base:base + t].reshape(-1)
        assert np.array_equal(tz[:k], z[r, s]) and (k == 0 or (tz[k:] == z[r, s[-1]]).all())
        assert np.array_equal(c["tile_rays"][base:base + t], np.repeat(rays[r:r + 1], t, 0))
        assert c["slot"][r, s].tolist() == list(range(32 * base, 32 * base + k)) and (c["slot"][r, ~mask[r]] == -1).all()
        base += t
    # by hand: S = 64, ray 1 has one survivor and ray 2 thirty-one; ray 0 has none and owns no tile
    if S == 64:
        assert c["tile_src"][0, 0] == 64 + int(np.nonzero(mask[1])[0][0]) and (c["tile_src"][0, 1:] == -1).all()
        assert (c["tile_src"][1, :31] >= 128).all() and c["tile_src"][1, 31] == -1 and (c["tile_src"][2] >= 192).all()
        assert c["counts"] == (1 + 1 + 1 + 2 + 2 + 2, 224)


def test_compaction_rule_of_nothing_and_of_everything():
    rays, z, _ = hand_made(3, 40)
    none = compaction_rule(np.zeros((3, 40), bool), rays, z)
    assert none["counts"] == (0, 0) and none["tile_src"].shape == (0, 32) and (none["slot"] == -1).all()
    full = compaction_rule(np.ones((3, 40), bool), rays, z)
    assert full["counts"] == (6, 120)
    assert full["tile_src"][1].tolist() == list(range(32, 40)) + [-1] * 24 and full["slot"][1].tolist() == list(range(64, 96)) + list(range(96, 104))
    assert compaction_rule(np.zeros((0, 40), bool), np.zeros((0, 6)), np.zeros((0, 40)))["counts"] == (0, 0)


# ---------------------------------------------------------------------------------------------------
# refusals before any HIP call
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def occ():
    from nerf_pytorch_paeng_amd import _occ
    from nerf_pytorch_paeng_amd.build import build_occ_library
    build_occ_library()
    _occ.lib()
    return _occ


def _grid(occ, res=(64, 64, 64)):
    return occ.Grid((C.c_float * 3)(-1.5, -1.5, -1.5), (C.c_float * 3)(1.5, 1.5, 1.5), (C.c_int32 * 3)(*res), 1)


GOOD_COMPACT = dict(grid=True, bits=0x1000, rays=0x2000, z=0x3000, n=256, S=64, tile_rays=0x4000, tile_z=0x5000, tile_src=0x6000, slot=0x7000,
                    counts=0x8000, scratch=0x100000, nbytes=None)
COMPACT_REFUSALS = {
    "NULL grid": dict(grid=False), "NULL bits": dict(bits=None), "NULL rays": dict(rays=None), "NULL z": dict(z=None),
    "NULL tile_rays": dict(tile_rays=None), "NULL tile_z": dict(tile_z=None), "NULL tile_src": dict(tile_src=None), "NULL slot": dict(slot=None),
    "NULL counts": dict(counts=None), "NULL scratch": dict(scratch=None), "negative n": dict(n=-1), "S of zero": dict(S=0), "S of 1025": dict(S=1025),
    "short scratch": dict(nbytes=-1), "unaligned scratch": dict(scratch=0x100010),
    "2^31 tile lanes": dict(n=1 << 26, S=32, nbytes=1 << 40), "2^31 tile lanes, ragged S": dict(n=1 << 25, S=33, nbytes=1 << 40),
    "bad grid": dict(grid="bad"),
}


@pytest.mark.parametrize("case", sorted(COMPACT_REFUSALS))
def test_compact_refusals_answer_einval_with_a_message_before_any_hip_call(occ, case):
    """The pointers are made-up addresses that are never dereferenced: a call that got as far as HIP would answer MI_OCC_EHIP on a machine
    without a GPU (and could not be made safely on one with a GPU)."""
    a = dict(GOOD_COMPACT, **COMPACT_REFUSALS[case])
    L = occ.lib()
    need = L.mi_occ_compact_scratch_bytes(256)
    assert need >= 256 * 8
    nbytes = need if a["nbytes"] is None else (need - 1 if a["nbytes"] == -1 else a["nbytes"])
    g = _grid(occ, res=(0, 1, 1)) if a["grid"] == "bad" else _grid(occ)
    rc = L.mi_occ_compact(C.byref(g) if a["grid"] else None, a["bits"], a["rays"], a["z"], a["n"], a["S"], a["tile_rays"], a["tile_z"], a["tile_src"],
                          a["slot"], a["counts"], a["scratch"], nbytes, None)
    msg = occ.last_error()
    assert rc == EINVAL, (case, rc, msg)
    assert msg and "HIP error" not in msg, (case, msg)


def test_compact_scratch_bytes(occ):
    L = occ.lib()
    a256 = lambda v: (v + 255) & ~255
    for n in (0, 1, 257, 1024, 1025, 4096, 1 << 20):
        assert L.mi_occ_compact_scratch_bytes(n) == a256(n * 8) + a256(-(-n // 1024) * 8) + 256
    assert L.mi_occ_compact_scratch_bytes(-1) == 0 and occ.last_error()
    assert L.mi_occ_compact_scratch_bytes(1 << 26) == 0 and "HIP error" not in occ.last_error()


def test_scatter_and_gather_refusals_answer_einval_before_any_hip_call(occ):
    L = occ.lib()
    calls = {
        "scatter NULL tile_vals": lambda: L.mi_occ_scatter_raw(None, 0x2000, 4, 64, 0x3000, None),
        "scatter NULL slot": lambda: L.mi_occ_scatter_raw(0x1000, None, 4, 64, 0x3000, None),
        "scatter NULL out": lambda: L.mi_occ_scatter_raw(0x1000, 0x2000, 4, 64, None, None),
        "scatter negative n": lambda: L.mi_occ_scatter_raw(0x1000, 0x2000, -1, 64, 0x3000, None),
        "scatter S of zero": lambda: L.mi_occ_scatter_raw(0x1000, 0x2000, 4, 0, 0x3000, None),
        "scatter S of 1025": lambda: L.mi_occ_scatter_raw(0x1000, 0x2000, 4, 1025, 0x3000, None),
        "scatter 2^31 tile lanes": lambda: L.mi_occ_scatter_raw(0x1000, 0x2000, 1 << 25, 33, 0x3000, None),
        "scatter unaligned out": lambda: L.mi_occ_scatter_raw(0x1000, 0x2000, 4, 64, 0x3004, None),
        "gather NULL src": lambda: L.mi_occ_gather_raw(None, 0x2000, 4, 0x3000, None),
        "gather NULL tile_src": lambda: L.mi_occ_gather_raw(0x1000, None, 4, 0x3000, None),
        "gather NULL out": lambda: L.mi_occ_gather_raw(0x1000, 0x2000, 4, None, None),
        "gather negative n_tiles": lambda: L.mi_occ_gather_raw(0x1000, 0x2000, -1, 0x3000, None),
        "gather 2^31 tile lanes": lambda: L.mi_occ_gather_raw(0x1000, 0x2000, 1 << 26, 0x3000, None),
        "gather unaligned src": lambda: L.mi_occ_gather_raw(0x1008, 0x2000, 4, 0x3000, None),
    }
    for case, call in calls.items():
        rc = call()
        msg = occ.last_error()
        assert rc == EINVAL and msg and "HIP error" not in msg, (case, rc, msg)


# ---------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------
def test_train_occupancy_is_refused_where_it_cannot_work_and_occupancy_stays_inference_only(occ):
    from nerf_pytorch_paeng_amd import nerf_process as NP
    from nerf_pytorch_paeng_amd import occupancy, occupancy_train
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    from nerf_pytorch_paeng_amd.model import NeRF
    g = occupancy.OccupancyGrid(-1.5, 1.5, (8, 4, 2)).set_bits(np.array([0x80000001, 0x0000ffff], np.uint32))
    model = NeRF(2, 128, 63, 27)
    rays, o, d = torch.zeros(4, 6), torch.zeros(4, 3), torch.zeros(4, 3)
    with torch.no_grad():                                            # no gradients: the keyword is refused, not ignored
        with pytest.raises(MiNerfError, match="train_occupancy"):
            NP.render_rays(rays, model, None, None, train_occupancy=g)
        with pytest.raises(MiNerfError, match="train_occupancy"):
            NP.batchify_rays_and_render_by_chunk(o, d, model, None, 2, 2, None, None, train_occupancy=g)
    frozen = NeRF(2, 128, 63, 27).requires_grad_(False)
    with torch.enable_grad(), pytest.raises(MiNerfError, match="train_occupancy"):
        NP.render_rays(rays, frozen, None, None, train_occupancy=g)
    with torch.enable_grad():
        for not_a_grid in ("grid", 3, np.zeros(2, np.uint32), object()):
            with pytest.raises(MiNerfError, match="OccupancyGrid"):
                NP.render_rays(rays, model, None, None, train_occupancy=not_a_grid)
            with pytest.raises(MiNerfError, match="OccupancyGrid"):
                NP.batchify_rays_and_render_by_chunk(o, d, model, None, 2, 2, None, None, train_occupancy=not_a_grid)
        with pytest.raises(MiNerfError, match="OccupancyGrid"):
            occupancy_train.render_train(rays, model, None, "grid")
        for flags in (dict(bf16=True), dict(f16=True), dict(bf16=True, coarse_f16s=True), dict(bf16=True, coarse_f16=True)):
            with pytest.raises(MiNerfError, match="fp32 or f16s"):
                NP.render_rays(rays, model, None, None, train_occupancy=g, **flags)
            with pytest.raises(MiNerfError, match="fp32 or f16s"):
                NP.batchify_rays_and_render_by_chunk(o, d, model, None, 2, 2, None, None, train_occupancy=g, **flags)
        # occupancy= with gradients enabled is what it was: an inference feature
        with pytest.raises(MiNerfError, match="inference"):
            NP.render_rays(rays, model, None, None, occupancy=g)
        with pytest.raises(MiNerfError, match="inference"):
            NP.batchify_rays_and_render_by_chunk(o, d, model, None, 2, 2, None, None, occupancy=g)
    with pytest.raises(MiNerfError, match="coarse"):
        g.compact(rays, torch.zeros(4, 8), network="both")


def test_binding_names_the_new_entries_and_the_abi(occ):
    assert occ.ABI_VERSION == 2 and occ.lib().mi_occ_abi_version() == 2
    assert {"mi_occ_compact_scratch_bytes", "mi_occ_compact", "mi_occ_scatter_raw", "mi_occ_gather_raw"} <= set(occ.SIGNATURES)
