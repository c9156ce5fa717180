"""The compact grid of include/mi_nerf_vox.h (mi_vox_index, mi_vox_pack, mi_vox_render_sparse, mi_vox_record_bytes) and
baked.SparseRadianceGrid without a GPU: every refusal answers MI_VOX_EINVAL with a message before any HIP call; a C99 program links
against the new entries; the restatement the GPU tests compare with (tests/vox_sparse_restate.py) has the properties the header states;
the grid object knows its sizes, survives a file and widens back to a dense grid."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import vox_sparse_restate as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1


@pytest.fixture(scope="module")
def vox():
    from nerf_pytorch_paeng_amd import _vox
    from nerf_pytorch_paeng_amd.build import build_vox_library
    build_vox_library()
    _vox.lib()
    return _vox


def _grid(vox, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), res=(20, 20, 20)):
    return vox.Grid((C.c_float * 3)(*lo), (C.c_float * 3)(*hi), (C.c_int32 * 3)(*res))


# ---------------------------------------------------------------------------------------------------
# sizes
# ---------------------------------------------------------------------------------------------------
def test_record_bytes_and_the_index_scratch_follow_their_formulas(vox):
    L = vox.lib()
    assert [L.mi_vox_record_bytes(B, vox.FMT_F32) for B in (1, 4, 9)] == [16, 64, 128]
    assert [L.mi_vox_record_bytes(B, vox.FMT_F16) for B in (1, 4, 9)] == [8, 32, 64]
    for B in (0, 2, 3, 5, 8, 10, 16):
        assert L.mi_vox_record_bytes(B, vox.FMT_F32) == 0 and L.mi_vox_record_bytes(B, vox.FMT_F16) == 0
    for fmt in (-1, 2, 7):
        assert L.mi_vox_record_bytes(9, fmt) == 0
    for B in (1, 4, 9):
        for fmt in (vox.FMT_F32, vox.FMT_F16):
            assert L.mi_vox_record_bytes(B, fmt) == SR.record_bytes(B, fmt) == L.mi_vox_record_floats(B) * (4, 2)[fmt]
    for res in ((1, 1, 1), (5, 4, 3), (20, 12, 9), (65, 3, 9), (512, 512, 512)):
        need = L.mi_vox_index_scratch_bytes(C.byref(_grid(vox, res=res)))
        points = math.prod(r + 1 for r in res)
        assert need % 16 == 0 and 16 <= need <= 4 * points + 16, (res, need)             # never more than a count per point
    assert L.mi_vox_index_scratch_bytes(C.byref(_grid(vox, res=(512, 512, 512)))) < 1 << 20
    assert L.mi_vox_index_scratch_bytes(None) == 0 and "grid" in vox.last_error()
    assert L.mi_vox_index_scratch_bytes(C.byref(_grid(vox, res=(0, 8, 8)))) == 0 and "res" in vox.last_error()


# ---------------------------------------------------------------------------------------------------
# refusals: made-up addresses that are never dereferenced -- every call below is refused before the first HIP call
# ---------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
GOOD = dict(lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), res=(20, 12, 9), B=9, fmt=1, sigma=0x40000, slot=0x50000, count=0x60000, scratch=0x70000,
            scratch_short=0, src=0x80000, M=1000, table=0x90000, skip=0xA0000, rays=0xB0000, n=257, step=0.05, near=0.0, far=6.0, T_min=0.0,
            bg=(1.0, 1.0, 1.0), use_skip=1, cfg=True, rgb=0xC0000, disp=0xD0000, acc=0xE0000, depth=0xF0000, visited=0x100000, grid=True)
POINTS = 21 * 13 * 10
# case -> (overrides, the entries it applies to: i index, k pack, r render_sparse)
REFUSALS = {
    "NULL grid": (dict(grid=False), "ikr"),
    "res 0": (dict(res=(20, 0, 9)), "ikr"),
    "res 513": (dict(res=(513, 12, 9)), "ikr"),
    "res negative": (dict(res=(20, 12, -1)), "ikr"),
    "lo above hi": (dict(lo=(1.0, -1.0, -1.0), hi=(-1.0, 1.0, 1.0)), "ikr"),
    "empty axis": (dict(lo=(-1.0, 1.0, -1.0)), "ikr"),
    "NaN box": (dict(hi=(1.0, 1.0, NAN)), "ikr"),
    "infinite box": (dict(hi=(INF, 1.0, 1.0)), "ikr"),
    "B 2": (dict(B=2), "kr"),
    "B 0": (dict(B=0), "kr"),
    "B 16": (dict(B=16), "kr"),
    "fmt 2": (dict(fmt=2), "kr"),
    "fmt negative": (dict(fmt=-1), "kr"),
    "M negative": (dict(M=-1), "kr"),
    "M above the lattice's points": (dict(M=POINTS + 1), "kr"),
    "NULL slot": (dict(slot=None), "ir"),
    "NULL sigma": (dict(sigma=None), "ir"),
    "NULL count": (dict(count=None), "i"),
    "NULL scratch": (dict(scratch=None), "i"),
    "scratch one byte short": (dict(scratch_short=1), "i"),
    "scratch of no bytes": (dict(scratch_short=None), "i"),
    "scratch not 16-byte aligned": (dict(scratch=0x70008), "i"),
    "count not 8-byte aligned": (dict(count=0x60004), "i"),
    "slot not 4-byte aligned": (dict(slot=0x50002), "ikr"),
    "sigma not 4-byte aligned": (dict(sigma=0x40002), "ir"),
    "NULL src": (dict(src=None), "k"),
    "src not 16-byte aligned": (dict(src=0x80008), "k"),
    "NULL table with records": (dict(table=None), "kr"),
    "table not 16-byte aligned": (dict(table=0x90008), "kr"),
    "NULL skip": (dict(skip=None), "r"),
    "NULL cfg": (dict(cfg=False), "r"),
    "step 0": (dict(step=0.0), "r"),
    "step negative": (dict(step=-0.05), "r"),
    "step NaN": (dict(step=NAN), "r"),
    "step infinite": (dict(step=INF), "r"),
    "too many steps": (dict(step=2.0 * math.sqrt(3.0) / 65536.0), "r"),
    "near above far": (dict(near=6.0, far=2.0), "r"),
    "near NaN": (dict(near=NAN), "r"),
    "T_min negative": (dict(T_min=-0.1), "r"),
    "T_min 1": (dict(T_min=1.0), "r"),
    "T_min NaN": (dict(T_min=NAN), "r"),
    "bg NaN": (dict(bg=(1.0, NAN, 1.0)), "r"),
    "use_skip 2": (dict(use_skip=2), "r"),
    "n negative": (dict(n=-1), "r"),
    "NULL rays": (dict(rays=None), "r"),
    "NULL rgb": (dict(rgb=None), "r"),
    "rays not 4-byte aligned": (dict(rays=0xB0002), "r"),
    "acc not 4-byte aligned": (dict(acc=0xE0001), "r"),
    "visited not 4-byte aligned": (dict(visited=0x100002), "r"),
}


def _call(mod, entry, a):
    L = mod.lib()
    g = C.byref(_grid(mod, a["lo"], a["hi"], a["res"])) if a["grid"] else None
    if entry == "i":
        need = L.mi_vox_index_scratch_bytes(C.byref(_grid(mod, res=GOOD["res"])))
        have = 0 if a["scratch_short"] is None else need - a["scratch_short"]
        rc = L.mi_vox_index(g, a["sigma"], a["slot"], a["count"], a["scratch"], have, None)
    elif entry == "k":
        rc = L.mi_vox_pack(g, a["B"], a["fmt"], a["src"], a["slot"], a["M"], a["table"], None)
    else:
        cfg = C.byref(mod.RenderCfg(a["step"], a["near"], a["far"], a["T_min"], (C.c_float * 3)(*a["bg"]), a["use_skip"])) if a["cfg"] else None
        rc = L.mi_vox_render_sparse(g, a["B"], a["fmt"], a["sigma"], a["slot"], a["table"], a["M"], a["skip"], a["rays"], a["n"], cfg, a["rgb"], a["disp"],
                                    a["acc"], a["depth"], a["visited"], None)
    return rc, mod.last_error()


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_answer_einval_with_a_message_before_any_hip_call(vox, case):
    over, entries = REFUSALS[case]
    for entry in entries:
        rc, msg = _call(vox, entry, dict(GOOD, **over))
        assert rc == EINVAL, (case, entry, rc, msg)
        assert msg and "HIP error" not in msg, (case, entry, msg)


def test_the_good_arguments_of_the_refusal_table_reach_the_device(vox):
    """The table's base case is refused by nothing: each entry gets as far as its launch, which fails here for want of a device
    (MI_VOX_EHIP) -- so every refusal above is owed to its one override.  Nullable arguments may be NULL; nothing is launched for no work."""
    if torch.cuda.is_available():
        pytest.skip("made-up addresses must not reach a real device")
    for entry in "ikr":
        for fmt in (0, 1):
            rc, msg = _call(vox, entry, dict(GOOD, fmt=fmt))
            assert rc == 2 and "HIP error" in msg, (entry, fmt, rc, msg)
    for over in (dict(disp=None, acc=None, depth=None, visited=None), dict(skip=None, use_skip=0), dict(far=INF), dict(M=0, table=None), dict(M=POINTS),
                 dict(B=1, fmt=1, table=0x90010)):
        rc, msg = _call(vox, "r", dict(GOOD, **over))
        assert rc == 2 and "HIP error" in msg, (over, rc, msg)
    rc, msg = _call(vox, "k", dict(GOOD, slot=None))                                   # the one-to-one form
    assert rc == 2 and "HIP error" in msg, (rc, msg)
    assert _call(vox, "k", dict(GOOD, M=0, src=None, table=None, slot=None))[0] == 0
    assert _call(vox, "r", dict(GOOD, n=0, rays=None, rgb=None))[0] == 0


def test_header_compiles_as_c99_and_the_new_entries_link_and_answer(tmp_path, vox):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not found")
    pkg = os.path.dirname(vox.LIB_PATH)
    exe = str(tmp_path / "vox_sparse_consumer")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "vox_sparse_consumer.c"), "-L", pkg, "-lmi_nerf_vox", f"-Wl,-rpath,{pkg}", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"vox sparse c_abi consumer ok: ABI {vox.ABI_VERSION}" in run.stdout
    assert vox.ABI_VERSION == 2 and vox.FMT_F32 == 0 and vox.FMT_F16 == 1
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_vox.h")).read()
    assert "#define MI_VOX_FMT_F32 0" in hdr and "#define MI_VOX_FMT_F16 1" in hdr and "THE COMPACT GRID" in hdr


# ---------------------------------------------------------------------------------------------------
# the restatement's own properties
# ---------------------------------------------------------------------------------------------------
def _fields():
    rng = np.random.default_rng(18)
    out = []
    for P in ((4, 5, 6), (10, 13, 21), (25, 25, 25), (3, 2, 66)):
        out.append(np.zeros(P, np.float32))
        out.append(np.full(P, 0.5, np.float32))
        out.append(np.where(rng.uniform(size=P) < 0.01, 1.0, 0.0).astype(np.float32))
        blob = np.zeros(P, np.float32)
        blob[:P[0] // 2, :P[1] // 2, :P[2] // 2] = rng.uniform(0.0, 2.0, (P[0] // 2, P[1] // 2, P[2] // 2)) > 1.0
        out.append(blob)
        corner = np.zeros(P, np.float32)
        corner[-1, -1, -1] = 1e-30                                                       # one dense point in the last corner: clipping
        out.append(corner)
    return out


def test_restatement_active_set_is_the_one_bake_field_evaluates_and_slots_count_in_flat_order():
    for sigma in _fields():
        act = SR.active_set(sigma)
        pooled = torch.nn.functional.max_pool3d(torch.from_numpy((sigma > 0).astype(np.float32))[None, None], 3, stride=1, padding=1)[0, 0] > 0
        assert np.array_equal(act, pooled.numpy())
        slot, M = SR.slots(sigma)
        assert slot.dtype == np.int32 and slot.shape == sigma.shape and M == act.sum()
        flat, aflat = slot.reshape(-1), act.reshape(-1)
        assert (flat[~aflat] == -1).all() and np.array_equal(flat[aflat], np.arange(M))       # the exclusive running count, in flat order
        run = 0
        for i in range(0, flat.size, max(1, flat.size // 97)):                                # ... and restated point by point on a sample
            run = int(aflat[:i].sum())
            assert flat[i] == (run if aflat[i] else -1)
        # two active neighbours along x have consecutive slots
        both = act[:, :, :-1] & act[:, :, 1:]
        assert (slot[:, :, 1:][both] == slot[:, :, :-1][both] + 1).all()
        # every corner of a cell with a dense corner is active: what the render rule can read lies in the table
        dense = sigma > 0
        Pz, Py, Px = sigma.shape
        cell = np.zeros((Pz - 1, Py - 1, Px - 1), bool)
        every = np.ones((Pz - 1, Py - 1, Px - 1), bool)
        for e in range(8):
            ex, ey, ez = e & 1, (e >> 1) & 1, e >> 2
            cell |= dense[ez:Pz - 1 + ez, ey:Py - 1 + ey, ex:Px - 1 + ex]
            every &= act[ez:Pz - 1 + ez, ey:Py - 1 + ey, ex:Px - 1 + ex]
        assert (every | ~cell).all()
    assert SR.slots(np.zeros((3, 3, 3), np.float32))[1] == 0
    s, M = SR.slots(np.ones((3, 4, 5), np.float32))
    assert M == 60 and np.array_equal(s.reshape(-1), np.arange(60))


def test_restatement_table_and_its_dense_grid():
    rng = np.random.default_rng(19)
    sigma = _fields()[8]                                                                      # (10, 13, 21), the octant blob
    slot, M = SR.slots(sigma)
    assert 0 < M < sigma.size
    coef = rng.normal(0, 1, sigma.shape + (16,)).astype(np.float32)
    coef[..., 12:] = 0
    coef[2, 3, 4, 0:4] = (70000.0, -1e9, 6.1e-5 * 0.37, 2049.0)                               # beyond the range, a subnormal, a tie
    for fmt, dtype in ((SR.FMT_F32, np.float32), (SR.FMT_F16, np.float16)):
        table = SR.table_of(coef, slot, M, fmt)
        assert table.shape == (M, 16) and table.dtype == dtype
        act = slot >= 0
        with np.errstate(over="ignore"):                                                     # 70000 and -1e9 become +-inf on purpose
            want = coef[act].astype(dtype)
        assert np.array_equal(table.view(np.uint16 if fmt else np.uint32), want.view(np.uint16 if fmt else np.uint32))
        back = SR.to_dense(slot, table, M)
        assert back.dtype == np.float32 and not back[~act].any()
        assert np.array_equal(back[act].view(np.uint32), want.astype(np.float32).view(np.uint32))
    if slot[2, 3, 4] >= 0:
        half = SR.table_of(coef, slot, M, SR.FMT_F16)[slot[2, 3, 4]]
        assert half[0] == np.inf and half[1] == -np.inf and half[3] == 2048.0 and 0 < half[2] < 6.1e-5
    # a slot outside [0, M) is a zero record
    edit = slot.copy()
    edit[act.nonzero()[0][0], act.nonzero()[1][0], act.nonzero()[2][0]] = M + 5
    assert not SR.to_dense(edit, SR.table_of(coef, slot, M, SR.FMT_F32), M)[act.nonzero()[0][0], act.nonzero()[1][0], act.nonzero()[2][0]].any()


# ---------------------------------------------------------------------------------------------------
# baked.SparseRadianceGrid on the host
# ---------------------------------------------------------------------------------------------------
def test_the_sparse_grid_object_knows_its_sizes_survives_a_file_and_widens_to_a_dense_grid(vox, tmp_path):
    from nerf_pytorch_paeng_amd import baked
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    for storage, dtype, rb in (("fp32", torch.float32, 64), ("f16", torch.float16, 32)):
        g = baked.SparseRadianceGrid(-1.0, (1.0, 2.0, 3.0), (17, 9, 33), B=4, storage=storage)
        assert g.points == (34, 10, 18) and g.skip_shape == (5, 2, 3) and g.record_floats == 16 and g.record_bytes == rb and g.device is None
        assert g.storage == storage and g.count == 0 and g.nbytes == 8 * 34 * 10 * 18 + 30
        with pytest.raises(MiNerfError, match="holds nothing"):
            g.render(torch.zeros(1, 6))
        g.allocate("cpu")
        assert g.coef is None and g.table.shape == (0, 16) and g.table.dtype == dtype and (g.slot == -1).all() and g.slot.dtype == torch.int32
        with pytest.raises(MiNerfError, match="HIP device"):
            g.render(torch.zeros(1, 6))
        # a hand-made grid: three active points, numbered in flat order
        g.sigma[3, 2, 1] = 2.5
        g.slot[3, 2, 0], g.slot[3, 2, 1], g.slot[3, 2, 2] = 0, 1, 2
        g.table = torch.arange(48.0).reshape(3, 16).to(dtype)
        g.count = 3
        g.skip[0, 0, 0] = 1
        assert g.nbytes == 8 * 34 * 10 * 18 + 30 + 3 * rb
        d = g.to_dense()
        assert type(d) is baked.RadianceGrid and d.coef.shape == (34, 10, 18, 16) and d.coef.dtype == torch.float32
        assert torch.equal(d.coef[3, 2, :3], torch.arange(48.0).reshape(3, 16)) and int((d.coef != 0).sum()) == 47
        assert torch.equal(d.sigma, g.sigma) and torch.equal(d.skip, g.skip)
        assert np.array_equal(d.coef.numpy(), SR.to_dense(g.slot.numpy(), g.table.numpy(), 3))
        g.slot[3, 2, 2] = 7                                                              # outside the table: a zero record, as the renderer reads it
        assert not g.to_dense().coef[3, 2, 2].any()
        g.slot[3, 2, 2] = 2
        path = str(tmp_path / f"{storage}.npz")
        g.save(path)
        h = baked.SparseRadianceGrid.load(path)
        assert (h.lo, h.hi, h.res, h.B, h.storage, h.count) == (g.lo, g.hi, g.res, g.B, storage, 3) and h.nbytes == g.nbytes
        assert h.table.dtype == dtype and torch.equal(h.table, g.table) and torch.equal(h.slot, g.slot) and torch.equal(h.sigma, g.sigma) and torch.equal(h.skip, g.skip)
        with np.load(path) as f:
            assert sorted(f.files) == sorted(["lo", "hi", "res", "B", "storage", "sigma", "slot", "table", "skip"])
    for bad in (dict(storage="bf16"), dict(storage="dense"), dict(B=2), dict(res=513)):
        with pytest.raises(MiNerfError):
            baked.SparseRadianceGrid(**dict(dict(lo=-1.0, hi=1.0, res=8, B=9), **bad))
    with pytest.raises(MiNerfError, match="bake dense, then compact"):
        baked.bake_field(lambda rays, z: None, -1.0, 1.0, 8, B=1, device="cpu", shell="neighbours", storage="sparse")
    with pytest.raises(MiNerfError, match="storage"):
        baked.bake_field(lambda rays, z: None, -1.0, 1.0, 8, B=1, device="cpu", storage="f16")
