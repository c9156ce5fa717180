"""libmi_nerf_occ.so / include/mi_nerf_occ.h without a GPU: the header is C99 and a C program links against the library; the header, the ctypes
table (nerf_pytorch_paeng_amd/_occ.py) and the library's dynamic symbols name the same entries; libmi_nerf.so is what it was (exactly the names
of _lib.SIGNATURES) and the new library exports nothing of it but links against it; every refusal answers MI_OCC_EINVAL with a message before
any HIP call; the word count and the workspace layout are the ones restated here.  ``cell_rule`` (numpy fp32, written from the header, not from
the kernel) is the restatement the GPU tests compare mi_occ_mark with; it checks itself on hand-made points."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
f32 = np.float32


# ---------------------------------------------------------------------------------------------------
# restatements (from include/mi_nerf_occ.h)
# ---------------------------------------------------------------------------------------------------
def grid_scale(lo, hi, res):
    return [f32(res[i]) / (f32(hi[i]) - f32(lo[i])) for i in range(3)]


def cell_rule(lo, hi, res, outside_occupied, bits_u32, rays, z):
    """THE CELL RULE: rays [n,6] fp32, z [n,S] fp32 numpy -> bool [n,S].  Every operation is one fp32 numpy operation (rounded once)."""
    rays, z = np.asarray(rays, f32), np.asarray(z, f32)
    scale = grid_scale(lo, hi, res)
    inside = np.ones(z.shape, bool)
    c = []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(3):
            prod = (rays[:, 3 + i:4 + i] * z).astype(f32)
            p = (rays[:, i:i + 1] + prod).astype(f32)
            ci = np.floor(((p - f32(lo[i])).astype(f32) * scale[i]).astype(f32))
            inside &= (ci >= 0) & (ci < res[i])
            c.append(ci)
    ix, iy, iz = (np.where(inside, ci, 0).astype(np.int64) for ci in c)
    b = (iz * res[1] + iy) * res[0] + ix
    bit = (np.asarray(bits_u32, np.uint32)[b >> 5] >> (b & 31).astype(np.uint32)) & 1
    return np.where(inside, bit.astype(bool), bool(outside_occupied))


def grid_words(res):
    return (res[0] * res[1] * res[2] + 31) // 32


def a256(v):
    return (v + 255) & ~255


def workspace_layout(Sc, Nf, n):
    St = Sc + Nf
    T = n * ((St + 31) // 32)
    names = ["z_c", "raw_c", "weights_c", "z_f", "raw_f", "t_rand", "u", "slot", "tile_rays", "tile_z", "tile_src", "tile_raw", "counters"]
    sizes = [a256(n * Sc * 4), a256(n * Sc * 16), a256(n * Sc * 4), a256(n * St * 4) if Nf else 0, a256(n * St * 16) if Nf else 0, a256(n * Sc * 4),
             a256(n * Nf * 4) if Nf else 0, a256(n * St * 4), a256(T * 24), a256(T * 128), a256(T * 128), a256(T * 512), 256]
    out, off = {}, 0
    for k, s in zip(names, sizes):
        out[k] = off
        off += s
    out["total"] = off
    return out


# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def occ():
    """The library is built when the tree is fresh (a no-op when it is up to date), like tests/conftest.py does for libmi_nerf.so."""
    from nerf_pytorch_paeng_amd import _occ
    from nerf_pytorch_paeng_amd.build import build_occ_library
    build_occ_library()
    _occ.lib()
    return _occ


def test_cell_rule_restatement_on_hand_made_points():
    lo, hi, res = (0.0, 0.0, 0.0), (4.0, 2.0, 1.0), (4, 2, 1)
    bits = np.array([0b10100101], np.uint32)                       # cells 0, 2, 5, 7 of 8
    rays = np.array([[0.5, 0.5, 0.5, 1.0, 0.0, 0.0], [0.5, 1.5, 0.5, 1.0, 0.0, 0.0], [0.5, 0.5, 0.5, 0.0, 0.0, 1.0]], f32)
    z = np.array([[0.0, 1.0, 2.0, 3.0, 3.5, -1.0]] * 3, f32)
    for outside in (False, True):
        got = cell_rule(lo, hi, res, outside, bits, rays, z)
        assert got[0].tolist() == [True, False, True, False, outside, outside]      # cells 0..3, then x = 4 (hi is outside) and x = -0.5
        assert got[1].tolist() == [False, True, False, True, outside, outside]      # cells 4..7
        assert got[2].tolist() == [True, outside, outside, outside, outside, outside]      # z = 0.5 is cell 0; 1.5 .. leave the box; -0.5 too
    nan = cell_rule(lo, hi, res, True, bits, rays[:1], np.array([[np.nan]], f32))
    assert nan.tolist() == [[True]] and not cell_rule(lo, hi, res, False, bits, rays[:1], np.array([[np.nan]], f32))[0, 0]


def test_header_compiles_as_c99_and_the_library_links_and_answers(tmp_path, occ):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not found")
    pkg = os.path.dirname(occ.LIB_PATH)
    exe = str(tmp_path / "occ_consumer")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "occ_consumer.c"), "-L", pkg, "-lmi_nerf_occ", f"-Wl,-rpath,{pkg}", f"-Wl,-rpath-link,{pkg}",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"occ c_abi consumer ok: ABI {occ.ABI_VERSION}" in run.stdout


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def test_header_table_and_symbols_agree_and_the_libraries_do_not_mix(occ):
    from nerf_pytorch_paeng_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_occ.h")).read()
    declared = set(re.findall(r"\b(mi_occ_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(occ.SIGNATURES), declared ^ set(occ.SIGNATURES)
    new = _exports(occ.LIB_PATH)
    assert {n for n in new if n.startswith("mi_occ_")} == declared
    assert not [n for n in new if n.startswith("mi_nerf_") or n.startswith("mi_iqa_")]
    old = _exports(_lib.LIB_PATH)
    assert {n for n in old if n.startswith("mi_")} == set(_lib.SIGNATURES)            # libmi_nerf.so: its entries and nothing of this
    assert not set(occ.SIGNATURES) & set(_lib.SIGNATURES)
    assert "mi_occ_" not in open(os.path.join(ROOT, "include", "mi_nerf.h")).read()
    assert occ.lib().mi_occ_abi_version() == occ.ABI_VERSION == int(re.search(r"#define MI_OCC_ABI_VERSION (\d+)", hdr).group(1))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [n for n in sorted(declared) if n not in doc] == []


def test_the_library_links_against_libmi_nerf_beside_itself_and_calls_public_entries_only(occ):
    from nerf_pytorch_paeng_amd import _lib
    dyn = subprocess.run(["readelf", "-d", occ.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "[libmi_nerf.so]" in dyn and "$ORIGIN" in dyn
    und = subprocess.run(["nm", "-D", "--undefined-only", occ.LIB_PATH], capture_output=True, text=True, check=True).stdout
    used = {ln.split()[-1] for ln in und.splitlines() if ln.split()[-1].startswith("mi_nerf_")}
    assert used == {"mi_nerf_mlp_rays", "mi_nerf_mlp_rays_f16s", "mi_nerf_mlp_rays_bf16", "mi_nerf_fill_uniform", "mi_nerf_stratified_z", "mi_nerf_composite",
                    "mi_nerf_fine_z", "mi_nerf_last_error"}
    assert used <= set(_lib.SIGNATURES)


# ---------------------------------------------------------------------------------------------------
def _grid(occ, lo=(-1.5, -1.5, -1.5), hi=(1.5, 1.5, 1.5), res=(64, 64, 64), outside=1):
    return occ.Grid((C.c_float * 3)(*lo), (C.c_float * 3)(*hi), (C.c_int32 * 3)(*res), outside)


def _cfg(Sc=64, Nf=128, mode=0, det=0, reserved=0):
    from nerf_pytorch_paeng_amd._lib import RenderCfg
    return RenderCfg(2.0, 6.0, Sc, Nf, det, mode, 0, reserved, 0)


def _net():
    from nerf_pytorch_paeng_amd._lib import Net
    return Net(8, 256, 4, 10, 4)


@pytest.mark.parametrize("res", [(1, 1, 1), (5, 3, 1), (32, 1, 1), (33, 1, 1), (64, 64, 64), (128, 96, 80), (512, 512, 512), (7, 11, 13)])
def test_grid_words_match_the_restatement(occ, res):
    assert occ.lib().mi_occ_grid_words(C.byref(_grid(occ, res=res))) == grid_words(res)


@pytest.mark.parametrize("shape", [(64, 128, 1), (64, 128, 4096), (64, 0, 1000), (3, 5, 17), (33, 31, 129), (1, 0, 7), (128, 256, 65536), (64, 128, 0)])
def test_workspace_layout_matches_the_restatement(occ, shape):
    Sc, Nf, n = shape
    wl = occ.WorkspaceLayout()
    cfg = _cfg(Sc, Nf)
    assert occ.lib().mi_occ_render_workspace_layout(C.byref(cfg), n, C.byref(wl)) == 0, occ.last_error()
    want = workspace_layout(Sc, Nf, n)
    assert {k: getattr(wl, k) for k, _ in occ.WorkspaceLayout._fields_} == want
    assert occ.lib().mi_occ_render_workspace_bytes(C.byref(cfg), n) == want["total"]


GOOD_RENDER = dict(net=True, packed_c=0x1000, packed_f=0x2000, cfg={}, grid={}, bits_c=0x3000, bits_f=0x3000, rays=0x4000, n=256, t_rand=None, u=None,
                   ws=0x100000, ws_bytes=1 << 40, rgb_c=0x5000, disp_c=0x6000, rgb_f=0x7000, disp_f=0x8000)
RENDER_REFUSALS = {
    "mode bf16 pinned 64": dict(cfg=dict(mode=2)),
    "mode bf16 pinned 32": dict(cfg=dict(mode=3)),
    "mode retired 4": dict(cfg=dict(mode=4)),
    "mode f16s+bf16": dict(cfg=dict(mode=6)),
    "mode f16": dict(cfg=dict(mode=8)),
    "mode f16+bf16": dict(cfg=dict(mode=9)),
    "mode unknown": dict(cfg=dict(mode=77)),
    "NULL net": dict(net=False),
    "NULL packed_coarse": dict(packed_c=None),
    "NULL packed_fine with Nf > 0": dict(packed_f=None),
    "NULL bits_coarse": dict(bits_c=None),
    "NULL bits_fine with Nf > 0": dict(bits_f=None),
    "NULL rays": dict(rays=None),
    "NULL workspace": dict(ws=None),
    "NULL rgb_c": dict(rgb_c=None),
    "NULL disp_c": dict(disp_c=None),
    "NULL rgb_f with Nf > 0": dict(rgb_f=None),
    "NULL disp_f with Nf > 0": dict(disp_f=None),
    "short workspace": dict(ws_bytes=1 << 20),
    "unaligned workspace": dict(ws=0x100010),
    "negative n": dict(n=-1),
    "Sc of zero": dict(cfg=dict(Sc=0)),
    "two coarse samples with a fine pass": dict(cfg=dict(Sc=2)),
    "too many samples": dict(cfg=dict(Sc=512, Nf=513)),
    "too many rays for int32 lanes": dict(n=1 << 24),
    "reserved not zero": dict(cfg=dict(reserved=1)),
    "grid res of zero": dict(grid=dict(res=(64, 0, 64))),
    "grid res too large": dict(grid=dict(res=(513, 64, 64))),
    "grid box empty": dict(grid=dict(lo=(1.5, -1.5, -1.5))),
    "grid box not finite": dict(grid=dict(hi=(float("inf"), 1.5, 1.5))),
}


@pytest.mark.parametrize("case", sorted(RENDER_REFUSALS))
def test_render_refusals_answer_einval_with_a_message_before_any_hip_call(occ, case):
    """The pointers are made-up addresses that are never dereferenced: every call here is refused before the first HIP call (a call that got
    as far as one would answer MI_OCC_EHIP, "HIP error ... no ROCm-capable device", on a machine without a GPU)."""
    a = dict(GOOD_RENDER, **RENDER_REFUSALS[case])
    cfg, grid, net = _cfg(**a["cfg"]), _grid(occ, **a["grid"]), _net()
    st = occ.Stats()
    L = occ.lib()
    rc = L.mi_occ_render_rays(C.byref(net) if a["net"] else None, a["packed_c"], a["packed_f"], C.byref(cfg), C.byref(grid), a["bits_c"], a["bits_f"],
                              a["rays"], a["n"], a["t_rand"], a["u"], a["ws"], a["ws_bytes"], a["rgb_c"], a["disp_c"], a["rgb_f"], a["disp_f"], C.byref(st), None)
    msg = L.mi_occ_last_error().decode()
    assert rc == EINVAL, (case, rc, msg)
    assert msg and "HIP error" not in msg, (case, msg)


def test_render_null_cfg_and_grid_are_refused(occ):
    L, net, st = occ.lib(), _net(), occ.Stats()
    tail = (0x3000, 0x3000, 0x4000, 256, None, None, 0x100000, 1 << 40, 0x5000, 0x6000, 0x7000, 0x8000, C.byref(st), None)
    assert L.mi_occ_render_rays(C.byref(net), 0x1000, 0x2000, None, C.byref(_grid(occ)), *tail) == EINVAL and occ.last_error()
    assert L.mi_occ_render_rays(C.byref(net), 0x1000, 0x2000, C.byref(_cfg()), None, *tail) == EINVAL and "grid" in occ.last_error()
    assert L.mi_occ_render_workspace_bytes(None, 4) == 0 and L.mi_occ_render_workspace_bytes(C.byref(_cfg(Sc=0)), 4) == 0


def test_the_other_entries_refuse_before_any_hip_call(occ):
    L, g, net = occ.lib(), _grid(occ), _net()
    need = L.mi_occ_bake_scratch_bytes(C.byref(g), 2)
    S, rows = 64 * 2, 128 * 128
    R = min(rows, -(-(1 << 22) // S))
    assert need == a256(R * 24) + a256(R * S * 4) + a256(R * S * 16)
    good = dict(grid=g, bits=0x1000, net=net, packed=0x2000, mode=0, sub=2, sigma=0.0, acc=0, scratch=0x100000, nbytes=need)
    bad = {"mode f16": dict(mode=8), "mode two families": dict(mode=6), "sub 0": dict(sub=0), "sub 5": dict(sub=5), "NULL bits": dict(bits=None),
           "NULL packed": dict(packed=None), "NULL scratch": dict(scratch=None), "short scratch": dict(nbytes=need - 1), "NaN threshold": dict(sigma=float("nan")),
           "unaligned scratch": dict(scratch=0x100008), "bad grid": dict(grid=_grid(occ, res=(0, 1, 1)))}
    for case, kw in bad.items():
        a = dict(good, **kw)
        rc = L.mi_occ_bake(C.byref(a["grid"]), a["bits"], C.byref(a["net"]), a["packed"], a["mode"], a["sub"], a["sigma"], a["acc"], a["scratch"], a["nbytes"], None)
        assert rc == EINVAL and occ.last_error() and "HIP error" not in occ.last_error(), (case, rc, occ.last_error())
    assert L.mi_occ_bake(C.byref(g), 0x1000, None, 0x2000, 0, 2, 0.0, 0, 0x100000, need, None) == EINVAL
    assert L.mi_occ_bake_scratch_bytes(C.byref(g), 0) == 0 and L.mi_occ_bake_scratch_bytes(None, 2) == 0
    for rc in (L.mi_occ_dilate(C.byref(g), 0x1000, 0x2000, 3, None), L.mi_occ_dilate(C.byref(g), 0x1000, 0x2000, -1, None),
               L.mi_occ_dilate(C.byref(g), 0x1000, 0x1000, 1, None), L.mi_occ_dilate(C.byref(g), None, 0x2000, 1, None),
               L.mi_occ_dilate(None, 0x1000, 0x2000, 1, None),
               L.mi_occ_count(C.byref(g), None, 0x2000, None), L.mi_occ_count(C.byref(g), 0x1000, None, None), L.mi_occ_count(C.byref(g), 0x1000, 0x2004, None),
               L.mi_occ_mark(C.byref(g), None, 0x2000, 0x3000, 4, 8, 0x4000, None), L.mi_occ_mark(C.byref(g), 0x1000, 0x2000, 0x3000, 4, 8, None, None),
               L.mi_occ_mark(C.byref(g), 0x1000, 0x2000, 0x3000, -1, 8, 0x4000, None), L.mi_occ_mark(C.byref(g), 0x1000, 0x2000, 0x3000, 4, 0, 0x4000, None)):
        assert rc == EINVAL and occ.last_error() and "HIP error" not in occ.last_error()
    assert L.mi_occ_grid_words(None) == 0 and "grid" in occ.last_error()


def test_python_surface_without_a_gpu(tmp_path, occ):
    from nerf_pytorch_paeng_amd import nerf_process as NP
    from nerf_pytorch_paeng_amd import occupancy, ops
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    g = occupancy.OccupancyGrid(-1.5, 1.5, (8, 4, 2), outside_occupied=False)
    assert g.words == 2 and g.cells == 64
    with pytest.raises(MiNerfError):
        g.fraction()                                               # no bits yet
    with pytest.raises(MiNerfError):
        occupancy.OccupancyGrid(0.0, 1.0, 513)
    with pytest.raises(MiNerfError):
        occupancy.OccupancyGrid(1.0, 1.0, 8)
    bits = np.array([0x80000001, 0x0000ffff], np.uint32)
    g.set_bits(bits)
    g.save(str(tmp_path / "grid.npz"))
    h = occupancy.OccupancyGrid.load(str(tmp_path / "grid.npz"))
    assert (h.lo, h.hi, h.res, h.outside_occupied) == (g.lo, g.hi, g.res, False)
    assert h.bits.numpy().view(np.uint32).tolist() == bits.tolist()
    for flags in (dict(f16=True), dict(bf16=True, coarse_f16s=True), dict(bf16=True, coarse_f16=True)):
        with pytest.raises(MiNerfError):
            occupancy.check_precision(ops.precision(**flags))
    for flags in ({}, dict(bf16=True), dict(f16s=True)):
        occupancy.check_precision(ops.precision(**flags))
    # training with a grid is refused (and so is anything that is not a grid)
    from nerf_pytorch_paeng_amd.model import NeRF
    model = NeRF(2, 128, 63, 27)
    with torch.enable_grad(), pytest.raises(MiNerfError, match="inference"):
        NP.render_rays(torch.zeros(4, 6), model, None, None, occupancy=g)
    with torch.enable_grad(), pytest.raises(MiNerfError, match="inference"):
        NP.batchify_rays_and_render_by_chunk(torch.zeros(4, 3), torch.zeros(4, 3), model, None, 2, 2, None, None, occupancy=g)
