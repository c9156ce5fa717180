"""libmi_nerf_mesh.so / include/mi_nerf_mesh.h without a GPU.  ``mesh_rule`` (numpy fp32, written from the header, without a case table) is the
restatement the GPU tests compare mi_mesh_count / mi_mesh_emit with; it is held to its own properties here: closed oriented manifolds on
random and non-finite lattices, Euler characteristic 2 and the interpolation bound on a sphere.  Then the usual library checks: the header is
C99 and a C program links against the library; header, ctypes table and exported symbols agree; the library calls exactly four entries of
libmi_nerf.so and exports nothing of the others; the scratch formulas are the ones restated here; every refusal answers MI_MESH_EINVAL with
a message before any HIP call; the PLY writer round-trips."""
import ctypes as C
import math
import os
import re
import shutil
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
f32 = np.float32
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]       # lexicographic


# ---------------------------------------------------------------------------------------------------
# restatement (from include/mi_nerf_mesh.h)
# ---------------------------------------------------------------------------------------------------
def lattice_axes(lo, hi, res):
    """(step [3], [x_x(j), x_y(j), x_z(j)]): fp32, every operation rounded once."""
    step = [(f32(hi[i]) - f32(lo[i])) / f32(res[i]) for i in range(3)]
    return step, [(f32(lo[i]) + (np.arange(res[i] + 1).astype(f32) * step[i]).astype(f32)).astype(f32) for i in range(3)]


def edge_delta(e):
    return ((e + 1) & 1, ((e + 1) >> 1) & 1, ((e + 1) >> 2) & 1)


def tet_corners(q):
    """The four corner offsets (x, y, z) of tetrahedron q, in corner order."""
    p = PERMS[q]
    c1 = [0, 0, 0]
    c1[p[0]] = 1
    c2 = list(c1)
    c2[p[1]] = 1
    return [(0, 0, 0), tuple(c1), tuple(c2), (1, 1, 1)]


def tet_triangles(q, inside):
    """Triangles of tetrahedron q for the inside flags of its four corners: a list of triangles, each three edges (corner, corner), wound."""
    corners = tet_corners(q)
    ins = [k for k in range(4) if inside[k]]
    outs = [k for k in range(4) if not inside[k]]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 2:
        (A, B), (Cc, D) = ins, outs
        tris = [[(A, Cc), (A, D), (B, D)], [(A, Cc), (B, D), (B, Cc)]]
    else:
        A = ins[0] if len(ins) == 1 else outs[0]
        tris = [[(A, k) for k in range(4) if k != A]]
    cen = lambda ks: [Fraction(sum(corners[k][i] for k in ks), len(ks)) for i in range(3)]
    d = [o - i for o, i in zip(cen(outs), cen(ins))]
    wound = []
    for tri in tris:
        m = [[corners[a][i] + corners[b][i] for i in range(3)] for a, b in tri]          # midpoints, doubled: exact integers
        u, v = [m[1][i] - m[0][i] for i in range(3)], [m[2][i] - m[0][i] for i in range(3)]
        n = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
        dot = sum(ni * di for ni, di in zip(n, d))
        assert dot != 0
        wound.append(tri if dot > 0 else [tri[0], tri[2], tri[1]])
    return wound


def mesh_rule(f, lo, hi, iso, want_normals=True):
    """THE RULE: f [P_z,P_y,P_x] fp32 numpy -> (verts [V,3] fp32, tris [T,3] int32, normals [V,3] fp32 or None)."""
    f = np.asarray(f, f32)
    iso = f32(iso)
    Pz, Py, Px = f.shape
    res = (Px - 1, Py - 1, Pz - 1)
    step, x = lattice_axes(lo, hi, res)
    inside = f > iso                                                  # a NaN is outside
    crossed = np.zeros((Pz, Py, Px, 7), bool)
    for e in range(7):
        dx, dy, dz = edge_delta(e)
        crossed[:Pz - dz, :Py - dy, :Px - dx, e] = inside[:Pz - dz, :Py - dy, :Px - dx] != inside[dz:, dy:, dx:]
    vid = (np.cumsum(crossed.ravel()) - 1).reshape(crossed.shape)     # vertex number of a crossed edge: increasing edge id 7 flat(j) + e
    jz, jy, jx, e = np.nonzero(crossed)
    delta = np.array([edge_delta(k) for k in range(7)])
    bx, by, bz = jx + delta[e, 0], jy + delta[e, 1], jz + delta[e, 2]
    with np.errstate(all="ignore"):
        fa, fb = f[jz, jy, jx], f[bz, by, bx]
        t = ((iso - fa).astype(f32) / (fb - fa).astype(f32)).astype(f32)
        t = np.fmin(np.fmax(t, f32(0)), f32(1)).astype(f32)           # fmaxf / fminf: a NaN becomes 0
        verts = np.zeros((len(t), 3), f32)
        for i, (ja, jb) in enumerate(((jx, bx), (jy, by), (jz, bz))):
            xa, xb = x[i][ja], x[i][jb]
            verts[:, i] = (xa + (t * (xb - xa).astype(f32)).astype(f32)).astype(f32)
        normals = None
        if want_normals:
            g = []
            for i, axis in enumerate((2, 1, 0)):                          # x is the last array axis
                fm = np.moveaxis(f, axis, 0)
                gi = np.empty_like(fm)
                gi[1:-1] = ((fm[2:] - fm[:-2]).astype(f32) / (f32(2) * step[i])).astype(f32)
                gi[0] = ((fm[1] - fm[0]).astype(f32) / step[i]).astype(f32)
                gi[-1] = ((fm[-1] - fm[-2]).astype(f32) / step[i]).astype(f32)
                g.append(np.moveaxis(gi, 0, axis))
            gv = []
            for gi in g:
                ga, gb = gi[jz, jy, jx], gi[bz, by, bx]
                gv.append((ga + (t * (gb - ga).astype(f32)).astype(f32)).astype(f32))
            ln = np.sqrt((((gv[0] * gv[0]).astype(f32) + (gv[1] * gv[1]).astype(f32)).astype(f32) + (gv[2] * gv[2]).astype(f32)).astype(f32)).astype(f32)
            ok = (ln > 0) & np.isfinite(ln)
            normals = np.stack([np.where(ok, (-gi / ln).astype(f32), f32(0)) for gi in gv], -1).astype(f32)
    # triangles: per tetrahedron and inside pattern, the cells that show it
    Cz, Cy, Cx = Pz - 1, Py - 1, Px - 1
    cz, cy, cx = np.meshgrid(np.arange(Cz), np.arange(Cy), np.arange(Cx), indexing="ij")
    cell = (cz * Cy + cy) * Cx + cx
    rows = []
    for q in range(6):
        corners = tet_corners(q)
        flags = [inside[cz + c[2], cy + c[1], cx + c[0]] for c in corners]
        for pat in range(1, 15):
            want = [bool((pat >> k) & 1) for k in range(4)]
            sel = np.ones(cell.shape, bool)
            for k in range(4):
                sel &= flags[k] == want[k]
            if not sel.any():
                continue
            for ti, tri in enumerate(tet_triangles(q, want)):
                ids = []
                for a, b in tri:
                    a, b = min(a, b), max(a, b)
                    ca, cb = corners[a], corners[b]
                    d = tuple(cb[i] - ca[i] for i in range(3))
                    ee = (d[0] | d[1] << 1 | d[2] << 2) - 1
                    ids.append(vid[cz[sel] + ca[2], cy[sel] + ca[1], cx[sel] + ca[0], ee])
                rows.append(np.stack([cell[sel], np.full(sel.sum(), q), np.full(sel.sum(), ti), *ids], -1))
    if rows:
        r = np.concatenate(rows, 0)
        r = r[np.lexsort((r[:, 2], r[:, 1], r[:, 0]))]
        tris = r[:, 3:].astype(np.int32)
    else:
        tris = np.zeros((0, 3), np.int32)
    return verts, tris, normals


def directed_edges(tris):
    t = np.asarray(tris, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], 0)


def is_closed_oriented_manifold(tris):
    """Every directed triangle edge occurs exactly once and its reverse exactly once."""
    e = directed_edges(tris)
    if len(e) == 0:
        return True
    key = e[:, 0] * (int(e.max()) + 1) + e[:, 1]
    rev = e[:, 1] * (int(e.max()) + 1) + e[:, 0]
    u, n = np.unique(key, return_counts=True)
    return bool((n == 1).all()) and np.array_equal(u, np.unique(rev))


def euler_characteristic(n_verts, tris):
    e = np.sort(directed_edges(tris), -1)
    return n_verts - len(np.unique(e, axis=0)) + len(tris)


def random_lattice(seed=0, shape=(7, 8, 9), non_finite=False):
    """[P_z,P_y,P_x] = 7 x 8 x 9 points uniform in [0,1] with the boundary forced to 0; ``non_finite``: half of the interior values replaced by
    NaN, +inf, -inf and values exactly equal to iso = 0.5."""
    rng = np.random.default_rng(seed)
    f = rng.random(shape).astype(f32)
    if non_finite:
        special = np.array([np.nan, np.inf, -np.inf, 0.5], f32)
        pick = rng.random(shape) < 0.5
        f = np.where(pick, special[rng.integers(0, 4, shape)], f).astype(f32)
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = 0, 0, 0, 0, 0, 0
    return f


def sphere_lattice(res, R=0.5, lo=-1.0, hi=1.0):
    """f = R - |p| at the lattice points of the box lo..hi (fp64 formula on the fp32 lattice positions, rounded to fp32 once)."""
    _, x = lattice_axes((lo,) * 3, (hi,) * 3, (res,) * 3)
    zz, yy, xx = np.meshgrid(x[2].astype(np.float64), x[1].astype(np.float64), x[0].astype(np.float64), indexing="ij")
    return (R - np.sqrt(xx * xx + yy * yy + zz * zz)).astype(f32)


def a256(v):
    return (v + 255) & ~255


def density_scratch_bytes(res):
    Px, Py, Pz = (r + 1 for r in res)
    R = min(Py * Pz, -(-1024 // Px))
    return a256(24 * R) + a256(4 * R * Px) + a256(16 * R * Px)


def extract_scratch_bytes(res):
    N = (res[0] + 1) * (res[1] + 1) * (res[2] + 1)
    Cn = res[0] * res[1] * res[2]
    return a256(N) + a256(4 * N) + a256(4 * Cn) + a256(4 * (-(-N // 1024)))


# ---------------------------------------------------------------------------------------------------
# the restatement itself
# ---------------------------------------------------------------------------------------------------
def test_the_rule_gives_every_tetrahedron_pattern_wound_triangles():
    seen = 0
    for q in range(6):
        assert len(set(tet_corners(q))) == 4
        for pat in range(16):
            tris = tet_triangles(q, [bool((pat >> k) & 1) for k in range(4)])
            assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[bin(pat).count("1")]
            seen += len(tris)
    assert seen == 6 * (8 * 1 + 6 * 2)
    assert sorted(edge_delta(e) for e in range(7)) == sorted((a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1) if a + b + c)


@pytest.mark.parametrize("non_finite", [False, True])
@pytest.mark.parametrize("seed", [0, 1])
def test_random_lattices_give_closed_oriented_manifolds(seed, non_finite):
    f = random_lattice(seed, non_finite=non_finite)
    verts, tris, normals = mesh_rule(f, (-1, -1, -1), (1, 1, 1), 0.5)
    assert len(tris) > 100 and len(verts) > 100
    assert tris.min() == 0 and tris.max() == len(verts) - 1 and len(np.unique(tris)) == len(verts)      # every vertex is used: welded
    assert is_closed_oriented_manifold(tris)
    assert np.isfinite(verts).all() and np.isfinite(normals).all()
    assert (verts >= -1).all() and (verts <= 1).all()


def test_sphere_euler_bound_outward_normals_and_inscribed_volume():
    from nerf_pytorch_paeng_amd import mesh
    R, res = 0.5, 16
    verts, tris, normals = mesh_rule(sphere_lattice(res, R), (-1, -1, -1), (1, 1, 1), 0.0)
    assert is_closed_oriented_manifold(tris)
    assert euler_characteristic(len(verts), tris) == 2
    L = math.sqrt(3.0) * 2.0 / res
    bound = L * L / (8.0 * (R - L))
    dist = np.abs(np.linalg.norm(verts.astype(np.float64), axis=-1) - R)
    assert dist.max() <= bound, (dist.max(), bound)
    v = verts.astype(np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    # Six lattice points (+-0.5 on an axis) lie ON this sphere: they are outside (f == iso), t is 0 on every crossed edge from them, and the
    # triangles around them collapse to a point -- 36 triangles with a normal of exactly (0, 0, 0).  Every triangle that has a normal points outwards.
    n = np.cross(b - a, c - a)
    dots = np.einsum("ij,ij->i", n, (a + b + c) / 3.0)
    flat = (n == 0).all(-1)
    assert int(flat.sum()) == 36 and (dots[~flat] > 0).all() and (dots[flat] == 0).all()
    assert (np.einsum("ij,ij->i", normals.astype(np.float64), v) > 0).all()          # the gradient normals point outwards too
    m = mesh.Mesh(torch.from_numpy(verts), torch.from_numpy(tris), torch.from_numpy(normals))
    assert 0.0 < m.volume() < 4.0 / 3.0 * math.pi * R ** 3
    assert 0.0 < m.area() < 4.0 * math.pi * R ** 2
    assert abs(m.volume() - float(np.einsum("ij,ij->", a, np.cross(b, c)) / 6.0)) < 1e-12


# ---------------------------------------------------------------------------------------------------
# the library without a GPU
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def msh():
    """The library is built when the tree is fresh (a no-op when it is up to date), like tests/conftest.py does for libmi_nerf.so."""
    from nerf_pytorch_paeng_amd import _mesh
    from nerf_pytorch_paeng_amd.build import build_mesh_library
    build_mesh_library()
    _mesh.lib()
    return _mesh


def test_header_compiles_as_c99_and_the_library_links_and_answers(tmp_path, msh):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not found")
    pkg = os.path.dirname(msh.LIB_PATH)
    exe = str(tmp_path / "mesh_consumer")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "mesh_consumer.c"), "-L", pkg, "-lmi_nerf_mesh", f"-Wl,-rpath,{pkg}", f"-Wl,-rpath-link,{pkg}",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"mesh c_abi consumer ok: ABI {msh.ABI_VERSION}" in run.stdout


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def test_header_table_and_symbols_agree_and_the_libraries_do_not_mix(msh):
    from nerf_pytorch_paeng_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_mesh.h")).read()
    declared = set(re.findall(r"\b(mi_mesh_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(msh.SIGNATURES), declared ^ set(msh.SIGNATURES)
    new = _exports(msh.LIB_PATH)
    assert {n for n in new if n.startswith("mi_mesh_")} == declared
    assert not [n for n in new if n.startswith(("mi_nerf_", "mi_occ_", "mi_iqa_", "mi_scene_"))]
    old = _exports(_lib.LIB_PATH)
    assert {n for n in old if n.startswith("mi_")} == set(_lib.SIGNATURES)            # libmi_nerf.so: its entries and nothing of this
    for other in ("mi_nerf.h", "mi_nerf_iqa.h", "mi_nerf_occ.h", "mi_nerf_scene.h"):
        assert "mi_mesh_" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert msh.lib().mi_mesh_abi_version() == msh.ABI_VERSION == int(re.search(r"#define MI_MESH_ABI_VERSION (\d+)", hdr).group(1))
    for name, value in (("MAX_RES", msh.MAX_RES), ("MIN_SLAB_POINTS", msh.MIN_SLAB_POINTS), ("SCAN_TILE", msh.SCAN_TILE)):
        assert int(re.search(rf"#define MI_MESH_{name} (\d+)", hdr).group(1)) == value
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [n for n in sorted(declared) if n not in doc] == []


def test_the_library_links_against_libmi_nerf_beside_itself_and_calls_four_entries_only(msh):
    dyn = subprocess.run(["readelf", "-d", msh.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "[libmi_nerf.so]" in dyn
    runpath = re.search(r"\((?:RUNPATH|RPATH)\).*\[(.*)\]", dyn).group(1)
    assert runpath.split(":")[0] == "$ORIGIN", runpath
    for other in ("libmi_nerf_occ", "libmi_nerf_iqa", "libmi_nerf_scene"):
        assert other not in dyn
    und = subprocess.run(["nm", "-D", "--undefined-only", msh.LIB_PATH], capture_output=True, text=True, check=True).stdout
    used = {ln.split()[-1] for ln in und.splitlines() if ln.split()[-1].startswith("mi_")}
    assert used == {"mi_nerf_mlp_rays", "mi_nerf_mlp_rays_f16s", "mi_nerf_mlp_rays_bf16", "mi_nerf_last_error"}


def _grid(msh, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), res=(32, 32, 32)):
    return msh.Grid((C.c_float * 3)(*lo), (C.c_float * 3)(*hi), (C.c_int32 * 3)(*res))


def _net():
    from nerf_pytorch_paeng_amd._lib import Net
    return Net(8, 256, 4, 10, 4)


@pytest.mark.parametrize("res", [(1, 1, 1), (5, 3, 1), (8, 7, 6), (39, 8, 8), (64, 3, 2), (128, 128, 128), (512, 512, 512), (1023 // 2, 1, 1), (7, 11, 13)])
def test_scratch_sizes_match_the_restatement(msh, res):
    g = _grid(msh, res=res)
    assert msh.lib().mi_mesh_density_scratch_bytes(C.byref(g)) == density_scratch_bytes(res)
    assert msh.lib().mi_mesh_extract_scratch_bytes(C.byref(g)) == extract_scratch_bytes(res)


def test_the_smallest_density_scratch_of_a_40_9_9_point_lattice_holds_less_than_half_of_it(msh):
    """What the GPU test of the slab loop rests on: the smallest scratch is one slab of ceil(1024 / 40) = 26 rows of the 81, and no 27th fits."""
    res = (39, 8, 8)
    need = msh.lib().mi_mesh_density_scratch_bytes(C.byref(_grid(msh, res=res)))
    assert need == a256(24 * 26) + a256(4 * 26 * 40) + a256(16 * 26 * 40)
    assert (need - 768) // (24 + 20 * 40) < 27 < 81 / 2


BAD_GRIDS = {"res 0": dict(res=(32, 0, 32)), "res 513": dict(res=(513, 32, 32)), "lo == hi": dict(lo=(1.0, -1.0, -1.0)), "lo > hi": dict(lo=(-1.0, 2.0, -1.0)),
             "inf box": dict(hi=(float("inf"), 1.0, 1.0)), "nan box": dict(lo=(-1.0, -1.0, float("nan"))),
             "extent overflows": dict(lo=(-3e38,) * 3, hi=(3e38,) * 3)}


def _refused(msh, rc, case):
    msg = msh.last_error()
    assert rc == EINVAL, (case, rc, msg)
    assert msg and "HIP error" not in msg, (case, msg)


def test_refusals_answer_einval_with_a_message_before_any_hip_call(msh):
    """The pointers are made-up addresses that are never dereferenced: every call here is refused before the first HIP call (a call that got
    as far as one would answer MI_MESH_EHIP on a machine without a GPU)."""
    L, g, net = msh.lib(), _grid(msh), _net()
    dn, en = L.mi_mesh_density_scratch_bytes(C.byref(g)), L.mi_mesh_extract_scratch_bytes(C.byref(g))
    assert dn > 0 and en > 0
    big = 1 << 40
    dens = dict(grid=g, net=net, packed=0x1000, mode=0, f=0x2000, scratch=0x100000, nbytes=dn)
    bad = {"NULL packed": dict(packed=None), "NULL f": dict(f=None), "NULL scratch": dict(scratch=None), "short scratch": dict(nbytes=dn - 1),
           "unaligned scratch": dict(scratch=0x100010), "mode f16": dict(mode=8), "mode bf16 pinned": dict(mode=2), "mode two families": dict(mode=6),
           "mode unknown": dict(mode=77), "mode negative": dict(mode=-1)}
    bad.update({"grid " + k: dict(grid=_grid(msh, **v)) for k, v in BAD_GRIDS.items()})
    for case, kw in bad.items():
        a = dict(dens, **kw)
        _refused(msh, L.mi_mesh_density(C.byref(a["grid"]), C.byref(a["net"]), a["packed"], a["mode"], a["f"], a["scratch"], a["nbytes"], None), case)
    _refused(msh, L.mi_mesh_density(C.byref(g), None, 0x1000, 0, 0x2000, 0x100000, dn, None), "NULL net")
    _refused(msh, L.mi_mesh_density(None, C.byref(net), 0x1000, 0, 0x2000, 0x100000, dn, None), "NULL grid")

    cnt = dict(grid=g, f=0x2000, iso=0.5, scratch=0x100000, nbytes=en, counts=0x3000)
    bad = {"NULL f": dict(f=None), "NULL scratch": dict(scratch=None), "NULL counts": dict(counts=None), "unaligned counts": dict(counts=0x3004),
           "short scratch": dict(nbytes=en - 1), "unaligned scratch": dict(scratch=0x100010), "NaN iso": dict(iso=float("nan"))}
    bad.update({"grid " + k: dict(grid=_grid(msh, **v)) for k, v in BAD_GRIDS.items()})
    for case, kw in bad.items():
        a = dict(cnt, **kw)
        _refused(msh, L.mi_mesh_count(C.byref(a["grid"]), a["f"], a["iso"], a["scratch"], a["nbytes"], a["counts"], None), "count " + case)
    _refused(msh, L.mi_mesh_count(None, 0x2000, 0.5, 0x100000, en, 0x3000, None), "count NULL grid")

    emt = dict(grid=g, f=0x2000, iso=0.5, scratch=0x100000, nbytes=en, V=100, T=200, verts=0x4000, tris=0x5000, normals=None)
    bad = {"NULL f": dict(f=None), "NULL scratch": dict(scratch=None), "NULL verts": dict(verts=None), "NULL tris": dict(tris=None),
           "short scratch": dict(nbytes=en - 1), "NaN iso": dict(iso=float("nan")), "vertices above int32": dict(V=1 << 31),
           "triangles above int32": dict(T=1 << 31), "counts far above": dict(V=1 << 40, T=1 << 63)}
    bad.update({"grid " + k: dict(grid=_grid(msh, **v)) for k, v in BAD_GRIDS.items()})
    for case, kw in bad.items():
        a = dict(emt, **kw)
        _refused(msh, L.mi_mesh_emit(C.byref(a["grid"]), a["f"], a["iso"], a["scratch"], a["nbytes"], a["V"], a["T"], a["verts"], a["tris"], a["normals"], None),
                 "emit " + case)
    _refused(msh, L.mi_mesh_emit(None, 0x2000, 0.5, 0x100000, big, 1, 1, 0x4000, 0x5000, None, None), "emit NULL grid")
    for k, v in BAD_GRIDS.items():
        bg = _grid(msh, **v)
        assert L.mi_mesh_density_scratch_bytes(C.byref(bg)) == 0 and msh.last_error(), k
        assert L.mi_mesh_extract_scratch_bytes(C.byref(bg)) == 0 and msh.last_error(), k
    assert L.mi_mesh_extract_scratch_bytes(None) == 0 and "grid" in msh.last_error()


def test_python_surface_without_a_gpu(msh):
    from nerf_pytorch_paeng_amd import mesh, ops
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    for bad in ("f16", "fp16", ops.precision(f16=True), ops.precision(bf16=True, coarse_f16s=True), ops.precision(bf16=True, points_per_wave=64)):
        with pytest.raises(MiNerfError):
            mesh.check_precision(bad)
    assert [mesh.check_precision(p).mode for p in (None, "fp32", "bf16", "f16s")] == [0, 0, 1, 5]
    with pytest.raises(MiNerfError):
        mesh.extract(torch.zeros(4, 4, 4), -1.0, 1.0, 0.5)              # a CPU tensor: no fallback
    with pytest.raises(MiNerfError):
        mesh.extract(torch.zeros(4, 4), -1.0, 1.0, 0.5)
    g = mesh.c_grid(-1.0, (1.0, 2.0, 3.0), 8)
    assert list(g.lo) == [-1.0] * 3 and list(g.hi) == [1.0, 2.0, 3.0] and list(g.res) == [8, 8, 8]
    rays, z = mesh.lattice_rows((-1.0, 0.0, 1.0), (1.0, 1.0, 3.0), (4, 2, 1))
    assert rays.shape == (3 * 2, 6) and z.shape == (6, 5)
    assert rays[:, 0].tolist() == [-1.0] * 6 and rays[:, 1].tolist() == [0.0, 0.5, 1.0] * 2 and rays[:, 2].tolist() == [1.0] * 3 + [3.0] * 3
    assert rays[:, 3:].tolist() == [[1.0, 0.0, 0.0]] * 6 and z[4].tolist() == [0.0, 0.5, 1.0, 1.5, 2.0]


def parse_ply(data):
    """A reader for what write_ply writes (binary little-endian, scalar vertex properties, one uchar-counted int list per face)."""
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    fmt = {"float": "f", "uchar": "B", "int": "i"}
    elements = []
    for ln in lines[2:]:
        w = ln.split()
        if w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property":
            elements[-1][2].append(tuple(w[1:]))
    out, off = {}, 0
    for name, n, props in elements:
        rows = []
        for _ in range(n):
            row = {}
            for p in props:
                if p[0] == "list":
                    (k,) = struct.unpack_from("<" + fmt[p[1]], body, off)
                    off += struct.calcsize(fmt[p[1]])
                    row[p[3]] = list(struct.unpack_from(f"<{k}{fmt[p[2]]}", body, off))
                    off += k * struct.calcsize(fmt[p[2]])
                else:
                    (row[p[1]],) = struct.unpack_from("<" + fmt[p[0]], body, off)
                    off += struct.calcsize(fmt[p[0]])
            rows.append(row)
        out[name] = rows
    assert off == len(body)
    return out


def test_ply_round_trips_a_hand_made_two_triangle_mesh(tmp_path):
    from nerf_pytorch_paeng_amd import mesh
    verts = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.5], [0.0, 1.0, -0.25]])
    tris = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    normals = torch.tensor([[0.0, 0.0, 1.0]] * 3 + [[0.0, 0.6, 0.8]])
    colors = torch.tensor([[0.0, 0.5, 1.0], [0.25, 0.25, 0.25], [1.0, 1.0, 1.0], [0.1, 0.2, 0.4]])
    for nrm, col in ((normals, colors), (normals, None), (None, colors), (None, None)):
        path = str(tmp_path / "m.ply")
        mesh.Mesh(verts, tris, nrm, col).save_ply(path)
        got = parse_ply(open(path, "rb").read())
        assert [[v["x"], v["y"], v["z"]] for v in got["vertex"]] == verts.tolist()
        assert [f["vertex_indices"] for f in got["face"]] == tris.tolist()
        assert ("nx" in got["vertex"][0]) == (nrm is not None) and ("red" in got["vertex"][0]) == (col is not None)
        if nrm is not None:
            assert [[v["nx"], v["ny"], v["nz"]] for v in got["vertex"]] == normals.tolist()
        if col is not None:
            assert [[v["red"], v["green"], v["blue"]] for v in got["vertex"]] == [[0, 128, 255], [64, 64, 64], [255, 255, 255], [26, 51, 102]]
    m = mesh.Mesh(verts[:3], tris[:1])
    assert m.area() == pytest.approx(0.5 * math.sqrt(1.25), rel=1e-15) and m.volume() == 0.0 and m.colors is None and m.normals is None
