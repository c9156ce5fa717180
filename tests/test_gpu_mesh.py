"""Mesh extraction on the GPU (include/mi_nerf_mesh.h).  mi_mesh_count + mi_mesh_emit equal the numpy restatement of THE RULE
(tests/test_mesh_cpu.py: written from the header, without a case table): the counts, the triangles as integers, the vertices bit for bit,
the normals bit for bit too (the bar was 2e-6 per component; they came out bit-equal on every lattice, so equality is asserted); closed lattices give closed oriented manifolds on the device too.  mi_mesh_density equals channel 3 of
ops.mlp_rays* on the restated rows bit for bit, in one slab and in several.  A solid sphere comes out closed, with Euler characteristic 2,
within one cell diagonal of its surface and with its volume between the bracketing spheres'.  colorize is sigmoid of ops.mlp_rays on its own
rays; an extraction on a stream of its own equals the default stream's."""
import math

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import mesh, ops, scenes, synthetic, weights
from tests.test_mesh_cpu import (density_scratch_bytes, euler_characteristic, is_closed_oriented_manifold, mesh_rule, random_lattice,
                                 sphere_lattice)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32


def scattered_lattice(shape, seed):
    """Uniform values in [0,1]; nothing is forced at the boundary, so the surface is cut open there."""
    return np.random.default_rng(seed).random(shape).astype(f32)


LATTICES = {
    "random 9x8x7": lambda: (random_lattice(0), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 0.5, True),
    "non-finite 9x8x7": lambda: (random_lattice(1, non_finite=True), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 0.5, True),
    "sphere 33^3": lambda: (sphere_lattice(32), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 0.0, True),
    # P_x = 65: a row one longer than a wave; 3 x 4 x 65 = 780 points
    "P_x 65": lambda: (scattered_lattice((3, 4, 65), 2), (-1.0, 0.0, 2.0), (3.0, 0.5, 2.25), 0.5, False),
    # 5 x 11 x 13 = 715 points, 480 cells: neither a multiple of 256; and a box whose steps are not exact in fp32
    "715 points": lambda: (scattered_lattice((5, 11, 13), 3), (-0.7, -1.1, 0.3), (0.9, 1.3, 1.0), 0.5, False),
    # 101 x 102 x 103 = 1 061 106 points: 1 037 blocks of the prefix sums, more than the 1 024 the block over the block sums takes at once
    "1037 scan blocks": lambda: (scattered_lattice((101, 102, 103), 4), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 0.99, False),
}


def _compare(f, lo, hi, iso, closed, label):
    want_v, want_t, want_n = mesh_rule(f, lo, hi, iso)
    got = mesh.extract(torch.from_numpy(f).to(DEV), lo, hi, iso)
    gv, gt, gn = got.verts.cpu().numpy(), got.tris.cpu().numpy(), got.normals.cpu().numpy()
    assert gv.shape == want_v.shape and gt.shape == want_t.shape, (label, gv.shape, want_v.shape, gt.shape, want_t.shape)
    assert gt.dtype == np.int32 and np.array_equal(gt, want_t), label
    assert np.array_equal(gv.view(np.uint32), want_v.view(np.uint32)), (label, int((gv.view(np.uint32) != want_v.view(np.uint32)).sum()))
    nd = float(np.abs(gn - want_n).max()) if gn.size else 0.0
    nbits = int((gn.view(np.uint32) != want_n.view(np.uint32)).sum())
    assert np.isfinite(gn).all() and nbits == 0, (label, nd, nbits)
    if closed:
        assert is_closed_oriented_manifold(gt), label
    return len(gv), len(gt), nd, nbits


@pytest.mark.parametrize("name", sorted(LATTICES))
def test_count_and_emit_equal_the_rule(name):
    f, lo, hi, iso, closed = LATTICES[name]()
    V, T, nd, nbits = _compare(f, lo, hi, iso, closed, name)
    print(f"\n[mesh {name}] {V} vertices, {T} triangles; normals max |diff| {nd:.2e}, components that differ in a bit {nbits} of {3 * V}")
    assert V > 100 and T > 100
    no_normals = mesh.extract(torch.from_numpy(f).to(DEV), lo, hi, iso, normals=False)
    assert no_normals.normals is None and no_normals.verts.shape[0] == V and no_normals.tris.shape[0] == T


def test_one_cell_over_all_256_corner_patterns():
    """2 x 2 x 2 points: every entry of every tetrahedron's case table, with interpolation weights that are not 1/2."""
    rng = np.random.default_rng(5)
    total = 0
    for pat in range(256):
        inside = np.array([(pat >> k) & 1 for k in range(8)], bool).reshape(2, 2, 2)
        mag = rng.random((2, 2, 2)).astype(f32) * f32(0.45)
        f = np.where(inside, f32(0.55) + mag, f32(0.45) - mag).astype(f32)
        V, T, _, _ = _compare(f, (0.0, 0.0, 0.0), (1.0, 2.0, 3.0), 0.5, False, f"pattern {pat}")
        assert (T == 0) == (pat in (0, 255)) and (V == 0) == (pat in (0, 255))
        total += T
    assert total > 256 * 6


def test_an_empty_lattice_gives_an_empty_mesh():
    m = mesh.extract(torch.zeros(4, 5, 6, device=DEV), -1.0, 1.0, 0.5)
    assert m.verts.shape == (0, 3) and m.tris.shape == (0, 3) and m.normals.shape == (0, 3) and m.area() == 0.0 and m.volume() == 0.0


def test_emit_writes_nothing_beyond_the_capacities_it_is_given():
    import ctypes as C
    from nerf_pytorch_paeng_amd import _mesh
    from nerf_pytorch_paeng_amd._lib import dev_ptr, stream_ptr
    f = torch.from_numpy(random_lattice(0)).to(DEV)
    full = mesh.extract(f, -1.0, 1.0, 0.5)
    V, T = full.verts.shape[0], full.tris.shape[0]
    g = mesh.c_grid(-1.0, 1.0, (8, 7, 6))
    L = _mesh.lib()
    nbytes = L.mi_mesh_extract_scratch_bytes(C.byref(g))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    verts = torch.full((V, 3), -7.0, device=DEV)
    nrm = torch.full((V, 3), -7.0, device=DEV)
    tris = torch.full((T, 3), -7, dtype=torch.int32, device=DEV)
    st = stream_ptr(DEV)
    _mesh.check(L.mi_mesh_count(C.byref(g), dev_ptr(f), 0.5, dev_ptr(scratch, "s", torch.uint8, 256), nbytes, dev_ptr(counts, "c", torch.int64, 8), st), "count")
    Vc, Tc = V // 2, T // 3
    _mesh.check(L.mi_mesh_emit(C.byref(g), dev_ptr(f), 0.5, dev_ptr(scratch, "s", torch.uint8, 256), nbytes, Vc, Tc, dev_ptr(verts), dev_ptr(tris, "t", torch.int32),
                               dev_ptr(nrm), st), "emit")
    torch.cuda.synchronize()
    assert counts.tolist() == [V, T]
    assert torch.equal(verts[:Vc], full.verts[:Vc]) and torch.equal(tris[:Tc], full.tris[:Tc]) and torch.equal(nrm[:Vc], full.normals[:Vc])
    assert bool((verts[Vc:] == -7.0).all()) and bool((tris[Tc:] == -7).all()) and bool((nrm[Vc:] == -7.0).all())


# ---------------------------------------------------------------------------------------------------
# network -> lattice
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def networks():
    return {"2x64": weights.PackedNeRF.from_state_dict(synthetic.make_state_dict(2, 2, 64, skips=()), DEV),
            "8x256": weights.PackedNeRF.from_state_dict(synthetic.make_state_dict(0, 8, 256), DEV)}


LO, HI = (-1.2, -1.0, -0.8), (1.1, 1.3, 0.9)


@pytest.mark.parametrize("family", ["fp32", "f16s", "bf16"])
@pytest.mark.parametrize("net_name", ["2x64", "8x256"])
def test_density_equals_channel_3_of_the_fused_entry_on_the_restated_rows(networks, net_name, family):
    packed = networks[net_name]
    prec = mesh.check_precision(family)
    net, blob_c, blob_f = packed.kernel_blobs(prec)
    for res, minimum in (((5, 4, 3), False), ((39, 8, 8), True)):                 # 6 x 5 x 4 points whole; 40 x 9 x 9 in slabs of 26 of its 81 rows
        scratch = None
        if minimum:
            scratch = torch.empty(density_scratch_bytes(res), dtype=torch.uint8, device=DEV)
        for which, blob in (("fine", blob_f), ("coarse", blob_c)):
            got = mesh.density_lattice(packed, LO, HI, res, network=which, precision=family, scratch=scratch)
            rays, z = mesh.lattice_rows(LO, HI, res, DEV)
            want = ops.mlp_rays(net, blob, rays, z, bf16=family == "bf16", f16s=family == "f16s")[..., 3].reshape(res[2] + 1, res[1] + 1, res[0] + 1)
            differ = int((got.view(torch.int32) != want.view(torch.int32)).sum())
            print(f"\n[density {net_name} {family} res {res} {which} min-scratch={minimum}] values that differ {differ} of {got.numel()}, "
                  f"max |diff| {float((got - want).abs().max()):.2e}, density range {float(want.min()):.3g} .. {float(want.max()):.3g}")
            assert got.shape == want.shape and bool(torch.isfinite(want).all())
            assert differ == 0
    assert float(want.max()) > float(want.min())


# ---------------------------------------------------------------------------------------------------
# end to end on a known surface
# ---------------------------------------------------------------------------------------------------
def test_a_solid_sphere_comes_out_closed_and_within_a_cell_diagonal():
    R, res, sigma = 0.4, 32, 64.0
    scene = scenes.SolidScene([scenes.sphere((0.0, 0.0, 0.0), R, (0.8, 0.3, 0.2), sigma=sigma)])
    rays, z = mesh.lattice_rows(-1.0, 1.0, res, DEV)
    f = scene.field(rays, z)[..., 3].reshape(res + 1, res + 1, res + 1).contiguous()
    assert sorted(set(f.flatten().tolist())) == [0.0, sigma]
    m = mesh.extract(f, -1.0, 1.0, 0.5 * sigma)
    tris = m.tris.cpu().numpy()
    V = m.verts.shape[0]
    L = math.sqrt(3.0) * 2.0 / res
    dist = (m.verts.double().norm(dim=-1) - R).abs()
    ball = lambda r: 4.0 / 3.0 * math.pi * r ** 3
    print(f"\n[solid sphere] {V} vertices, {len(tris)} triangles, max distance from the surface {float(dist.max()):.4f} (cell diagonal {L:.4f}), "
          f"volume {m.volume():.5f} (sphere {ball(R):.5f}), area {m.area():.4f} (sphere {4 * math.pi * R * R:.4f})")
    assert V > 500 and is_closed_oriented_manifold(tris)
    assert euler_characteristic(V, tris) == 2
    assert float(dist.max()) <= L
    assert ball(R - L) < m.volume() < ball(R + L)


# ---------------------------------------------------------------------------------------------------
# colours, streams
# ---------------------------------------------------------------------------------------------------
def test_colorize_is_sigmoid_of_the_fused_entry_on_its_own_rays(networks):
    packed = networks["2x64"]
    f = torch.from_numpy(sphere_lattice(16)).to(DEV)
    m = mesh.extract(f, -1.0, 1.0, 0.0)
    m.normals[::5] = 0.0                                               # flat spots: seen along (0, 0, 1)
    assert m.colors is None
    for which, blob in (("fine", packed.fine), ("coarse", packed.coarse)):
        assert m.colorize(packed, network=which) is m
        rays, z = m.color_rays()
        assert torch.equal(rays[:, :3], m.verts) and float(z.abs().max()) == 0.0 and z.shape == (m.verts.shape[0], 1)
        assert torch.equal(rays[::5, 3:], torch.tensor([0.0, 0.0, 1.0], device=DEV).expand_as(rays[::5, 3:])) and torch.equal(rays[1::5, 3:], -m.normals[1::5])
        want = torch.sigmoid(ops.mlp_rays(packed.net, blob, rays, z)[:, 0, :3])
        assert m.colors.shape == (m.verts.shape[0], 3) and torch.equal(m.colors, want)
        assert float(m.colors.min()) >= 0.0 and float(m.colors.max()) <= 1.0 and float(m.colors.max()) > float(m.colors.min())


def test_an_extraction_on_a_stream_of_its_own_equals_the_default_streams(networks):
    f = torch.from_numpy(sphere_lattice(32)).to(DEV)
    want = mesh.extract(f, -1.0, 1.0, 0.0)
    want_f = mesh.density_lattice(networks["2x64"], LO, HI, (39, 8, 8))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        got = mesh.extract(f, -1.0, 1.0, 0.0)
        got_f = mesh.density_lattice(networks["2x64"], LO, HI, (39, 8, 8))
    side.synchronize()
    assert torch.equal(got.verts, want.verts) and torch.equal(got.tris, want.tris) and torch.equal(got.normals, want.normals) and torch.equal(got_f, want_f)
