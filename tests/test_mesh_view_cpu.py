"""THE VIEW of include/mi_nerf_mesh.h without a GPU.  The numpy restatement (tests/mesh_view_restate.py) is held to its own properties: two
triangles that share an edge cover every pixel centre exactly once (also with vertices and edges exactly on centres), coverage does not
change under a cyclic rotation of the vertices, cull 1 and 2 partition what cull 0 draws, extract's winding is front from outside, and the
integers stay far inside int64 at the guard band.  Then the library: the C99 consumer, the scratch formula, every refusal answering
MI_MESH_EINVAL with a message before any HIP call, the empty cases, and Mesh.render's refusals."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import mesh_view_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1


# ---------------------------------------------------------------------------------------------------
# the restatement itself
# ---------------------------------------------------------------------------------------------------
def _count(H, W, X, Y, z, tris, cull=0):
    n = np.zeros((H, W), np.int64)
    for tri in tris:
        pix, st = R.coverage(X, Y, z, tri, H, W, cull)
        if st is not None:
            np.add.at(n, pix, 1)
    return n


def random_quads(n=200, seed=11):
    """Convex quads (perturbed parallelograms) in a 24 x 20 frame, in 24.8 fixed point.  A third are snapped so that every vertex lies exactly on
    a pixel centre (multiples of 256: horizontal, vertical and diagonal edges through centres included), a third have two such vertices."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        c = rng.integers(2 * 256, 18 * 256, 2)
        u = rng.integers(-6 * 256, 6 * 256, 2)
        v = rng.integers(-6 * 256, 6 * 256, 2)
        q = np.array([c, c + u, c + u + v + rng.integers(-300, 300, 2), c + v], np.int64)
        kind = len(out) % 3
        if kind == 0:
            q = (q // 256) * 256
        elif kind == 1:
            q[[0, 2]] = (q[[0, 2]] // 256) * 256
        cross = [R.orient(*q[i], *q[(i + 1) % 4], *q[(i + 2) % 4]) for i in range(4)]
        if all(x > 0 for x in cross) or all(x < 0 for x in cross):                # strictly convex: both diagonals split it
            out.append(q)
    return out


def test_two_triangles_of_a_quad_cover_every_pixel_centre_exactly_once():
    H, W = 20, 24
    seen_on_centre = 0
    for k, q in enumerate(random_quads()):
        X, Y, z = q[:, 0], q[:, 1], np.ones(4, np.float32)
        split = [(0, 1, 2), (0, 2, 3)] if k % 2 == 0 else [(1, 2, 3), (1, 3, 0)]
        n = _count(H, W, X, Y, z, split)
        assert n.max() <= 1, (k, q.tolist())
        other = _count(H, W, X, Y, z, [(1, 2, 3), (1, 3, 0)] if k % 2 == 0 else [(0, 1, 2), (0, 2, 3)])
        assert np.array_equal(n, other), (k, q.tolist())                          # the quad's coverage does not depend on the diagonal
        # against the definition on exact rationals: a centre strictly inside the quad is covered, one strictly outside is not
        py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        s = 1 if R.orient(*q[0], *q[1], *q[2]) > 0 else -1
        e = [s * R.orient(*q[i], *q[(i + 1) % 4], 256 * px, 256 * py) for i in range(4)]
        inside, outside = np.all([x > 0 for x in e], 0), np.any([x < 0 for x in e], 0)
        assert (n[inside] == 1).all() and (n[outside] == 0).all(), (k, q.tolist())
        seen_on_centre += int((~inside & ~outside).sum())
    assert seen_on_centre > 300                                                   # centres exactly on an outline were met, and often


def test_a_tiling_of_centred_squares_covers_each_centre_once():
    """A 5 x 4 grid of squares with every vertex ON a pixel centre, each split along a diagonal (alternating): all edges run through centres."""
    X, Y, tris = [], [], []
    for j in range(5):
        for i in range(6):
            X.append(256 * 3 * i)
            Y.append(256 * 3 * j)
    for j in range(4):
        for i in range(5):
            a, b, c, d = j * 6 + i, j * 6 + i + 1, (j + 1) * 6 + i + 1, (j + 1) * 6 + i
            tris += [(a, b, c), (a, c, d)] if (i + j) % 2 else [(b, c, d), (b, d, a)]
    n = _count(13, 16, np.array(X), np.array(Y), np.ones(len(X), np.float32), tris)
    assert (n[:12, :15] == 1).all() and (n[12] == 0).all() and (n[:, 15] == 0).all()     # the top-left rule: the bottom row and right column stay out


def test_coverage_is_invariant_under_rotation_and_cull_partitions():
    rng = np.random.default_rng(3)
    H, W = 16, 16
    fronts = 0
    for _ in range(200):
        p = rng.integers(-2 * 256, 18 * 256, (3, 2))
        on_centre = rng.random(3) < 0.3
        p[on_centre] = (p[on_centre] // 256) * 256                                 # some vertices exactly on pixel centres
        X, Y, z = p[:, 0].astype(np.int64), p[:, 1].astype(np.int64), np.ones(3, np.float32)
        base = _count(H, W, X, Y, z, [(0, 1, 2)])
        assert np.array_equal(base, _count(H, W, X, Y, z, [(1, 2, 0)])) and np.array_equal(base, _count(H, W, X, Y, z, [(2, 0, 1)]))
        assert np.array_equal(base, _count(H, W, X, Y, z, [(0, 2, 1)]))              # and under the other winding, with cull 0
        c1, c2 = _count(H, W, X, Y, z, [(0, 1, 2)], cull=1), _count(H, W, X, Y, z, [(0, 1, 2)], cull=2)
        assert np.array_equal(c1 + c2, base) and (c1.sum() == 0 or c2.sum() == 0)
        A2 = R.orient(X[0], Y[0], X[1], Y[1], X[2], Y[2])
        if base.sum():
            assert (c1.sum() > 0) == (A2 < 0)                                      # front = A2 < 0 survives cull 1
            fronts += int(A2 < 0)
    assert 20 < fronts < 180


def test_an_outward_wound_sphere_is_front_from_outside():
    """The winding of mi_mesh_emit (normals towards lower density: outwards for a solid) is FRONT: cull 1 keeps the near side of a sphere, and
    the silhouette of cull 1, cull 2 and cull 0 is the same."""
    verts, tris = R.uv_sphere(8, 12, 1.0, (0, 0, 0))
    n = np.cross(verts[tris[:, 1]] - verts[tris[:, 0]], verts[tris[:, 2]] - verts[tris[:, 0]])
    assert (np.einsum("ij,ij->i", n, verts[tris].mean(1)) > 0).all()               # wound outwards
    cam = R.scene_camera((30, -30))
    X, Y, z, valid, _, _ = R.project(cam, 1e-3, verts)
    assert valid.all()
    t0, d0 = R.raster(64, 64, 0, X, Y, z, tris)
    t1, d1 = R.raster(64, 64, 1, X, Y, z, tris)
    t2, d2 = R.raster(64, 64, 2, X, Y, z, tris)
    assert (t0 >= 0).sum() > 500 and np.array_equal(t0 >= 0, t1 >= 0) and np.array_equal(t0 >= 0, t2 >= 0)
    assert np.array_equal(t0, t1) and np.array_equal(d0, d1)                       # the visible side is the front
    assert (d2[t2 >= 0] > d1[t2 >= 0]).all()                                       # the back faces lie behind it
    # the ray of pixel (32, 32), half a pixel off the axis, meets the unit sphere at 4 - 1 = 3 (to 1e-3); the inscribed polyhedron lies behind the
    # sphere by at most the sagitta of a facet, 1 - cos(pi/16) cos(pi/12) = 0.0527 (half a step in latitude and in longitude)
    assert 3.0 - 1e-3 <= float(d0[32, 32]) <= 3.0 + 0.0527 + 1e-3


def test_the_integer_path_stays_inside_int64_at_the_guard_band():
    G, far = R.GUARD, 256 * (R.MAX_DIM - 1)
    worst = 0
    corners = [(-G, -G), (G, -G), (G, G), (-G, G)]
    for a in corners:
        for b in corners:
            for c in corners:
                for P in ((0, 0), (far, 0), (0, far), (far, far)):
                    vals = [R.orient(*a, *b, *c), R.orient(*a, *b, *P), R.orient(*b, *c, *P), R.orient(*c, *a, *P)]
                    worst = max(worst, max(abs(v) for v in vals))
    assert worst < 1 << 48 and worst.bit_length() <= 48                            # the header's bound; int64 holds 2^63
    # numpy's int64 path gives the same values as Python's integers there
    X, Y = np.array([-G, G, G]), np.array([-G, -G, G])
    st = R.setup(X, Y, np.ones(3, np.float32), (0, 1, 2))
    e = R.edge_values(st[2], np.array([R.MAX_DIM - 1]), np.array([R.MAX_DIM - 1]))
    assert [int(v[0]) for v in e] == [dx * (far - ay) - dy * (far - ax) for ax, ay, dx, dy, _ in st[2]]


def test_projection_puts_make_o_ds_ray_points_on_their_pixel_centres():
    """A point o + t d on the ray make_o_d gives pixel (i, j) projects to screen (i, j) with z = t."""
    cam = R.camera(48, 64, 70.0, 65.0, 31.5, 23.5, R.look_at(123, 40, 4.0))
    c2w = cam.c2w.astype(np.float64)
    pts, want = [], []
    for (i, j, t) in ((0, 0, 2.0), (63, 47, 3.5), (10, 40, 1.25), (31, 23, 6.0)):
        d = c2w[:, :3] @ np.array([(i - cam.cx) / cam.fx, -(j - cam.cy) / cam.fy, -1.0])
        pts.append(c2w[:, 3] + t * d)
        want.append((i, j, t))
    X, Y, z, valid, sx, sy = R.project(cam, 1e-3, np.asarray(pts, np.float32))
    assert valid.all()
    for k, (i, j, t) in enumerate(want):
        assert abs(sx[k] - i) < 1e-4 and abs(sy[k] - j) < 1e-4 and abs(z[k] - t) < 1e-5 and abs(X[k] - 256 * i) <= 1 and abs(Y[k] - 256 * j) <= 1


# ---------------------------------------------------------------------------------------------------
# the library without a GPU
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def msh():
    from nerf_pytorch_paeng_amd import _mesh
    from nerf_pytorch_paeng_amd.build import build_mesh_library
    build_mesh_library()
    _mesh.lib()
    return _mesh


def test_the_view_consumer_compiles_as_c99_links_and_answers(tmp_path, msh):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not found")
    pkg = os.path.dirname(msh.LIB_PATH)
    exe = str(tmp_path / "mesh_view_consumer")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "mesh_view_consumer.c"), "-L", pkg, "-lmi_nerf_mesh", f"-Wl,-rpath,{pkg}", f"-Wl,-rpath-link,{pkg}",
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mesh view c_abi consumer ok: ABI 2" in run.stdout and msh.ABI_VERSION == 2


@pytest.mark.parametrize("hw", [(1, 1), (7, 5), (64, 64), (130, 67), (800, 800), (16384, 16384)])
def test_the_raster_scratch_matches_the_headers_formula(msh, hw):
    assert msh.lib().mi_mesh_raster_scratch_bytes(*hw) == R.raster_scratch_bytes(*hw)
    assert (msh.VIEW_MAX_DIM, msh.VIEW_GUARD, msh.VIEW_LARGE_BOX, msh.VIEW_QUEUE) == (R.MAX_DIM, R.GUARD, R.LARGE_BOX, R.QUEUE)
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_mesh.h")).read()
    for name, value in (("MAX_DIM", R.MAX_DIM), ("GUARD", R.GUARD), ("LARGE_BOX", R.LARGE_BOX), ("QUEUE", R.QUEUE)):
        assert f"#define MI_MESH_VIEW_{name} {value} " in hdr


def _cam(msh, **kw):
    a = dict(H=64, W=48, fx=70.0, fy=70.0, cx=23.5, cy=31.5, c2w=[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4])
    a.update(kw)
    return msh.Camera(a["H"], a["W"], a["fx"], a["fy"], a["cx"], a["cy"], (C.c_float * 12)(*a["c2w"]))


def _refused(msh, rc, case):
    msg = msh.last_error()
    assert rc == EINVAL, (case, rc, msg)
    assert msg and "HIP error" not in msg, (case, msg)


def test_refusals_answer_einval_with_a_message_before_any_hip_call(msh):
    """The pointers are made-up addresses that are never dereferenced: every call here is refused before the first HIP call (a call that got
    as far as one would answer MI_MESH_EHIP on a machine without a GPU)."""
    L = msh.lib()
    nan, inf, big = float("nan"), float("inf"), 1 << 31
    need = L.mi_mesh_raster_scratch_bytes(64, 48)
    assert need > 0
    for hw in ((0, 48), (64, 0), (-1, 48), (64, -3), (16385, 48), (64, 16385)):
        assert L.mi_mesh_raster_scratch_bytes(*hw) == 0 and msh.last_error(), hw

    prj = dict(cam=_cam(msh), near=0.1, verts=0x1000, V=10, X=0x2000, Y=0x3000, z=0x4000)
    bad = {"near 0": dict(near=0.0), "near negative": dict(near=-1.0), "near NaN": dict(near=nan), "NULL verts": dict(verts=None), "NULL X": dict(X=None),
           "NULL Y": dict(Y=None), "NULL z": dict(z=None), "misaligned verts": dict(verts=0x1002), "misaligned X": dict(X=0x2001),
           "misaligned z": dict(z=0x4002), "V negative": dict(V=-1), "V above int32": dict(V=big), "H 0": dict(cam=_cam(msh, H=0)),
           "W negative": dict(cam=_cam(msh, W=-4)), "H above the maximum": dict(cam=_cam(msh, H=16385)), "fx 0": dict(cam=_cam(msh, fx=0.0)),
           "fy NaN": dict(cam=_cam(msh, fy=nan)), "cx inf": dict(cam=_cam(msh, cx=inf)), "pose NaN": dict(cam=_cam(msh, c2w=[1, 0, 0, 0, 0, nan, 0, 0, 0, 0, 1, 4]))}
    for case, kw in bad.items():
        a = dict(prj, **kw)
        _refused(msh, L.mi_mesh_project(C.byref(a["cam"]), a["near"], a["verts"], a["V"], a["X"], a["Y"], a["z"], None), "project " + case)
    _refused(msh, L.mi_mesh_project(None, 0.1, 0x1000, 10, 0x2000, 0x3000, 0x4000, None), "project NULL cam")

    ras = dict(H=64, W=48, cull=0, box=0, X=0x2000, Y=0x3000, z=0x4000, V=10, tris=0x5000, T=6, scratch=0x100000, nbytes=need, tri=0x6000, depth=0x7000)
    bad = {"H 0": dict(H=0), "W 0": dict(W=0), "H negative": dict(H=-2), "W above the maximum": dict(W=16385), "cull -1": dict(cull=-1), "cull 3": dict(cull=3),
           "large_box negative": dict(box=-1), "NULL X": dict(X=None), "NULL Y": dict(Y=None), "NULL z": dict(z=None), "NULL tris": dict(tris=None),
           "misaligned Y": dict(Y=0x3002), "misaligned tris": dict(tris=0x5001), "V above int32": dict(V=big), "T above int32": dict(T=big),
           "T negative": dict(T=-1), "NULL scratch": dict(scratch=None), "misaligned scratch": dict(scratch=0x100010), "short scratch": dict(nbytes=need - 1),
           "no output": dict(tri=None, depth=None), "misaligned tri_out": dict(tri=0x6002), "misaligned depth_out": dict(depth=0x7001)}
    for case, kw in bad.items():
        a = dict(ras, **kw)
        _refused(msh, L.mi_mesh_raster(a["H"], a["W"], a["cull"], a["box"], a["X"], a["Y"], a["z"], a["V"], a["tris"], a["T"], a["scratch"], a["nbytes"],
                                       a["tri"], a["depth"], None), "raster " + case)

    bg = (C.c_float * 3)(1.0, 1.0, 1.0)
    shd = dict(H=64, W=48, X=0x2000, Y=0x3000, z=0x4000, V=10, tris=0x5000, T=6, tri_in=0x6000, colors=0x7000, normals=0x8000, bg=bg, rgb=0x9000, disp=0xa000,
               acc=0xb000, depth=0xc000, normal=0xd000)
    bad = {"H 0": dict(H=0), "W above the maximum": dict(W=16385), "NULL X": dict(X=None), "NULL tris": dict(tris=None), "NULL tri_in": dict(tri_in=None),
           "misaligned tri_in": dict(tri_in=0x6002), "V above int32": dict(V=big), "T above int32": dict(T=big), "V negative": dict(V=-5),
           "no output": dict(rgb=None, disp=None, acc=None, depth=None, normal=None), "NULL colors with rgb": dict(colors=None),
           "NULL normals with normal": dict(normals=None), "NULL bg with rgb": dict(bg=None), "misaligned rgb": dict(rgb=0x9001), "misaligned acc": dict(acc=0xb002),
           "misaligned colors": dict(colors=0x7002)}
    for case, kw in bad.items():
        a = dict(shd, **kw)
        _refused(msh, L.mi_mesh_shade(a["H"], a["W"], a["X"], a["Y"], a["z"], a["V"], a["tris"], a["T"], a["tri_in"], a["colors"], a["normals"], a["bg"], a["rgb"],
                                      a["disp"], a["acc"], a["depth"], a["normal"], None), "shade " + case)


def test_an_empty_vertex_list_projects_to_nothing_without_a_device(msh):
    """V == 0 launches nothing, so mi_mesh_project answers MI_MESH_OK here, where any HIP call would fail.  (T == 0 and V == 0 in mi_mesh_raster
    still clear and resolve the frame: tests/test_gpu_mesh_view.py.  H W == 0 cannot occur: H == 0 or W == 0 is refused, above.)"""
    assert msh.lib().mi_mesh_project(C.byref(_cam(msh)), 0.1, None, 0, None, None, None, None) == 0


def test_render_refuses_by_name_without_a_gpu(msh):
    from nerf_pytorch_paeng_amd import mesh
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    K = [[70.0, 0.0, 23.5], [0.0, 72.0, 31.5], [0.0, 0.0, 1.0]]
    cam = mesh.Camera(64, 48, K, torch.eye(4)[:3])
    assert (cam.c.H, cam.c.W, cam.c.fx, cam.c.fy, cam.c.cx, cam.c.cy) == (64, 48, 70.0, 72.0, 23.5, 31.5) and cam.device is None
    assert list(mesh.Camera(64, 48, K, np.eye(4)).c.c2w) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    with pytest.raises(MiNerfError, match="pose"):
        mesh.Camera(64, 48, K, np.eye(3))
    verts = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    tris = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(MiNerfError, match="colorize"):
        mesh.Mesh(verts, tris).render(cam)
    with pytest.raises(MiNerfError, match="normals"):
        mesh.Mesh(verts, tris, colors=torch.ones(3, 3)).render(cam, normals=True)
    with pytest.raises(MiNerfError, match="HIP device"):
        mesh.Mesh(verts, tris, colors=torch.ones(3, 3)).render(cam)                # a CPU mesh: no fallback
    with pytest.raises(MiNerfError, match="HIP device"):
        mesh.Mesh(verts, tris).project(cam)
    with pytest.raises(MiNerfError, match="mesh.Camera"):
        mesh.Mesh(verts, tris, colors=torch.ones(3, 3)).render(K)


def test_the_harness_refuses_baked_and_mesh_view_together():
    from types import SimpleNamespace
    from nerf_pytorch_paeng_amd import harness, mesh
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    m = mesh.Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), colors=torch.ones(3, 3))
    with pytest.raises(MiNerfError, match="mesh_view"):
        harness._frozen(None, SimpleNamespace(baked=object(), mesh_view=m))
    assert harness._frozen(None, SimpleNamespace(mesh_view=m)) is None
    assert harness._device_of(None, SimpleNamespace(mesh_view=m)) == torch.device("cpu")
