"""THE VIEW of include/mi_nerf_mesh.h on the GPU against its numpy restatement (tests/mesh_view_restate.py: float64 the comparator, float32 the
same operations in the same order).  Bars: with e_ref = max|f32 restatement - f64| and e_hip = max|HIP - f64| on the same inputs,
e_hip <= max(4 e_ref, ulp), ulp one fp32 unit in the last place at the output's largest magnitude.  Coverage is integer arithmetic, so the
winners are compared EXACTLY: on the device's own snapped integers for projected scenes (with the one exception the test states), and on
shapes built directly in fixed point, whose depths are equal or far apart, for every frame size and cull mode.  Every test prints what it
measured before it asserts."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import _mesh, harness, mesh, ops, scenes
from nerf_pytorch_paeng_amd._lib import dev_ptr, stream_ptr
from tests import mesh_view_restate as R
from tests.test_mesh_cpu import sphere_lattice

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32
IMIN = -(1 << 31)
SENT = 12345.0


def ulp_at(x):
    return float(np.spacing(f32(np.max(np.abs(x))))) if np.size(x) else 0.0


def bar(got, ref64, ref32, what):
    """(e_hip, e_ref, allowed) over finite reference values; prints the three."""
    got, ref64, ref32 = (np.asarray(a, np.float64) for a in (got, ref64, ref32))
    e_hip = float(np.max(np.abs(got - ref64))) if got.size else 0.0
    e_ref = float(np.max(np.abs(ref32 - ref64))) if got.size else 0.0
    allowed = max(4.0 * e_ref, ulp_at(ref64))
    print(f"\n[view {what}] e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  allowed {allowed:.3e}  n {got.size}", end="")
    return e_hip, e_ref, allowed


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


def ccam(cam):
    return _mesh.Camera(cam.H, cam.W, float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy), (C.c_float * 12)(*cam.c2w.reshape(-1).tolist()))


def pycam(cam):
    K = [[cam.fx, 0.0, cam.cx], [0.0, cam.fy, cam.cy], [0.0, 0.0, 1.0]]
    return mesh.Camera(cam.H, cam.W, K, cam.c2w)


def dev_project(cam, near, verts):
    V = len(verts)
    v = dev(verts, f32)
    X, Y, z = torch.empty(V, dtype=torch.int32, device=DEV), torch.empty(V, dtype=torch.int32, device=DEV), torch.empty(V, device=DEV)
    _mesh.check(_mesh.lib().mi_mesh_project(C.byref(ccam(cam)), float(near), dev_ptr(v), V, dev_ptr(X, "X", torch.int32), dev_ptr(Y, "Y", torch.int32),
                                            dev_ptr(z), stream_ptr(DEV)), "mi_mesh_project")
    return X.cpu().numpy(), Y.cpu().numpy(), z.cpu().numpy()


class Soup:
    """A triangle list in fixed point on the device: what mi_mesh_raster and mi_mesh_shade take."""

    def __init__(self, X, Y, z, tris):
        self.Xh, self.Yh = np.asarray(X, np.int64), np.asarray(Y, np.int64)
        self.zh, self.th = np.asarray(z, f32), np.asarray(tris, np.int64).reshape(-1, 3)
        self.V, self.T = len(self.Xh), len(self.th)
        self.X, self.Y, self.z = dev(self.Xh, np.int32), dev(self.Yh, np.int32), dev(self.zh, f32)
        self.tris = dev(self.th, np.int32)

    def args(self):
        p = lambda t: dev_ptr(t, "t", torch.int32)
        return (p(self.X) if self.V else None, p(self.Y) if self.V else None, dev_ptr(self.z) if self.V else None, self.V, p(self.tris) if self.T else None, self.T)


def dev_raster(s, H, W, cull=0, large_box=0, counters=False):
    L = _mesh.lib()
    n = L.mi_mesh_raster_scratch_bytes(H, W)
    scratch = torch.empty(n, dtype=torch.uint8, device=DEV)
    tri, depth = torch.empty(H, W, dtype=torch.int32, device=DEV), torch.empty(H, W, device=DEV)
    _mesh.check(L.mi_mesh_raster(H, W, cull, large_box, *s.args(), dev_ptr(scratch, "scratch", torch.uint8, 256), n, dev_ptr(tri, "tri", torch.int32), dev_ptr(depth),
                                 stream_ptr(DEV)), "mi_mesh_raster")
    if counters:
        off = R.a256(8 * H * W)
        c = scratch[off:off + 24].cpu().numpy().view(np.uint32)
        return tri.cpu().numpy(), depth.cpu().numpy(), (int(c[0]), int(c[1]), int(c[2]) | int(c[3]) << 32, int(c[4]) | int(c[5]) << 32)
    return tri.cpu().numpy(), depth.cpu().numpy()


OUTS = (("rgb", 3), ("disp", 1), ("acc", 1), ("depth", 1), ("normal", 3))


def dev_shade(s, H, W, tri, colors, normals, bg, want=("rgb", "disp", "acc", "depth", "normal"), guard=64):
    """The outputs named in ``want`` (the others are passed as NULL), each inside a buffer with ``guard`` sentinel floats either side; returns
    the outputs and whether every sentinel survived."""
    tri_d = dev(tri, np.int32)
    col = None if colors is None else dev(colors, f32)
    nrm = None if normals is None else dev(normals, f32)
    bufs = {k: torch.full((H * W * ch + 2 * guard,), SENT, device=DEV) for k, ch in OUTS}
    ptr = lambda k: bufs[k].data_ptr() + 4 * guard if k in want else None
    _mesh.check(_mesh.lib().mi_mesh_shade(H, W, *s.args(), dev_ptr(tri_d, "tri", torch.int32), dev_ptr(col), dev_ptr(nrm), (C.c_float * 3)(*bg), ptr("rgb"), ptr("disp"),
                                          ptr("acc"), ptr("depth"), ptr("normal"), stream_ptr(DEV)), "mi_mesh_shade")
    out, intact = {}, True
    for k, ch in OUTS:
        b = bufs[k].cpu().numpy()
        body = b[guard:len(b) - guard]
        intact &= bool((b[:guard] == SENT).all() and (b[len(b) - guard:] == SENT).all())
        if k in want:
            out[k] = body.reshape((H, W, 3) if ch == 3 else (H, W))
        else:
            intact &= bool((body == SENT).all())
    return out, intact


# ---------------------------------------------------------------------------------------------------
# 1. project
# ---------------------------------------------------------------------------------------------------
POSES = [(30, -30, 4.0), (0, 0, 4.0), (123, 40, 3.0), (271, 5, 5.0)]


def project_case(V, pose, seed):
    """V random vertices in the box +-1.5; from V = 7 on: one behind the camera, one NaN per axis, one far beyond the guard band along each screen
    axis, and ``near`` set to the fp32 depth of vertex 6 exactly, so that it fails z > near by equality."""
    cam = R.camera(48, 64, 70.0, 66.0, 31.5, 23.5, R.look_at(*pose))
    rng = np.random.default_rng(seed)
    verts = (rng.random((V, 3)) * 3.0 - 1.5).astype(f32)
    near = 1e-3
    if V >= 7:
        c2w = cam.c2w.astype(np.float64)
        right, up, back, eye = c2w[:, 0], c2w[:, 1], c2w[:, 2], c2w[:, 3]
        verts[0] = (eye + 2.0 * back).astype(f32)                                  # behind the camera
        verts[1, 0], verts[2, 1], verts[3, 2] = np.nan, np.nan, np.nan
        verts[4] = (eye - 10.0 * back + 1e6 * right).astype(f32)                   # z = 10, 256 sx = 256 * 70 * 1e5: far beyond 2^22
        verts[5] = (eye - 10.0 * back - 1e6 * up).astype(f32)
        verts[6] = (eye - 2.0 * back + 0.1 * right + 0.2 * up).astype(f32)         # in front of the box: most of the others lie behind it
        near = float(R.project(cam, 1e-3, verts, f32)[2][6])
        assert 1.9 < near < 2.1
    return cam, near, verts


@pytest.mark.parametrize("pose", range(4))
@pytest.mark.parametrize("V", [1, 7, 1000])
def test_project_matches_the_restatement(V, pose):
    cam, near, verts = project_case(V, POSES[pose], 100 * pose + V)
    X, Y, z = dev_project(cam, near, verts)
    X32, Y32, z32, ok32, sx32, sy32 = R.project(cam, near, verts, f32)
    X64, Y64, z64, ok64, sx64, sy64 = R.project(cam, near, verts, np.float64)
    ok = z != 0
    assert np.array_equal(ok, ok32), (np.nonzero(ok != ok32), near)
    assert (X[~ok] == IMIN).all() and (Y[~ok] == IMIN).all() and (z[~ok] == 0).all()
    if V >= 7:
        assert not ok[:7].any() and not ok32[:7].any() and (V == 7 or ok[7:].sum() > 100)
    both = ok & ok64
    e_hip, e_ref, allowed = bar(z[both], z64[both], z32[both], f"project z V={V} pose={pose}")
    assert e_hip <= allowed
    for name, got, s64, s32 in (("X", X, sx64, sx32), ("Y", Y, sy64, sy32)):
        e_ref_s = float(np.max(np.abs(s32[both].astype(np.float64) - s64[both]))) if both.any() else 0.0
        allowed = 0.5 + 256.0 * max(4.0 * e_ref_s, ulp_at(s64[both]))
        worst = float(np.max(np.abs(got[both] - 256.0 * s64[both]))) if both.any() else 0.0
        exact = int((got[both] == (X64 if name == "X" else Y64)[both]).sum())
        print(f"  {name}: max |{name} - 256 s64| {worst:.4f} allowed {allowed:.4f}; equal to the float64 snap {exact} of {int(both.sum())}", end="")
        assert worst <= allowed
        assert np.array_equal(got[ok], (X32 if name == "X" else Y32)[ok])           # nothing is contracted: the fp32 restatement bit for bit


def test_an_empty_vertex_list_and_mesh_project():
    m = mesh.Mesh(torch.empty(0, 3, device=DEV), torch.empty(0, 3, dtype=torch.int32, device=DEV))
    X, Y, z = m.project(pycam(R.scene_camera((0, 0))))
    assert X.shape == Y.shape == z.shape == (0,) and X.dtype == torch.int32
    verts, tris, _, _ = R.two_spheres_two_quads()
    cam = R.scene_camera((30, -30))
    X, Y, z = mesh.Mesh(dev(verts, f32), dev(tris, np.int32)).project(pycam(cam), near=0.5)
    Xd, Yd, zd = dev_project(cam, 0.5, verts)
    assert np.array_equal(X.cpu().numpy(), Xd) and np.array_equal(Y.cpu().numpy(), Yd) and np.array_equal(z.cpu().numpy(), zd)


# ---------------------------------------------------------------------------------------------------
# 2. raster, exact layer: the device's own integers through the float64 restatement
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_views():
    """Per view of the 64 x 64 scene: the device's projection, its raster, and the two restatements on the device's integers (computed once)."""
    verts, tris, colors, normals = R.two_spheres_two_quads()
    out = []
    for view in R.SCENE_VIEWS:
        cam = R.scene_camera(view)
        X, Y, z = dev_project(cam, 1e-3, verts)
        s = Soup(X, Y, z, tris)
        tri, depth = dev_raster(s, 64, 64)
        t64, d64 = R.raster(64, 64, 0, s.Xh, s.Yh, s.zh, tris, np.float64)
        t32, d32 = R.raster(64, 64, 0, s.Xh, s.Yh, s.zh, tris, f32)
        out.append(SimpleNamespace(view=view, cam=cam, s=s, tri=tri, depth=depth, t64=t64, d64=d64, t32=t32, d32=d32, colors=colors, normals=normals, tris=tris))
    return out


@pytest.mark.parametrize("k", range(4))
def test_raster_equals_the_restatement_on_the_devices_integers(scene_views, k):
    c = scene_views[k]
    covered = c.t64 >= 0
    assert np.array_equal(c.tri >= 0, covered) and covered.sum() > 1000
    agree = c.tri == c.t64
    same = covered & (c.t32 == c.t64)
    e_ref_rel = float(np.max(np.abs(c.d32[same].astype(np.float64) - c.d64[same]) / c.d64[same]))      # what fp32 allows the depth, relative
    excepted = 0
    for py, px in zip(*np.nonzero(~agree)):
        # the stated exception: the device's winner covers the pixel too and its float64 depth is within 4 e_ref (relative) of the restatement's winner's
        cov, d_dev = R.tri_depth_at(c.s.Xh, c.s.Yh, c.s.zh, c.tris, int(c.tri[py, px]), py, px)
        assert cov and abs(d_dev - c.d64[py, px]) <= 4.0 * e_ref_rel * c.d64[py, px], (py, px, c.tri[py, px], c.t64[py, px], d_dev, c.d64[py, px])
        excepted += 1
    share = excepted / int(covered.sum())
    sel = agree & covered
    e_hip, e_ref2, allowed = bar(c.depth[sel], c.d64[sel], c.d32[sel], f"raster depth view={c.view}")
    print(f"  covered {int(covered.sum())}, excepted pixels {excepted} (share {share:.4%}); fp32 restatement disagrees at {int((c.t32 != c.t64).sum())}; "
          f"relative e_ref {e_ref_rel:.3e}", end="")
    assert share <= 0.005
    assert e_hip <= allowed
    assert (c.depth[~covered] == 0).all() and (c.tri[~covered] == -1).all()
    assert np.array_equal(c.depth.view(np.uint32)[sel & same], c.d32.view(np.uint32)[sel & same])      # nothing is contracted: the fp32 restatement bit for bit


# ---------------------------------------------------------------------------------------------------
# 3. raster on shapes built directly in fixed point
# ---------------------------------------------------------------------------------------------------
def px(*pts):
    """Pixel coordinates (floats) -> 24.8 integers."""
    return [(int(round(256 * x)), int(round(256 * y))) for x, y in pts]


def soup_of(tri_pts, zs=None, tris=None):
    pts = [p for t in tri_pts for p in t]
    z = np.ones(len(pts), f32) if zs is None else np.repeat(np.asarray(zs, f32), 3)
    if tris is None:
        tris = np.arange(len(pts)).reshape(-1, 3)
    return Soup([p[0] for p in pts], [p[1] for p in pts], z, tris)


def micro_triangles(H, W, n=5000, seed=5):
    """n random triangles of a few pixels with vertices of their own; triangle t lies at depth 1 + t / 100, so overlapping ones are far apart."""
    rng = np.random.default_rng(seed)
    c = rng.random((n, 1, 2)) * [W + 4, H + 4] - 2
    p = np.rint(256 * (c + rng.random((n, 3, 2)) * 5.0 - 2.5)).astype(np.int64)
    p[::7] = (p[::7] // 256) * 256                                                 # every seventh with all vertices on pixel centres
    return Soup(p[:, :, 0].ravel(), p[:, :, 1].ravel(), np.repeat(1.0 + np.arange(n) / 100.0, 3).astype(f32), np.arange(3 * n).reshape(-1, 3))


def shapes(H, W):
    w, h = float(W), float(H)
    quad = px((0.6, 0.4), (0.8 * w + 0.3, 0.7), (0.9 * w, 0.85 * h + 0.1), (0.3, 0.9 * h))
    S = {
        "one triangle": soup_of([px((0.3 * w, 0.2 * h), (0.9 * w + 0.37, 0.5 * h), (0.2 * w, 0.9 * h + 0.41))]),
        "the whole frame (large class)": soup_of([px((-10, -10), (3 * w + 10, -10), (-10, 3 * h + 10))]),
        "partly off each side": soup_of([px((-3.3, 0.2 * h), (2.6, 0.5 * h), (-2.1, 0.8 * h)), px((w - 2.2, 0.1 * h), (w + 4.7, 0.4 * h), (w - 1.4, 0.9 * h)),
                                         px((0.2 * w, -3.1), (0.8 * w, -2.2), (0.5 * w, 2.7)), px((0.1 * w, h + 3.3), (0.9 * w, h + 1.2), (0.4 * w, h - 2.8))],
                                        zs=[1, 2, 3, 4]),
        "wholly off each side": soup_of([px((-9, 1), (-2, 2), (-5, 7)), px((w + 1, 1), (w + 6, 2), (w + 3, 7)), px((1, -9), (5, -2), (2, -1.2)),
                                         px((1, h + 0.1), (5, h + 3), (2, h + 6))]),
        "smaller than a pixel, no centre": soup_of([px((2.2, 2.2), (2.7, 2.3), (2.4, 2.8)), px((0.1, 0.1), (0.9, 0.2), (0.5, 0.9))]),
        "zero area": soup_of([px((1, 1), (3, 3), (5, 5)), px((2, 2), (2, 2), (4, 1)), px((3, 1), (3, 1), (3, 1))]),
        "vertices on centres, edges through centres": soup_of([px((1, 1), (5, 1), (1, 5)), px((5, 5), (5, 1), (1, 5)), px((0, 0), (0, 3), (3, 0))], zs=[1, 1, 2]),
        "a quad, first order": Soup([q[0] for q in quad], [q[1] for q in quad], np.ones(4, f32), [(0, 1, 2), (0, 2, 3)]),
        "a quad, second order": Soup([q[0] for q in quad], [q[1] for q in quad], np.ones(4, f32), [(0, 2, 3), (0, 1, 2)]),
        "a quad, other diagonal and winding": Soup([q[0] for q in quad], [q[1] for q in quad], np.ones(4, f32), [(1, 3, 2), (3, 1, 0)]),
        "coincident triangles at equal depth": soup_of([px((0.1 * w, 0.1 * h), (0.9 * w, 0.3 * h), (0.4 * w, 0.95 * h))] * 3, zs=[2, 2, 2],
                                                       tris=[(3, 4, 5), (0, 1, 2), (6, 7, 8), (0, 1, 2)]),
        "index outside [0, V)": Soup(*zip(*px((0, 0), (w, 0), (0, h))), np.ones(3, f32), [(0, 1, 3), (-1, 1, 2), (0, 2 ** 31 - 1, 2), (0, 1, 2), (IMIN, 0, 1)]),
        "box of 30, 32 and 33 pixels": soup_of([px((0.5, 0.5), (5.4, 0.6), (3.0, 6.4)), px((10.5, 0.5), (14.4, 0.6), (12.0, 8.4)),
                                                px((20.5, 0.5), (23.4, 0.6), (22.0, 11.4))]),      # 5 x 6, 4 x 8, 3 x 11: around MI_MESH_VIEW_LARGE_BOX
        "5000 micro-triangles": micro_triangles(H, W),
    }
    bad = soup_of([px((0.1 * w, 0.1 * h), (0.9 * w, 0.3 * h), (0.4 * w, 0.95 * h))] * 7)
    z = bad.zh.copy()
    X = bad.Xh.copy()
    z[0], z[3], z[6], z[9] = 0.0, np.nan, -1.0, np.inf
    X[0] = IMIN
    X[12] = R.GUARD + 1
    X[15] = -R.GUARD - 1                                                           # triangle 6 alone is valid
    S["invalid vertices"] = Soup(X, bad.Yh, z, bad.th)
    return S


@pytest.mark.parametrize("cull", [0, 1, 2])
@pytest.mark.parametrize("hw", [(1, 1), (7, 5), (64, 64), (130, 67)])
def test_raster_of_fixed_point_shapes_is_exactly_the_restatements(hw, cull):
    H, W = hw
    drawn = {}
    for name, s in shapes(H, W).items():
        tri, depth = dev_raster(s, H, W, cull)
        want_t, want_d = R.raster(H, W, cull, s.Xh, s.Yh, s.zh, s.th, np.float64)
        assert np.array_equal(tri, want_t), (name, hw, cull, int((tri != want_t).sum()))
        assert ((depth == 0) == (tri < 0)).all()
        cov = tri >= 0
        if cov.any():
            assert np.max(np.abs(depth[cov] - want_d[cov]) / want_d[cov]) < 1e-6, name
        drawn[name] = int(cov.sum())
        for box in (1, 12, 31, 33, 256, 1 << 30):                                     # the size class a triangle lands in changes no bit
            t2, d2 = dev_raster(s, H, W, cull, large_box=box)
            assert np.array_equal(t2, tri) and np.array_equal(d2.view(np.uint32), depth.view(np.uint32)), (name, box)
    print(f"\n[view shapes {H}x{W} cull {cull}] covered pixels: {drawn}", end="")
    assert drawn["smaller than a pixel, no centre"] == 0 and drawn["zero area"] == 0 and drawn["wholly off each side"] == 0
    if cull == 0:
        assert drawn["the whole frame (large class)"] == H * W and drawn["invalid vertices"] == drawn["coincident triangles at equal depth"]
        assert drawn["invalid vertices"] > 0 or H * W == 1                           # in the 1 x 1 frame that triangle misses the one centre
        assert drawn["a quad, first order"] == drawn["a quad, second order"] == drawn["a quad, other diagonal and winding"]
    else:
        assert drawn["the whole frame (large class)"] == (0 if cull == 1 else H * W)         # it is wound clockwise on the screen: a back face


def test_the_smaller_number_wins_an_exact_tie_and_the_classes_are_counted():
    H, W = 64, 64
    s = shapes(H, W)["coincident triangles at equal depth"]
    tri, _, (met, by_lane, atomics, lowered) = dev_raster(s, H, W, counters=True)
    assert set(np.unique(tri)) == {-1, 0}                                          # triangles 0..3 are the same triangle: number 0 wins everywhere
    covered = int((tri == 0).sum())
    assert (met, by_lane, atomics) == (4, 0, 4 * covered)                          # four large triangles, each sample one atomic update
    assert covered <= lowered <= 4 * covered                                       # how many of them lowered a word depends on the order they came in
    assert _mesh.VIEW_LARGE_BOX == 32
    s = shapes(H, W)["box of 30, 32 and 33 pixels"]
    _, _, (met, by_lane, _, _) = dev_raster(s, H, W, counters=True)
    assert (met, by_lane) == (1, 2)                                                # 5 x 6 and 4 x 8 stay with a lane, 3 x 11 goes to a wave
    _, _, (met, by_lane, _, _) = dev_raster(s, H, W, large_box=31, counters=True)
    assert (met, by_lane) == (2, 1)


def test_a_full_queue_leaves_the_rest_to_the_lanes():
    """More large triangles than MI_MESH_VIEW_QUEUE holds (large_box = 1: every box of two pixels or more is large): the ones beyond the queue are
    walked by their own lane and the frame is the default threshold's bit for bit.  95 536 triangles on 130 x 67 pixels also make this the test with
    the most updates per word."""
    H, W, n = 130, 67, _mesh.VIEW_QUEUE + 30000                                   # about 0.84 of them have a box of two pixels or more
    s = micro_triangles(H, W, n=n, seed=9)
    tri, depth = dev_raster(s, H, W)
    t2, d2, (met, by_lane, _, _) = dev_raster(s, H, W, large_box=1, counters=True)
    print(f"\n[view queue] large triangles met {met}, drawn by a lane {by_lane}", end="")
    assert met > _mesh.VIEW_QUEUE and by_lane >= met - _mesh.VIEW_QUEUE
    assert np.array_equal(tri, t2) and np.array_equal(depth.view(np.uint32), d2.view(np.uint32)) and (tri >= 0).sum() > 0.9 * H * W
    # every word is ONE sample: the depth half is the depth of the triangle in the other half (at about 19 samples per pixel from 374 blocks, an
    # update whose operands change in flight shows here: the form of the atomic without a return did that, see csrc/mesh_view.hip `sample`)
    out, _ = dev_shade(s, H, W, tri, None, None, (1.0, 1.0, 1.0), want=("depth",))
    assert np.array_equal(out["depth"].view(np.uint32), depth.view(np.uint32)) and depth[tri >= 0].min() >= 1.0


def test_an_empty_triangle_list_clears_the_frame():
    for s in (Soup([], [], [], np.zeros((0, 3))), Soup([0, 256, 0], [0, 0, 256], [1, 1, 1], np.zeros((0, 3))), Soup([], [], [], [(0, 1, 2)])):
        tri, depth = dev_raster(s, 7, 5)
        assert (tri == -1).all() and (depth == 0).all()
    m = mesh.Mesh(torch.empty(0, 3, device=DEV), torch.empty(0, 3, dtype=torch.int32, device=DEV), colors=torch.empty(0, 3, device=DEV))
    frame = m.render(pycam(R.scene_camera((0, 0))), bg=(0.25, 0.5, 0.75))
    assert torch.equal(frame.rgb, torch.tensor([0.25, 0.5, 0.75], device=DEV).expand(64, 64, 3)) and frame.normal is None
    assert float(frame.acc.abs().max()) == 0 and float(frame.depth.abs().max()) == 0 and float(frame.disp.abs().max()) == 0 and bool((frame.tri == -1).all())


# ---------------------------------------------------------------------------------------------------
# 4. determinism
# ---------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical(scene_views):
    c = scene_views[0]
    micro = micro_triangles(64, 64)
    rng = np.random.default_rng(1)
    for s, colors in ((c.s, c.colors), (micro, rng.random((micro.V, 3)).astype(f32))):
        runs = []
        for _ in range(2):
            tri, depth = dev_raster(s, 64, 64)
            out, _ = dev_shade(s, 64, 64, tri, colors, None, (1.0, 1.0, 1.0), want=("rgb",))
            runs.append((tri, depth.view(np.uint32), out["rgb"].view(np.uint32)))
        assert all(np.array_equal(a, b) for a, b in zip(*runs))


# ---------------------------------------------------------------------------------------------------
# 5. shade
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4))
def test_shade_matches_the_restatement_on_the_devices_winners(scene_views, k):
    c = scene_views[k]
    bg = (0.25, 0.5, 0.75)
    colors = (c.colors * 2.0 - 0.5).astype(f32)                                    # a quarter below 0, a quarter above 1: clamped
    out, intact = dev_shade(c.s, 64, 64, c.tri, colors, c.normals, bg)
    r64 = R.shade(64, 64, c.s.Xh, c.s.Yh, c.s.zh, c.tris, c.tri, colors, c.normals, bg, np.float64)
    r32 = R.shade(64, 64, c.s.Xh, c.s.Yh, c.s.zh, c.tris, c.tri, colors, c.normals, bg, f32)
    assert intact
    cov = c.tri >= 0
    for name in ("rgb", "disp", "depth", "normal"):
        e_hip, e_ref, allowed = bar(out[name][cov], r64[name][cov], r32[name][cov], f"shade {name} view={c.view}")
        assert np.isfinite(out[name]).all() and e_hip <= allowed, name
    assert np.array_equal(out["acc"], cov.astype(f32)) and np.array_equal(out["rgb"][~cov], np.broadcast_to(np.asarray(bg, f32), out["rgb"][~cov].shape))
    assert (out["disp"][~cov] == 0).all() and (out["depth"][~cov] == 0).all() and (out["normal"][~cov] == 0).all()
    assert np.array_equal(out["depth"].view(np.uint32), c.depth.view(np.uint32))    # the depth of the visibility pass, bit for bit
    rgb = out["rgb"][cov]
    assert rgb.min() == 0.0 and rgb.max() == 1.0 and (rgb == 0).sum() > 50 and (rgb == 1).sum() > 50
    nl = np.linalg.norm(out["normal"][cov].astype(np.float64), axis=-1)
    assert np.max(np.abs(nl - 1.0)) < 1e-6


def test_a_nan_colour_stays_in_its_own_triangles_and_null_outputs_are_not_written(scene_views):
    c = scene_views[0]
    bg = (1.0, 1.0, 1.0)
    full, intact = dev_shade(c.s, 64, 64, c.tri, c.colors, c.normals, bg)
    assert intact
    for want in (("rgb",), ("disp",), ("acc",), ("depth",), ("normal",), ("disp", "acc")):
        out, intact = dev_shade(c.s, 64, 64, c.tri, c.colors if "rgb" in want else None, c.normals if "normal" in want else None, bg, want=want)
        assert intact, want                                                        # the guards, and the whole body of every output passed as NULL
        assert all(np.array_equal(out[k].view(np.uint32), full[k].view(np.uint32)) for k in want), want
    v = int(c.tris[c.tri[c.tri >= 0][0]][0])                                       # a vertex of a visible triangle
    colors = c.colors.copy()
    colors[v, 1] = np.nan
    out, _ = dev_shade(c.s, 64, 64, c.tri, colors, None, bg, want=("rgb",))
    uses = np.zeros(c.tri.shape, bool)
    uses[c.tri >= 0] = (c.tris[c.tri[c.tri >= 0]] == v).any(-1)
    nan = np.isnan(out["rgb"])
    assert uses.sum() > 0 and np.array_equal(nan[..., 1], uses) and not nan[..., 0].any() and not nan[..., 2].any()
    assert np.array_equal(out["rgb"][~uses].view(np.uint32), full["rgb"][~uses].view(np.uint32))
    r32 = R.shade(64, 64, c.s.Xh, c.s.Yh, c.s.zh, c.tris, c.tri, colors, None, bg, f32)
    assert np.array_equal(np.isnan(r32["rgb"]), nan)


def test_mesh_render_is_the_three_entries(scene_views):
    c = scene_views[2]
    verts, tris, colors, normals = R.two_spheres_two_quads()
    m = mesh.Mesh(dev(verts, f32), dev(tris, np.int32), dev(normals, f32), dev(colors, f32))
    frame = m.render(pycam(c.cam), bg=(0.0, 0.5, 1.0), normals=True)
    out, _ = dev_shade(c.s, 64, 64, c.tri, colors, normals, (0.0, 0.5, 1.0))
    assert np.array_equal(frame.tri.cpu().numpy(), c.tri)
    for k in ("rgb", "disp", "acc", "depth", "normal"):
        assert np.array_equal(getattr(frame, k).cpu().numpy().view(np.uint32), out[k].view(np.uint32)), k
    front, back = m.render(pycam(c.cam), cull=1), m.render(pycam(c.cam), cull=2)
    both = (front.tri >= 0) | (back.tri >= 0)
    assert torch.equal(both, frame.tri >= 0) and int((front.tri >= 0).sum()) > 500 and int((back.tri >= 0).sum()) > 500
    assert m.render(pycam(c.cam)).normal is None
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        again = m.render(pycam(c.cam), bg=(0.0, 0.5, 1.0), normals=True)
    side.synchronize()
    assert torch.equal(again.rgb, frame.rgb) and torch.equal(again.tri, frame.tri) and torch.equal(again.depth, frame.depth)


# ---------------------------------------------------------------------------------------------------
# 6. end to end on an analytic sphere
# ---------------------------------------------------------------------------------------------------
def test_an_extracted_sphere_has_the_analytic_silhouette_and_depth():
    Rs, res, dist, focal, H, W = 0.6, 32, 4.0, 70.0, 64, 64
    f = torch.from_numpy(sphere_lattice(res, Rs)).to(DEV)
    m = mesh.extract(f, -1.0, 1.0, 0.0)
    m.colors = torch.full((m.verts.shape[0], 3), 0.5, device=DEV)
    cam = R.camera(H, W, focal, focal, 31.5, 31.5, R.look_at(30, -30, dist))
    frame = m.render(pycam(cam), cull=1)
    acc, depth = frame.acc.cpu().numpy(), frame.depth.cpu().numpy()
    # the ray of pixel (i, j): o + t d with d as make_o_d gives it (not normalised, d_z = -1 in the camera frame, so t is the depth of THE VIEW)
    c2w = cam.c2w.astype(np.float64)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(ii - 31.5) / focal, -(jj - 31.5) / focal, -np.ones_like(ii, np.float64)], -1) @ c2w[:, :3].T
    o = c2w[:, 3]
    dd, od = (d * d).sum(-1), d @ o

    def first_hit(r):                                                              # t of the first intersection with the sphere of radius r (NaN: none)
        disc = od * od - dd * (o @ o - r * r)
        with np.errstate(invalid="ignore"):
            return (-od - np.sqrt(disc)) / dd

    hit = first_hit(Rs)
    inside = ~np.isnan(hit)
    # silhouette: equal to the analytic disc except where the 3 x 3 neighbourhood of the pixel holds both kinds (within one pixel of its edge)
    pad = np.pad(inside, 1, mode="edge")
    nb = np.stack([pad[a:a + H, b:b + W] for a in range(3) for b in range(3)])
    clear = nb.all(0) | ~nb.any(0)
    assert clear.sum() > 0.8 * H * W and inside.sum() > 300
    assert np.array_equal(acc[clear] > 0, inside[clear])
    # depth.  Every mesh vertex lies within dv = L^2 / (8 (R - L)) of the sphere (docs/design/16_mesh.md 16.4; L = sqrt(3) h the cell diagonal).  The snap
    # moves a vertex by at most half a unit of 1/256 pixel along each screen axis, and the fp32 projection by far less: at most sw = sqrt(2) / 256
    # pixel in all, which at depth z <= dist + 1 is sw (dist + 1) / focal in space.  So the surface that is drawn is a set of flat triangles
    # whose vertices v_k have | |v_k| - R | <= dv + sw' and whose edges are at most L' = L + 2 sw' long (all of a cell).  A point of such a triangle,
    # p = sum l_k v_k, has |p| <= max |v_k| <= R + dv + sw' (the norm is convex) and |p|^2 = sum l_k |v_k|^2 - sum_{k<l} l_k l_l |v_k - v_l|^2
    # >= (R - dv - sw')^2 - L'^2 / 3 (the chord sagitta; sum_{k<l} l_k l_l <= 1/3).  The drawn surface is closed and lies between the spheres of
    # radius r_in and r_out, so the first hit of a ray with it lies between its first hits with those two spheres; the depth is
    # perspective-correct, exact on a flat triangle up to fp32 rounding (1e-5 here).
    h = 2.0 / res
    L = math.sqrt(3.0) * h
    dv = L * L / (8.0 * (Rs - L))
    sw = math.sqrt(2.0) / 256.0 * (dist + 1.0) / focal
    r_out = Rs + dv + sw
    r_in = math.sqrt((Rs - dv - sw) ** 2 - (L + 2 * sw) ** 2 / 3.0)
    t_out, t_in = first_hit(r_out), first_hit(r_in)
    p = o + hit[..., None] * d
    with np.errstate(invalid="ignore"):
        cosine = -(p * d).sum(-1) / (np.linalg.norm(p, axis=-1) * np.sqrt(dd))
        sel = inside & (cosine >= 0.5)
    assert sel.sum() > 200 and not np.isnan(t_in[sel]).any() and (acc[sel] == 1).all()
    err = np.abs(depth[sel] - hit[sel])
    allowed = np.maximum(hit[sel] - t_out[sel], t_in[sel] - hit[sel]) + 1e-5
    print(f"\n[view sphere] {int(m.tris.shape[0])} triangles, covered {int((acc > 0).sum())} (analytic {int(inside.sum())}); r_in {r_in:.5f} r_out {r_out:.5f}; "
          f"max |depth - analytic| {err.max():.5f} at cosine >= 0.5 ({int(sel.sum())} pixels), allowed there up to {allowed.max():.5f}, "
          f"largest share of its bound {np.max(err / allowed):.3f}", end="")
    assert (depth[sel] >= t_out[sel] - 1e-5).all() and (depth[sel] <= t_in[sel] + 1e-5).all()


# ---------------------------------------------------------------------------------------------------
# 7. the harness
# ---------------------------------------------------------------------------------------------------
def test_the_harness_renders_every_pose_from_the_mesh(tmp_path):
    H, W = 24, 24
    f = torch.from_numpy(sphere_lattice(16, 0.9)).to(DEV)
    m = mesh.extract(f, -1.0, 1.0, 0.0)
    m.colors = (m.verts * 0.5 + 0.5).clamp(0, 1).contiguous()
    K = scenes.scaled_camera((H, W))
    poses = harness.get_render_pose(n_angle=3, single_angle=-1, phi=-30.0, nf=4.0, device=DEV).float()
    opts = SimpleNamespace(data_type="blender", n_angle=3, single_angle=-1, phi=-30.0, nf=4.0, exp_name="mesh", mesh_view=m)
    rgbs, disps = harness.render(0, None, None, K, None, (H, W), opts, save_dir=str(tmp_path / "video"))
    gt = torch.rand(3, H, W, 3, generator=torch.Generator().manual_seed(8)).to(DEV)
    res = harness.test(0, [0, 1, 2], None, None, gt, K, poses, (H, W), opts, keep_frames=True)
    assert rgbs.shape == (3, H, W, 3) and disps.shape == (3, H, W) and rgbs.dtype == np.uint8
    for i in range(3):
        frame = m.render(mesh.Camera(H, W, K, poses[i]))
        want_rgb = ops.to8b(frame.rgb).cpu().numpy()
        want_disp = ops.to8b(frame.disp, ops.nanmax(frame.disp)).cpu().numpy()
        assert np.array_equal(rgbs[i], want_rgb) and np.array_equal(disps[i], want_disp)
        assert np.array_equal(res["frames"][i][0], want_rgb) and np.array_equal(res["frames"][i][1][..., 0], want_disp)
        assert 100 < int((frame.acc > 0).sum()) < H * W
        mse = float(((frame.rgb - gt[i]) ** 2).mean())
        assert res["loss"][i] == pytest.approx(mse, rel=1e-5) and res["psnr"][i] == pytest.approx(-10.0 * math.log10(mse), rel=1e-5)
    assert len(res["psnr"]) == 3 and all(math.isfinite(v) for v in res["psnr"] + res["loss"]) and res["mean_psnr"] == pytest.approx(np.mean(res["psnr"]))
    assert (tmp_path / "video" / "2_rgb.png").exists()
