"""THE VIEW of include/mi_nerf_mesh.h restated in numpy, written from the header comment.  ``dtype`` switches the floating point: float64 is the
comparator, float32 runs the same operations in the same order (every numpy operation on float32 arrays rounds once) and measures what the
arithmetic allows.  Snapping and coverage are int64 / Python integers in both.  Not a test module: tests/test_mesh_view_cpu.py holds it to
its own properties, tests/test_gpu_mesh_view.py compares the device with it."""
from types import SimpleNamespace

import numpy as np

GUARD = 1 << 22
MAX_DIM = 16384
LARGE_BOX = 32
QUEUE = 65536
INT32_MIN = -(1 << 31)


def a256(v):
    return (v + 255) & ~255


def raster_scratch_bytes(H, W):
    return a256(8 * H * W) + a256(24 + 4 * QUEUE)


def camera(H, W, fx, fy, cx, cy, c2w):
    return SimpleNamespace(H=int(H), W=int(W), fx=fx, fy=fy, cx=cx, cy=cy, c2w=np.asarray(c2w, np.float64)[:3, :4].astype(np.float32))


def look_at(azimuth_deg, elevation_deg, radius):
    """c2w [3,4] of a camera on a sphere around the origin that looks at the origin (it looks along its own -z, y up), in float32."""
    az, el = np.deg2rad(azimuth_deg), np.deg2rad(elevation_deg)
    eye = radius * np.array([np.cos(el) * np.sin(az), np.sin(el), np.cos(el) * np.cos(az)])
    back = eye / np.linalg.norm(eye)
    right = np.cross([0.0, 1.0, 0.0], back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    return np.concatenate([np.stack([right, up, back], 1), eye[:, None]], 1).astype(np.float32)


def project(cam, near, verts, dtype=np.float64):
    """(X, Y int64 [V], z dtype [V], valid bool [V], sx, sy dtype [V]).  Invalid: X = Y = INT32_MIN, z = 0."""
    T = dtype
    v = np.asarray(verts, np.float32).astype(T).reshape(-1, 3)
    R = cam.c2w.astype(T)
    with np.errstate(all="ignore"):
        d = [v[:, k] - R[k, 3] for k in range(3)]
        p = [(R[0, i] * d[0] + R[1, i] * d[1]) + R[2, i] * d[2] for i in range(3)]
        z = -p[2]
        sx = T(cam.cx) + (T(cam.fx) * p[0]) / z
        sy = T(cam.cy) - (T(cam.fy) * p[1]) / z
        fx8, fy8 = T(256) * sx, T(256) * sy
        valid = (z > T(np.float32(near))) & np.isfinite(z) & (np.abs(fx8) <= GUARD) & (np.abs(fy8) <= GUARD)
        X = np.where(valid, np.rint(np.where(valid, fx8, 0)), INT32_MIN).astype(np.int64)
        Y = np.where(valid, np.rint(np.where(valid, fy8, 0)), INT32_MIN).astype(np.int64)
    return X, Y, np.where(valid, z, T(0)).astype(T), valid, sx, sy


def orient(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def setup(X, Y, z, tri, cull=0):
    """The per-triangle part of Coverage on Python integers, or None when the triangle is not drawn.  Returns (s, a2, edges) with
    edges[k] = (ax, ay, dx, dy, top_left) of e_k."""
    V = len(X)
    idx = [int(i) for i in tri]
    if any(i < 0 or i >= V for i in idx):
        return None
    vx, vy, vz = [int(X[i]) for i in idx], [int(Y[i]) for i in idx], [float(z[i]) for i in idx]
    for k in range(3):
        if not (vz[k] > 0 and np.isfinite(vz[k]) and abs(vx[k]) <= GUARD and abs(vy[k]) <= GUARD):
            return None
    A2 = orient(vx[0], vy[0], vx[1], vy[1], vx[2], vy[2])
    if A2 == 0 or (cull == 1 and A2 > 0) or (cull == 2 and A2 < 0):
        return None
    s = -1 if A2 < 0 else 1
    edges = []
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        dx, dy = s * (vx[b] - vx[a]), s * (vy[b] - vy[a])
        edges.append((vx[a], vy[a], dx, dy, dy < 0 or (dy == 0 and dx > 0)))
    return s, s * A2, edges, (vx, vy)


def edge_values(edges, px, py):
    """e_k at the pixels (px, py) (int64 arrays of pixel numbers): P = (256 px, 256 py)."""
    Px, Py = 256 * px.astype(np.int64), 256 * py.astype(np.int64)
    return [dx * (Py - ay) - dy * (Px - ax) for ax, ay, dx, dy, _ in edges]


def depth_weights(e, a2, zs, dtype):
    """(w_k, depth) of Depth."""
    T = dtype
    with np.errstate(all="ignore"):
        w = [(ek.astype(T) / T(a2)) / T(zk) for ek, zk in zip(e, zs)]
        return w, T(1) / ((w[0] + w[1]) + w[2])


def coverage(X, Y, z, tri, H, W, cull=0):
    """(py, px) int64 arrays of the pixels triangle ``tri`` covers, and its set-up (None, None when it is not drawn)."""
    st = setup(X, Y, z, tri, cull)
    if st is None:
        return None, None
    _, _, edges, (vx, vy) = st
    x0, x1 = max(0, -(-min(vx) // 256)), min(W - 1, max(vx) // 256)
    y0, y1 = max(0, -(-min(vy) // 256)), min(H - 1, max(vy) // 256)
    if x0 > x1 or y0 > y1:
        return (np.zeros(0, np.int64), np.zeros(0, np.int64)), st
    py, px = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
    e = edge_values(edges, px, py)
    inside = np.ones(px.shape, bool)
    for ek, (_, _, _, _, top_left) in zip(e, edges):
        inside &= (ek > 0) | ((ek == 0) & top_left)
    return (py[inside], px[inside]), st


def raster(H, W, cull, X, Y, z, tris, dtype=np.float64):
    """(tri int32 [H,W], depth dtype [H,W]): Coverage, Depth, Visibility.  Triangles in increasing number with a strict comparison: ties go to
    the smaller number."""
    tri_out = np.full((H, W), -1, np.int32)
    depth_out = np.zeros((H, W), dtype)
    zf = np.asarray(z, np.float32)
    for t, tri in enumerate(np.asarray(tris).reshape(-1, 3)):
        pix, st = coverage(X, Y, zf, tri, H, W, cull)
        if st is None or len(pix[0]) == 0:
            continue
        _, a2, edges, _ = st
        py, px = pix
        _, d = depth_weights(edge_values(edges, px, py), a2, [zf[int(i)] for i in tri], dtype)
        better = (tri_out[py, px] < 0) | (d < depth_out[py, px])
        tri_out[py[better], px[better]] = t
        depth_out[py[better], px[better]] = d[better]
    return tri_out, depth_out


def tri_depth_at(X, Y, z, tris, t, py, px, dtype=np.float64):
    """(covered, depth) of triangle ``t`` at ONE pixel."""
    st = setup(X, Y, np.asarray(z, np.float32), np.asarray(tris).reshape(-1, 3)[t], 0)
    if st is None:
        return False, None
    _, a2, edges, _ = st
    e = edge_values(edges, np.array([px]), np.array([py]))
    cov = all((ek[0] > 0) or (ek[0] == 0 and ed[4]) for ek, ed in zip(e, edges))
    _, d = depth_weights(e, a2, [np.asarray(z, np.float32)[int(i)] for i in np.asarray(tris).reshape(-1, 3)[t]], dtype)
    return cov, d[0]


def shade(H, W, X, Y, z, tris, tri_in, colors, normals, bg, dtype=np.float64):
    """dict(rgb, disp, acc, depth, normal) of Shade from the winners ``tri_in`` [H,W]."""
    T = dtype
    tris = np.asarray(tris).reshape(-1, 3)
    zf = np.asarray(z, np.float32)
    out = dict(rgb=np.broadcast_to(np.asarray(bg, np.float32).astype(T), (H, W, 3)).copy(), disp=np.zeros((H, W), T), acc=np.zeros((H, W), T),
               depth=np.zeros((H, W), T), normal=np.zeros((H, W, 3), T))
    col = None if colors is None else np.asarray(colors, np.float32).astype(T)
    nrm = None if normals is None else np.asarray(normals, np.float32).astype(T)
    for t in np.unique(tri_in):
        if t < 0 or t >= len(tris):
            continue
        st = setup(X, Y, zf, tris[t], 0)
        if st is None:
            continue
        _, a2, edges, _ = st
        py, px = np.nonzero(tri_in == t)
        w, d = depth_weights(edge_values(edges, px, py), a2, [zf[int(i)] for i in tris[t]], T)
        out["depth"][py, px], out["acc"][py, px] = d, T(1)
        with np.errstate(all="ignore"):
            out["disp"][py, px] = T(1) / d
            if col is not None:
                for ch in range(3):
                    c = ((w[0] * col[tris[t][0], ch] + w[1] * col[tris[t][1], ch]) + w[2] * col[tris[t][2], ch]) * d
                    out["rgb"][py, px, ch] = np.where(c < 0, T(0), np.where(c > 1, T(1), c))          # a NaN stays a NaN
            if nrm is not None:
                n = [((w[0] * nrm[tris[t][0], ch] + w[1] * nrm[tris[t][1], ch]) + w[2] * nrm[tris[t][2], ch]) * d for ch in range(3)]
                ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
                ok = (ln > 0) & np.isfinite(ln)
                for ch in range(3):
                    out["normal"][py, px, ch] = np.where(ok, n[ch] / np.where(ok, ln, T(1)), T(0))
    return out


# ---------------------------------------------------------------------------------------------------
# scenes shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------
def uv_sphere(n_lat, n_lon, r, centre):
    """A latitude / longitude sphere wound outwards: (verts float32 [V,3], tris int32 [T,3])."""
    verts = [(0.0, r, 0.0)]
    for a in range(1, n_lat):
        th = np.pi * a / n_lat
        for b in range(n_lon):
            ph = 2 * np.pi * b / n_lon
            verts.append((r * np.sin(th) * np.sin(ph), r * np.cos(th), r * np.sin(th) * np.cos(ph)))
    verts.append((0.0, -r, 0.0))
    ring = lambda a, b: 1 + (a - 1) * n_lon + b % n_lon
    tris = []
    for b in range(n_lon):
        tris.append((0, ring(1, b), ring(1, b + 1)))
        tris.append((len(verts) - 1, ring(n_lat - 1, b + 1), ring(n_lat - 1, b)))
    for a in range(1, n_lat - 1):
        for b in range(n_lon):
            tris.append((ring(a, b), ring(a + 1, b), ring(a + 1, b + 1)))
            tris.append((ring(a, b), ring(a + 1, b + 1), ring(a, b + 1)))
    return (np.asarray(verts, np.float64) + np.asarray(centre, np.float64)).astype(np.float32), np.asarray(tris, np.int32)


def two_spheres_two_quads():
    """Two interpenetrating spheres (16 x 24, r = 1 at the origin; 12 x 16, r = 0.7 at (0.6, 0.3, 0.2)) and two crossing quads of half-width
    1.3: (verts, tris, colors, normals)."""
    v1, t1 = uv_sphere(16, 24, 1.0, (0, 0, 0))
    v2, t2 = uv_sphere(12, 16, 0.7, (0.6, 0.3, 0.2))
    h = 1.3
    q = np.array([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0], [0, -h, -h], [0, -h, h], [0, h, h], [0, h, -h]], np.float32)
    tq = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    verts = np.concatenate([v1, v2, q]).astype(np.float32)
    tris = np.concatenate([t1, t2 + len(v1), tq + len(v1) + len(v2)]).astype(np.int32)
    rng = np.random.default_rng(7)
    colors = rng.random((len(verts), 3)).astype(np.float32)
    normals = rng.standard_normal((len(verts), 3)).astype(np.float32)
    return verts, tris, colors, normals


SCENE_VIEWS = [(30, -30), (0, 0), (123, 40), (271, 5)]


def scene_camera(view):
    return camera(64, 64, 70.0, 70.0, 31.5, 31.5, look_at(view[0], view[1], 4.0))
