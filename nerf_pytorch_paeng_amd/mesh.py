"""Triangle meshes from a trained NeRF on the device (include/mi_nerf_mesh.h, libmi_nerf_mesh.so).

    f = mesh.density_lattice(model, lo=-1.2, hi=1.2, res=128)          # raw density of the fine network at the 129^3 lattice points
    m = mesh.extract(f, -1.2, 1.2, iso=10.0)                           # marching tetrahedra: welded vertices, int32 triangles, normals
    m.colorize(model).save_ply("scene.ply")

    frame = m.render(mesh.Camera(H, W, K, pose))                       # THE VIEW: rgb, disp, acc, depth, tri of the mesh from a pinhole camera

``extract`` takes a field from anywhere -- a network, ``SolidScene.field`` on the lattice rows, a formula -- and follows THE RULE of the
header: where the surface stays off the lattice boundary the mesh is a closed oriented manifold with normals towards lower density; a
surface that reaches the boundary is left open there.  ``extract`` reads the two counts back once (the one host synchronisation of the
path); everything else queues on the current stream.  There is no fallback: a missing library or a failed call raises ``MiNerfError``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _mesh, ops
from ._lib import MiNerfError, as_f32_dev, dev_ptr, stream_ptr
from ._mesh import Grid

# lattice points handed to the network per slab by density_lattice (scratch: 20 bytes per point)
SLAB_POINTS = 1 << 22
_FAMILIES = ("fp32", "f16s", "bf16")


def _triple(v, cast) -> Tuple:
    if isinstance(v, (int, float)):
        return (cast(v),) * 3
    t = tuple(cast(x) for x in v)
    if len(t) != 3:
        raise MiNerfError(f"expected a scalar or three values (x, y, z), got {v!r}")
    return t


def c_grid(lo, hi, res) -> Grid:
    """mi_mesh_grid of a box: ``lo`` / ``hi`` / ``res`` a scalar or (x, y, z); ``res`` counts cells."""
    return Grid((C.c_float * 3)(*_triple(lo, float)), (C.c_float * 3)(*_triple(hi, float)), (C.c_int32 * 3)(*_triple(res, int)))


def check_precision(precision) -> "ops.Precision":
    """One kernel family evaluates the lattice: "fp32" (default), "f16s" or "bf16", or an ops.Precision naming one of them for both networks."""
    if precision is None:
        precision = "fp32"
    if isinstance(precision, str):
        if precision not in _FAMILIES:
            raise MiNerfError(f"precision {precision!r}: one of {_FAMILIES}")
        precision = ops.precision(**({} if precision == "fp32" else {precision: True}))
    if precision.coarse != precision.fine or precision.fine not in _FAMILIES or precision.points_per_wave != 0:
        raise MiNerfError(f"the density lattice runs fp32, f16s or bf16 (got coarse {precision.coarse}, fine {precision.fine})")
    return precision


def _blob(model_or_packed, network: str, prec: "ops.Precision"):
    from .weights import packed_for
    if network not in ("coarse", "fine"):
        raise MiNerfError(f"network must be 'coarse' or 'fine', got {network!r}")
    packed = packed_for(model_or_packed)
    net, blob_c, blob_f = packed.kernel_blobs(prec)
    return packed.device, net, (blob_f if network == "fine" else blob_c)


def lattice_rows(lo, hi, res, device=None):
    """(rays [P_y P_z, 6], z [P_y P_z, P_x]) of the lattice rows as the header lays them out: what mi_mesh_density evaluates, for fields
    that take rays (``SolidScene.field``).  numpy fp32 on the host, every operation rounded once."""
    f32 = np.float32
    lo, hi, res = _triple(lo, float), _triple(hi, float), _triple(res, int)
    step = [(f32(hi[i]) - f32(lo[i])) / f32(res[i]) for i in range(3)]
    x = [(f32(lo[i]) + (np.arange(res[i] + 1).astype(f32) * step[i]).astype(f32)).astype(f32) for i in range(3)]
    Px, Py, Pz = (r + 1 for r in res)
    rays = np.zeros((Pz, Py, 6), f32)
    rays[..., 0] = f32(lo[0])
    rays[..., 1] = x[1][None, :]
    rays[..., 2] = x[2][:, None]
    rays[..., 3] = 1.0
    z = np.broadcast_to((np.arange(Px).astype(f32) * step[0]).astype(f32), (Pz * Py, Px)).copy()
    rays_t, z_t = torch.from_numpy(rays.reshape(-1, 6)), torch.from_numpy(z)
    return (rays_t, z_t) if device is None else (rays_t.to(device), z_t.to(device))


def density_lattice(model_or_packed, lo, hi, res, network: str = "fine", precision=None, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Raw density (channel 3, before the ReLU) of one network at every lattice point: float [P_z, P_y, P_x] on the model's device
    (mi_mesh_density).  ``precision``: "fp32" (default) | "f16s" | "bf16".  ``scratch``: a uint8 device tensor to run the slabs in (at least
    mi_mesh_density_scratch_bytes; default: room for SLAB_POINTS points per slab)."""
    prec = check_precision(precision)
    dev, net, blob = _blob(model_or_packed, network, prec)
    g = c_grid(lo, hi, res)
    L = _mesh.lib()
    need = int(L.mi_mesh_density_scratch_bytes(C.byref(g)))
    if need == 0:
        raise MiNerfError(f"mi_mesh_density refused: {_mesh.last_error()}")
    Px, Py, Pz = (r + 1 for r in g.res)
    if scratch is None:
        rows = min(Py * Pz, max(1, -(-SLAB_POINTS // Px)))
        scratch = torch.empty(max(need, 768 + rows * (24 + 20 * Px)), dtype=torch.uint8, device=dev)
    f = torch.empty(Pz, Py, Px, dtype=torch.float32, device=dev)
    with ops._guard(dev):
        _mesh.check(L.mi_mesh_density(C.byref(g), C.byref(net), dev_ptr(blob, "packed", torch.uint8, 16), prec.mode, dev_ptr(f, "f"),
                                      dev_ptr(scratch, "scratch", torch.uint8, 256), scratch.numel(), stream_ptr(dev)), "mi_mesh_density")
    return f


class Camera:
    """The pinhole camera of ``make_o_d`` for ``Mesh.render``: ``H`` rows, ``W`` columns, the harness's ``K`` ([[fx, 0, cx], [0, fy, cy], ...]) and a
    camera-to-world ``pose`` [3,4] or [4,4] (a tensor on any device, or host numbers).  The values are read to the host once, here, like
    ops.make_o_d does per call; a pose that lives on a HIP device ties the camera to that device."""

    def __init__(self, H: int, W: int, K, pose):
        k = K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)
        self.device = pose.device if isinstance(pose, torch.Tensor) and pose.is_cuda else None
        p = np.asarray(pose.detach().cpu().numpy() if isinstance(pose, torch.Tensor) else pose, dtype=np.float32)
        if p.shape not in ((3, 4), (4, 4)):
            raise MiNerfError(f"pose must be [3,4] or [4,4], got {list(p.shape)}")
        self.H, self.W = int(H), int(W)
        self.c = _mesh.Camera(self.H, self.W, float(np.float32(k[0][0])), float(np.float32(k[1][1])), float(np.float32(k[0][2])),
                              float(np.float32(k[1][2])), (C.c_float * 12)(*p[:3, :4].reshape(-1).tolist()))


class Frame:
    """What ``Mesh.render`` returns: ``rgb`` [H,W,3], ``disp``, ``acc``, ``depth`` [H,W] float, ``tri`` [H,W] int32 (-1 where nothing is drawn) and
    ``normal`` [H,W,3] or None, all on the mesh's device."""

    def __init__(self, rgb, disp, acc, depth, tri, normal=None):
        self.rgb, self.disp, self.acc, self.depth, self.tri, self.normal = rgb, disp, acc, depth, tri, normal


class Mesh:
    """An indexed triangle mesh on the device: ``verts`` float [V,3], ``tris`` int32 [T,3], ``normals`` float [V,3] or None (unit, towards
    lower density; zero where the field is flat), ``colors`` float [V,3] in [0,1] or None (``colorize``)."""

    def __init__(self, verts: torch.Tensor, tris: torch.Tensor, normals: Optional[torch.Tensor] = None, colors: Optional[torch.Tensor] = None):
        self.verts, self.tris, self.normals, self.colors = verts, tris, normals, colors

    def colorize(self, model_or_packed, network: str = "fine") -> "Mesh":
        """Colour every vertex with the network's answer AT the vertex, seen along minus the normal ((0,0,1) where the normal is zero or
        there are no normals): one ray per vertex with depth 0 through ops.mlp_rays (fp32; one sample is the smallest the fused entry
        takes), then sigmoid of channels 0..2."""
        dev, net, blob = _blob(model_or_packed, network, check_precision(None))
        if self.verts.device != dev:
            raise MiNerfError(f"the mesh lives on {self.verts.device}, the network on {dev}")
        rays, z = self.color_rays()
        if rays.shape[0] == 0:
            self.colors = torch.empty(0, 3, dtype=torch.float32, device=dev)
            return self
        self.colors = torch.sigmoid(ops.mlp_rays(net, blob, rays, z)[:, 0, :3]).contiguous()
        return self

    def color_rays(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(rays [V,6], z [V,1]) that ``colorize`` evaluates."""
        V = self.verts.shape[0]
        d = torch.zeros_like(self.verts)
        d[:, 2] = 1.0
        if self.normals is not None:
            zero = (self.normals == 0).all(-1, keepdim=True)
            d = torch.where(zero, d, -self.normals)
        return torch.cat([self.verts, d], -1).contiguous(), torch.zeros(V, 1, dtype=torch.float32, device=self.verts.device)

    def _corners(self):
        v = self.verts.double()
        t = self.tris.long()
        return v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]

    def area(self) -> float:
        a, b, c = self._corners()
        return float(0.5 * torch.linalg.cross(b - a, c - a).norm(dim=-1).sum())

    def volume(self) -> float:
        """Signed volume by the divergence theorem (fp64): positive for a closed mesh whose normals point outwards."""
        a, b, c = self._corners()
        return float((a * torch.linalg.cross(b, c)).sum() / 6.0)

    def _view_args(self, camera: Camera):
        if not isinstance(camera, Camera):
            raise MiNerfError(f"camera must be a mesh.Camera, got {type(camera).__name__}")
        dev = self.verts.device
        if dev.type != "cuda":
            raise MiNerfError(f"the mesh must live on a HIP device (got {dev}); this path has no CPU fallback")
        if camera.device is not None and camera.device != dev:
            raise MiNerfError(f"the mesh lives on {dev}, the camera's pose on {camera.device}")
        for name, t in (("tris", self.tris), ("colors", self.colors), ("normals", self.normals)):
            if t is not None and t.device != dev:
                raise MiNerfError(f"the mesh's {name} live on {t.device}, its verts on {dev}")
        return dev, int(self.verts.shape[0]), int(self.tris.shape[0])

    def project(self, camera: Camera, near: float = 1e-3) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(X, Y int32 [V], z float [V]) of mi_mesh_project: 24.8 fixed-point screen coordinates and depths; an invalid vertex (behind ``near``,
        not finite, beyond the guard band) is X = Y = INT32_MIN, z = 0."""
        dev, V, _ = self._view_args(camera)
        X = torch.empty(V, dtype=torch.int32, device=dev)
        Y = torch.empty(V, dtype=torch.int32, device=dev)
        z = torch.empty(V, dtype=torch.float32, device=dev)
        with ops._guard(dev):
            _mesh.check(_mesh.lib().mi_mesh_project(C.byref(camera.c), float(near), dev_ptr(as_f32_dev(self.verts), "verts") if V else None, V,
                                                    dev_ptr(X, "X", torch.int32) if V else None, dev_ptr(Y, "Y", torch.int32) if V else None,
                                                    dev_ptr(z, "z") if V else None, stream_ptr(dev)), "mi_mesh_project")
        return X, Y, z

    def render(self, camera: Camera, near: float = 1e-3, cull: int = 0, bg=(1.0, 1.0, 1.0), normals: bool = False) -> "Frame":
        """THE VIEW of include/mi_nerf_mesh.h: project, raster, shade, queued on the current stream without a host synchronisation.  ``cull``: 0 draws
        both windings, 1 drops back faces, 2 front faces (``extract``'s winding is front from outside).  Needs ``colors`` (``colorize``, or any
        [V,3] tensor); ``normals=True`` also shades the per-vertex normals.  A mesh without triangles renders ``bg``."""
        if self.colors is None:
            raise MiNerfError("Mesh.render needs per-vertex colours: call colorize(model) first, or set mesh.colors to a [V,3] tensor")
        if normals and self.normals is None:
            raise MiNerfError("Mesh.render(normals=True) needs per-vertex normals (extract(..., normals=True))")
        dev, V, T = self._view_args(camera)
        if tuple(self.colors.shape) != (V, 3):
            raise MiNerfError(f"colors must be [{V},3], got {list(self.colors.shape)}")
        H, W = camera.H, camera.W
        L = _mesh.lib()
        nbytes = int(L.mi_mesh_raster_scratch_bytes(H, W))
        if nbytes == 0:
            raise MiNerfError(f"mi_mesh_raster refused: {_mesh.last_error()}")
        X, Y, z = self.project(camera, near)
        i32 = lambda t, name: dev_ptr(t, name, torch.int32)
        with ops._guard(dev):
            st = stream_ptr(dev)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            tri = torch.empty(H, W, dtype=torch.int32, device=dev)
            out = {k: torch.empty(H, W, *tail, dtype=torch.float32, device=dev) for k, tail in (("rgb", (3,)), ("disp", ()), ("acc", ()), ("depth", ()))}
            nrm = torch.empty(H, W, 3, dtype=torch.float32, device=dev) if normals else None
            tris = self.tris.contiguous()
            mesh_args = (i32(X, "X") if V else None, i32(Y, "Y") if V else None, dev_ptr(z, "z") if V else None, V, i32(tris, "tris") if T else None, T)
            _mesh.check(L.mi_mesh_raster(H, W, int(cull), 0, *mesh_args, dev_ptr(scratch, "scratch", torch.uint8, 256), nbytes, i32(tri, "tri"), None, st),
                        "mi_mesh_raster")
            _mesh.check(L.mi_mesh_shade(H, W, *mesh_args, i32(tri, "tri"), dev_ptr(as_f32_dev(self.colors), "colors") if V else None,
                                        dev_ptr(as_f32_dev(self.normals), "normals") if (normals and V) else None, (C.c_float * 3)(*(float(b) for b in bg)),
                                        dev_ptr(out["rgb"]), dev_ptr(out["disp"]), dev_ptr(out["acc"]), dev_ptr(out["depth"]), dev_ptr(nrm), st), "mi_mesh_shade")
        return Frame(out["rgb"], out["disp"], out["acc"], out["depth"], tri, nrm)

    def save_ply(self, path: str) -> None:
        """Binary little-endian PLY: positions, normals when present, uchar colours when present, triangles as uchar-counted int lists."""
        write_ply(path, self.verts.cpu().numpy(), self.tris.cpu().numpy(), None if self.normals is None else self.normals.cpu().numpy(),
                  None if self.colors is None else self.colors.cpu().numpy())


def write_ply(path: str, verts, tris, normals=None, colors=None) -> None:
    """Pure numpy, in the spirit of harness.write_png.  ``colors`` in [0,1] are stored as round(255 c)."""
    verts, tris = np.asarray(verts, "<f4").reshape(-1, 3), np.asarray(tris, "<i4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vert = np.zeros(len(verts), np.dtype(fields))
    for i, k in enumerate("xyz"):
        vert[k] = verts[:, i]
    if normals is not None:
        for i, k in enumerate(("nx", "ny", "nz")):
            vert[k] = np.asarray(normals, "<f4").reshape(-1, 3)[:, i]
    if colors is not None:
        c8 = np.clip(np.rint(np.asarray(colors, np.float64).reshape(-1, 3) * 255.0), 0, 255).astype(np.uint8)
        for i, k in enumerate(("red", "green", "blue")):
            vert[k] = c8[:, i]
    face = np.zeros(len(tris), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    face["n"] = 3
    face["v"] = tris
    names = {"<f4": "float", "u1": "uchar"}
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(verts)}"]
    head += [f"property {names[t]} {k}" for k, t in fields]
    head += [f"element face {len(tris)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())


def extract(field: torch.Tensor, lo, hi, iso: float, normals: bool = True) -> Mesh:
    """Marching tetrahedra over ``field`` [P_z, P_y, P_x] (a device tensor; res = P - 1 cells per axis) in the box lo..hi at level ``iso``:
    mi_mesh_count, ONE read-back of the two counts, mi_mesh_emit."""
    if not isinstance(field, torch.Tensor) or field.dim() != 3:
        raise MiNerfError("field must be a [P_z, P_y, P_x] tensor")
    field = as_f32_dev(field)
    dev = field.device
    Pz, Py, Px = field.shape
    g = c_grid(lo, hi, (Px - 1, Py - 1, Pz - 1))
    L = _mesh.lib()
    nbytes = int(L.mi_mesh_extract_scratch_bytes(C.byref(g)))
    if nbytes == 0:
        raise MiNerfError(f"mi_mesh_count refused: {_mesh.last_error()}")
    with ops._guard(dev):
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        st = stream_ptr(dev)
        _mesh.check(L.mi_mesh_count(C.byref(g), dev_ptr(field, "field"), float(iso), dev_ptr(scratch, "scratch", torch.uint8, 256), nbytes,
                                    dev_ptr(counts, "counts", torch.int64, 8), st), "mi_mesh_count")
        V, T = (int(c) for c in counts.tolist())                        # the one read-back: synchronises the current stream
        verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
        tris = torch.empty(T, 3, dtype=torch.int32, device=dev)
        nrm = torch.empty(V, 3, dtype=torch.float32, device=dev) if normals else None
        _mesh.check(L.mi_mesh_emit(C.byref(g), dev_ptr(field, "field"), float(iso), dev_ptr(scratch, "scratch", torch.uint8, 256), nbytes, V, T,
                                   dev_ptr(verts, "verts") if V else None, dev_ptr(tris, "tris", torch.int32) if T else None,
                                   dev_ptr(nrm, "normals") if (normals and V) else None, st), "mi_mesh_emit")
    return Mesh(verts, tris, nrm)
