"""THE VIEW of include/mi_nerf_mesh.h, measured: an 800 x 800 frame of an extracted mesh, stage by stage, next to the radiance grid's and the
fp32 network's frame of the same camera.

    python tools/mesh_view_probe.py [--res 16 128 256] [--reps 7] [--boxes 16 32 256] [--out profiles/r19_mesh_view.txt]

One process.  The scene is scenes.SolidScene.default() on the box +-1.2: its density on the lattice rows (``scene.field``), the mesh at half
the smallest density above 0 (the 16^3 lattice is there for the size classes: its triangles span some forty pixels, the others' a few), every vertex coloured by the field half a cell behind it (along minus its normal).  The frame is the lego
camera at azimuth 30, elevation -30, radius 4 (the view of docs/design/22_radiance_grid.md 22.7).  Per lattice and per value of large_box
(MI_MESH_VIEW_LARGE_BOX is the one the library ships): device time (HIP events) of mi_mesh_project, mi_mesh_raster and mi_mesh_shade, each the
median of ``--reps`` interleaved repetitions after a warm-up; the counters of the raster's scratch (large triangles met, triangles walked by a
lane, atomic updates issued); covered pixels; the PSNR of the frame against ``SolidScene.render`` of the same rays.  In the same loop: the
``opts.baked`` frame (256^3, B = 1, skipping on; device time) and the fp32 network frame (8 x 256, 64 + 128 samples; host clock around a
synchronise, as tools/vox_probe.py times it).
"""
import argparse
import ctypes as C
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pytorch_paeng_amd import _mesh, baked, mesh, scenes, synthetic, weights              # noqa: E402
from nerf_pytorch_paeng_amd import nerf_process as NP                                          # noqa: E402
from nerf_pytorch_paeng_amd._lib import dev_ptr, stream_ptr                                    # noqa: E402
from nerf_pytorch_paeng_amd.rays import make_o_d                                               # noqa: E402

BOX = 1.2


def scene_mesh(scene, res, dev):
    rays, z = mesh.lattice_rows(-BOX, BOX, res, dev)
    f = scene.field(rays, z)[..., 3].reshape(res + 1, res + 1, res + 1).contiguous()
    iso = 0.5 * float(f[f > 0].min())
    m = mesh.extract(f, -BOX, BOX, iso)
    inside = (m.verts - m.normals * (BOX / res)).contiguous()                        # half a cell behind the surface
    probe = torch.cat([inside, torch.zeros_like(inside)], -1)
    probe[:, 5] = 1.0
    m.colors = torch.sigmoid(scene.field(probe, torch.zeros(len(inside), 1, device=dev))[:, 0, :3]).contiguous()
    return m, iso


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1), out


class Stages:
    """The three entries on preallocated buffers, so that a repetition times the kernels and nothing else."""

    def __init__(self, m, cam, H, W):
        self.m, self.cam, self.H, self.W = m, cam, H, W
        dev = m.verts.device
        self.V, self.T = m.verts.shape[0], m.tris.shape[0]
        self.X, self.Y = (torch.empty(self.V, dtype=torch.int32, device=dev) for _ in range(2))
        self.z = torch.empty(self.V, device=dev)
        self.nbytes = int(_mesh.lib().mi_mesh_raster_scratch_bytes(H, W))
        self.scratch = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.tri = torch.empty(H, W, dtype=torch.int32, device=dev)
        self.rgb = torch.empty(H, W, 3, device=dev)
        self.disp, self.acc, self.depth = (torch.empty(H, W, device=dev) for _ in range(3))
        self.st = stream_ptr(dev)
        i32 = lambda t: dev_ptr(t, "t", torch.int32)
        self.mesh_args = (i32(self.X), i32(self.Y), dev_ptr(self.z), self.V, i32(m.tris), self.T)

    def project(self):
        _mesh.check(_mesh.lib().mi_mesh_project(C.byref(self.cam.c), 1e-3, dev_ptr(self.m.verts), self.V, *self.mesh_args[:3], self.st), "mi_mesh_project")

    def raster(self, box):
        _mesh.check(_mesh.lib().mi_mesh_raster(self.H, self.W, 0, box, *self.mesh_args, dev_ptr(self.scratch, "s", torch.uint8, 256), self.nbytes,
                                               dev_ptr(self.tri, "tri", torch.int32), None, self.st), "mi_mesh_raster")

    def shade(self):
        _mesh.check(_mesh.lib().mi_mesh_shade(self.H, self.W, *self.mesh_args, dev_ptr(self.tri, "tri", torch.int32), dev_ptr(self.m.colors), None,
                                              (C.c_float * 3)(1.0, 1.0, 1.0), dev_ptr(self.rgb), dev_ptr(self.disp), dev_ptr(self.acc), dev_ptr(self.depth), None,
                                              self.st), "mi_mesh_shade")

    def counters(self):
        off = (8 * self.H * self.W + 255) & ~255
        c = self.scratch[off:off + 24].cpu().numpy().view(np.uint32)
        return int(c[0]), int(c[1]), int(c[2]) | int(c[3]) << 32, int(c[4]) | int(c[5]) << 32


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[16, 128, 256])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--boxes", type=int, nargs="+", default=[16, 32, 256])
    ap.add_argument("--out", default=os.path.join("profiles", "r19_mesh_view.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    scene = scenes.SolidScene.default()
    K, H, W = synthetic.lego_camera()
    pose = torch.from_numpy(np.asarray(synthetic.pose_spherical(30.0, -30.0, 4.0), dtype=np.float32)).to(dev)
    o, d = make_o_d(W, H, K, pose[:3, :4])
    rays = torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1).contiguous()
    truth = scene.render(rays, 2.0, 6.0, want_all=False)
    cam = mesh.Camera(H, W, K, pose)
    lines = [f"mesh view probe: scenes.SolidScene.default() on the box +-{BOX:g}; frame {H} x {W}, azimuth 30, elevation -30, radius 4; device time (HIP events), "
             f"medians of {a.reps} interleaved repetitions after a warm-up; MI_MESH_VIEW_LARGE_BOX = {_mesh.VIEW_LARGE_BOX}"]
    stages = {}
    for res in a.res:
        m, iso = scene_mesh(scene, res, dev)
        stages[res] = Stages(m, cam, H, W)
        lines.append(f"lattice {res}^3, level {iso:g}: {m.verts.shape[0]} vertices, {m.tris.shape[0]} triangles")
    grid = baked.bake_field(scene.field, -BOX, BOX, 256, B=1, D=32, device=dev)
    packed = weights.PackedNeRF.from_state_dict(synthetic.make_state_dict(0, 8, 256), dev)
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=64, N_samples_f=128, perturb=1.0, chunk_rays=4096, chunk_pts=524288, data_type="blender", gpu_ids=[0],
                           rank=0, precision="fp32")
    variants = [(res, box) for res in a.res for box in a.boxes]
    t = {k: [] for k in [("project", res) for res in a.res] + [("shade", res) for res in a.res] + [("raster",) + v for v in variants] + ["baked", "network"]}
    stats = {}
    with torch.no_grad():
        for rep in range(a.reps + 1):                                 # the first pass warms up
            stages[a.res[0]].project()                                # untimed: the first launch after the network frame's synchronise pays for the idle device
            for res in a.res:
                s = stages[res]
                ms, _ = timed(s.project)
                t[("project", res)].append(ms)
                for box in a.boxes:
                    ms, _ = timed(lambda: s.raster(box))
                    t[("raster", res, box)].append(ms)
                    if not rep:
                        stats[(res, box)] = s.counters() + (int((s.tri >= 0).sum()),)
                s.raster(0)
                ms, _ = timed(s.shade)
                t[("shade", res)].append(ms)
                if not rep:
                    stats[res] = float(-10.0 * torch.log10(torch.mean((s.rgb.reshape(-1, 3) - truth) ** 2)))
            ms, rgb_b = timed(lambda: grid.render(rays, skip=True)[0])
            t["baked"].append(ms)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            NP.batchify_rays_and_render_by_chunk(o, d, packed, None, H, W, K, opts, seed=5)
            torch.cuda.synchronize()
            t["network"].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v[1:])) for k, v in t.items()}
    psnr_b = float(-10.0 * torch.log10(torch.mean((rgb_b - truth) ** 2)))
    lines.append(f"network frame (fp32, 8 x 256, 64 + 128 samples, host clock around a synchronise): {med['network']:9.1f} ms")
    lines.append(f"opts.baked frame (256^3, B = 1, skipping on, T_min 0): {med['baked']:9.3f} ms, PSNR to SolidScene.render {psnr_b:.3f} dB")
    lines.append("  res  large_box   project ms   raster ms    shade ms     frame ms   large triangles   by a lane   atomic updates   that lowered   covered pixels   PSNR to SolidScene.render")
    for res, box in variants:
        met, lane, atom, won, cov = stats[(res, box)]
        frame = med[("project", res)] + med[("raster", res, box)] + med[("shade", res)]
        lines.append(f"  {res:3d}  {box:9d}   {med[('project', res)]:10.4f}  {med[('raster', res, box)]:10.4f}  {med[('shade', res)]:10.4f}   {frame:10.4f}   {met:15d}   {lane:9d}   "
                     f"{atom:14d}   {won:12d}   {cov:14d}   {stats[res]:8.3f} dB")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
