"""Mesh extraction, measured: the three entries of include/mi_nerf_mesh.h timed one by one, and a trained scene's mesh held against the
solids it was trained on.

    python tools/mesh_probe.py [--res 128 256] [--reps 5] [--out profiles/r11_mesh.txt]
    python tools/mesh_probe.py --scene solid [--steps 1500] [--iso 10] [--out profiles/r11_mesh.txt]      (appends to the report)

Without ``--scene``: a synthetic 8 x 256 network (synthetic.make_state_dict), lattice of the box +-1.5; per resolution the device time
(HIP events, median of ``--reps`` after a warm-up) of mi_mesh_density (fp32), mi_mesh_count and mi_mesh_emit (with normals), the lattice
points per second of the first and the HBM bytes the other two move at the least, with the rate that makes.  The level is the median of
the lattice's density, so about half the points are inside: far more surface than a scene has, a hard case for count and emit.

``--scene solid``: scenes.SolidScene.default() trained as examples/train_eval_render.py trains it (tools/occ_probe.train_scene), the fine
network's lattice at ``--res`` over the box +-1.25, the mesh at ``--iso``; reports the share of the vertices that lie within one cell
diagonal of a primitive's surface (reported, not asserted), the counts, the area and the enclosed volume.
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nerf_pytorch_paeng_amd import mesh, scenes, synthetic, weights                            # noqa: E402
from nerf_pytorch_paeng_amd import _mesh                                                       # noqa: E402
from nerf_pytorch_paeng_amd._lib import dev_ptr, stream_ptr                                    # noqa: E402
from nerf_pytorch_paeng_amd._scene import BOX, CYLINDER, SPHERE                                # noqa: E402

import ctypes as C                                                                             # noqa: E402


def device_ms(fn, reps):
    """Median device time of fn() in ms over ``reps`` runs after one warm-up."""
    fn()
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return float(np.median(times))


def time_entries(packed, res, reps, box=1.5):
    dev = packed.device
    g = mesh.c_grid(-box, box, res)
    L = _mesh.lib()
    P = res + 1
    N, Cn = P ** 3, res ** 3
    field = [None]

    def density():
        field[0] = mesh.density_lattice(packed, -box, box, res)
    t_density = device_ms(density, reps)
    f = field[0]
    iso = float(f.flatten()[:: max(1, N // 100000)].median())
    nbytes = int(L.mi_mesh_extract_scratch_bytes(C.byref(g)))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    st = stream_ptr(dev)
    sp = dev_ptr(scratch, "scratch", torch.uint8, 256)

    def count():
        _mesh.check(L.mi_mesh_count(C.byref(g), dev_ptr(f), iso, sp, nbytes, dev_ptr(counts, "counts", torch.int64, 8), st), "mi_mesh_count")
    t_count = device_ms(count, reps)
    V, T = (int(c) for c in counts.tolist())
    verts = torch.empty(V, 3, device=dev)
    nrm = torch.empty(V, 3, device=dev)
    tris = torch.empty(T, 3, dtype=torch.int32, device=dev)

    def emit():
        _mesh.check(L.mi_mesh_emit(C.byref(g), dev_ptr(f), iso, sp, nbytes, V, T, dev_ptr(verts), dev_ptr(tris, "tris", torch.int32), dev_ptr(nrm), st), "mi_mesh_emit")
    t_emit = device_ms(emit, reps)
    # the least each pass moves: count reads f twice (points, cells) and writes mask + counts, then each prefix sum reads twice and writes once;
    # emit reads f, mask and the two prefix arrays once and writes the mesh
    b_count = 4 * N + N + 4 * N + 3 * 4 * N + 4 * N + 4 * Cn + 3 * 4 * Cn
    b_emit = 2 * (4 * N) + N + 4 * N + 4 * Cn + 24 * V + 12 * T
    return [
        f"res {res}^3 ({N} points, {Cn} cells), level {iso:.4g} (the lattice's median): {V} vertices, {T} triangles",
        f"  mi_mesh_density fp32 {t_density:9.3f} ms   {N / t_density / 1e3:8.1f} M points/s",
        f"  mi_mesh_count        {t_count:9.3f} ms   {b_count / 1e6:8.1f} MB at the least -> {b_count / t_count / 1e6:7.1f} GB/s",
        f"  mi_mesh_emit         {t_emit:9.3f} ms   {b_emit / 1e6:8.1f} MB at the least -> {b_emit / t_emit / 1e6:7.1f} GB/s",
    ]


def surface_distance(prims, p):
    """[n]: distance of the points p [n,3] (fp64) from the nearest primitive's surface (exact signed-distance forms of the three kinds)."""
    best = torch.full((p.shape[0],), float("inf"), dtype=torch.float64, device=p.device)
    for pr in prims:
        q = p - torch.tensor(list(pr.c), dtype=torch.float64, device=p.device)
        if pr.kind == SPHERE:
            d = q.norm(dim=-1) - pr.h[0]
        elif pr.kind == BOX:
            a = q.abs() - torch.tensor(list(pr.h), dtype=torch.float64, device=p.device)
            d = a.clamp_min(0).norm(dim=-1) + a.max(-1)[0].clamp_max(0)
        elif pr.kind == CYLINDER:
            ax = pr.axis
            others = [i for i in range(3) if i != ax]
            a = torch.stack([q[:, others].norm(dim=-1) - pr.h[0], q[:, ax].abs() - pr.h[1]], -1)
            d = a.clamp_min(0).norm(dim=-1) + a.max(-1)[0].clamp_max(0)
        else:
            raise ValueError(pr.kind)
        best = torch.minimum(best, d.abs())
    return best


def main_solid(a):
    from occ_probe import train_scene
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    packed, _ = train_scene(dev, a.steps, a.size, a.views, "solid")
    scene = scenes.SolidScene.default()
    lines = ["", f"trained scene: scenes.SolidScene.default(), {a.views} views {a.size} x {a.size}, {a.steps} training steps, fp32; fine network, box +-{a.box:g}, level {a.iso:g}"]
    for res in a.res:
        with torch.no_grad():
            m = mesh.extract(mesh.density_lattice(packed, -a.box, a.box, res), -a.box, a.box, a.iso)
        diag = math.sqrt(3.0) * 2.0 * a.box / res
        d = surface_distance(scene.prims, m.verts.double())
        lines.append(f"res {res}^3: {m.verts.shape[0]} vertices, {m.tris.shape[0]} triangles, area {m.area():.3f}, enclosed volume {m.volume():.4f}; "
                     f"within one cell diagonal ({diag:.4f}) of a primitive's surface: {float((d <= diag).double().mean()):.4f} of the vertices "
                     f"(median distance {float(d.median()):.4f}, 95th percentile {float(d.quantile(0.95)):.4f})")
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "r11_mesh.txt"))
    ap.add_argument("--scene", default=None, choices=["solid"])
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--iso", type=float, default=10.0)
    ap.add_argument("--box", type=float, default=1.25)
    ap.add_argument("--size", type=int, default=48)
    ap.add_argument("--views", type=int, default=12)
    a = ap.parse_args(argv)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.scene == "solid":
        lines = main_solid(a)
        mode = "a"
    else:
        dev = torch.device("cuda:0")
        packed = weights.PackedNeRF.from_state_dict(synthetic.make_state_dict(0, 8, 256), dev)
        lines = [f"mesh probe: synthetic 8 x 256 network, lattice of the box +-1.5, device time (HIP events), median of {a.reps} after a warm-up"]
        for res in a.res:
            lines += time_entries(packed, res, a.reps)
        mode = "w"
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, mode) as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
