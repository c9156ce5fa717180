"""Device time of mi_iqa_ssim and what SSIM adds to harness.test (profiles/r08_iqa_ssim.txt).

    python tools/iqa_probe.py            one MI355X; prints the lines of the profile file

hipEvents around each of 20 launches after 3 warm-up launches, median; bytes the kernel must read = 2 * N * H * W * 12."""
import os
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_pytorch_paeng_amd import harness, ops, synthetic                      # noqa: E402
from nerf_pytorch_paeng_amd import nerf_process as NP                            # noqa: E402
from nerf_pytorch_paeng_amd.model import NeRF, get_positional_encoder            # noqa: E402

DEV = torch.device("cuda:0")
STREAM_TBS = 6.0                                                                 # rays_rgb_kernel, the project's streaming kernels


def time_ssim(n, H, W, **kw):
    g = torch.Generator().manual_seed(n)
    pred, target = torch.rand(n, H, W, 3, generator=g).to(DEV), torch.rand(n, H, W, 3, generator=g).to(DEV)
    for _ in range(3):
        ops.ssim(pred, target, **kw)
    ms = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.ssim(pred, target, **kw)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    med = statistics.median(ms)
    gbs = 2 * n * H * W * 12 / (med * 1e-3) / 1e9
    print(f"mi_iqa_ssim {n:3d} x {H}x{W} {str(kw or ''):24s}: median {med * 1e3:9.1f} us (min {min(ms) * 1e3:.1f}, max {max(ms) * 1e3:.1f})  "
          f"{gbs:8.1f} GB/s of required reads = {gbs / (STREAM_TBS * 1e3) * 100:5.1f} % of {STREAM_TBS} TB/s")


def time_harness():
    D, Wd, Hs, Ws = 4, 128, 20, 24
    model = NeRF(D, Wd, 63, 27).to(DEV)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in synthetic.make_state_dict(13, D, Wd).items()})
    posenc = get_positional_encoder(10), get_positional_encoder(4)
    K = np.array([[30.0, 0, Ws / 2], [0, 30.0, Hs / 2], [0, 0, 1]])
    poses = harness.get_render_pose(n_angle=3, phi=-30.0, nf=4.0).to(DEV)
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=32, N_samples_f=32, perturb=0.0, chunk_rays=4096, chunk_pts=524288,
                           data_type="blender", gpu_ids=[0], rank=0, exp_name="probe", n_angle=3, single_angle=-1, phi=-30.0, nf=4.0)
    gt = torch.rand(3, Hs, Ws, 3, generator=torch.Generator().manual_seed(4)).to(DEV)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(13):                                                    # alternating, 3 warm-up rounds
            for flag in (False, True):
                NP.manual_seed(7)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                harness.test(0, [0, 1, 2], posenc, model, gt, K, poses, (Hs, Ws), opts, save_dir=os.path.join(tmp, str(flag)), ssim=flag)
                torch.cuda.synchronize()
                if rep >= 3:
                    out.setdefault(flag, []).append((time.perf_counter() - t0) * 1e3)
    a, b = statistics.median(out[False]), statistics.median(out[True])
    print(f"harness.test, 3 poses of 20x24, frames and _result.txt written: median of 10 alternating runs  {a:.2f} ms without, {b:.2f} ms with ssim=True "
          f"(+{(b - a) / 3 * 1e3:.0f} us per frame; spread of the runs without: {min(out[False]):.2f} .. {max(out[False]):.2f} ms)")


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0))
    time_ssim(1, 800, 800)
    time_ssim(40, 800, 800)
    time_ssim(40, 800, 800, return_map=True)
    time_ssim(40, 800, 800, downsample=0)
    time_ssim(40, 378, 504)
    time_harness()
