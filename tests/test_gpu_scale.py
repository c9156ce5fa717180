"""Full-size frames and the 8-GPU geometry on one GPU.

BASELINE config #3 is "lego full 800x800 test render, ray batches sharded over 8 GPUs, RCCL tile gather"; config #4's frame is the
378x504 fern frame through the NDC warp.  What a one-GPU box can establish about them:

* the full-size frame as `dist.render_frame` renders it (one slab of 640 000 rays) agrees bit for bit with `render_rays` on a random
  subset of its pixels (jitter keyed on the GLOBAL ray index) and, on a smaller subset, with the CPU oracle within the bars of
  `test_config2_all_rays_vs_oracle` (reference caller: test.py:36-53);
* the 8 row blocks of `shard_rows(H, 8, r)` rendered one after the other and assembled like `gather_tiles` does are bit-identical
  to the one-rank frame (800 rows: 8 x 100; 378 rows: 48, 48, 47 x 6);
* `bench.py` runs end to end as a multi-rank job: 4 live ranks over gloo sharing the GPU, and rank r of 8 alone (BENCH_SOLO_RANK).
  The GPU pool admits at most 6 processes on a card at once (this pytest process is one of them), so 8 LIVE ranks on a one-GPU box
  are not possible; the 8-rank collective path itself is covered on CPU (tests/test_dist_cpu.py, gloo, world size 8).
"""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import dist as mdist
from nerf_pytorch_paeng_amd import nerf_process as NP
from nerf_pytorch_paeng_amd import ops, synthetic, weights
from oracle import restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SC, NF = 64, 128


def _scene(workload):
    fern = workload == "fern"
    K, H, W = synthetic.fern_camera() if fern else synthetic.lego_camera()
    pose = synthetic.fern_pose() if fern else synthetic.pose_spherical(3.0, -30.0, 4.0)
    opts = SimpleNamespace(near=0.0 if fern else 2.0, far=1.0 if fern else 6.0, N_samples_c=SC, N_samples_f=NF, perturb=1.0, chunk_rays=4096,
                           chunk_pts=524288, data_type="llff" if fern else "blender", gpu_ids=[0], rank=0)
    return K, H, W, pose, opts


@pytest.fixture(scope="module")
def sd():
    return synthetic.make_state_dict(0, 8, 256)


@pytest.fixture(scope="module")
def packed(sd):
    return weights.PackedNeRF.from_state_dict(sd, DEV)


@pytest.fixture(scope="module")
def frames(packed):
    """The one-rank full-size frames (rgb [H,W,3], disp [H,W]) of both workloads, rendered once per module."""
    out = {}
    for wl in ("lego", "fern"):
        K, H, W, pose, opts = _scene(wl)
        out[wl] = mdist.render_frame(H, W, K, pose, packed, opts, seed=7)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("workload", ["lego", "fern"])
def test_full_size_frame_pixels_match_render_rays_and_oracle(workload, packed, sd, frames):
    K, H, W, pose, opts = _scene(workload)
    rgb, disp = frames[workload]
    assert rgb.shape == (H, W, 3) and disp.shape == (H, W) and torch.isfinite(rgb).all() and torch.isfinite(disp).all()
    n_pix = 4096
    pix = torch.from_numpy(np.sort(np.random.RandomState(5).choice(H * W, n_pix, replace=False))).to(DEV)
    o_all, d_all = ops.make_o_d(W, H, K, pose, DEV)
    o, d = o_all.reshape(-1, 3)[pix].contiguous(), d_all.reshape(-1, 3)[pix].contiguous()
    op, dp = ops.make_o_d_pixels(W, H, K, pose, pix)                       # the per-pixel generator is the same function of the pixel
    assert torch.equal(op, o) and torch.equal(dp, d)
    # the frame's jitter for these pixels: generator keyed on (seed, global ray index = pixel index, sample)
    t_rand = ops.fill_uniform(7, 0, 0, H * W, SC, DEV)[pix].contiguous()
    u = ops.fill_uniform(7, 1, 0, H * W, NF, DEV)[pix].contiguous()
    rc, dc, rf, df = NP.batchify_rays_and_render_by_chunk(o, d, packed, None, H, W, K, opts, t_rand=t_rand, u=u)
    assert torch.equal(rf, rgb.reshape(-1, 3)[pix]) and torch.equal(df, disp.reshape(-1)[pix])        # bit-identical, any batch shape
    # ray_offset form for a contiguous run of pixels (what a shard passes): rows 300..301 of the frame
    r0 = min(300, H - 2)
    run = slice(r0 * W, (r0 + 2) * W)
    got = NP.batchify_rays_and_render_by_chunk(o_all.reshape(-1, 3)[run], d_all.reshape(-1, 3)[run], packed, None, H, W, K, opts, seed=7,
                                               ray_offset=r0 * W)
    assert torch.equal(got[2], rgb.reshape(-1, 3)[run]) and torch.equal(got[3], disp.reshape(-1)[run])
    # 256 of the pixels against the CPU oracle: coarse directly, fine with the depths pinned to the ones the HIP path sampled
    m = 256
    rays_m = torch.cat([o[:m], d[:m]], -1)
    if workload == "fern":
        on, dn = ops.ndc_rays(H, W, float(K[0][0]), 1.0, o[:m].contiguous(), d[:m].contiguous())
        rays_m = torch.cat([on, dn], -1)
    hip = NP.render_rays(rays_m.contiguous(), packed, None, opts, t_rand=t_rand[:m], u=u[:m], return_intermediates=True)
    assert torch.equal(hip["rgb_f"], rf[:m])
    cfg = R.PathConfig(near=opts.near, far=opts.far, data_type=opts.data_type)
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    with torch.no_grad():
        ref = R.batchify_rays_and_render_by_chunk(o[:m].cpu(), d[:m].cpu(), sd, H, W, K, cfg, t_rand[:m].cpu(), u[:m].cpu())
        rays_ref = rays_m.cpu()              # the pinned pass takes the HIP path's rays AND depths: what is left is the network + composite
        pin = R.render_rays(rays_ref, sd, cfg, t_rand[:m].cpu(), u[:m].cpu(), z_fine_override=hip["_z_f"].cpu())
    e_c = float((rc[:m].cpu() - ref[0]).abs().max())
    e_f = float((rf[:m].cpu() - pin["rgb_f"]).abs().max())
    bad = float(((rf[:m].cpu() - ref[2]).abs().max(-1)[0] > 1e-4).float().mean())
    print(f"{workload} {H}x{W} frame, {m} pixels vs oracle: rgb_c {e_c:.2e}, pinned rgb_f {e_f:.2e}, un-pinned pixels off by >1e-4: {bad:.4f}")
    # lego: observed ~1e-6.  fern: the oracle's own NDC warp feeds its un-pinned pass; an ulp of an NDC coordinate is amplified by
    # 2^9 in the top positional band, so the coarse bar there is the north star's 1e-4 (as test_batchify_F9[llff])
    assert e_c <= (1e-4 if workload == "fern" else 2e-5) and e_f <= 2e-5 and bad <= 0.02, (e_c, e_f, bad)


@pytest.mark.parametrize("workload", ["lego", "fern"])
def test_eight_row_blocks_assemble_to_the_one_rank_frame(workload, packed, frames):
    """What the 8 ranks of config #3 compute, one block after the other on this GPU, assembled as gather_tiles assembles them."""
    K, H, W, pose, opts = _scene(workload)
    rgb, disp = frames[workload]
    world = 8
    tiles = [mdist.render_shard(H, W, K, pose, packed, opts, world, r, seed=7) for r in range(world)]
    rows = [t.shape[0] // W for t in tiles]
    assert rows == ([100] * 8 if workload == "lego" else [48, 48, 47, 47, 47, 47, 47, 47])
    full = mdist.assemble_tiles(tiles, H, W)
    assert torch.equal(full[:, :3].reshape(H, W, 3), rgb) and torch.equal(full[:, 3].reshape(H, W), disp)


def test_eight_batch_shards_equal_the_batch(packed):
    """The 4096-ray metric under strong scaling: 8 contiguous 512-ray slices with jitter keyed on the global ray index give the
    rows of the whole batch, bit for bit (bench.py make_batch / shard_range)."""
    K, H, W, pose, opts = _scene("lego")
    pix = torch.from_numpy(synthetic.pixel_batch(H, W, 4096, 0)).to(DEV)
    o, d = ops.make_o_d_pixels(W, H, K, pose, pix)
    rays = torch.cat([o, d], -1).contiguous()
    whole = NP.render_rays(rays, packed, None, opts, seed=0)
    for r in range(8):
        first, n = mdist.shard_range(4096, 8, r)
        assert n == 512
        part = NP.render_rays(rays[first:first + n].contiguous(), packed, None, opts, seed=0, ray_offset=first)
        for k in ("rgb_c", "disp_c", "rgb_f", "disp_f"):
            assert torch.equal(part[k], whole[k][first:first + n]), (r, k)


def _bench(extra_args, env_extra, timeout=850):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "BENCH_SOLO_RANK"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *extra_args], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                                  # ONE JSON line
    return json.loads(lines[0])


@pytest.mark.timeout(900)
@pytest.mark.parametrize("workload", ["lego", "fern"])
def test_bench_four_live_ranks_time_both_gather_routes(workload, fake_rccl_lib, packed):
    """`python bench.py --gpus 4`: its own launcher, 4 workers, strong + weak legs, the sharded frame with its all-gather (ragged for
    fern: 95, 95, 94, 94 rows -- through the staging buffer and the un-pad kernel) -- timed through BOTH routes in the one run:
    torch.distributed (frame_ms) and mi_nerf_all_gather_tiles on the library's own communicator (frame_ms_c_abi), equal checksums.
    On a box with fewer than 4 GPUs the ranks share the card: gloo for the process group, tests/c_abi/fake_rccl.cpp in librccl's place."""
    real = torch.cuda.device_count() >= 4
    env = {} if real else {"BENCH_BACKEND": "gloo", "MI_NERF_RCCL_LIB": fake_rccl_lib, "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    j = _bench(["--gpus", "4", "--steps", "3", "--warmup", "1", "--frames", "1", "--no-cpu-baseline", "--no-f16s-leg", "--workload", workload], env)
    assert j["n_gpus"] == 4 and j["steps"] == 3 and j["scaling"] == "strong"
    assert j["config"]["rays_per_gpu"] == 1024 and j["value"] > 0 and j["value_weak"] > 0
    assert j["frame_ms"] > 0 and j["frame_hw"] == ([378, 504] if workload == "fern" else [800, 800])
    assert 0 < j["roofline"]["frac"] <= 1.0 and j["bf16"]["rays_per_s"] > 0
    # the line verifies its own collective: four ranks seen, the gathered frame identical on all of them, every rank's re-render of its
    # neighbour's row block (ragged for fern) equal to that block of the gathered frame
    c = j["collective"]
    assert c["world_size"] == 4 and c["backend"] == ("nccl" if real else "gloo")
    assert [r["rank"] for r in c["ranks"]] == [0, 1, 2, 3] and all(r["cus"] == 256 for r in c["ranks"])
    assert c["distinct_devices"] == (4 if real else 1)
    assert c["frame_equal_across_ranks"] is True and c["neighbour_tile_recomputed_equal"] is True and c["all_gather_ms"] > 0
    # the library's own route, same run: the tile gather bit-equal to the torch route's on every rank, then the same frame(s) timed through it
    ca = c["c_abi"]
    assert "error" not in ca and ca["equal_to_torch_route_on_every_rank"] is True and ca["world_size"] == 4 and ca["all_gather_ms"] > 0
    assert (ca["staging_bytes"] > 0) == (workload == "fern")
    assert ca["frame_checksum_equals_torch_route_on_every_rank"] is True
    assert j["frame_ms_c_abi"] > 0 and j["frame_checksum_c_abi"] == j["frame_checksum"]
    # ... and the frame it assembled from four tiles is, bit for bit, the frame ONE rank renders: `frame_checksum` (the fp32 bit patterns
    # of the last timed frame) of this line against a one-GPU run of the same command -- what BENCH (N = 1) and SCALE (N = 8) let a
    # reader check from the driver's records alone
    assert j["frame_checksum"] == c["frame_checksum_rank0"] and isinstance(j["frame_checksum"], int)
    if workload == "fern":
        # the same frame rendered by THIS process on one rank (dist.render_frame, the bench's weights / pose / seed), checksummed by bench.py's own function
        import bench
        K, H, W, _, opts = _scene("fern")
        one_rgb, one_disp = mdist.render_frame(H, W, K, synthetic.fern_pose(), packed, opts, seed=0)
        assert bench.frame_checksum(torch, one_rgb, one_disp) == j["frame_checksum"]
        return
    one = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "1", "--no-cpu-baseline", "--train-steps", "0", "--no-small-batch",
                  "--no-bf16-leg", "--no-f16s-leg", "--workload", workload], {})
    assert "collective" not in one and "frame_ms_c_abi" not in one and one["frame_checksum"] == j["frame_checksum"], (one["frame_checksum"], j["frame_checksum"])
    with open(os.path.join(ROOT, "BASELINE.json"), encoding="utf-8") as fh:
        assert one["metric"] == j["metric"] == json.load(fh)["metric"]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("workload,rank", [("fern", 2), ("lego", 7)])
def test_bench_one_rank_of_eight_alone(workload, rank):
    """Rank r of the driver's 8-GPU run, alone on this GPU: the 512-ray shard (both legs), its 100 (lego) or 47-48 (fern) frame rows."""
    j = _bench(["--gpus", "8", "--steps", "3", "--warmup", "1", "--frames", "1", "--no-cpu-baseline", "--workload", workload],
               {"BENCH_SOLO_RANK": "1", "RANK": str(rank), "LOCAL_RANK": "0", "WORLD_SIZE": "8"})
    assert j["n_gpus"] == 8 and j["config"]["rays_per_gpu"] == 512 and j["solo_rank"] == {**j["solo_rank"], "rank": rank, "of": 8, "n_gpus_measured": 1}
    assert "collective" not in j
    assert j["value"] > 0 and j["value_weak"] > 0 and j["frame_ms"] > 0
    assert j["bf16"]["rays_per_s"] > 0 and 0 < j["roofline"]["frac"] <= 1.0


@pytest.mark.timeout(600)
def test_bench_dump_outputs_are_what_the_timed_step_returned(packed, tmp_path):
    """`bench.py --dump-outputs DIR`: the four arrays render_rays hands its caller in the last timed step, float32, bit-equal to the
    same call made here on the bench's inputs (weights seed 0, lego pose, pixels of RandomState(0), jitter seed 0); `steps` is --steps."""
    j = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", "0", "--no-cpu-baseline", "--train-steps", "0", "--no-small-batch",
                "--no-bf16-leg", "--no-f16s-leg", "--dump-outputs", str(tmp_path)], {})
    assert j["steps"] == 2 and j["ms_per_step"] > 0
    K, H, W, _, opts = _scene("lego")
    pix = torch.from_numpy(synthetic.pixel_batch(H, W, 4096, 0)).to(DEV)
    o, d = ops.make_o_d_pixels(W, H, K, synthetic.pose_spherical(0.0, -30.0, 4.0), pix)
    rays = torch.cat([o, d], -1).contiguous()
    want = ops.render_rays(packed.net, packed.coarse, packed.fine, ops.render_cfg(opts.near, opts.far, SC, NF, False, False, seed=0, ray_offset=0),
                           rays, None, None)[:4]
    assert sorted(os.listdir(tmp_path)) == ["disp_c.npy", "disp_f.npy", "rgb_c.npy", "rgb_f.npy"]
    for name, t in zip(("rgb_c", "disp_c", "rgb_f", "disp_f"), want):
        got = np.load(os.path.join(tmp_path, name + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, t.cpu().numpy()), name
