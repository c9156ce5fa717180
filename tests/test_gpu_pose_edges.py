"""libmi_nerf_pose.so where tests/test_gpu_pose.py does not reach: the libm side of the sin / cos branch, a second ray per wave, the 80 KiB
LDS edge, every channel map and skip layer, 1024 samples, poisoned neighbours, and the second pixel per thread of the make_o_d reduction.

input_grad_kernel is fed SYNTHETIC deltas (tests/test_pose_cpu.py: SyntheticCase -- seeded randn written into the workspace views the kernel
reads, the rest of the workspace NaN), so the kernel stands alone: no backward-data error, no ReLU knife, no network forward.  The reference
is input_grad_rule in float64 with sin / cos evaluated at the fp32 points and view directions the forward forms (o + d * z with the product
rounded, then the sum: test_gpu_far_points.points); at |x| = 2048 one ulp of x is 0.12 rad in the top band, so a kernel that contracted
the product into an FMA, or took the wrong side's routine, misses d_pts -- one slope per point -- by orders of magnitude.  The bar is the
module's own: per output e32, the same rule in fp32 on the CPU against float64 relative to the largest entry, and the kernel within
max(3 e32, 2e-4).  Every case prints both; tests/test_pose_cpu.py holds every case to e32 < 1e-2 without a device."""
import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import ops, pose
from tests import test_gpu_far_points as F
from tests.test_gpu_pose import _camera, _o_d_check, bar
from tests.test_pose_cpu import (CHAIN, OUTPUTS, SyntheticCase, blind_sd, chain_autograd, chain_inputs, edge_specs, poisoned, rel_err, spec_id)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F64, F32 = torch.float64, torch.float32


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def launch_grid(c, n):
    """(grid, resident workgroups) of mi_pose_input_grad for n rays of this network, as docs/design/19_pose_gradients.md states them."""
    lds = ((2 if c.has_skip else 1) * c.W * 64 + (c.W // 2) * 32) * 4
    resident = cus() * (2 if lds <= 80 * 1024 else 1)
    return min((n + 3) // 4, resident), resident


def device_run(c: SyntheticCase, pick=None, rays=None, z=None):
    """pose.input_grad on the case's tensors (``pick``: these rays alone, in a launch of their own; ``rays`` / ``z``: others in their place).
    The workspace is NaN except for the three views the kernel is meant to read."""
    rays, z = c.rays if rays is None else rays, c.z if z is None else z
    idx = torch.arange(c.n) if pick is None else torch.as_tensor(pick)
    n, S, W = len(idx), c.S, c.W
    net = ops.make_net(c.D, W, c.skip if c.has_skip else -1, c.L_x, c.L_d)
    work = torch.full((ops.train_layout(net, n, S).work_bytes,), 0xFF, dtype=torch.uint8, device=DEV)
    v = ops.train_views(net, n, S, work=work)
    rows = lambda t: t.reshape(c.n, S, -1)[idx].reshape(n * S, -1).to(DEV)             # noqa: E731
    v["delta_h"][0].copy_(rows(c.delta_x0))
    if c.has_skip:
        v["delta_h"][c.skip + 1].copy_(rows(c.delta_skip))
    v["delta_d"].copy_(rows(c.delta_d))
    flat = ops.flatten_params(c.sd, "model_fine.", net, DEV)
    dev = lambda t: t[idx].contiguous().to(DEV)                                         # noqa: E731
    got = pose.input_grad(net, flat, dev(rays), dev(z), dev(c.raw), dev(c.d_raw), work, want_staged=True)
    torch.cuda.synchronize()
    return dict(zip(OUTPUTS, (g.cpu() for g in got)))


def check_rule(c, got, tag):
    """Every output within max(3 e32, 2e-4) of the float64 rule; -> {output: (e32, e_hip)}."""
    want, e32 = c.rule(F64), c.e32()
    seen = {k: (e32[k], rel_err(got[k], want[k])) for k in OUTPUTS}
    for k, (e, e_hip) in seen.items():
        print(f"input_grad {tag} {k}: e32 {e:.2e}  e_hip {e_hip:.2e}  bar {bar(e, 2e-4):.2e}")
        assert torch.isfinite(got[k]).all(), (tag, k)
        assert e < 1e-2, (tag, k, e)
    for k, (e, e_hip) in seen.items():
        assert e_hip <= bar(e, 2e-4), (tag, k, e, e_hip)
    return seen


def rows_of(out, i, S):
    """Ray i's part of every output."""
    return {"d_rays": out["d_rays"][i], "d_view": out["d_view"][i], "d_pts": out["d_pts"][i * S:(i + 1) * S], "d_emb": out["d_emb"][i * S:(i + 1) * S]}


# ---------------------------------------------------------------------------------------------------
# 1. the kernel against the rule
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", edge_specs("branch"), ids=spec_id)
def test_input_grad_at_the_sin_cos_branch(spec):
    """Rays placed at SINCOS_FAST_LIMIT (far_rays): all fast (the control), half of every ray and tile slow, all slow, the exact edge, one odd
    sample per tile.  channel_slope branches per channel on |2^k x|; the forward branched once per point."""
    c = SyntheticCase(spec)
    slow = F.is_slow(c.rays, c.z)
    assert bool(slow.any()) == (c.kind != "fast") and bool((~slow).any()) == (c.kind != "slow")
    check_rule(c, device_run(c), spec_id(spec))


@pytest.mark.parametrize("spec", edge_specs("maps") + edge_specs("samples") + edge_specs("lds"), ids=spec_id)
def test_input_grad_channel_maps_skip_layers_sample_counts_and_the_lds_edge(spec):
    """in_x below 64 and in_d below 32 (L_x = 5: one live column in the second block, leading dimension 33), the mixed (10, 0) and (0, 4), the
    skip layers 0 and D - 2 (which delta_h block and which block of the flat vector: every other delta of the workspace is NaN), 257 and 1024
    samples per ray, and W = 256 without a skip block, whose weight image is 80 KiB exactly."""
    c = SyntheticCase(spec)
    check_rule(c, device_run(c), spec_id(spec))


@pytest.mark.parametrize("spec", edge_specs("loop"), ids=spec_id)
def test_input_grad_ray_loop_beyond_the_resident_grid(spec):
    """More rays than four per resident workgroup: waves own a second (third, ...) ray.  The whole batch against the rule, and rays 0,
    4 * grid (the first second ray of workgroup 0) and n - 1 ALONE, in launches of one ray, equal their rows of the batch bit for bit."""
    c = SyntheticCase(spec, cus())
    grid, resident = launch_grid(c, c.n)
    assert c.n > 4 * resident and grid == resident, (c.n, grid, resident)
    got = device_run(c)
    check_rule(c, got, f"{spec_id(spec)} (n = {c.n}, grid {grid})")
    for i in (0, 4 * grid, c.n - 1):
        one, rows = device_run(c, pick=[i]), rows_of(got, i, c.S)
        assert all(torch.equal(one[k].reshape(rows[k].shape), rows[k]) for k in OUTPUTS), i


def test_input_grad_poisoned_rays_leave_their_neighbours_alone():
    """Nine rays: ray 1 with a NaN origin component, ray 4 with z = inf at one sample, ray 6 with d = 0; each shares a workgroup with clean
    rays.  The six others are bit-identical to the batch in which those three are clean too, and the poisoned rays have no finite value
    where the float64 rule (at the pinned points) has none."""
    c = SyntheticCase(edge_specs("isolation")[0])
    rays, z, bad = poisoned(c)
    clean_out = device_run(c)
    check_rule(c, clean_out, "isolation, clean batch")
    got = device_run(c, rays=rays, z=z)
    for i in range(c.n):
        if i not in bad:
            a, b = rows_of(got, i, c.S), rows_of(clean_out, i, c.S)
            assert all(torch.equal(a[k], b[k]) for k in OUTPUTS), i
    want = c.rule(F64, rays, z)
    for k in OUTPUTS:
        lost = ~torch.isfinite(want[k])
        assert not bool(torch.isfinite(got[k])[lost].any()), k
        kept = ~lost & torch.isfinite(got[k])                                            # where both are finite the bar holds as well
        scale = float(want[k][~lost].abs().max())
        e_hip = float((got[k].double() - want[k])[kept].abs().max()) / scale
        print(f"input_grad isolation, poisoned batch {k}: {int(lost.sum())} non-finite in the rule, {int((~torch.isfinite(got[k])).sum())} on the device; "
              f"finite entries e_hip {e_hip:.2e}")
        assert e_hip <= bar(c.e32()[k], 2e-4), (k, e_hip)
    assert int((~torch.isfinite(want["d_rays"])).sum()) == 2 + 6 + 3


# ---------------------------------------------------------------------------------------------------
# 2. one chain: fused training forward -> backward data -> input_grad at the branch
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16s", [False, True], ids=["fp32", "f16s"])
def test_the_training_chain_at_the_branch(f16s):
    """blind_net("d8w256") on straddle rays (5 x 33): ops.mlp_rays_train -> ops.mlp_backward(stage=1) -> pose.input_grad against float64
    autograd of gamma64 -> network -> rgb (tests/test_pose_cpu.py: chain_autograd), ReLU-knife points cut on both sides as in
    tests/test_gpu_pose.py.  It ties the points the fused forward encodes to the points the backward differentiates at."""
    rays, z, g_rgb = chain_inputs()
    sd, _, D, skips = F.blind_net(CHAIN["tag"])
    ref_sd = blind_sd(CHAIN["tag"])
    assert all(np.array_equal(sd[k], ref_sd[k]) for k in sd)
    prefix, n, S = CHAIN["prefix"], CHAIN["n"], CHAIN["S"]
    net = ops.make_net(D, F.NETS[CHAIN["tag"]][1], skips[0], F.L_X, F.L_D)
    fwd = ops.pack_module(sd, prefix, net, f16s=f16s).to(DEV)
    packed = ops.pack_module(sd, prefix, net).to(DEV)
    packed_bwd = ops.pack_module(sd, prefix, net, backward=True, f16s=f16s).to(DEV)
    flat = ops.flatten_params(sd, prefix, net, DEV)
    rd, zd = rays.to(DEV), z.to(DEV)
    raw, stash = ops.mlp_rays_train(net, fwd, rd, zd, f16s=f16s)
    v = ops.train_views(net, n, S, stash=stash)
    pre = chain_autograd(sd, rays, z, g_rgb, F64)["pre"]
    knife = ((v["stash_g"].cpu() > 0) != (pre["ad"] > 0)).any(dim=1)
    for l in range(D):
        knife |= ((v["stash_h"][l].cpu() > 0) != (pre[f"a{l}"] > 0)).any(dim=1)
    assert int(knife.sum()) <= max(3, n * S // 100), int(knife.sum())
    keep = ~knife
    want, w32 = chain_autograd(sd, rays, z, g_rgb, F64, keep), chain_autograd(sd, rays, z, g_rgb, F32, keep)
    d_raw = want["d_raw"].float().contiguous()
    d_raw_net = (d_raw.reshape(-1, 4) * keep.float()[:, None]).reshape(n, S, 4).contiguous().to(DEV)      # what reaches the network
    d_raw = d_raw.to(DEV)
    _, work = ops.mlp_backward(net, packed, packed_bwd, rd, zd, d_raw_net, stash, stage=1, f16s_dgrad=f16s)
    got = dict(zip(OUTPUTS, pose.input_grad(net, flat, rd, zd, raw, d_raw, work, want_staged=True)))
    torch.cuda.synchronize()
    seen = {k: (rel_err(w32[k], want[k]), rel_err(got[k], want[k])) for k in OUTPUTS}
    for k, (e32, e_hip) in seen.items():
        print(f"chain {CHAIN['tag']} {CHAIN['arr']} f16s={f16s} {k}: e32 {e32:.2e}  e_hip {e_hip:.2e}  bar {bar(e32, 2e-4):.2e}  ({int(knife.sum())} points cut)")
        assert e32 < 1e-2, (k, e32)
    for k, (e32, e_hip) in seen.items():
        assert e_hip <= bar(e32, 2e-4), (k, e32, e_hip)


# ---------------------------------------------------------------------------------------------------
# 3. the make_o_d reduction beyond one pixel per thread
# ---------------------------------------------------------------------------------------------------
def _grads(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)


@pytest.mark.parametrize("n,repeats", [(65536, False), (65537, False), (70000, True)], ids=["65536", "65537", "70000-repeats"])
def test_make_o_d_backward_long_pixel_lists(n, repeats):
    """65536 pixels are 256 full blocks of one pixel per thread; 65537 make chunk = 512, a second pixel per thread and a last block of one
    pixel; 70000 indices drawn WITH replacement, unsorted."""
    img_w, img_h = 401, 399
    K, k4, cam = _camera(img_w, img_h)
    rs = np.random.RandomState(n)
    pix = torch.from_numpy((rs.randint(0, img_w * img_h, n) if repeats else rs.choice(img_w * img_h, n, replace=False)).astype(np.int64))
    if repeats:
        assert len(np.unique(pix.numpy())) < n and not bool((pix[1:] >= pix[:-1]).all())
    g_o, g_d = _grads(n, n)
    d_pose, d_k4 = pose.make_o_d_backward(img_w, img_h, K, cam, g_o.to(DEV), g_d.to(DEV), pixels=pix.to(DEV))
    _o_d_check(f"pixels n={n}{' with repeats' if repeats else ''}", img_w, k4, cam, pix, g_o, g_d, d_pose, d_k4)
    again = pose.make_o_d_backward(img_w, img_h, K, cam, g_o.to(DEV), g_d.to(DEV), pixels=pix.to(DEV))
    assert torch.equal(again[0], d_pose) and torch.equal(again[1], d_k4)


@pytest.mark.parametrize("img_w,img_h,row0,n_rows", [(400, 400, 0, 400), (401, 399, 3, 396)], ids=["400x400-whole", "401x399-rows3-399"])
def test_make_o_d_backward_whole_images(img_w, img_h, row0, n_rows):
    """A 400 x 400 image is chunk = 768 on 209 blocks, the last one 256 pixels short of full; 401 x 399 rows [3, 399) has an odd width and a
    row offset.  The row form and the pixel list of the same rows are one sum."""
    n = n_rows * img_w
    K, k4, cam = _camera(img_w, img_h)
    pix = torch.arange(row0 * img_w, (row0 + n_rows) * img_w)
    g_o, g_d = _grads(n, n)
    d_pose, d_k4 = pose.make_o_d_backward(img_w, img_h, K, cam, g_o.to(DEV), g_d.to(DEV), row0=row0)
    _o_d_check(f"rows {img_w}x[{row0},+{n_rows})", img_w, k4, cam, pix, g_o, g_d, d_pose, d_k4)
    listed = pose.make_o_d_backward(img_w, img_h, K, cam, g_o.to(DEV), g_d.to(DEV), pixels=pix.to(DEV))
    assert torch.equal(listed[0], d_pose) and torch.equal(listed[1], d_k4)
