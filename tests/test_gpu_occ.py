"""Occupancy-grid rendering on the GPU (include/mi_nerf_occ.h).  The contract is the MASKED IDENTITY: mi_occ_render_rays equals, bit for bit, the
staged public path (mi_nerf_mlp_rays* over ALL samples | raw zeroed where mi_occ_mark answers 0 | mi_nerf_composite), and mi_occ_mark equals a numpy
fp32 restatement of the header's cell rule on every sample.  Bake, dilate and count are held against torch restatements, the fp32 render against
the CPU oracle at the project's parity bar (2e-5, docs/design/02_oracle_and_parity.md), and a trained scene's held-out PSNR with a baked grid
against the full render's at the bar for an alternative render mode (0.05 dB, README)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import harness, ops, synthetic, weights
from nerf_pytorch_paeng_amd import nerf_process as NP
from nerf_pytorch_paeng_amd import occupancy as OC
from oracle import restate as R
from tests.test_occ_cpu import cell_rule

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32
FAMILY = {"fp32": {}, "f16s": {"f16s": True}, "bf16": {"bf16": True}}
# Families whose masked identity holds bit for bit on the GPU (each lane of the network kernels evaluates its own point, whatever tile it sits
# in).  A family found otherwise is held to the parity bar 2e-5 instead and recorded in docs/design/14_occupancy.md.
BIT_EXACT = {"fp32": True, "f16s": True, "bf16": True}
PARITY_BAR = 2e-5


@pytest.fixture(scope="module")
def scene():
    sd = synthetic.make_state_dict(0, 8, 256)
    packed = weights.PackedNeRF.from_state_dict(sd, DEV)
    K, H, W = synthetic.lego_camera()
    pose = synthetic.pose_spherical(0.0, -30.0, 4.0)
    pix = torch.from_numpy(synthetic.pixel_batch(H, W, 256, 0)).to(DEV)
    o, d = ops.make_o_d_pixels(W, H, K, pose, pix)
    rays = torch.cat([o, d], -1).contiguous()
    return SimpleNamespace(sd=sd, packed=packed, rays=rays)


def random_grid(res=(32, 32, 32), lo=-1.5, hi=1.5, outside=True, seed=0, p=0.5):
    g = OC.OccupancyGrid(lo, hi, res, outside_occupied=outside)
    cells = np.random.RandomState(seed).rand(g.words * 32) < p
    cells[g.cells:] = False
    g.set_bits(np.packbits(cells, bitorder="little").view(np.uint32)).to(DEV)
    return g


def unpack(bits: torch.Tensor, res) -> torch.Tensor:
    """int32 words -> bool [rz, ry, rx]."""
    w = bits.cpu().numpy().view(np.uint32)
    cells = np.unpackbits(w.view(np.uint8), bitorder="little")[:res[0] * res[1] * res[2]]
    return torch.from_numpy(cells.astype(bool)).reshape(res[2], res[1], res[0])


def pack(cells: torch.Tensor) -> np.ndarray:
    flat = cells.reshape(-1).cpu().numpy().astype(bool)
    flat = np.concatenate([flat, np.zeros((-len(flat)) % 32, bool)])
    return np.packbits(flat, bitorder="little").view(np.uint32)


# ---------------------------------------------------------------------------------------------------
# 1. mark
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outside", [True, False])
@pytest.mark.parametrize("kind", ["blender", "ndc"])
def test_mark_equals_the_cell_rule_on_every_sample(scene, kind, outside):
    g = torch.Generator().manual_seed(3)
    if kind == "blender":
        rays = scene.rays
        z = ops.stratified_z(2.0, 6.0, torch.rand(rays.shape[0], 64, generator=g).to(DEV))
        grid = random_grid((32, 24, 40), -3.0, 3.0, outside, seed=1)
    else:
        K, H, W = synthetic.fern_camera()
        pix = torch.from_numpy(synthetic.pixel_batch(H, W, 256, 1)).to(DEV)
        o, d = ops.make_o_d_pixels(W, H, K, synthetic.fern_pose(), pix)
        o, d = ops.ndc_rays(H, W, float(K[0][0]), 1.0, o, d)
        rays = torch.cat([o, d], -1).contiguous()
        z = ops.stratified_z(0.0, 1.0, torch.rand(rays.shape[0], 64, generator=g).to(DEV))
        grid = random_grid((48, 36, 32), (-1.0, -0.8, -1.0), (1.0, 0.8, 0.9), outside, seed=2)      # an NDC box that cuts the frustum on every side
    got = grid.mark(rays, z).cpu().numpy().astype(bool)
    want = cell_rule(grid.lo, grid.hi, grid.res, outside, grid.bits.cpu().numpy().view(np.uint32), rays.cpu().numpy(), z.cpu().numpy())
    share = float(got.mean())
    print(f"\n[mark {kind} outside_occupied={outside}] evaluated share {share:.3f}, differing samples {int((got != want).sum())} of {got.size}")
    assert 0.05 < share < 0.95                                       # the case exercises both answers
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------
# 2. / 3. masked identity, all-occupied grid
# ---------------------------------------------------------------------------------------------------
def _masked_chain(net, blob, rays, z, mask, flags):
    raw = ops.mlp_rays(net, blob, rays, z, bf16=flags.get("bf16", False), f16s=flags.get("f16s", False))
    raw = torch.where(mask.bool()[..., None], raw, torch.zeros_like(raw))
    return ops.composite(raw, z, rays, want_all=True)


def _render(scene, family, grid, n=256, Sc=64, Nf=128):
    prec = ops.precision(**FAMILY[family])
    net, blob_c, blob_f = scene.packed.kernel_blobs(prec)
    cfg = ops.render_cfg(2.0, 6.0, Sc, Nf, False, **FAMILY[family])
    g = torch.Generator().manual_seed(11)
    t_rand, u = torch.rand(n, Sc, generator=g).to(DEV), torch.rand(n, Nf, generator=g).to(DEV)
    rays = scene.rays[:n].contiguous()
    rgb_c, disp_c, rgb_f, disp_f, ws, stats = OC.render_rays(net, blob_c, blob_f, cfg, grid, rays, t_rand, u)
    v = OC.workspace_views(cfg, n, ws)
    return SimpleNamespace(net=net, blob_c=blob_c, blob_f=blob_f, cfg=cfg, rays=rays, t_rand=t_rand, u=u, rgb_c=rgb_c, disp_c=disp_c, rgb_f=rgb_f,
                           disp_f=disp_f, stats=stats, ws=ws, **v)


def _compare(family, what, got, want):
    diff = int((got != want).sum())
    err = float((got - want).abs().max())
    print(f"[{family}] {what}: {diff} of {got.numel()} values differ, max |diff| {err:.3e}")
    return [] if (diff == 0 if BIT_EXACT[family] else err <= PARITY_BAR) else [(family, what, diff, err)]


@pytest.mark.parametrize("family", sorted(FAMILY))
def test_masked_identity(scene, family):
    grid = random_grid((32, 32, 32), -2.5, 2.5, True, seed=5)
    r = _render(scene, family, grid)
    flags = FAMILY[family]
    print()
    # the depths are the public stages' own
    assert torch.equal(r.z_c, ops.stratified_z(2.0, 6.0, r.t_rand))
    mask_c = grid.mark(r.rays, r.z_c)
    rgb, disp, _, wts, _ = _masked_chain(r.net, r.blob_c, r.rays, r.z_c, mask_c, flags)
    bad = _compare(family, "rgb_c", r.rgb_c, rgb) + _compare(family, "disp_c", r.disp_c, disp) + _compare(family, "weights_c", r.weights_c, wts)
    assert torch.equal(r.z_f, ops.fine_z(r.z_c, r.weights_c, 128, False, r.u))
    mask_f = grid.mark(r.rays, r.z_f)
    rgb, disp, _, _, _ = _masked_chain(r.net, r.blob_f, r.rays, r.z_f, mask_f, flags)
    bad += _compare(family, "rgb_f", r.rgb_f, rgb) + _compare(family, "disp_f", r.disp_f, disp)
    assert bad == []                                                 # every figure is printed above before this
    # every raw value is written: zeros exactly at the skipped samples
    assert float(r.raw_c[~mask_c.bool()].abs().max()) == 0.0 and float(r.raw_f[~mask_f.bool()].abs().max()) == 0.0
    s = r.stats
    assert (s["total_c"], s["total_f"]) == (256 * 64, 256 * 192)
    assert (s["evaluated_c"], s["evaluated_f"]) == (int(mask_c.sum()), int(mask_f.sum()))
    assert 0 <= s["padded_c"] < 32 * 256 * 2 and (s["evaluated_c"] + s["padded_c"]) % 32 == 0 and (s["evaluated_f"] + s["padded_f"]) % 32 == 0
    assert 0 < s["evaluated_c"] < s["total_c"] and 0 < s["evaluated_f"] < s["total_f"]
    _check_tiles(r, mask_f)


def _check_tiles(r, mask_f):
    """The tiles the cull kernel emitted for the fine pass (the last one, still in the workspace): every survivor sits in exactly one lane,
    in order within its ray, with its depth, its ray and its source index; padding carries -1 and repeats the ray's last surviving depth."""
    n, St = r.z_f.shape
    tiles = (r.stats["evaluated_f"] + r.stats["padded_f"]) // 32
    t = {k: v.cpu() for k, v in OC.tile_views(r.cfg, n, r.ws, tiles).items()}
    src, tz, slot = t["tile_src"].reshape(-1).long(), t["tile_z"].reshape(-1), t["slot"].reshape(-1).long()
    valid = src >= 0
    z_flat, m_flat = r.z_f.cpu().reshape(-1), mask_f.cpu().reshape(-1).bool()
    assert int(valid.sum()) == r.stats["evaluated_f"] and bool((src[~valid] == -1).all())
    assert torch.equal(torch.sort(src[valid])[0], torch.nonzero(m_flat).reshape(-1))          # each survivor once, nothing else
    assert torch.equal(tz[valid], z_flat[src[valid]])
    lanes = torch.arange(tiles * 32)
    assert torch.equal(slot[src[valid]], lanes[valid]) and bool((slot[~m_flat] == -1).all())
    src2, valid2, tz2 = src.reshape(tiles, 32), valid.reshape(tiles, 32), tz.reshape(tiles, 32)
    assert bool(valid2[:, 0].all())                                                          # a tile starts with a survivor
    ray_of = src2[:, 0] // St
    assert bool(((src2 // St == ray_of[:, None]) | ~valid2).all())                           # one ray per tile
    assert torch.equal(t["tile_rays"], r.rays.cpu()[ray_of])
    assert bool((valid2[:, 1:] <= valid2[:, :-1]).all())                                     # survivors first, then padding
    assert bool(((src2[:, 1:] > src2[:, :-1]) | ~valid2[:, 1:]).all())                       # in sample order
    last = tz2.gather(1, (valid2.sum(1) - 1)[:, None])
    assert bool(((tz2 == last) | valid2).all())                                              # padding repeats the last surviving depth


def test_all_occupied_grid_is_the_staged_full_path(scene):
    grid = OC.OccupancyGrid(-1.5, 1.5, 16)
    grid.set_bits(np.full(grid.words, 0xFFFFFFFF, np.uint32)).to(DEV)
    r = _render(scene, "fp32", grid)
    assert bool(grid.mark(r.rays, r.z_c).all()) and bool(grid.mark(r.rays, r.z_f).all()) and grid.fraction() == 1.0
    ones = torch.ones(256, 64, dtype=torch.uint8, device=DEV)
    rgb, disp, _, wts, _ = _masked_chain(r.net, r.blob_c, r.rays, r.z_c, ones, {})
    assert torch.equal(r.rgb_c, rgb) and torch.equal(r.disp_c, disp) and torch.equal(r.weights_c, wts)
    raw_f = ops.mlp_rays(r.net, r.blob_f, r.rays, r.z_f)                       # the staged full path: nothing zeroed
    rgb, disp, *_ = ops.composite(raw_f, r.z_f, r.rays, want_all=True)
    assert torch.equal(r.rgb_f, rgb) and torch.equal(r.disp_f, disp) and torch.equal(r.raw_f, raw_f)
    s = r.stats
    assert (s["evaluated_c"], s["evaluated_f"], s["padded_c"], s["padded_f"]) == (s["total_c"], s["total_f"], 0, 0)
    # an empty grid that also skips the outside evaluates nothing: white background, no network launch
    empty = OC.OccupancyGrid(-1.5, 1.5, 16, outside_occupied=False)
    empty.set_bits(np.zeros(empty.words, np.uint32)).to(DEV)
    e = _render(scene, "fp32", empty)
    assert e.stats["evaluated_c"] == e.stats["evaluated_f"] == e.stats["padded_c"] == 0
    assert float((e.rgb_f - 1.0).abs().max()) == 0.0 and float(e.raw_f.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------
# 4. CPU oracle
# ---------------------------------------------------------------------------------------------------
def test_render_vs_cpu_oracle_with_the_same_mask(scene):
    """oracle.restate embed / mlp_forward / post_process with raw zeroed by the SAME mask (mi_occ_mark of the depths the GPU used); the fine
    depths are pinned to the GPU's.  No ray is left out of either comparison."""
    n = 128
    grid = random_grid((32, 32, 32), -2.5, 2.5, True, seed=7)
    r = _render(scene, "fp32", grid, n=n)
    rays, sd = r.rays.cpu(), scene.sd

    def oracle(prefix, z, mask):
        raw = R.mlp_forward(sd, prefix, R.embed(rays, z, 10, 4), 8, 63, 27).reshape(n, z.shape[1], 4)
        raw = torch.where(mask.bool()[..., None], raw, torch.zeros_like(raw))
        return R.post_process(raw, z, rays[:, 3:])[0]

    z_c = R.stratified_z(n, 2.0, 6.0, 64, r.t_rand.cpu())
    e_c = float((r.rgb_c.cpu() - oracle("model_coarse.", z_c, grid.mark(r.rays, r.z_c).cpu())).abs().max())
    z_f = r.z_f.cpu()
    e_f = float((r.rgb_f.cpu() - oracle("model_fine.", z_f, grid.mark(r.rays, r.z_f).cpu())).abs().max())
    print(f"\n[oracle] rgb_c max err {e_c:.2e}, rgb_f (pinned depths) max err {e_f:.2e} over all {n} rays")
    assert e_c <= PARITY_BAR and e_f <= PARITY_BAR, (e_c, e_f)


def test_public_surface_matches_the_direct_call(scene):
    """nerf_process.render_rays(occupancy=grid) is the mi_occ_render_rays call: same numbers, stats returned with the intermediates; the default
    jitter is the generator's (what mi_nerf_render_rays draws); batchify slabs give the same frame."""
    grid = random_grid((32, 32, 32), -2.5, 2.5, True, seed=5)
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=64, N_samples_f=128, perturb=1.0, chunk_rays=4096, chunk_pts=524288, data_type="blender")
    r = _render(scene, "fp32", grid)
    with torch.no_grad():
        out = NP.render_rays(r.rays, scene.packed, None, opts, t_rand=r.t_rand, u=r.u, occupancy=grid, return_intermediates=True)
        assert torch.equal(out["rgb_f"], r.rgb_f) and torch.equal(out["disp_c"], r.disp_c) and out["_occ_stats"] == r.stats == grid.last_stats
        drawn = NP.render_rays(r.rays, scene.packed, None, opts, seed=9, ray_offset=100, occupancy=grid, return_intermediates=True)
        assert torch.equal(drawn["_t_rand"], ops.fill_uniform(9, 0, 100, 256, 64, DEV)) and torch.equal(drawn["_u"], ops.fill_uniform(9, 1, 100, 256, 128, DEV))
        assert torch.equal(drawn["_z_c"], ops.stratified_z(2.0, 6.0, drawn["_t_rand"]))
        none = NP.render_rays(r.rays, scene.packed, None, opts, seed=9, ray_offset=100, occupancy=grid)      # jitter drawn into the workspace
        assert torch.equal(none["rgb_f"], drawn["rgb_f"])
        old = OC.MAX_RAYS_PER_LAUNCH
        try:
            OC.MAX_RAYS_PER_LAUNCH = 100                               # three slabs of the 256 rays
            _, _, rgb_f, _ = NP.batchify_rays_and_render_by_chunk(r.rays[:, :3], r.rays[:, 3:], scene.packed, None, 800, 800, None, opts, seed=9,
                                                                  ray_offset=100, occupancy=grid)
        finally:
            OC.MAX_RAYS_PER_LAUNCH = old
        assert torch.equal(rgb_f, drawn["rgb_f"]) and grid.last_stats == drawn["_occ_stats"]


# ---------------------------------------------------------------------------------------------------
# bake, dilate, count
# ---------------------------------------------------------------------------------------------------
def lattice(grid, sub):
    """The bake lattice of the header as (rays [rows,6], z [rows,S]) in numpy fp32."""
    lo, hi, res = [f32(v) for v in grid.lo], [f32(v) for v in grid.hi], grid.res
    step = [(hi[i] - lo[i]) / f32(res[i] * sub) for i in range(3)]
    coord = [(lo[i] + ((np.arange(res[i] * sub).astype(f32) + f32(0.5)) * step[i]).astype(f32)).astype(f32) for i in range(3)]
    z = ((np.arange(res[0] * sub).astype(f32) + f32(0.5)) * step[0]).astype(f32)
    ny, nz = res[1] * sub, res[2] * sub
    rays = np.zeros((nz, ny, 6), f32)
    rays[..., 0] = lo[0]
    rays[..., 1] = coord[1][None, :]
    rays[..., 2] = coord[2][:, None]
    rays[..., 3] = 1.0
    return rays.reshape(-1, 6), np.broadcast_to(z, (ny * nz, len(z))).copy()


def cell_max_density(grid, sub, net, blob, flags):
    """[rz, ry, rx]: the largest raw density mi_nerf_mlp_rays* gives on a cell's sub^3 lattice points (a cell is occupied iff it exceeds sigma_min)."""
    rays, z = lattice(grid, sub)
    raw = ops.mlp_rays(net, blob, torch.from_numpy(rays).to(DEV), torch.from_numpy(z).to(DEV), bf16=flags.get("bf16", False), f16s=flags.get("f16s", False))
    rx, ry, rz = grid.res
    return raw[..., 3].reshape(rz, sub, ry, sub, rx, sub).amax(5).amax(3).amax(1)


@pytest.mark.parametrize("family,res,sub", [("fp32", (16, 12, 10), 2), ("fp32", (7, 5, 3), 3), ("bf16", (16, 12, 10), 1), ("f16s", (8, 8, 8), 4),
                                            ("fp32", (96, 96, 96), 2)])
def test_bake_equals_the_restatement(scene, family, res, sub):
    flags = FAMILY[family]
    net, blob_c, blob_f = scene.packed.kernel_blobs(ops.precision(**flags))
    grid = OC.OccupancyGrid(-1.5, (1.5, 1.2, 0.9), res)
    dens_c = cell_max_density(grid, sub, net, blob_c, flags)
    sigma = float(dens_c.median())                                   # a threshold that about half of the cells pass: both answers are exercised
    want_c = dens_c > sigma
    grid.bake(scene.packed, sub=sub, sigma_min=sigma, dilate=0, networks=("coarse",), **flags)
    got = unpack(grid.bits, res)
    print(f"\n[bake {family} {res} sub={sub}] occupied {grid.fraction():.3f}, differing cells {int((got != want_c.cpu()).sum())}")
    assert 0.02 < grid.fraction() < 0.98
    assert torch.equal(got, want_c.cpu())
    assert grid.count() == int(want_c.sum()) == int(np.unpackbits(grid.bits.cpu().numpy().view(np.uint8)).sum())
    if res[0] <= 16:                                                 # accumulate ORs: coarse, then fine into the same bits
        want_f = cell_max_density(grid, sub, net, blob_f, flags) > sigma
        grid.bake(scene.packed, sub=sub, sigma_min=sigma, dilate=0, networks=("coarse", "fine"), **flags)
        assert torch.equal(unpack(grid.bits, res), (want_c | want_f).cpu())
        grid.bake(scene.packed, sub=sub, sigma_min=sigma, dilate=0, networks=("fine",), **flags)
        assert torch.equal(unpack(grid.bits, res), want_f.cpu())     # accumulate == 0 clears first


@pytest.mark.parametrize("res", [(37, 21, 13), (64, 64, 64), (5, 1, 2)])
def test_dilate_and_count_equal_torch_restatements(res):
    grid = random_grid(res, -1.0, 1.0, True, seed=4, p=0.03)
    cells = unpack(grid.bits, res)
    assert grid.count() == int(cells.sum())
    for radius in (0, 1, 2):
        want = torch.nn.functional.max_pool3d(cells[None, None].float(), 2 * radius + 1, 1, radius)[0, 0] > 0
        out = grid.dilated(radius)
        assert torch.equal(unpack(out, res), want), radius
        assert np.array_equal(out.cpu().numpy().view(np.uint32), pack(want))      # the bits beyond the last cell stay 0
    # count ignores set bits beyond the last cell
    full = OC.OccupancyGrid(-1.0, 1.0, res).set_bits(np.full(grid.words, 0xFFFFFFFF, np.uint32)).to(DEV)
    assert full.count() == full.cells and full.fraction() == 1.0


# ---------------------------------------------------------------------------------------------------
# usefulness: a trained scene, held-out view with and without a baked grid
# ---------------------------------------------------------------------------------------------------
def test_trained_scene_heldout_psnr_with_a_baked_grid(tmp_path):
    """The synthetic scene of examples/train_eval_render.py (views of a fixed random NeRF), trained as the example trains it; bake with
    sigma_min=0, sub=2, dilate=1; the held-out view both ways with the same jitter.  PSNR against ground truth within 0.05 dB of the full
    render's; the evaluated share below 1 (no ratio is asserted)."""
    from nerf_pytorch_paeng_amd.model import NeRF, get_positional_encoder
    steps, views, H = int(os.environ.get("MI_NERF_OCC_TRAIN_STEPS", "600")), 12, 48
    W = H
    torch.manual_seed(0)
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=64, N_samples_f=128, perturb=1.0, chunk_rays=4096, chunk_pts=524288, data_type="blender",
                           gpu_ids=[0], rank=0, exp_name="occ", N_rays=1024, global_batch=True, idx_save=1 << 30, idx_print=1 << 30, precision="fp32")
    K800, _, _ = synthetic.lego_camera()
    K = np.array([[K800[0][0] * W / 800.0, 0, W / 2], [0, K800[1][1] * H / 800.0, H / 2], [0, 0, 1]])
    posenc = get_positional_encoder(10), get_positional_encoder(4)
    poses = harness.get_render_pose(n_angle=views + 2, phi=-30.0, nf=4.0)
    teacher = NeRF(8, 256, 63, 27).to(DEV)
    teacher.load_state_dict({k: torch.as_tensor(v) for k, v in synthetic.make_state_dict(77, 8, 256).items()})
    with torch.no_grad():
        images = torch.stack([harness._render_pose(teacher, posenc, K, poses[i].to(DEV), (H, W), opts)[0].reshape(H, W, 3) for i in range(views + 2)], 0)
    i_train, i_test = list(range(views)), [views]
    model = NeRF(8, 256, 63, 27, skips=[4]).to(DEV)
    optimizer = torch.optim.Adam(model.parameters(), lr=5e-4, betas=(0.9, 0.999))
    criterion = torch.nn.MSELoss()
    getter = harness.global_batch(images, K, poses, i_train, (H, W), DEV)
    for i in range(1, steps + 1):
        harness.train(i, i_train, images, (K, poses.numpy()), (H, W), model, criterion, posenc, optimizer, getter, None, opts)
    model.eval()
    packed = weights.packed_for(model)
    grid = OC.OccupancyGrid(-4.5, 4.5, 160).bake(packed, sub=2, sigma_min=0.0, dilate=1)     # holds every sample of every ray: cameras at radius 4, far 6

    def heldout(occupancy):
        NP.manual_seed(123)                                          # the same jitter both ways
        o = SimpleNamespace(**vars(opts), occupancy=occupancy)
        return harness.test(steps, i_test, posenc, packed, images[i_test], K, poses[i_test].to(DEV), (H, W), o)["psnr"][0]

    full, with_grid = heldout(None), heldout(grid)
    s = grid.last_stats
    share, padded = OC.evaluated_share(s), OC.padded_share(s)
    print(f"\n[trained, {steps} steps] held-out PSNR full {full:.3f} dB, with the grid {with_grid:.3f} dB; occupied cells {grid.fraction():.3f}, "
          f"evaluated share {share:.3f}, padded share {padded:.3f}")
    assert abs(with_grid - full) <= 0.05, (full, with_grid)
    assert share < 1.0, s
