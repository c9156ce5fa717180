"""The radiance grid on the GPU (include/mi_nerf_vox.h, nerf_pytorch_paeng_amd/baked.py) against the numpy restatement of the header's rule
(tests/vox_restate.py).  The bar is the project's: per output, e_hip <= max(4 e_ref, one ulp), e_hip the library's distance from the
float64 restatement, e_ref the float32 restatement's distance from it on the same case, one ulp that of the output's largest magnitude.
No ray is excluded.  Skipping changes no bit of any output but `visited`; early stopping stays within T_min; the projection, the skip
plane, a bake of a field with ground truth, a bake of a network and the plumbing (halves, streams, empty and nullable arguments, files,
the eval / video harness) follow."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import baked, harness, mesh, ops, scenes, synthetic, weights
from nerf_pytorch_paeng_amd._lib import MiNerfError
from tests import vox_restate as VR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32
OUTPUTS = ("rgb", "disp", "acc", "depth")
N_RAYS = (1, 7, 64, 257)


# ---------------------------------------------------------------------------------------------------
# grids and rays
# ---------------------------------------------------------------------------------------------------
def _blobs(P, rng, share_zero=0.6):
    """A field that is zero on about `share_zero` of the points, in blobs: coarse noise, repeated 3x per axis, cut at a quantile."""
    coarse = rng.normal(size=tuple(-(-p // 3) + 1 for p in P))
    fine = coarse.repeat(3, 0).repeat(3, 1).repeat(3, 2)[:P[0], :P[1], :P[2]]
    return fine > np.quantile(fine, share_zero)


GRID_SPECS = {
    "5x4x3": dict(res=(5, 4, 3), lo=(-1.0, -0.7, -0.5), hi=(0.9, 1.3, 0.8), seed=1, octant=False),
    "17x9x33": dict(res=(17, 9, 33), lo=(-1.1, -0.6, -1.0), hi=(1.0, 0.7, 1.2), seed=2, octant=False),
    "24^3 octant": dict(res=(24, 24, 24), lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), seed=3, octant=True),
}
_grids = {}


def grid_arrays(name, B):
    """(sigma [P_z,P_y,P_x], coef [P_z,P_y,P_x,R]) of a named grid, numpy fp32: sigma zero on about 60 % of the points, in blobs (the octant
    grid: all density where every index is in the lower half), random coefficients, zero padding."""
    spec = GRID_SPECS[name]
    rng = np.random.default_rng(spec["seed"])
    P = tuple(r + 1 for r in reversed(spec["res"]))
    mask = _blobs(P, rng)
    if spec["octant"]:
        keep = np.zeros(P, bool)
        keep[:P[0] // 2, :P[1] // 2, :P[2] // 2] = True
        mask = _blobs(P, rng, 0.3) & keep
    sigma = np.where(mask, rng.uniform(0.5, 12.0, P), 0.0).astype(f32)
    coef = np.zeros(P + (VR.record_floats(B),), f32)
    coef[..., :3 * B] = rng.normal(0.0, 0.8, P + (3 * B,))
    coef[..., :3] += f32(0.5 / VR.C0)                              # colours around 0.5, some beyond [0, 1]: the clamp is exercised
    return sigma, coef


def make_grid(name, B):
    """(RadianceGrid on the device, sigma, coef as numpy) -- built once per (name, B)."""
    if (name, B) not in _grids:
        spec = GRID_SPECS[name]
        sigma, coef = grid_arrays(name, B)
        g = baked.RadianceGrid(spec["lo"], spec["hi"], spec["res"], B).allocate(DEV)
        g.sigma.copy_(torch.from_numpy(sigma))
        g.coef.copy_(torch.from_numpy(coef))
        g.build_skip()
        _grids[(name, B)] = (g, sigma, coef)
    return _grids[(name, B)]


def make_rays(lo, hi, n, seed):
    """The first rays are one of each kind; random rays from outside, aimed into the box, follow."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rng = np.random.default_rng(seed)

    def towards(o, target, length=1.0):
        d = np.asarray(target) - np.asarray(o)
        return list(o) + list(d / np.linalg.norm(d) * length)

    special = [
        towards(c + (-3.0, 0.4, 0.7), c + 0.2 * h),                                    # entering from outside
        towards(c + 0.3 * h, c + (2.0, 1.0, -0.5)),                                      # origin inside the box
        [lo[0] - 1.0, c[1] + 0.3 * h[1], c[2] - 0.2 * h[2], 1.0, 0.0, 0.3],              # a direction component exactly 0, inside its slab
        [lo[0] - 1.0, hi[1] + 0.5, c[2], 1.0, 0.0, 0.3],                                 # ... outside its slab: a miss
        [lo[0] - 1.0, hi[1], c[2] + 0.1 * h[2], 1.0, 0.0, 0.0],                          # grazing a face: along the plane y = hi_y
        towards(c + (-3.0, 0.4, 0.7), c + (-6.0, 0.0, 0.0)),                             # a clean miss
        towards(c + (0.5, -3.0, 0.2), c - 0.3 * h, 0.5),                                 # |d| = 0.5
        towards(c + (0.3, 0.6, 3.0), c + 0.1 * h, 3.0),                                  # |d| = 3
        [np.nan, 0.0, 0.0, 1.0, 0.0, 0.0],                                               # a NaN ray
        list(c) + [0.0, 0.0, 0.0],                                                       # a zero direction
        [c[0], c[1], lo[2] - 2.0, 0.0, 0.0, 1.0],                                        # two zero components, straight up through the box
        towards(c + (3.0, 3.0, 3.0), hi - 1e-3 * h),                                     # clipping a corner: a short chord
    ]
    rows = special[:n]
    while len(rows) < n:
        v = rng.normal(size=3)
        o = c + v / np.linalg.norm(v) * rng.uniform(2.5, 3.5)
        rows.append(towards(o, c + rng.uniform(-0.9, 0.9, 3) * h, rng.choice([1.0, 1.0, 0.5, 2.0])))
    return np.asarray(rows, f32)


CFG = dict(near=0.3, far=3.2)                 # cuts the chords of rays that start inside (near) and of rays from distance 3 (far)
_cases = {}


def case(name, B):
    """Everything one (grid, B) case needs, computed once and left unchanged: 257 rays (the smaller ray sets are its prefixes), the float64
    and float32 restatements, the library's outputs with skipping off and on."""
    if (name, B) not in _cases:
        g, sigma, coef = make_grid(name, B)
        rays = make_rays(g.lo, g.hi, max(N_RAYS), 10 + B)
        step = 0.5 * g.cell_edge()
        ref64 = VR.render(g.lo, g.hi, g.res, B, sigma, coef, rays, step, CFG["near"], CFG["far"], dtype=np.float64)
        ref32 = VR.render(g.lo, g.hi, g.res, B, sigma, coef, rays, step, CFG["near"], CFG["far"], dtype=np.float32)
        _cases[(name, B)] = SimpleNamespace(grid=g, rays=rays, step=step, ref64=ref64, ref32=ref32)
    return _cases[(name, B)]


def run(g, rays, step, skip, T_min=0.0):
    out = g.render(torch.from_numpy(rays).to(DEV), step=step, near=CFG["near"], far=CFG["far"], T_min=T_min, skip=skip, visited=True)
    return {k: v.cpu().numpy() for k, v in zip(OUTPUTS + ("visited",), out)}


def bar(got, ref64, ref32):
    """(e_hip, e_ref, allowed) of one output."""
    e_hip = float(np.abs(got.astype(np.float64) - ref64).max())
    e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
    ulp = float(np.spacing(f32(np.abs(ref64).max())))
    return e_hip, e_ref, max(4.0 * e_ref, ulp)


# ---------------------------------------------------------------------------------------------------
# 1, 2. render against the restatement; skip on = skip off
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 4, 9))
@pytest.mark.parametrize("name", sorted(GRID_SPECS))
def test_render_meets_the_float64_restatement_and_skipping_changes_no_bit(name, B):
    c = case(name, B)
    assert np.isfinite(c.ref64["rgb"]).all() and (c.ref64["samples"] > 0).sum() >= 0.7 * len(c.rays) and (c.ref64["acc"] > 0.05).sum() >= 0.1 * len(c.rays)
    for n in N_RAYS:
        rays = c.rays[:n]
        off, on = run(c.grid, rays, c.step, False), run(c.grid, rays, c.step, True)
        for k in OUTPUTS:
            e_hip, e_ref, allowed = bar(off[k], c.ref64[k][:n], c.ref32[k][:n])
            print(f"\n[vox {name} B={B} n={n}] {k}: e_hip {e_hip:.3e}, e_ref {e_ref:.3e}, e_hip / e_ref {e_hip / e_ref if e_ref else float('nan'):.2f}, allowed {allowed:.3e}", end="")
            assert e_hip <= allowed, (name, B, n, k, e_hip, e_ref, allowed)
            assert np.array_equal(off[k].view(np.uint32), on[k].view(np.uint32)), (name, B, n, k)
        assert (on["visited"] <= off["visited"]).all()
        # with skipping off every sample is fetched; the fp32 count may differ from the float64 one by the last, truncated interval
        assert np.abs(off["visited"].astype(np.int64) - c.ref64["samples"][:n]).max() <= 1, (name, B, n)
    if name == "24^3 octant":
        assert on["visited"].sum() < off["visited"].sum()
        print(f"\n[vox {name} B={B}] visited: {int(on['visited'].sum())} with skipping, {int(off['visited'].sum())} without", end="")


def test_a_ray_through_empty_blocks_alone_fetches_nothing():
    """Density sits in the low octant; a ray along x at high y and z crosses three blocks, all empty with their margin."""
    g, sigma, _ = make_grid("24^3 octant", 4)
    assert sigma[14:, 14:, :].max() == 0 and g.skip.cpu().numpy()[2, 2, :].sum() == 0
    rays = np.array([[-3.0, 0.7, 0.7, 1.0, 0.0, 0.0], [-3.0, 0.62, 0.81, 1.0, 0.01, -0.01]], f32)
    step = 0.5 * g.cell_edge()
    off, on = run(g, rays, step, False), run(g, rays, step, True)
    assert (off["visited"] >= 28).all() and (on["visited"] == 0).all() and (on["visited"] < 2).all()      # t_far cuts the chord to 1.2: 29 samples in 2 blocks
    for k in OUTPUTS:
        assert np.array_equal(off[k].view(np.uint32), on[k].view(np.uint32)), k
    assert (on["rgb"] == 1.0).all() and not on["acc"].any()


# ---------------------------------------------------------------------------------------------------
# 3. early stop
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_min", (1e-2, 1e-3))
def test_early_stop_stays_within_T_min(T_min):
    c = case("17x9x33", 9)
    full = run(c.grid, c.rays, c.step, True)
    cut = run(c.grid, c.rays, c.step, True, T_min=T_min)
    for k in ("rgb", "acc"):
        _, _, allowed = bar(full[k], c.ref64[k], c.ref32[k])
        d = float(np.abs(cut[k].astype(np.float64) - full[k].astype(np.float64)).max())
        print(f"\n[vox early stop T_min={T_min}] {k}: max |diff| {d:.3e}", end="")
        assert d <= float(f32(T_min)) + allowed, (k, d)
    assert (cut["visited"] <= full["visited"]).all() and cut["visited"].sum() < full["visited"].sum()
    off = run(c.grid, c.rays, c.step, False, T_min=T_min)
    for k in OUTPUTS:
        assert np.array_equal(off[k].view(np.uint32), cut[k].view(np.uint32)), k


# ---------------------------------------------------------------------------------------------------
# 4. the projection
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 4, 9))
@pytest.mark.parametrize("many", (True, False))
def test_project_meets_the_float64_restatement(B, many):
    D, M = (32 if many else B), 1000
    rng = np.random.default_rng(20 + B)
    res = (11, 10, 9)
    N = 12 * 11 * 10
    raw = rng.uniform(-30.0, 30.0, (M, D, 4)).astype(f32)
    raw[rng.choice(M, 50, replace=False), 0, 3] = np.nan
    proj = baked.projection_matrix(D, B).astype(f32)
    index = rng.choice(N, M, replace=False).astype(np.int64)
    g = baked.RadianceGrid(-1.0, 1.0, res, B).allocate(DEV)
    g.sigma.fill_(-1.0)
    g.coef.fill_(7.0)
    g.project(torch.from_numpy(raw).to(DEV), torch.from_numpy(proj).to(DEV), torch.from_numpy(index).to(DEV))
    sigma, coef = g.sigma.cpu().numpy().reshape(-1), g.coef.cpu().numpy().reshape(N, -1)
    s64, r64 = VR.project(raw, proj, B, np.float64)
    _, r32 = VR.project(raw, proj, B, np.float32)
    assert np.array_equal(sigma[index].view(np.uint32), s64.view(np.uint32)) and (s64 >= 0).all() and (s64 == 0).sum() >= 50     # a max: exact
    e_hip, e_ref, allowed = bar(coef[index], r64, r32)
    print(f"\n[vox project B={B} D={D}] e_hip {e_hip:.3e}, e_ref {e_ref:.3e}, allowed {allowed:.3e}", end="")
    assert e_hip <= allowed, (e_hip, e_ref, allowed)
    assert not coef[index][:, 3 * B:].any()                                                                                     # padding exactly zero
    rest = np.setdiff1d(np.arange(N), index)
    assert (sigma[rest] == -1.0).all() and (coef[rest] == 7.0).all()                                                             # the others untouched
    # a caller that filled sigma itself: the records alone
    g.sigma.fill_(-2.0)
    g.project(torch.from_numpy(raw).to(DEV), torch.from_numpy(proj).to(DEV), torch.from_numpy(index).to(DEV), write_sigma=False)
    assert (g.sigma == -2.0).all() and np.array_equal(g.coef.cpu().numpy().reshape(N, -1), coef)


# ---------------------------------------------------------------------------------------------------
# 5. the skip plane
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", ((17, 9, 20), (8, 8, 8), (5, 4, 3), (24, 24, 24), (33, 16, 7), (65, 3, 9)))
def test_build_skip_equals_the_restatement(res):
    rng = np.random.default_rng(sum(res))
    P = tuple(r + 1 for r in reversed(res))
    fields = [np.zeros(P, f32), np.where(rng.uniform(size=P) < 0.004, 1.0, 0.0).astype(f32), np.where(_blobs(P, rng, 0.8), 2.0, 0.0).astype(f32)]
    face = np.zeros(P, f32)
    face[min(3, P[0] - 1), min(4, P[1] - 1), min(8, P[2] - 1)] = 1e-30              # one occupied point, on a block face where the lattice reaches it
    fields.append(face)
    g = baked.RadianceGrid(-1.0, 1.0, res, 1).allocate(DEV)
    for i, s in enumerate(fields):
        g.skip.fill_(9)
        g.sigma.copy_(torch.from_numpy(s))
        got = g.build_skip().skip.cpu().numpy()
        want = VR.build_skip(s, res)
        assert got.shape == want.shape and np.array_equal(got, want), (res, i, int((got != want).sum()))
    if res[0] > 8:
        assert want[0, 0, 0] == 1 and want[0, 0, 1] == 1 and want.sum() == 2             # the point on the face x = 8 sets both neighbours


# ---------------------------------------------------------------------------------------------------
# 6. a bake of a field with ground truth
# ---------------------------------------------------------------------------------------------------
def _psnr(a, b):
    return -10.0 * math.log10(float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def test_bake_of_a_solid_scene_renders_as_its_restatement_does():
    """The kernel's PSNR to the truth is within 0.05 dB of the float64 restatement's on the same grid.  The grid's own quality at this
    resolution is reported, not asserted.  Measured: see docs/design/22_radiance_grid.md."""
    scene = scenes.SolidScene.default()
    g = baked.bake_field(scene.field, -1.2, 1.2, 48, B=1, device=DEV)
    assert g.sigma.max() > 0 and float((g.sigma > 0).float().mean()) < 0.5
    H = W = 64
    K = scenes.scaled_camera((H, W))
    pose = torch.from_numpy(synthetic.pose_spherical(30.0, -30.0, 4.0)).to(DEV)
    o, d = ops.make_o_d(W, H, K, pose, DEV)
    rays = torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1).contiguous()
    truth = scene.render(rays, 2.0, 6.0)[0].cpu().numpy()
    got = g.render(rays)[0].cpu().numpy()
    ref = VR.render(g.lo, g.hi, g.res, 1, g.sigma.cpu().numpy(), g.coef.cpu().numpy(), rays.cpu().numpy(), 0.5 * g.cell_edge(), 0.0, math.inf)["rgb"]
    p_hip, p_ref = _psnr(got, truth), _psnr(ref, truth)
    print(f"\n[vox solid scene res 48 B=1, 64x64] PSNR to the truth: kernel {p_hip:.3f} dB, float64 restatement {p_ref:.3f} dB; "
          f"kernel to restatement max |diff| {np.abs(got - ref).max():.2e}", end="")
    assert abs(p_hip - p_ref) <= 0.05, (p_hip, p_ref)
    assert (truth.min(1) < 0.9).mean() > 0.1                       # the view shows the objects, not the background alone


def test_the_neighbours_shell_holds_the_mean_of_its_dense_neighbours():
    scene = scenes.SolidScene.default()
    a = baked.bake_field(scene.field, -1.2, 1.2, 20, B=4, device=DEV)
    b = baked.bake_field(scene.field, -1.2, 1.2, 20, B=4, device=DEV, shell="neighbours")
    sigma, ca, cb = a.sigma.cpu().numpy(), a.coef.cpu().numpy().astype(np.float64), b.coef.cpu().numpy()
    assert torch.equal(a.sigma, b.sigma) and torch.equal(a.skip, b.skip)
    dense = sigma > 0
    pad = np.pad(dense, 1)
    P = sigma.shape
    count = sum(pad[dz:dz + P[0], dy:dy + P[1], dx:dx + P[2]].astype(int) for dz in range(3) for dy in range(3) for dx in range(3))
    shell = ~dense & (count > 0)
    assert shell.sum() > 100 and np.array_equal(cb[~shell], ca[~shell].astype(f32))          # everything but the shell is as the field gave it
    cpad = np.pad(ca * dense[..., None], ((1, 1), (1, 1), (1, 1), (0, 0)))
    total = sum(cpad[dz:dz + P[0], dy:dy + P[1], dx:dx + P[2]] for dz in range(3) for dy in range(3) for dx in range(3))
    want = total[shell] / count[shell][:, None]
    assert np.abs(cb[shell] - want).max() <= 1e-5 * max(1.0, np.abs(want).max())                # fp32 sums of at most 26 records
    with pytest.raises(MiNerfError, match="shell"):
        baked.bake_field(scene.field, -1.2, 1.2, 20, B=4, device=DEV, shell="nearest")


# ---------------------------------------------------------------------------------------------------
# 7. a bake of a network
# ---------------------------------------------------------------------------------------------------
def test_bake_of_a_network_projects_the_networks_own_answers():
    sd = synthetic.make_state_dict(3, 4, 64)
    packed = weights.PackedNeRF.from_state_dict(sd, DEV)
    B, D, res = 9, 32, 12
    dens = mesh.density_lattice(packed, -1.0, 1.0, res)
    for sigma_min in (0.0, float(dens.flatten().kthvalue(int(0.9 * dens.numel()))[0])):
        g = baked.RadianceGrid(-1.0, 1.0, res, B).bake(packed, D=D, sigma_min=sigma_min)
        want_sigma = torch.where(dens > sigma_min, dens, torch.zeros_like(dens))
        assert torch.equal(g.sigma, want_sigma) and (sigma_min > 0 or torch.equal(g.sigma, torch.relu(dens)))
        active = torch.nn.functional.max_pool3d((want_sigma > 0).float()[None, None], 3, stride=1, padding=1)[0, 0] > 0
        index = torch.nonzero(active.reshape(-1)).reshape(-1)
        m = index.numel()
        assert 0 < m and (sigma_min == 0 or m < dens.numel())
        x = baked.lattice_positions(g.lo, g.hi, g.res, index)
        omega = torch.from_numpy(baked.fibonacci_directions(D).astype(f32)).to(DEV)
        rays = torch.cat([x[:, None, :].expand(m, D, 3), omega[None].expand(m, D, 3)], -1).reshape(m * D, 6).contiguous()
        _, net, blob = mesh._blob(packed, "fine", mesh.check_precision(None))
        raw = ops.mlp_rays(net, blob, rays, torch.zeros(m * D, 1, device=DEV)).reshape(m, D, 4).cpu().numpy()
        proj = baked.projection_matrix(D, B).astype(f32)
        _, r64 = VR.project(raw, proj, B, np.float64)
        _, r32 = VR.project(raw, proj, B, np.float32)
        coef = g.coef.reshape(-1, g.record_floats).cpu().numpy()
        e_hip, e_ref, allowed = bar(coef[index.cpu().numpy()], r64, r32)
        print(f"\n[vox network bake sigma_min={sigma_min:.3g}] {m} of {dens.numel()} points active; coef e_hip {e_hip:.3e}, e_ref {e_ref:.3e}, allowed {allowed:.3e}", end="")
        assert e_hip <= allowed, (e_hip, e_ref, allowed)
        assert not coef[~active.reshape(-1).cpu().numpy()].any()                       # inactive points keep zero records
        assert np.array_equal(g.skip.cpu().numpy(), VR.build_skip(g.sigma.cpu().numpy(), g.res))
        # the lattice positions are the header's: lo + j * step, each rounded once
        step = (f32(1.0) - f32(-1.0)) / f32(res)
        assert np.array_equal(x.cpu().numpy()[:, 0], (f32(-1.0) + ((index.cpu().numpy() % (res + 1)).astype(f32) * step).astype(f32)).astype(f32))


# ---------------------------------------------------------------------------------------------------
# 8. plumbing
# ---------------------------------------------------------------------------------------------------
def test_halves_streams_empty_and_nullable_arguments_files():
    c = case("17x9x33", 4)
    g = c.grid
    rays = torch.from_numpy(c.rays).to(DEV)
    whole = g.render(rays, step=c.step, visited=True)
    a, b = g.render(rays[:100].contiguous(), step=c.step, visited=True), g.render(rays[100:].contiguous(), step=c.step, visited=True)
    for w, x, y in zip(whole, a, b):
        assert torch.equal(w.view(torch.int32), torch.cat([x, y]).view(torch.int32))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = g.render(rays, step=c.step, visited=True)
    side.synchronize()
    for w, x in zip(whole, other):
        assert torch.equal(w.view(torch.int32), x.view(torch.int32))
    empty = g.render(torch.empty(0, 6, device=DEV), step=c.step)
    assert [tuple(t.shape) for t in empty] == [(0, 3), (0,), (0,), (0,)]
    alone = g.render(rays, step=c.step, want_all=False)
    assert isinstance(alone, torch.Tensor) and torch.equal(alone.view(torch.int32), whole[0].view(torch.int32))
    no_plane = g.render(rays, step=c.step, skip=False, want_all=False)
    assert torch.equal(no_plane.view(torch.int32), whole[0].view(torch.int32))
    with pytest.raises(MiNerfError):
        g.render(torch.from_numpy(c.rays), step=c.step)                               # a host tensor
    with pytest.raises(MiNerfError):
        g.render(rays[:, :5], step=c.step)
    with pytest.raises(MiNerfError, match="step"):
        g.render(rays, step=0.0)
    with pytest.raises(MiNerfError, match="samples per ray"):
        g.render(rays, step=1e-6)


def test_save_and_load_round_trip(tmp_path):
    c = case("5x4x3", 9)
    path = str(tmp_path / "grid.npz")
    c.grid.save(path)
    h = baked.RadianceGrid.load(path, DEV)
    assert (h.lo, h.hi, h.res, h.B) == (c.grid.lo, c.grid.hi, c.grid.res, c.grid.B) and h.nbytes == c.grid.nbytes
    assert torch.equal(h.sigma, c.grid.sigma) and torch.equal(h.coef, c.grid.coef) and torch.equal(h.skip, c.grid.skip)
    rays = torch.from_numpy(c.rays).to(DEV)
    for x, y in zip(h.render(rays, step=c.step), c.grid.render(rays, step=c.step)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_the_harness_renders_poses_from_the_grid_and_leaves_the_network_out(tmp_path):
    """opts.baked: harness.render and harness.test return the uint8 frames of RadianceGrid.render on make_o_d's rays and the PSNR against
    given images; the model they are handed is None, so any use of a network would raise."""
    from nerf_pytorch_paeng_amd.rays import make_o_d
    g, _, _ = make_grid("24^3 octant", 9)
    H, W = 20, 24
    K = scenes.scaled_camera((H, W))
    opts = SimpleNamespace(data_type="blender", n_angle=2, single_angle=-1, phi=-30.0, nf=4.0, exp_name="baked", baked=g, baked_T_min=1e-3)
    poses = harness.get_render_pose(n_angle=2, single_angle=-1, phi=-30.0, nf=4.0, device=DEV).float()
    want_rgb, want_disp, want_f = [], [], []
    for p in poses:
        o, d = make_o_d(W, H, K, p[:3, :4])
        rgb, disp, _, _ = g.render(torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1), T_min=1e-3)
        want_f.append(rgb)
        want_rgb.append(ops.to8b(rgb).reshape(H, W, 3).cpu().numpy())
        want_disp.append(ops.to8b(disp, ops.nanmax(disp)).reshape(H, W).cpu().numpy())
    rgbs, disps = harness.render(0, None, None, K, None, (H, W), opts, save_dir=str(tmp_path / "video"))
    assert rgbs.shape == (2, H, W, 3) and rgbs.dtype == np.uint8 and disps.shape == (2, H, W)
    for i in range(2):
        assert np.array_equal(rgbs[i], want_rgb[i]) and np.array_equal(disps[i], want_disp[i])
    assert (rgbs < 250).any() and (tmp_path / "video" / "1_rgb.png").exists()
    gt = torch.rand(2, H, W, 3, generator=torch.Generator().manual_seed(8)).to(DEV)
    res = harness.test(0, [0, 1], None, None, gt, K, poses, (H, W), opts, keep_frames=True)
    for i in range(2):
        mse = float(((want_f[i] - gt[i].reshape(-1, 3)) ** 2).mean())
        assert abs(res["psnr"][i] - (-10.0 * math.log10(mse))) <= 1e-3
        assert np.array_equal(res["frames"][i][0], want_rgb[i])
    # baked_step is honoured: a coarser march gives other frames
    coarse, _ = harness.render(0, None, None, K, None, (H, W), SimpleNamespace(**dict(vars(opts), baked_step=4.0 * g.cell_edge())))
    assert not np.array_equal(coarse, rgbs)
