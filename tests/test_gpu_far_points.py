"""The fused encoders at far, edge-of-range and non-finite points.

Every fused MLP kernel computes gamma(x) in registers and branches ONCE per point: the Cody-Waite + Cephes reduction (sin_cos_fast) while
max|p| * 2^9 < SINCOS_FAST_LIMIT, the libm path (sin_cos_slow) beyond -- the bf16 kernel has no libm path and clamps instead.  The lego /
fern points of the other GPU tests reach 3e3 rad, so here the rays are placed AT the branch: about half the samples of every ray and of
every 16- / 32-sample tile on each side of it, one odd sample per tile, the exact edge, all fast (the control), all slow, and NaN / Inf.

The networks are COORDINATE-BLIND: the three raw-coordinate columns of linear_x.0 and of the skip layer's gamma(x) block are zero, so
|p| = 2000 does not drown the sinusoid channels -- raw stays O(1) and one wrong channel (a sin <-> cos swap, an error of 1e-3) moves it by
far more than any bar below.  The reference is float64: points in fp32 exactly as the reference computes them (o + d * z, the product
rounded, then the sum), gamma in float64 of those fp32 points, the network in float64.  e_ref is what the reference's own fp32 arithmetic
(R.embed + R.mlp_forward) is away from that, on the same inputs."""
import functools
import math

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import nerf_process as NP
from nerf_pytorch_paeng_amd import ops, synthetic, weights
from oracle import restate as R
from tests.test_f16_mode_cpu import mlp_forward_f16
from tests.test_gpu_f16 import f16_net_alone, launch_shape
from tests.test_gpu_parity import close, make_opts
from tests.test_gpu_train import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.from_numpy

LIMIT = 1048576.0            # SINCOS_FAST_LIMIT of nerf_pytorch_paeng_amd/csrc/common.h (2^20; 4e6 before this module existed)
EDGE = LIMIT / 512.0         # |coordinate| at which the top band's argument reaches the limit: exactly representable
L_X, L_D, IN_X, IN_D = 10, 4, 63, 27

#        tag       D    W  skip
NETS = {"d8w256": (8, 256, 4), "d4w128": (4, 128, 1), "d3w512": (3, 512, 0), "d3w384": (3, 384, -1), "d3w256": (3, 256, 0)}


@functools.lru_cache(maxsize=None)
def blind_net(tag):
    """(state dict, PackedNeRF, D, skips) of a coordinate-blind network: synthetic.make_state_dict with zero weights on the raw coordinates."""
    D, W, skip = NETS[tag]
    skips = (skip,) if skip >= 0 else ()
    sd = synthetic.make_state_dict(70 + D + W, D, W, skips=skips)
    for net in ("model_coarse.", "model_fine."):
        for layer in [0] + [s + 1 for s in skips if s + 1 < D]:            # the skip layer reads [gamma(x), h]: gamma(x) first
            w = sd[f"{net}linear_x.{layer}.weight"].copy()
            w[:, :3] = 0.0
            sd[f"{net}linear_x.{layer}.weight"] = w
    return sd, weights.PackedNeRF.from_state_dict(sd, DEV), D, skips


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def far_rays(arr, n, S, seed=0):
    """rays [n, 6], z [n, S] (CPU, fp32).  Per ray z = sorted(U[0.8, 1.2]) * scale * EDGE / max_c |d_c|: the largest coordinate of the
    ray's points runs from 0.8 to 1.2 x scale x EDGE (+- the origin, |o_c| <= 1)."""
    g = torch.Generator().manual_seed(1000 * seed + 37 * n + S)
    o = torch.rand(n, 3, generator=g) * 2 - 1
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    base = (EDGE / d.abs().max(-1)[0])[:, None]
    u = torch.sort(0.8 + 0.4 * torch.rand(n, S, generator=g), -1)[0]
    pos = torch.arange(S) % 32                                             # position inside the 32-sample tile
    if arr == "fast":
        z = u * 0.5 * base
    elif arr == "straddle":
        z = u * base
    elif arr == "slow":
        z = u * 1.3 * base
    elif arr.startswith("one_slow"):
        z = torch.where(pos == int(arr[8:]), 1.1 * base.expand(n, S), u * 0.5 * base)
    elif arr.startswith("one_fast"):
        z = torch.where(pos == int(arr[8:]), 0.5 * base.expand(n, S), u * 1.3 * base)
    elif arr == "log":                                                     # |p| from 1e2 to 1.2e4: knows no limit
        z = torch.sort(torch.exp(math.log(1e2) + math.log(1.2e2) * torch.rand(n, S, generator=g)), -1)[0] / d.abs().max(-1)[0][:, None]
    elif arr == "huge":                                                    # |p| from 1e6 to 1e30 (bf16: the clamp)
        z = torch.sort(torch.exp(math.log(1e6) + math.log(1e24) * torch.rand(n, S, generator=g)), -1)[0] / d.abs().max(-1)[0][:, None]
    elif arr == "edge":                                                    # o = 0, d = +-axis, z = EDGE (slow) and the float below it (fast)
        assert (n, S) == (6, 2)
        o = torch.zeros(6, 3)
        d = torch.cat([torch.eye(3), -torch.eye(3)])
        z = torch.tensor([EDGE, float(np.nextafter(np.float32(EDGE), np.float32(0)))]).expand(6, 2)
    else:
        raise ValueError(arr)
    return torch.cat([o, d], -1).contiguous(), z.contiguous().float()


def points(rays, z):
    return rays[:, None, :3] + rays[:, None, 3:] * z[..., None]            # fp32: product rounded, then the sum (nerf_process.py:69-70)


def is_slow(rays, z):
    """The kernels' branch, per point: not (max|p| * 2^9 < LIMIT)."""
    return ~(points(rays, z).abs().max(-1)[0] * 512.0 < LIMIT)


def check_arrangement(arr, rays, z):
    """The inputs are what they claim to be."""
    slow = is_slow(rays, z)
    n, S = z.shape
    tiles = [slow[:, t:t + 32] for t in range(0, S, 32)]
    if arr == "fast":
        assert not slow.any()
    elif arr == "slow":
        assert slow.all()
    elif arr == "straddle" and S >= 17:
        share = float(slow.float().mean())
        assert 0.3 <= share <= 0.7, share
        assert all(bool(r.any()) and not bool(r.all()) for r in slow)       # both sides on every ray
    elif arr.startswith("one_slow"):
        k = int(arr[8:])
        assert all(bool((t.sum(-1) == (1 if k < t.shape[1] else 0)).all()) for t in tiles) and bool(slow[:, k].all())
    elif arr.startswith("one_fast"):
        k = int(arr[8:])
        assert all(bool(((~t).sum(-1) == (1 if k < t.shape[1] else 0)).all()) for t in tiles) and not bool(slow[:, k].any())
    elif arr == "edge":
        assert bool(slow[:, 0].all()) and not bool(slow[:, 1].any())


def gamma64(rays, z):
    """[n*S, 90] float64: gamma in float64 of the fp32 points and of the fp32 unit view directions."""
    n, S = z.shape
    d = rays[:, 3:]
    view = d / torch.norm(d, dim=-1, keepdim=True)
    gx = R.posenc(points(rays, z).reshape(-1, 3).double(), L_X)
    gd = R.posenc(view[:, None, :].expand(n, S, 3).reshape(-1, 3).double(), L_D)
    return torch.cat([gx, gd], -1)


def oracle(tag, rays, z, taps=None, prefix="model_fine."):
    """(ref64 [n, S, 4], e_ref): the float64 network on gamma64, and how far the reference's own fp32 arithmetic is from it."""
    sd, _, D, skips = blind_net(tag)
    n, S = z.shape
    with torch.no_grad():
        ref64 = R.mlp_forward(sd, prefix, gamma64(rays, z), D, IN_X, IN_D, skips=skips, dtype=torch.float64, taps=taps).reshape(n, S, 4)
        ref32 = R.mlp_forward(sd, prefix, R.embed(rays, z, L_X, L_D), D, IN_X, IN_D, skips=skips).reshape(n, S, 4)
    return ref64, max_err(ref32, ref64)


def max_err(got, ref, mask=None):
    """max |got - ref| over the entries finite in ``ref``; the NaN placement must be the reference's exactly."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bad_g, bad_r = ~torch.isfinite(got), ~torch.isfinite(ref)
    assert torch.equal(bad_g, bad_r), ("non-finite placement", bad_g.nonzero()[:6].tolist(), bad_r.nonzero()[:6].tolist())
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    ok = ~bad_r if mask is None else (~bad_r & mask)
    return float((got - ref)[ok].abs().max()) if ok.any() else 0.0


def same_bits(a, b):
    a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    fa, fb = a.view(torch.float32), b.view(torch.float32)
    return torch.equal(torch.isnan(fa), torch.isnan(fb)) and torch.equal(a[~torch.isnan(fa)], b[~torch.isnan(fb)])


ODD = [f"one_{kind}{k}" for kind in ("slow", "fast") for k in (0, 15, 16, 31)]
#       arrangement, n, S
CASES = [("fast", 5, 33), ("straddle", 70, 96), ("straddle", 5, 17), ("straddle", 1, 1), ("straddle", 1, 48), ("slow", 5, 48), ("slow", 1, 33),
         ("edge", 6, 2), ("log", 70, 48)] + [(a, (5, 1, 5, 5)[i % 4], (96, 48, 33, 96)[i % 4]) for i, a in enumerate(ODD)]
BITE = [c for c in CASES if c[0] != "fast"]          # the cases that run the slow branch


# ---------------------------------------------------------------------------------------------------
# fp32 (W = 128 / 256) and wide (384 / 512) kernels
# ---------------------------------------------------------------------------------------------------
def check_fp32(tag, rays, z, what, singles=None, unfused=True):
    sd, packed, D, skips = blind_net(tag)
    n, S = z.shape
    rd, zd = rays.to(DEV), z.to(DEV)
    raw = ops.mlp_rays(packed.net, packed.fine, rd, zd)
    pick = list(range(n)) if singles is None else singles
    ref64, e_ref = oracle(tag, rays[pick], z[pick])
    e_gpu = max_err(raw[pick], ref64)
    print(f"fp32 {tag} {what} n={n} S={S}: |gpu-fp64| {e_gpu:.2e}  e_ref {e_ref:.2e}  raw scale {float(ref64[torch.isfinite(ref64)].abs().max()):.2f}")
    assert e_gpu <= max(4 * e_ref, 5e-5), (e_gpu, e_ref)
    for i in pick:                                                         # a ray alone (always the tile-major walk) == its rows in the batch
        one = ops.mlp_rays(packed.net, packed.fine, rd[i:i + 1].contiguous(), zd[i:i + 1].contiguous())
        assert same_bits(one[0], raw[i]), i
    if unfused:                                                            # embed kernel -> embedded-input kernel
        raw2 = ops.mlp_embedded(packed.net, packed.fine, ops.embed(rd, zd, L_X, L_D)).reshape(n, S, 4)
        fin = torch.isfinite(raw)
        assert torch.equal(fin, torch.isfinite(raw2))
        close(raw2[fin], raw[fin], 2e-4, 1e-4)
    return raw


@pytest.mark.parametrize("arr,n,S", CASES)
@pytest.mark.parametrize("tag", ["d4w128", "d8w256", "d3w384", "d3w512"])
def test_fp32_and_wide_kernels_at_the_branch(tag, arr, n, S):
    """ops.mlp_rays against float64 under the rule of test_mlp_rays_fused_vs_oracle, err <= max(4 e_ref, 5e-5); every ray alone equals
    its rows in the batch bit for bit; the unfused route within that test's 2e-4 / 1e-4."""
    rays, z = far_rays(arr, n, S)
    check_arrangement(arr, rays, z)
    check_fp32(tag, rays, z, arr)


@pytest.mark.parametrize("tag", ["d3w256", "d3w384", "d3w512"])
def test_ray_major_launch_at_the_branch(tag):
    """1500 rays x 33 samples: the ray-major walk (a wave keeps a ray's view-direction term across its chunks), half of every tile slow.
    The oracle and the single-ray identity on six picked rays, as test_mlp_rays_walks_agree does."""
    n, S = 1500, 33
    rays, z = far_rays("straddle", n, S)
    check_arrangement("straddle", rays, z)
    raw = check_fp32(tag, rays, z, "straddle, ray-major", singles=[0, 1, n // 3, n // 2 + 1, n - 2, n - 1])
    assert torch.isfinite(raw).all()


# ---------------------------------------------------------------------------------------------------
# training forward and backward
# ---------------------------------------------------------------------------------------------------
def train_blobs(tag, f16s, prefix="model_fine."):
    sd, _, D, skips = blind_net(tag)
    net = weights.infer_net(sd)
    fwd = ops.pack_module(sd, prefix, net, f16s=f16s).to(DEV)
    return sd, net, fwd


@pytest.mark.parametrize("tag,f16s,n,S", [("d4w128", False, 5, 48), ("d8w256", False, 70, 33), ("d8w256", True, 5, 48), ("d8w256", True, 70, 33)])
def test_training_forward_at_the_branch(tag, f16s, n, S):
    """The STASH instantiations: raw equals the inference kernel's bit for bit (as test_mlp_rays_walks_agree / test_mlp_backward_vs_autograd
    hold it), and the layer-0 rows of the activation stash -- W values per point, one matrix product behind the encodings -- equal relu of
    the oracle's float64 a0 tap under the family's rule."""
    sd, net, blob = train_blobs(tag, f16s)
    rays, z = far_rays("straddle", n, S, seed=1)
    check_arrangement("straddle", rays, z)
    rd, zd = rays.to(DEV), z.to(DEV)
    raw, stash = ops.mlp_rays_train(net, blob, rd, zd, f16s=f16s)
    assert torch.equal(raw, ops.mlp_rays(net, blob, rd, zd, f16s=f16s))
    taps64, taps32 = {}, {}
    D, skips = net.D, ((net.skip,) if net.skip >= 0 else ())
    with torch.no_grad():
        if f16s:
            ref64 = R.mlp_forward_f16split(sd, "model_fine.", gamma64(rays, z), D, IN_X, IN_D, skips=skips).reshape(n, S, 4)
        else:
            ref64 = None
        full64 = R.mlp_forward(sd, "model_fine.", gamma64(rays, z), D, IN_X, IN_D, skips=skips, dtype=torch.float64, taps=taps64).reshape(n, S, 4)
        full32 = R.mlp_forward(sd, "model_fine.", R.embed(rays, z, L_X, L_D), D, IN_X, IN_D, skips=skips, taps=taps32).reshape(n, S, 4)
    floor = 2e-5 if f16s else 5e-5
    e_ref = max_err(full32, full64)
    e_raw = max_err(raw, ref64 if f16s else full64)
    h0 = ops.train_views(net, n, S, stash=stash)["stash_h"][0]
    e_ref0 = max_err(torch.relu(taps32["a0"]), torch.relu(taps64["a0"]))
    e_h0 = max_err(h0, torch.relu(taps64["a0"]))
    print(f"training forward {tag} f16s={f16s} n={n} S={S}: raw {e_raw:.2e} (e_ref {e_ref:.2e}); stash_h[0] {e_h0:.2e} (e_ref {e_ref0:.2e})")
    assert e_raw <= max(4 * e_ref, floor), (e_raw, e_ref)
    assert e_h0 <= max(4 * e_ref0, floor), (e_h0, e_ref0)


@pytest.mark.parametrize("tag,f16s", [("d4w128", False), ("d8w256", True)])
def test_backward_at_the_branch(tag, f16s):
    """One backward case per path through the machinery of test_mlp_backward_vs_autograd (points whose ReLU signs differ between the two
    forwards get a zero output gradient on both sides): the gradient of linear_x.0.weight against float64 autograd under that test's 2e-4
    of the largest entry -- applied to the sinusoid columns [3:63] and to the raw columns [0:3] SEPARATELY: the raw columns' gradients are
    2000 times larger (they multiply the coordinates), and one maximum over the tensor would let them hide the encodings."""
    n, S, prefix = 10, 33, "model_coarse."
    sd, net, fwd = train_blobs(tag, f16s, prefix)
    D, skips = net.D, ((net.skip,) if net.skip >= 0 else ())
    packed = ops.pack_module(sd, prefix, net).to(DEV)
    packed_bwd = ops.pack_module(sd, prefix, net, backward=True, f16s=f16s).to(DEV)
    rays, z = far_rays("straddle", n, S, seed=2)
    check_arrangement("straddle", rays, z)
    d_raw = torch.randn(n, S, 4, generator=torch.Generator().manual_seed(5))
    rd, zd = rays.to(DEV), z.to(DEV)
    raw, stash = ops.mlp_rays_train(net, fwd, rd, zd, f16s=f16s)
    x64 = gamma64(rays, z)

    def autograd64(d_out):
        psd = {k: torch.as_tensor(v).double().requires_grad_(True) for k, v in sd.items() if k.startswith(prefix)}
        taps = {}
        out = R.mlp_forward(psd, prefix, x64, D, IN_X, IN_D, skips, dtype=torch.float64, taps=taps)
        (out * d_out.reshape(-1, 4).double()).sum().backward()
        return out.detach(), psd[prefix + "linear_x.0.weight"].grad, taps

    _, _, taps0 = autograd64(d_raw)
    v0 = ops.train_views(net, n, S, stash=stash)
    knife = ((v0["stash_g"].cpu() > 0) != (taps0["ad"].detach() > 0)).any(dim=1)
    for l in range(D):
        knife |= ((v0["stash_h"][l].cpu() > 0) != (taps0[f"a{l}"].detach() > 0)).any(dim=1)
    assert int(knife.sum()) <= max(3, n * S // 100), int(knife.sum())
    d_raw = (d_raw.reshape(-1, 4) * (~knife).float()[:, None]).reshape(n, S, 4).contiguous()
    raw_want, want, _ = autograd64(d_raw)
    assert rel_err(raw.reshape(-1, 4), raw_want) < 2e-5
    grads, _ = ops.mlp_backward(net, packed, packed_bwd, rd, zd, d_raw.to(DEV), stash, f16s_wgrad=f16s, f16s_dgrad=f16s)
    assert ops.param_names(net)[0] == "linear_x.0.weight"
    got = grads[:want.numel()].reshape(want.shape)
    e_sin, e_raw = rel_err(got[:, 3:63], want[:, 3:63]), rel_err(got[:, 0:3], want[:, 0:3])
    print(f"backward {tag} f16s={f16s}: d linear_x.0.weight sinusoid columns {e_sin:.2e} (max |g| {float(want[:, 3:].abs().max()):.2e}), "
          f"raw columns {e_raw:.2e} (max |g| {float(want[:, :3].abs().max()):.2e})")
    assert e_sin < 2e-4 and e_raw < 2e-4, (e_sin, e_raw)


# ---------------------------------------------------------------------------------------------------
# split precision (f16s) and f16
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arr,n,S", CASES)
def test_f16s_kernel_at_the_branch(arr, n, S):
    """mlp_rays_f16s against R.mlp_forward_f16split (its rounding points, float64 accumulation) on the float64 encodings: max(4 e_ref, 2e-5)."""
    tag = "d8w256"
    sd, packed, D, skips = blind_net(tag)
    rays, z = far_rays(arr, n, S)
    check_arrangement(arr, rays, z)
    got = ops.mlp_rays(packed.net, packed.f16s()[1], rays.to(DEV), z.to(DEV), f16s=True)
    with torch.no_grad():
        ref = R.mlp_forward_f16split(sd, "model_fine.", gamma64(rays, z), D, IN_X, IN_D, skips=skips).reshape(n, S, 4)
    _, e_ref = oracle(tag, rays, z)
    e_gpu = max_err(got, ref)
    print(f"f16s {arr} n={n} S={S}: |gpu - restatement| {e_gpu:.2e}  e_ref {e_ref:.2e}")
    assert e_gpu <= max(4 * e_ref, 2e-5), (e_gpu, e_ref)


def f16_oracles(tag, rays, z):
    sd, _, D, skips = blind_net(tag)
    n, S = z.shape
    with torch.no_grad():
        ref64 = mlp_forward_f16(sd, "model_fine.", gamma64(rays, z), D, IN_X, IN_D, skips=skips, dtype=torch.float64).reshape(n, S, 4)
        ref32 = mlp_forward_f16(sd, "model_fine.", R.embed(rays, z, L_X, L_D), D, IN_X, IN_D, skips=skips, dtype=torch.float32).reshape(n, S, 4)
    return ref64, max_err(ref32, ref64)


F16_BIG = [("straddle", 1100, 33)]                                         # > 100 rays (the two-phase 64 + 32 launch on 256 CUs): the D = 3 network


def test_f16_cases_run_both_launch_shapes():
    shapes = {launch_shape(n, S) for _, n, S in CASES + F16_BIG}
    assert "32" in shapes and shapes & {"64", "64+32"}, shapes


@pytest.mark.parametrize("arr,n,S", CASES + F16_BIG)
def test_f16_kernel_at_the_branch(arr, n, S):
    """MI_NERF_MODE_F16 through time_mlp_rays against mlp_forward_f16 under test_f16_network_vs_oracle's rule, max(4 e_ref, 2e-5) with e_ref the
    f16 oracle's own fp32 noise (rounding-boundary flips included); the small cases run the 32-point launch shape, the large one the 64-point shape as well."""
    tag = "d8w256" if n <= 100 else "d3w256"
    _, packed, _, _ = blind_net(tag)
    rays, z = far_rays(arr, n, S)
    check_arrangement(arr, rays, z)
    got = f16_net_alone(packed, rays.to(DEV), z.to(DEV))
    ref64, e_ref = f16_oracles(tag, rays, z)
    e_gpu = max_err(got, ref64)
    print(f"f16 {arr} n={n} S={S} ({launch_shape(n, S)}-point launch): |gpu - oracle64| {e_gpu:.2e}  e_ref {e_ref:.2e}")
    assert e_gpu <= max(4 * e_ref, 2e-5), (e_gpu, e_ref)


# ---------------------------------------------------------------------------------------------------
# bf16: accuracy where its reduction is in range, the stated contract beyond
# ---------------------------------------------------------------------------------------------------
def bf16_all_shapes(packed, rays, z):
    outs = [ops.mlp_rays(packed.net, packed.bf16()[1], rays.to(DEV), z.to(DEV), bf16=True, points_per_wave=ppw) for ppw in (0, 32, 64)]
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2])     # a point's arithmetic does not depend on the launch shape
    return outs[0].cpu()


def bf16_rule(raw16, ref16, rows):
    """test_fewer_encoding_frequencies' rule on the rows picked: mean |err| / mean |ref| per channel < 2e-3, max |err| < 0.2."""
    e = (raw16 - ref16).abs()[rows]
    rel = max(float(e[:, c].mean() / ref16[rows][:, c].abs().mean()) for c in range(4))
    return rel, float(e.max())


@pytest.mark.parametrize("arr,n,S", [("fast", 5, 33), ("fast", 70, 96), ("log", 70, 48)])
def test_bf16_kernel_below_the_limit(arr, n, S):
    sd, packed, D, skips = blind_net("d8w256")
    rays, z = far_rays(arr, n, S)
    check_arrangement(arr, rays, z)
    raw16 = bf16_all_shapes(packed, rays, z).reshape(-1, 4)
    assert torch.isfinite(raw16).all()
    with torch.no_grad():
        ref16 = R.mlp_forward_bf16(sd, "model_fine.", gamma64(rays, z).float(), D, IN_X, IN_D, skips=skips)
    rows = ~is_slow(rays, z).reshape(-1)                                    # the log-uniform family: its fast side
    assert int(rows.sum()) >= 100
    rel, emax = bf16_rule(raw16, ref16, rows)
    print(f"bf16 {arr} n={n} S={S}: {int(rows.sum())} points below the limit, mean |err| / mean |ref| {rel:.2e}, max |err| {emax:.3e}")
    assert rel < 2e-3 and emax < 0.2, (rel, emax)


def l1_bound(sd, prefix, D, skips, g=1.1):
    """Layer-wise l1 bound of |raw| (float64, bf16-rounded weights) for ANY encoding with |gamma| <= g on the channels that carry weight.
    g = 1.1: angle doubling multiplies the defect of s^2 + c^2 - 1 by at most 4 per octave (s' = 2 s c, c' = 1 - 2 s^2 give
    s'^2 + c'^2 - 1 = 4 s^2 (s^2 + c^2 - 1)); nine octaves from at most 6e-7 give 0.16, so |gamma| <= sqrt(1.16) < 1.08.  Each bf16
    rounding of an activation adds a factor 1 + 2^-8."""
    up = 1.0 + 2.0 ** -8
    wq = lambda name: R.bf16_round(torch.as_tensor(sd[f"{prefix}{name}.weight"]).float()).double().abs()
    b = lambda name: torch.as_tensor(sd[f"{prefix}{name}.bias"]).double().abs()
    W = wq("linear_feat").shape[0]
    h = torch.full((IN_X,), g, dtype=torch.float64)
    gx = h.clone()
    for i in range(D):
        h = (wq(f"linear_x.{i}") @ h + b(f"linear_x.{i}")) * up
        if i in skips:
            h = torch.cat([gx, h])
    sigma = wq("linear_density") @ h + b("linear_density")
    feat = (wq("linear_feat") @ h + b("linear_feat")) * up
    wd = torch.as_tensor(sd[f"{prefix}linear_d.weight"]).double().abs()
    wd[:, :W] = wq("linear_d")[:, :W]
    hd = (wd @ torch.cat([feat, torch.full((IN_D,), g, dtype=torch.float64)]) + b("linear_d")) * up
    rgb = wq("linear_color") @ hd + b("linear_color")
    return torch.cat([rgb, sigma]) * (1.0 + 1e-4)                          # fp32 accumulation


@pytest.mark.parametrize("arr,n,S", [("straddle", 70, 96), ("slow", 5, 48), ("huge", 70, 48), ("huge", 5, 17), ("one_slow16", 5, 33), ("edge", 6, 2)])
def test_bf16_contract_beyond_the_limit(arr, n, S):
    """The bf16 kernel has no libm path: it clamps the octave-0 remainder and doubles the angle.  Its contract beyond the limit: finite
    inputs give finite, BOUNDED encodings -- so raw is finite and inside the network's l1 bound for |gamma| <= 1.1 -- in every launch shape."""
    sd, packed, D, skips = blind_net("d8w256")
    rays, z = far_rays(arr, n, S)
    check_arrangement(arr, rays, z)
    assert torch.isfinite(points(rays, z)).all()
    raw16 = bf16_all_shapes(packed, rays, z)
    bound = l1_bound(sd, "model_fine.", D, skips)
    worst = (raw16.double().abs().reshape(-1, 4).max(0)[0] / bound)
    print(f"bf16 {arr} n={n} S={S}: max |raw| / l1 bound per channel {[f'{float(v):.3f}' for v in worst]} (bound {[f'{float(v):.1f}' for v in bound]})")
    assert torch.isfinite(raw16).all()
    assert bool((raw16.double().abs().reshape(-1, 4) <= bound).all()), worst


# ---------------------------------------------------------------------------------------------------
# non-finite inputs inside a batch of otherwise normal far rays
# ---------------------------------------------------------------------------------------------------
def poisoned_batch(arr):
    """5 rays x 33 samples: ray 1 has a NaN origin component, ray 3 a zero direction, sample (2, 16) an infinite depth."""
    rays, z = far_rays(arr, 5, 33, seed=3)
    rays[1, 1] = float("nan")
    rays[3, 3:] = 0.0
    z[2, 16] = float("inf")
    return rays, z


def check_placement(ref64):
    """What the reference does with these inputs (so the kernels are held to exactly this through max_err's NaN-placement check):
    the NaN-origin ray and the infinite-depth sample are NaN in all four outputs; the reference divides the zero direction by |d| = 0, so
    that ray's colours are NaN at every sample while its density, which does not see the direction, is finite."""
    nan = torch.isnan(ref64)
    assert bool(nan[1].all()) and bool(nan[2, 16].all()) and bool(nan[3, :, :3].all()) and not bool(nan[3, :, 3].any())
    nan[1] = False; nan[2, 16] = False; nan[3, :, :3] = False
    assert not bool(nan.any()) and bool(torch.isfinite(ref64[3, :, 3]).all())


@pytest.mark.parametrize("family", ["d4w128", "d8w256", "d3w384", "d3w512", "f16s", "f16", "bf16"])
def test_non_finite_points_stay_where_they_are(family):
    """One launch of 5 rays x 33 samples with a NaN origin component (ray 1), an infinite depth (sample (2, 16)) and a zero direction (ray 3):
    the NaN placement must be the float64 reference's exactly, every other output is held to the family's rule.

    This test found a defect: the ReLU of the fp32 / wide kernels (v_max_i32) and of the bf16 kernel (v_pk_max_i16) was an INTEGER maximum,
    which keeps a NaN whose sign bit is clear and turns one whose sign bit is set into 0 -- and 0 / 0 of the view direction is 0xffc00000
    on this device, as is what an infinite coordinate leaves behind.  The fp32 and wide kernels returned four finite numbers for the
    infinite-depth sample and 99 finite colours for the zero-direction ray, the bf16 kernel no NaN at all.  They now use the
    NaN-propagating maxima v_maximum3_f32 / v_pk_maximum3_f16 (mlp_core.h relu_pinned, mlp_half_core.h pack_stage), as the f16 / f16s
    kernels always did."""
    arr = "fast" if family == "bf16" else "straddle"
    rays, z = poisoned_batch(arr)
    rd, zd = rays.to(DEV), z.to(DEV)
    if family in NETS:
        ref64, e_ref = oracle(family, rays, z)
        check_placement(ref64)
        raw = check_fp32(family, rays, z, "non-finite")                    # oracle, single rays, unfused route
        assert bool(torch.isfinite(raw[3, :, 3]).all())
        return
    tag = "d8w256"
    sd, packed, D, skips = blind_net(tag)
    full64, e_ref = oracle(tag, rays, z)
    check_placement(full64)
    if family == "f16s":
        got = ops.mlp_rays(packed.net, packed.f16s()[1], rd, zd, f16s=True)
        with torch.no_grad():
            ref = R.mlp_forward_f16split(sd, "model_fine.", gamma64(rays, z), D, IN_X, IN_D, skips=skips).reshape(5, 33, 4)
        e = max_err(got, ref)
        print(f"f16s non-finite: {e:.2e} (e_ref {e_ref:.2e})")
        assert e <= max(4 * e_ref, 2e-5), (e, e_ref)
    elif family == "f16":
        got = f16_net_alone(packed, rd, zd)
        ref64, e16 = f16_oracles(tag, rays, z)
        e = max_err(got, ref64)
        print(f"f16 non-finite: {e:.2e} (e_ref {e16:.2e})")
        assert e <= max(4 * e16, 2e-5), (e, e16)
    else:
        got = bf16_all_shapes(packed, rays, z)
        with torch.no_grad():
            ref16 = R.mlp_forward_bf16(sd, "model_fine.", gamma64(rays, z).float(), D, IN_X, IN_D, skips=skips).reshape(5, 33, 4)
        max_err(got, ref16)                                                # the NaN placement
        good = torch.isfinite(ref16).all(-1).reshape(-1)
        rel, emax = bf16_rule(got.reshape(-1, 4), ref16.reshape(-1, 4), good)
        dens = float((got[3, :, 3] - ref16[3, :, 3]).abs().max())
        print(f"bf16 non-finite: mean |err| / mean |ref| {rel:.2e}, max |err| {emax:.3e}; zero-direction ray's density {dens:.3e}")
        assert rel < 2e-3 and emax < 0.2 and dens < 0.2, (rel, emax, dens)


# ---------------------------------------------------------------------------------------------------
# the stage kernels
# ---------------------------------------------------------------------------------------------------
def posenc_bars(arg):
    """Per channel, by its own argument (the stage kernels branch per channel): 3e-7 on the fast path, 2e-6 on the libm path -- the two
    bars of test_posenc_embed_F5."""
    return torch.where(arg.abs() < LIMIT, torch.tensor(3e-7, dtype=torch.float64), torch.tensor(2e-6, dtype=torch.float64))


def band_args(x, L):
    """[n, 3 + 6 L] the argument of every channel of gamma_L(x) (float64; the identity channels: 0)."""
    cols = [torch.zeros_like(x)]
    for k in range(L):
        cols += [x * 2.0 ** k, x * 2.0 ** k]
    return torch.cat(cols, -1)


@pytest.mark.parametrize("arr,n,S", [("straddle", 70, 96), ("straddle", 5, 17), ("one_slow0", 5, 96), ("one_slow31", 5, 33), ("one_fast15", 5, 48),
                                     ("one_fast16", 1, 33), ("edge", 6, 2)])
def test_embed_kernel_at_the_branch(arr, n, S):
    rays, z = far_rays(arr, n, S)
    emb = ops.embed(rays.to(DEV), z.to(DEV), L_X, L_D).cpu().double()
    want = gamma64(rays, z)
    assert torch.equal(emb[:, :3], want[:, :3])                            # the fp32 points themselves: no contraction
    d = (emb - want).abs()
    bars = posenc_bars(band_args(points(rays, z).reshape(-1, 3).double(), L_X))
    over = d[:, :IN_X] / bars
    print(f"embed {arr} n={n} S={S}: position channels max |err| {float(d[:, :IN_X].max()):.2e} (worst err / bar {float(over.max()):.2f}), "
          f"direction channels {float(d[:, IN_X:].max()):.2e}")
    assert float(over.max()) <= 1.0, float(over.max())
    assert float(d[:, IN_X:].max()) <= 5e-6


@pytest.mark.parametrize("decade", range(7))
def test_posenc_sweep(decade):
    """ops.posenc (L = 10) over 2e5 rows per decade of the TOP band's argument |x * 2^9| from 1 to 1e7, both signs (decade 0 also +-0),
    against float64: 3e-7 wherever the fast path is taken, 2e-6 on the libm path.  The lower bands cover the smaller arguments."""
    g = torch.Generator().manual_seed(decade)
    n = 200000
    mag = torch.exp(math.log(10.0 ** decade) + math.log(10.0) * torch.rand(n, 3, generator=g)) / 512.0
    x = (mag * (torch.randint(0, 2, (n, 3), generator=g) * 2 - 1)).float()
    if decade == 0:
        x[0] = torch.tensor([0.0, -0.0, 0.0]); x[1] = torch.tensor([-0.0, 0.0, -0.0])
    got = ops.posenc(x.to(DEV), L_X).cpu()
    xd = x.double()
    want = R.posenc(xd, L_X)
    assert torch.equal(got[:, :3], x) and torch.isfinite(got).all()
    d = (got.double() - want).abs()
    arg = band_args(xd, L_X)
    fast = arg.abs() < LIMIT
    e_fast = float(d[fast].max())
    e_libm = float(d[~fast].max()) if (~fast).any() else 0.0
    top = float(d[:, -6:].max())
    print(f"posenc sweep |x * 2^9| in [1e{decade}, 1e{decade + 1}): top band max |err| {top:.2e}; all bands: fast path {e_fast:.2e} "
          f"({int(fast.sum())} values), libm path {e_libm:.2e} ({int((~fast).sum())} values)")
    if decade == 0:
        assert bool((got[:2, 3:6] == 0.0).all()) and bool((got[:2, 6:9] == 1.0).all())
    assert e_fast <= 3e-7, e_fast
    assert e_libm <= 2e-6, e_libm


# ---------------------------------------------------------------------------------------------------
# one whole step
# ---------------------------------------------------------------------------------------------------
def test_whole_step_at_the_branch_fused_equals_staged():
    """fp32 render_rays with near / far = 0.8 / 1.2 x EDGE on 6 rays, 33 + 17 samples, injected uniforms: equal to the staged sequence of
    entry points bit for bit, as test_largest_sample_counts_fused_equals_staged holds it at lego depths."""
    n, Sc, Nf = 6, 33, 17
    _, packed, _, _ = blind_net("d4w128")
    g = torch.Generator().manual_seed(9)
    o = torch.rand(n, 3, generator=g) * 2 - 1
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    d = d / d.abs().max(-1)[0][:, None]                                    # the largest component is +-1: depth = largest coordinate
    rays = torch.cat([o, d], -1).contiguous().to(DEV)
    near, far = 0.8 * EDGE, 1.2 * EDGE
    t_rand, u = T(R.counter_uniform(1, 0, 0, n, Sc)).to(DEV), T(R.counter_uniform(1, 1, 0, n, Nf)).to(DEV)
    out = NP.render_rays(rays, packed, None, make_opts(near=near, far=far, N_samples_c=Sc, N_samples_f=Nf), t_rand=t_rand, u=u)
    z_c = ops.stratified_z(near, far, t_rand)
    slow = is_slow(rays.cpu(), z_c.cpu())
    assert bool(slow.any(-1).all()) and not bool(slow.all(-1).any())        # both branches on every ray
    rgb_c, disp_c, _, w_c, _ = ops.composite(ops.mlp_rays(packed.net, packed.coarse, rays, z_c), z_c, rays, want_all=True)
    z_f = ops.fine_z(z_c, w_c, Nf, False, u)
    rgb_f, disp_f, *_ = ops.composite(ops.mlp_rays(packed.net, packed.fine, rays, z_f), z_f, rays)
    assert torch.equal(out["rgb_c"], rgb_c) and torch.equal(out["disp_c"], disp_c)
    assert torch.equal(out["rgb_f"], rgb_f) and torch.equal(out["disp_f"], disp_f) and torch.isfinite(rgb_f).all()
