"""LazyAdam (nerf_pytorch_paeng_amd/optim.py over mi_optim_adam_step_lazy) on the device: THE LAZY UPDATE of include/mi_nerf_optim.h.

THE COMPARATOR is tests/test_gpu_optim.py's, measured and never a literal: e_hip <= max(4 e_ref, ulp) per tensor and per quantity, with THE
ORACLE of tests/test_optim_lazy_cpu.py (torch.optim.Adam on the CPU, untouched elements put back after every step) in float64 as the oracle
and in float32 as the reference.  Everything that the rule states as an identity is compared bit for bit."""
import pytest
import torch

from nerf_pytorch_paeng_amd import baked, baked_train
from nerf_pytorch_paeng_amd.optim import FusedAdam, LazyAdam
from tests.test_gpu_optim import (CH, DEV, OFFSET_G, OFFSET_P, SHAPES, compare, device_params, make_grads, make_values, same_bits, set_grads,
                                  state_of)
from tests.test_optim_lazy_cpu import lazy_run

pytestmark = pytest.mark.gpu
ALL_SHAPES = SHAPES + [OFFSET_P, OFFSET_G]
OFF_P, OFF_G = (len(SHAPES),), (len(SHAPES) + 1,)
NAN = float("nan")


def lazy_dev_run(values, grads_per_step, offset_p=(), offset_g=(), groups=None, opt_state=None, **kw):
    ps = device_params(values, offset_p, offset_g)
    spec = ps if groups is None else [dict(params=[ps[i] for i in idx], **over) for idx, over in groups]
    opt = LazyAdam(spec, **kw)
    if opt_state is not None:
        opt.load_state_dict(opt_state)
    for grads in grads_per_step:
        set_grads(ps, grads, offset_g)
        opt.step()
    return ps, opt


def ibits(t):
    return t.detach().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------
# 1. where the predicate and the chunking can go wrong
# ---------------------------------------------------------------------------------------------------
def _keep(pattern, n):
    """Which elements of a flat tensor of n elements keep their gradient (the others get exactly zero)."""
    k = torch.zeros(n, dtype=torch.bool)
    if pattern == "scattered":
        k[:] = True                                           # make_grads' own zeros, one element in ten
    elif pattern == "all zero":
        pass
    elif pattern == "first element":
        k[:1] = True
    elif pattern == "last element":                           # the 1-3 element tail of (5,), (257,), (CH + 1,), (3 CH + 1,), (1029,), (517,) included
        k[-1:] = True
    elif pattern == "one in a 16-byte piece":                 # components 1, 2, 3, 0 of four pieces, in two waves and two chunks
        for i in (1, 4 * 70 + 2, 4 * 300 + 3, CH + 4 * 9):
            k[i:i + 1] = True
    elif pattern == "a wave's pieces zero beside a touched wave":   # threads 0-63 own elements 0-255 of a chunk's first quarter, threads 64-127 the next 256
        k[256:512] = True
        k[CH + 1024 + 512:CH + 1024 + 768] = True
    elif pattern == "chunk 0 zero, chunk 1 touched":
        k[CH:2 * CH] = True
    else:
        raise ValueError(pattern)
    return k


PATTERNS = ("scattered", "all zero", "first element", "last element", "one in a 16-byte piece", "a wave's pieces zero beside a touched wave",
            "chunk 0 zero, chunk 1 touched")


def pattern_grads(shapes, seed, pattern):
    return [g * _keep(pattern, g.numel()).view(g.shape) for g in make_grads(shapes, seed)]


@pytest.mark.parametrize("steps", [1, 20])
@pytest.mark.parametrize("pattern", PATTERNS + ("a different pattern on every step",))
def test_chunk_edges_and_gradient_patterns_against_the_oracle(pattern, steps):
    values = make_values(ALL_SHAPES, 1)
    if pattern in PATTERNS:
        grads = [pattern_grads(ALL_SHAPES, 100 + k, pattern) for k in range(steps)]
    else:
        grads = [pattern_grads(ALL_SHAPES, 100 + k, PATTERNS[(k + 2) % len(PATTERNS)]) for k in range(steps)]
    ref64 = state_of(*lazy_run(values, grads, torch.float64, lr=1e-3))
    ref32 = state_of(*lazy_run(values, grads, torch.float32, lr=1e-3))
    ps, opt = lazy_dev_run(values, grads, OFF_P, OFF_G, lr=1e-3)
    compare(f"{pattern}, {steps} step(s)", state_of(ps, opt), ref32, ref64)
    assert all(int(opt.state_dict()["state"][i]["step"]) == steps for i in range(len(ALL_SHAPES)))
    assert all(p.grad is None or not bool(p.grad.any()) for p in ps)                           # consumed


# ---------------------------------------------------------------------------------------------------
# 2. untouched means untouched
# ---------------------------------------------------------------------------------------------------
def test_untouched_elements_keep_every_bit_of_p_and_both_moments():
    values = make_values(ALL_SHAPES, 2)
    ps = device_params(values, OFF_P, OFF_G)
    opt = LazyAdam(ps, lr=1e-2, clamp_min=0.1)                 # a clamp that most elements violate: it must not reach an untouched one
    set_grads(ps, [torch.zeros_like(v) for v in values], OFF_G)
    opt.step()                                                 # lays the arenas out; moves nothing
    assert all(torch.equal(p.detach().cpu(), v) for p, v in zip(ps, values))
    g = torch.Generator().manual_seed(20)
    grads = make_grads(ALL_SHAPES, 21)                         # one element in ten is +0: most 16-byte pieces are mixed
    for i, (p, gr) in enumerate(zip(ps, grads)):
        st = opt.state[p]
        n = p.numel()
        st["exp_avg"].copy_((torch.randn(*p.shape, generator=g) * 0.1).to(DEV))
        st["exp_avg_sq"].copy_(torch.rand(*p.shape, generator=g).to(DEV))
        flat = gr.view(-1)
        flat[1::7] = -0.0                                      # a negative zero is untouched
        if n > 300:
            flat[256:300] = 0.0                                # a run of whole pieces
            with torch.no_grad():                              # untouched elements may hold anything: a NaN, an inf, a negative zero, a denormal
                for j, x in zip((257, 258, 259, 260), (NAN, float("inf"), -0.0, 1e-42)):
                    p.view(-1)[j] = x
                    st["exp_avg"].view(-1)[j] = x
    before = [tuple(ibits(t).clone() for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])) for p in ps]
    set_grads(ps, grads, OFF_G)
    opt.step()
    mixed = 0
    for p, gr, b in zip(ps, grads, before):
        if p.numel() == 0:
            continue
        un = (gr == 0).to(DEV)
        after = tuple(ibits(t) for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]))
        for a, b0 in zip(after, b):
            assert torch.equal(a[un], b0[un])
        if bool((~un).any()):
            assert bool((after[1][~un] != b[1][~un]).any()) and bool((p.detach()[~un] >= 0.1).all())     # the touched ones moved, and were clamped
        if p.data_ptr() % 16 == 0 and p.grad.data_ptr() % 16 == 0:
            piece = un.view(-1)[:p.numel() // 4 * 4].view(-1, 4)
            mixed += int((piece.any(1) & ~piece.all(1)).sum())
    assert mixed > 1000                                                                            # untouched beside touched in one 16-byte piece


# ---------------------------------------------------------------------------------------------------
# 3. all touched equals plain
# ---------------------------------------------------------------------------------------------------
def _nonzero_grads(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [(0.5 + torch.rand(*s, generator=g)) * torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0) * 1e-2 for s in shapes]


def test_with_every_element_touched_no_clamp_and_no_consume_the_bits_are_the_plain_steps():
    values = make_values(ALL_SHAPES, 3)
    grads = [_nonzero_grads(ALL_SHAPES, 300 + k) for k in range(5)]
    ps, opt = lazy_dev_run(values, grads, OFF_P, OFF_G, lr=1e-3, consume=False)
    qs = device_params(values, OFF_P, OFF_G)
    ref = FusedAdam(qs, lr=1e-3)
    for gs in grads:
        set_grads(qs, gs, OFF_G)
        ref.step()
    assert same_bits(state_of(ps, opt), state_of(qs, ref))


# ---------------------------------------------------------------------------------------------------
# 4. consume
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("consume", [True, False])
def test_consume_leaves_plus_zero_where_a_gradient_was_and_without_it_no_gradient_bit_changes(consume):
    values = make_values(ALL_SHAPES, 4)
    grads = make_grads(ALL_SHAPES, 400)
    for gr in grads:
        gr.view(-1)[2::9] = -0.0
    ps = device_params(values, OFF_P, OFF_G)
    opt = LazyAdam(ps, lr=1e-3, consume=consume)
    set_grads(ps, grads, OFF_G)
    before = [ibits(p.grad).clone() for p in ps]
    opt.step()
    for p, b in zip(ps, before):
        a = ibits(p.grad)
        if consume:
            was_zero = (b & 0x7fffffff) == 0
            assert bool(((a == 0) | was_zero).all()) and not bool(p.grad.any())      # (a -0 beside a touched element may have become +0)
        else:
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------
# 5. clamp
# ---------------------------------------------------------------------------------------------------
def test_clamp_lands_touched_elements_on_p_min_leaves_untouched_ones_and_keeps_a_nan():
    n = CH + 7
    v = torch.full((n,), 0.01)
    v[3], v[CH + 5] = -1.0, -1.0                               # below p_min already: one stays untouched, one is touched
    g = torch.zeros(n)
    g[0], g[5], g[CH + 5], g[CH + 6], g[9] = 1.0, -1.0, 1.0, 1.0, NAN
    # lr 0.1: the first Adam step moves a touched element by 0.1 against its gradient's sign
    ps, opt = lazy_dev_run([v, v.clone()], [[g, g.clone()]], groups=[((0,), dict(clamp_min=0.0)), ((1,), dict())], lr=0.1)
    p, q = ps[0].detach().cpu(), ps[1].detach().cpu()
    assert p[0] == 0.0 and p[CH + 5] == 0.0 and p[CH + 6] == 0.0 and ibits(p)[0] == 0           # sent below p_min: on p_min (+0)
    assert abs(float(p[5]) - 0.11) < 1e-6                                                       # moved up: not clamped
    assert p[3] == -1.0 and p[1] == 0.01                                                       # untouched, below p_min or not
    assert bool(torch.isnan(p[9])) and bool(torch.isnan(q[9]))
    assert abs(float(q[0]) + 0.09) < 1e-6 and abs(float(q[CH + 5]) + 1.1) < 1e-6 and q[3] == -1.0   # the group without a clamp
    ref = lazy_run([v, v.clone()], [[g, g.clone()]], torch.float32, clamp=[0.0, None], lr=0.1)
    for a, b in zip(state_of(ps, opt), state_of(*ref)):
        assert all(torch.equal(torch.isnan(x), torch.isnan(y)) for x, y in zip(a, b))
        assert torch.allclose(a[0].nan_to_num(), b[0].nan_to_num(), atol=1e-6)


# ---------------------------------------------------------------------------------------------------
# 6. determinism
# ---------------------------------------------------------------------------------------------------
def test_two_runs_and_a_side_stream_run_give_the_same_bits():
    shapes = [(5,), (CH + 1,), (3 * CH + 1,), OFFSET_G]
    values, grads = make_values(shapes, 6), [make_grads(shapes, 600 + k) for k in range(3)]
    want = state_of(*lazy_dev_run(values, grads, offset_g=(3,), lr=1e-3, clamp_min=-0.2))
    assert same_bits(state_of(*lazy_dev_run(values, grads, offset_g=(3,), lr=1e-3, clamp_min=-0.2)), want)
    ps = device_params(values)
    opt = LazyAdam(ps, lr=1e-3, clamp_min=-0.2)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    for gs in grads:
        set_grads(ps, gs, offset_g=(3,))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            opt.step()
        s.synchronize()
    assert same_bits(state_of(ps, opt), want)


# ---------------------------------------------------------------------------------------------------
# 7. drift: what the feature exists for
# ---------------------------------------------------------------------------------------------------
def test_a_region_that_no_gradient_reaches_any_more_stops_moving_and_under_torch_adam_it_does_not():
    n = 3 * CH + 1
    A, B = slice(10, 1500), slice(CH + 5, 2 * CH + 300)        # disjoint; both cross piece, wave and chunk borders
    values = make_values([(n,)], 7)
    grads = []
    for k in range(15):
        g = torch.zeros(n)
        region = A if k < 5 else B
        g[region] = _nonzero_grads([(n,)], 700 + k)[0][region]
        grads.append([g])
    ps, opt = lazy_dev_run(values, grads[:5], lr=1e-2)
    at5 = [t.clone() for t in state_of(ps, opt)[0]]
    for gs in grads[5:]:
        set_grads(ps, gs)
        opt.step()
    at15 = state_of(ps, opt)[0]
    for a, b in zip(at5, at15):
        assert torch.equal(ibits(a[A]), ibits(b[A]))                                             # region A: every bit of p, exp_avg, exp_avg_sq
    assert not torch.equal(at5[0][B], at15[0][B])                                                # region B moved
    # torch.optim.Adam on the CPU keeps pushing region A with its momentum: the assertion above is not vacuous
    q = torch.nn.Parameter(values[0].clone())
    ref = torch.optim.Adam([q], lr=1e-2, foreach=False)
    snap = None
    for k, gs in enumerate(grads):
        q.grad = gs[0].clone()
        ref.step()
        if k == 4:
            snap = q.detach().clone()
    assert bool((snap[A] != q.detach()[A]).all())
    assert int(opt.state_dict()["state"][0]["step"]) == 15


# ---------------------------------------------------------------------------------------------------
# 8. checkpoint interchange
# ---------------------------------------------------------------------------------------------------
def _cpu_state(sd):
    return {"state": {k: {kk: vv.cpu() for kk, vv in st.items()} for k, st in sd["state"].items()}, "param_groups": sd["param_groups"]}


def test_a_lazy_adam_state_dict_loads_into_torch_adam_and_back():
    shapes = [(5,), (257,), (CH + 1,), (37, 11), OFFSET_G]
    values = make_values(shapes, 8)
    grads = [make_grads(shapes, 800 + k) for k in range(11)]
    ref64 = state_of(*lazy_run(values, grads, torch.float64, lr=2e-3))
    ref32 = state_of(*lazy_run(values, grads, torch.float32, lr=2e-3))
    # here -> torch.optim.Adam (THE ORACLE steps one): the next step
    ps, opt = lazy_dev_run(values, grads[:10], offset_g=(4,), lr=2e-3)
    sd = opt.state_dict()
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 10.0 for st in sd["state"].values())
    mid = [p.detach().cpu() for p in ps]
    compare("10 here + 1 in torch", state_of(*lazy_run(mid, grads[10:], torch.float32, opt_state=_cpu_state(sd), lr=2e-3)), ref32, ref64)
    # torch.optim.Adam -> here
    ps_t, opt_t = lazy_run(values, grads[:10], torch.float32, lr=2e-3)
    ps, opt = lazy_dev_run([p.detach() for p in ps_t], grads[10:], offset_g=(4,), opt_state=opt_t.state_dict(), lr=2e-3, clamp_min=-5.0)
    compare("10 in torch + 1 here", state_of(ps, opt), ref32, ref64)
    assert all(float(st["step"]) == 11.0 for st in opt.state_dict()["state"].values())
    assert opt.param_groups[0]["clamp_min"] == -5.0                                              # a checkpoint without a clamp keeps the optimiser's
    # here -> FusedAdam -> here: the same bits as staying here
    ps1, opt1 = lazy_dev_run(values, grads[:10], lr=2e-3)
    mid_opt = FusedAdam(device_params([p.detach().cpu() for p in ps1]), lr=2e-3)
    mid_opt.load_state_dict(opt1.state_dict())
    ps2, opt2 = lazy_dev_run([p.detach().cpu() for p in ps1], grads[10:], opt_state=mid_opt.state_dict(), lr=2e-3)
    assert same_bits(state_of(ps2, opt2), state_of(*lazy_dev_run(values, grads, lr=2e-3)))


# ---------------------------------------------------------------------------------------------------
# 9. finetune's direct path: 24^3, B = 4, allocate(), skip=False, the 6 views of 32 x 32, 60 steps, seed 0 (tests/test_gpu_lattice_reg.py)
# ---------------------------------------------------------------------------------------------------
LR_SIGMA, STEPS = 0.5, 60


@pytest.fixture(scope="module")
def views():
    from tests.test_gpu_lattice_reg import _views
    return _views()


def _empty():
    return baked.RadianceGrid(-1.2, 1.2, 24, B=4).allocate(DEV)


def test_finetune_lazy_path_starts_where_adam_starts_learns_and_restores_the_grid(views):
    rays, target = views
    first = baked_train.finetune(_empty(), rays, target, steps=1, skip=False, lr_sigma=LR_SIGMA, seed=0)
    grid = _empty()
    losses = baked_train.finetune(grid, rays, target, steps=STEPS, skip=False, lr_sigma=LR_SIGMA, seed=0, optimizer=LazyAdam)
    assert losses.shape == (STEPS,) and bool(torch.isfinite(losses).all())
    assert torch.equal(ibits(losses[:1]), ibits(first))                                          # same draw, same render, same expression
    tenth = STEPS // 10
    head, tail = float(losses[:tenth].mean()), float(losses[-tenth:].mean())
    print(f"\n[finetune lazy, 24^3 B=4 from nothing, {STEPS} steps] data loss first / last tenth {head:.5f} / {tail:.5f}", end="")
    assert tail < head
    assert not grid.sigma.requires_grad and not grid.coef.requires_grad and grid.sigma.grad is None and grid.coef.grad is None
    assert bool((grid.sigma >= 0).all()) and bool((grid.sigma > 0).any())


def test_finetune_lazy_path_keeps_every_bit_of_the_half_of_the_grid_no_ray_reaches():
    """Rays that run along z at constant x in [-1.0, -0.1]: their samples interpolate lattice points of x index <= 12 (x = 0); with one cell of
    margin every element of x index >= 14 is out of reach.  That half is prefilled with values a dense sweep would alter: negative sigma (a
    clamp_ over the grid would zero it) and non-zero records."""
    g = torch.Generator().manual_seed(9)
    n = 2048
    o = torch.stack([-1.0 + 0.9 * torch.rand(n, generator=g), -1.0 + 2.0 * torch.rand(n, generator=g), torch.full((n,), 3.0)], -1)
    d = torch.nn.functional.normalize(torch.stack([torch.zeros(n), 0.2 * (torch.rand(n, generator=g) - 0.5), -torch.ones(n)], -1), dim=-1)
    rays = torch.cat([o, d], -1).contiguous().to(DEV)
    target = torch.rand(n, 3, generator=g).to(DEV)
    grid = _empty()
    far = slice(14, None)
    with torch.no_grad():
        grid.sigma[..., far] = -(0.1 + torch.rand(grid.sigma[..., far].shape, generator=g)).to(DEV)
        grid.coef[..., far, :] = torch.randn(grid.coef[..., far, :].shape, generator=g).to(DEV)
    s0, c0 = ibits(grid.sigma).clone(), ibits(grid.coef).clone()
    baked_train.finetune(grid, rays, target, steps=20, batch=1024, skip=False, lr_sigma=LR_SIGMA, seed=0, optimizer=LazyAdam)
    s1, c1 = ibits(grid.sigma), ibits(grid.coef)
    assert torch.equal(s1[..., far], s0[..., far]) and torch.equal(c1[..., far, :], c0[..., far, :])
    assert bool((s1[..., :13] != s0[..., :13]).any()) and bool((c1[..., :13, :] != c0[..., :13, :]).any())   # the reached half trained


def test_finetune_lazy_path_with_regularisers_finishes_with_finite_losses(views):
    rays, target = views
    grid = _empty()
    losses = baked_train.finetune(grid, rays, target, steps=STEPS, skip=False, lr_sigma=LR_SIGMA, seed=0, optimizer=LazyAdam, tv_sigma=0.01, sparsity=0.01)
    assert losses.shape == (STEPS,) and bool(torch.isfinite(losses).all()) and bool((grid.sigma >= 0).all())
    assert grid.sigma.grad is None and grid.coef.grad is None
