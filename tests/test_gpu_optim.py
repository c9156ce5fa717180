"""FusedAdam (nerf_pytorch_paeng_amd/optim.py over libmi_nerf_optim.so) on the device against torch.optim.Adam on the CPU.

THE COMPARATOR is measured, never a literal (the form tests/test_gpu_parity.py uses for the MLP): for the same inputs torch.optim.Adam
(foreach=False) runs on the CPU in float64 (the oracle) and in float32 (the reference).  Per tensor and separately for p, exp_avg and
exp_avg_sq, e_ref is the reference's max abs error against the oracle and the kernel must satisfy e_hip <= max(4 e_ref, ulp), ulp being one
float32 ulp of that tensor's largest magnitude in the oracle.  The pairs are printed."""
import io

import numpy as np
import pytest
import torch

from nerf_pytorch_paeng_amd import _optim
from nerf_pytorch_paeng_amd.optim import FusedAdam

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CH = _optim.CHUNK
MAXT = _optim.MAX_TENSORS
# where the chunking can go wrong: around the 16-byte vector, around a wave and a workgroup, around one, two and three chunks; nothing; 2-D
SHAPES = [(1,), (3,), (4,), (5,), (255,), (256,), (257,), (CH - 1,), (CH,), (CH + 1,), (2 * CH - 1,), (3 * CH + 1,), (0,), (37, 11)]
OFFSET_P, OFFSET_G = (1029,), (517,)         # a parameter that starts 4 bytes into its storage; one whose gradient alone does


def make_values(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) * 0.3 for s in shapes]


def make_grads(shapes, seed, scale=1.0):
    """Magnitudes spread over 1e-8 .. 1, both signs, one element in ten exactly zero (v = 0 meets eps)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in shapes:
        mag = 10.0 ** (-8.0 * torch.rand(*s, generator=g))
        sign = torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0)
        keep = (torch.rand(*s, generator=g) >= 0.1).float()
        out.append((mag * sign * keep * scale).float())
    return out


def torch_run(values, grads_per_step, dtype, cls=torch.optim.Adam, clip=None, groups=None, opt_state=None, **kw):
    """torch.optim.Adam (or AdamW) on the CPU in ``dtype``, single-tensor loop.  ``groups``: [(indices, overrides)]; ``clip``:
    clip_grad_norm_ before every step; ``opt_state``: a state dict to resume from.  -> (parameters, optimizer, norms)."""
    ps = [torch.nn.Parameter(v.to(dtype).clone()) for v in values]
    spec = ps if groups is None else [dict(params=[ps[i] for i in idx], **over) for idx, over in groups]
    opt = cls(spec, foreach=False, **kw)
    if opt_state is not None:
        opt.load_state_dict(opt_state)
    norms = []
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.to(dtype).clone()
        if clip is not None:
            norms.append(torch.nn.utils.clip_grad_norm_([p for p in ps if p.grad is not None], clip, foreach=False))
        opt.step()
    return ps, opt, norms


def state_of(ps, opt):
    """[(p, exp_avg, exp_avg_sq)] per parameter (None for one that never stepped)."""
    out = []
    for p in ps:
        st = opt.state.get(p, {})
        out.append((p.detach().cpu(), st["exp_avg"].detach().cpu(), st["exp_avg_sq"].detach().cpu()) if "exp_avg" in st else None)
    return out


def ulp_of(t):
    m = float(t.abs().max()) if t.numel() else 0.0
    return float(np.spacing(np.float32(m)))


def compare(what, hip, ref32, ref64):
    """THE COMPARATOR over every tensor and each of p / exp_avg / exp_avg_sq; prints the worst pair per quantity and asserts all."""
    worst = {}
    bad = []
    for i, (h, r32, r64) in enumerate(zip(hip, ref32, ref64)):
        assert (h is None) == (r64 is None), (what, i)
        if h is None or r64[0].numel() == 0:
            continue
        for name, a, b, c in zip(("p", "exp_avg", "exp_avg_sq"), h, r32, r64):
            e_hip, e_ref = float((a.double() - c).abs().max()), float((b.double() - c).abs().max())
            bound = max(4.0 * e_ref, ulp_of(c))
            if e_hip / bound >= worst.get(name, (0.0,))[0]:
                worst[name] = (e_hip / bound, e_hip, e_ref, i)
            if not e_hip <= bound:
                bad.append((name, i, tuple(c.shape), e_hip, e_ref, bound))
    print(f"{what}: " + "  ".join(f"{k}: e_hip {v[1]:.2e} e_ref {v[2]:.2e} ({v[0]:.2f} of the bound, tensor {v[3]})" for k, v in worst.items()))
    assert not bad, (what, bad)


def device_params(values, offset_p=(), offset_g=()):
    """Parameters on the device; those listed in ``offset_p`` are views that start 4 bytes into their storage, and ``offset_g`` names the
    ones whose gradients will be (see set_grads)."""
    ps = []
    for i, v in enumerate(values):
        if i in offset_p:
            base = torch.zeros(v.numel() + 1, device=DEV)
            base[1:] = v.reshape(-1).to(DEV)
            p = torch.nn.Parameter(base[1:].view(v.shape))
            assert p.data_ptr() % 16 == 4
        else:
            p = torch.nn.Parameter(v.to(DEV).clone())
        ps.append(p)
    return ps


def set_grads(ps, grads, offset_g=()):
    for i, (p, g) in enumerate(zip(ps, grads)):
        if g is None:
            p.grad = None
        elif i in offset_g:
            base = torch.zeros(g.numel() + 1, device=DEV)
            base[1:] = g.reshape(-1).to(DEV)
            p.grad = base[1:].view(g.shape)
            assert p.grad.data_ptr() % 16 == 4 and p.data_ptr() % 16 == 0
        else:
            p.grad = g.to(DEV).clone()


def fused_run(values, grads_per_step, offset_p=(), offset_g=(), groups=None, opt_state=None, **kw):
    ps = device_params(values, offset_p, offset_g)
    spec = ps if groups is None else [dict(params=[ps[i] for i in idx], **over) for idx, over in groups]
    opt = FusedAdam(spec, **kw)
    if opt_state is not None:
        opt.load_state_dict(opt_state)
    for grads in grads_per_step:
        set_grads(ps, grads, offset_g)
        opt.step()
    return ps, opt


def bits(state):
    return [None if s is None else tuple(t.clone() for t in s) for s in state]


def same_bits(a, b):
    return all((x is None and y is None) or all(torch.equal(s.view(torch.int32), t.view(torch.int32)) for s, t in zip(x, y)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------
# 1. shapes where the chunking can go wrong
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 20])
@pytest.mark.parametrize("mode", ["plain", "l2", "decoupled"])
def test_chunk_edges_views_and_zero_gradients_against_torch(mode, steps):
    shapes = SHAPES + [OFFSET_P, OFFSET_G]
    off_p, off_g = (len(SHAPES),), (len(SHAPES) + 1,)
    values = make_values(shapes, 1)
    grads = [make_grads(shapes, 100 + k) for k in range(steps)]
    kw = dict(lr=1e-3, weight_decay=0.0 if mode == "plain" else 1e-2)
    cls = torch.optim.AdamW if mode == "decoupled" else torch.optim.Adam
    ref64 = state_of(*torch_run(values, grads, torch.float64, cls, **kw)[:2])
    ref32 = state_of(*torch_run(values, grads, torch.float32, cls, **kw)[:2])
    ps, opt = fused_run(values, grads, off_p, off_g, decoupled_weight_decay=mode == "decoupled", **kw)
    compare(f"{mode}, {steps} step(s)", state_of(ps, opt), ref32, ref64)
    assert all(int(opt.state_dict()["state"][i]["step"]) == steps for i in range(len(shapes)))


# ---------------------------------------------------------------------------------------------------
# 2. more tensors than one launch holds
# ---------------------------------------------------------------------------------------------------
def test_more_tensors_than_one_launch_holds_are_each_updated_once():
    n = 2 * MAXT + 2
    shapes = [(1 + i % 7,) for i in range(n)]
    g = torch.Generator().manual_seed(200)
    values = make_values(shapes, 2)
    grads = [[(0.5 + torch.rand(*s, generator=g)) * torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0) for s in shapes]]   # none is zero
    ref64 = state_of(*torch_run(values, grads, torch.float64, lr=1e-2)[:2])
    ref32 = state_of(*torch_run(values, grads, torch.float32, lr=1e-2)[:2])
    for kw in (dict(), dict(max_grad_norm=1e9)):
        ps, opt = fused_run(values, grads, lr=1e-2, **kw)
        got = state_of(ps, opt)
        compare(f"{n} tensors {kw}", got, ref32, ref64)
        assert all(bool((g[0] != v).all()) for g, v in zip(got, values))                       # every tensor moved (once: the comparator)
        assert all(int(opt.state_dict()["state"][i]["step"]) == 1 for i in range(n))


# ---------------------------------------------------------------------------------------------------
# 3. PyTorch's bookkeeping
# ---------------------------------------------------------------------------------------------------
def test_grad_none_two_groups_zero_grad_and_version_counters():
    shapes = [(5,), (300,), (CH + 3,), (7, 3)]
    values = make_values(shapes, 3)
    g1, g2 = make_grads(shapes, 300), make_grads(shapes, 301)
    g1[1] = None                                                                               # no gradient in the first step
    groups = [((0, 1), dict(lr=1e-2)), ((2, 3), dict(lr=1e-4, betas=(0.8, 0.99)))]
    ref64 = state_of(*torch_run(values, [g1, g2], torch.float64, groups=groups)[:2])
    ref32 = state_of(*torch_run(values, [g1, g2], torch.float32, groups=groups)[:2])
    ps = device_params(values)
    opt = FusedAdam([dict(params=[ps[i] for i in idx], **over) for idx, over in groups])
    set_grads(ps, g1)
    v0 = [p._version for p in ps]
    opt.step()
    assert torch.equal(ps[1].detach().cpu(), values[1]) and ps[1] not in opt.state              # grad=None: its bits and its (absent) step
    v1 = [p._version for p in ps]
    assert [b > a for a, b in zip(v0, v1)] == [True, False, True, True]
    opt.zero_grad(set_to_none=False)
    assert all(p.grad is not None and not bool(p.grad.any()) for i, p in enumerate(ps) if i != 1)
    opt.zero_grad()
    assert all(p.grad is None for p in ps)
    before = [p.detach().clone() for p in ps]
    opt.step()                                                                                 # nothing has a gradient: nothing happens
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, ps)) and [p._version for p in ps] == v1
    set_grads(ps, g2)
    opt.step()
    assert all(p._version > v for p, v in zip(ps, v1))
    compare("two groups, grad=None", state_of(ps, opt), ref32, ref64)
    steps = [int(opt.state_dict()["state"][i]["step"]) for i in range(4)]
    assert steps == [2, 1, 2, 2], steps


@pytest.mark.parametrize("guarded", [False, True])
def test_a_group_added_after_the_first_step_keeps_the_state_of_the_others(guarded):
    """add_param_group lays the arenas out again: moments and step counts of the parameters that were there move with them."""
    shapes = [(5,), (CH + 1,), (300,)]
    values = make_values(shapes, 11)
    grads = [make_grads(shapes, 1100 + k) for k in range(3)]

    def run(make_params, cls, dtype, **kw):
        ps = make_params(dtype)
        opt = cls(ps[:2], lr=1e-3, **kw)
        for k, gs in enumerate(grads):
            if k == 1:
                opt.add_param_group({"params": [ps[2]], "lr": 1e-2})
            for p, g in zip(ps, gs):
                p.grad = g.to(device=p.device, dtype=dtype).clone()
            opt.step()
        return ps, opt
    cpu = lambda dtype: [torch.nn.Parameter(v.to(dtype).clone()) for v in values]              # noqa: E731
    ref64 = state_of(*run(cpu, torch.optim.Adam, torch.float64, foreach=False))
    ref32 = state_of(*run(cpu, torch.optim.Adam, torch.float32, foreach=False))
    ps, opt = run(lambda dtype: device_params(values), FusedAdam, torch.float32, **(dict(skip_nonfinite=True) if guarded else {}))
    compare("a group added after the first step", state_of(ps, opt), ref32, ref64)
    assert [int(opt.state_dict()["state"][i]["step"]) for i in range(3)] == [3, 3, 2]


# ---------------------------------------------------------------------------------------------------
# 4. the real set
# ---------------------------------------------------------------------------------------------------
def test_one_step_on_the_48_tensors_of_the_model_from_a_training_backward():
    from types import SimpleNamespace
    from nerf_pytorch_paeng_amd import synthetic, train_path
    from nerf_pytorch_paeng_amd.model import NeRF
    sd = synthetic.make_state_dict(0, 8, 256)
    model = NeRF(8, 256, 63, 27).to(DEV)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    params = list(model.parameters())
    assert len(params) == 48
    n, Sc, Nf = 32, 24, 24
    g = torch.Generator().manual_seed(0)
    o = torch.tensor([0.0, 0.0, 4.0]).expand(n, 3)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0]), dim=-1)
    rays = torch.cat([o, d], -1).contiguous().to(DEV)
    target = torch.rand(n, 3, generator=g).to(DEV)
    opts = SimpleNamespace(near=2.0, far=6.0, N_samples_c=Sc, N_samples_f=Nf, perturb=1.0)
    out = train_path.render_train(rays, model, opts, seed=0)
    (torch.mean((out["rgb_c"] - target) ** 2) + torch.mean((out["rgb_f"] - target) ** 2)).backward()
    values = [p.detach().cpu().clone() for p in params]
    grads = [[p.grad.detach().cpu().clone() for p in params]]
    assert all(bool(torch.isfinite(x).all()) for x in grads[0]) and sum(int(x.count_nonzero()) for x in grads[0]) > 1000
    ref64 = state_of(*torch_run(values, grads, torch.float64, lr=5e-4)[:2])
    ref32 = state_of(*torch_run(values, grads, torch.float32, lr=5e-4)[:2])
    opt = FusedAdam(params, lr=5e-4)
    opt.step()
    compare("NeRF(8, 256), 48 tensors", state_of(params, opt), ref32, ref64)


# ---------------------------------------------------------------------------------------------------
# 5. checkpoint interchange
# ---------------------------------------------------------------------------------------------------
INTERCHANGE_SHAPES = [(5,), (257,), (CH + 1,), (37, 11), OFFSET_G]


def _cpu_state(sd):
    return {"state": {k: {kk: vv.cpu() for kk, vv in st.items()} for k, st in sd["state"].items()}, "param_groups": sd["param_groups"]}


@pytest.mark.parametrize("guarded", [False, True])
def test_a_checkpoint_moves_between_fused_adam_and_torch_adam_both_ways(guarded):
    shapes = INTERCHANGE_SHAPES
    values = make_values(shapes, 5)
    grads = [make_grads(shapes, 500 + k) for k in range(20)]
    kw = dict(lr=2e-3, weight_decay=1e-3)
    extra = dict(skip_nonfinite=True) if guarded else {}
    ref64 = state_of(*torch_run(values, grads, torch.float64, **kw)[:2])
    ref32 = state_of(*torch_run(values, grads, torch.float32, **kw)[:2])
    # here -> torch
    ps, opt = fused_run(values, grads[:10], **kw, **extra)
    sd = opt.state_dict()
    assert set(sd["param_groups"][0]) == set(torch.optim.Adam([torch.zeros(1)]).state_dict()["param_groups"][0])
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 10.0 for st in sd["state"].values())
    mid = [p.detach().cpu() for p in ps]
    ps_t, opt_t, _ = torch_run(mid, grads[10:], torch.float32, opt_state=_cpu_state(sd), **kw)
    compare("10 here + 10 in torch", state_of(ps_t, opt_t), ref32, ref64)
    # torch -> here
    ps_t, opt_t, _ = torch_run(values, grads[:10], torch.float32, **kw)
    ps, opt = fused_run([p.detach() for p in ps_t], grads[10:], opt_state=opt_t.state_dict(), **kw, **extra)
    compare("10 in torch + 10 here", state_of(ps, opt), ref32, ref64)
    assert all(float(st["step"]) == 20.0 for st in opt.state_dict()["state"].values())
    # here -> here
    ps1, opt1 = fused_run(values, grads[:10], **kw, **extra)
    ps2, opt2 = fused_run([p.detach().cpu() for p in ps1], grads[10:], opt_state=opt1.state_dict(), **kw, **extra)
    ps3, opt3 = fused_run(values, grads, **kw, **extra)
    assert same_bits(state_of(ps2, opt2), state_of(ps3, opt3))
    # the clones: a saved state dict is as large as torch's, not one arena per tensor
    sizes = []
    for o in (opt3, torch_run(values, grads[:1], torch.float32, **kw)[1]):
        buf = io.BytesIO()
        torch.save(o.state_dict(), buf)
        sizes.append(buf.tell())
    print("saved bytes: FusedAdam", sizes[0], "torch.optim.Adam", sizes[1])
    assert sizes[0] <= 1.01 * sizes[1], sizes


# ---------------------------------------------------------------------------------------------------
# 6. - 8. the guarded step
# ---------------------------------------------------------------------------------------------------
def test_guarded_without_clipping_is_plain_bit_for_bit_and_its_norm_is_reproducible():
    shapes = SHAPES + [OFFSET_P, OFFSET_G]
    off_p, off_g = (len(SHAPES),), (len(SHAPES) + 1,)
    values = make_values(shapes, 6)
    grads = [make_grads(shapes, 600 + k) for k in range(3)]
    plain = state_of(*fused_run(values, grads, off_p, off_g, lr=1e-3, weight_decay=1e-2))
    ps, opt = fused_run(values, grads, off_p, off_g, lr=1e-3, weight_decay=1e-2, max_grad_norm=1e6, skip_nonfinite=True)
    assert same_bits(state_of(ps, opt), plain)                                                  # the coefficient clamps to exactly 1
    assert int(opt.skipped_steps) == 0
    # the norm of the last step against float64, bounded by what clip_grad_norm_ in float32 on the CPU itself is off by
    flat = [g.double() for g in grads[-1]]
    norm64 = float(torch.sqrt(sum((g * g).sum() for g in flat)))
    norm32 = float(torch_run(values, grads[-1:], torch.float32, clip=1e6)[2][0])
    e_hip, e_ref = abs(float(opt.last_grad_norm) - norm64), abs(norm32 - norm64)
    print(f"norm: float64 {norm64:.9e}  e_hip {e_hip:.2e}  e_ref {e_ref:.2e}")
    assert e_hip <= max(4 * e_ref, float(np.spacing(np.float32(norm64))))
    # two calls, identical bits
    ps2, opt2 = fused_run(values, grads, off_p, off_g, lr=1e-3, weight_decay=1e-2, max_grad_norm=1e6, skip_nonfinite=True)
    assert torch.equal(opt2.last_grad_norm.view(torch.int32), opt.last_grad_norm.view(torch.int32)) and same_bits(state_of(ps2, opt2), plain)


def test_guarded_clipping_follows_clip_grad_norm():
    shapes = SHAPES + [OFFSET_G]
    values = make_values(shapes, 7)
    grads = [make_grads(shapes, 700 + k) for k in range(4)]
    norm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads[0])))
    max_norm = norm / 10.0
    ref64 = state_of(*torch_run(values, grads, torch.float64, clip=max_norm, lr=1e-3)[:2])
    ref32 = state_of(*torch_run(values, grads, torch.float32, clip=max_norm, lr=1e-3)[:2])
    ps, opt = fused_run(values, grads, offset_g=(len(SHAPES),), lr=1e-3, max_grad_norm=max_norm)
    compare("clipped to a tenth of the norm", state_of(ps, opt), ref32, ref64)
    assert torch.equal(ps[4].grad.cpu(), grads[-1][4])                                          # the gradients themselves are not scaled


@pytest.mark.parametrize("where", ["inf in the first element of the first tensor", "nan in the last element of the last tensor"])
def test_guarded_skipping_leaves_every_word_and_the_step_count(where):
    shapes = [(CH + 1,), (300,), (2 * CH + 3,)]                                                 # the last element of the last tensor: the scalar tail
    values = make_values(shapes, 8)
    good = [make_grads(shapes, 800 + k) for k in range(3)]
    poisoned = [g.clone() for g in make_grads(shapes, 810)]
    if where.startswith("inf"):
        poisoned[0][0] = float("inf")
    else:
        poisoned[-1][-1] = float("nan")
    ps, opt = fused_run(values, good[:2], lr=1e-3, skip_nonfinite=True)
    before = bits(state_of(ps, opt))
    t_before = opt._tstate.clone()
    set_grads(ps, poisoned)
    opt.step()
    assert same_bits(state_of(ps, opt), before) and torch.equal(opt._tstate.view(torch.int32), t_before.view(torch.int32))
    assert int(opt.skipped_steps) == 1 and not np.isfinite(float(opt.last_grad_norm))
    assert all(float(st["step"]) == 2.0 for st in opt.state_dict()["state"].values())
    # a skipped FIRST step: the next finite step is the oracle's first
    ps, opt = fused_run(values, [poisoned], lr=1e-3, skip_nonfinite=True)
    assert all(torch.equal(p.detach().cpu(), v) for p, v in zip(ps, values)) and int(opt.skipped_steps) == 1
    set_grads(ps, good[0])
    opt.step()
    ref64 = state_of(*torch_run(values, good[:1], torch.float64, lr=1e-3)[:2])
    ref32 = state_of(*torch_run(values, good[:1], torch.float32, lr=1e-3)[:2])
    compare("the step after a skipped one", state_of(ps, opt), ref32, ref64)
    assert int(opt.skipped_steps) == 1 and all(float(st["step"]) == 1.0 for st in opt.state_dict()["state"].values())


def test_without_skip_nonfinite_a_nan_propagates_as_in_pytorch():
    shapes = [(CH + 1,), (300,)]
    values = make_values(shapes, 9)
    grads = make_grads(shapes, 900)
    grads[1][-1] = float("nan")
    ps_t, opt_t, _ = torch_run(values, [grads], torch.float32, lr=1e-3)
    ps, opt = fused_run(values, [grads], lr=1e-3)
    for a, b in zip(state_of(ps, opt), state_of(ps_t, opt_t)):
        assert all(torch.equal(torch.isnan(x), torch.isnan(y)) for x, y in zip(a, b))
    assert bool(torch.isnan(ps[1][-1])) and not bool(torch.isnan(ps[1][:-1]).any()) and not bool(torch.isnan(ps[0]).any())
    # with clipping the NaN norm makes every gradient NaN, as clip_grad_norm_ does
    ps_t, opt_t, _ = torch_run(values, [grads], torch.float32, clip=1.0, lr=1e-3)
    ps, opt = fused_run(values, [grads], lr=1e-3, max_grad_norm=1.0)
    assert all(bool(torch.isnan(p).all()) for p in ps_t) and all(bool(torch.isnan(p).all()) for p in ps)


# ---------------------------------------------------------------------------------------------------
# 9. side stream
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guarded", [False, True])
def test_a_step_on_a_side_stream_gives_the_bits_of_the_default_stream(guarded):
    shapes = [(5,), (CH + 1,), (3 * CH + 1,), OFFSET_G]
    values, grads = make_values(shapes, 10), [make_grads(shapes, 1000)]
    kw = dict(lr=1e-3, max_grad_norm=0.5) if guarded else dict(lr=1e-3)
    want = state_of(*fused_run(values, grads, offset_g=(3,), **kw))
    ps = device_params(values)
    opt = FusedAdam(ps, **kw)
    set_grads(ps, grads[0], offset_g=(3,))
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        opt.step()
    s.synchronize()
    assert same_bits(state_of(ps, opt), want)
