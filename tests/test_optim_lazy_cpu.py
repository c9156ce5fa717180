"""THE LAZY UPDATE (include/mi_nerf_optim.h: mi_optim_adam_step_lazy, nerf_pytorch_paeng_amd/optim.py: LazyAdam) without a GPU: the entry is
declared, bound and exported at ABI 2; every refusal answers MI_OPTIM_EINVAL with a message before any HIP call; a C99 program links against
it; LazyAdam refuses host tensors and a weight decay; and THE ORACLE that tests/test_gpu_optim_lazy.py compares the kernel with is itself
checked here.

THE ORACLE (``lazy_run``): torch.optim.Adam(foreach=False) stepped on the full tensor; after each step p, exp_avg and exp_avg_sq are put back
to their pre-step values wherever g == 0 (so -0.0 is untouched and NaN is touched), and the clamp is applied to the touched elements."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

from tests.test_optim_cpu import EINVAL, GOOD, INF, NAN, ROOT, _arr, optim_lib  # noqa: F401  (optim_lib is a fixture)


# ---------------------------------------------------------------------------------------------------
# THE ORACLE
# ---------------------------------------------------------------------------------------------------
def lazy_run(values, grads_per_step, dtype, clamp=None, opt_state=None, **kw):
    """THE ORACLE in ``dtype`` on the CPU.  ``clamp``: None, one number, or one per tensor (None: that tensor is not clamped).
    -> (parameters, optimizer)."""
    ps = [torch.nn.Parameter(v.to(dtype).clone()) for v in values]
    lows = clamp if isinstance(clamp, (list, tuple)) else [clamp] * len(ps)
    opt = torch.optim.Adam(ps, foreach=False, **kw)
    if opt_state is not None:
        opt.load_state_dict(opt_state)
    for grads in grads_per_step:
        before = []
        for p, g in zip(ps, grads):
            p.grad = g.to(dtype).clone()
            st = opt.state.get(p, {})
            zero = torch.zeros_like(p)
            before.append((p.detach().clone(), st["exp_avg"].clone() if "exp_avg" in st else zero, st["exp_avg_sq"].clone() if "exp_avg_sq" in st else zero.clone()))
        opt.step()
        with torch.no_grad():
            for p, g, (p0, m0, v0), lo in zip(ps, grads, before, lows):
                un = g.to(dtype) == 0
                st = opt.state[p]
                if lo is not None:
                    p.copy_(torch.where(p < lo, torch.full_like(p, lo), p))      # a NaN compares false and stays
                p.copy_(torch.where(un, p0, p))
                st["exp_avg"].copy_(torch.where(un, m0, st["exp_avg"]))
                st["exp_avg_sq"].copy_(torch.where(un, v0, st["exp_avg_sq"]))
    return ps, opt


def _moments(ps, opt):
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps]


def test_the_oracle_with_no_zero_gradient_is_torch_adam_exactly_in_float64():
    g = torch.Generator().manual_seed(0)
    values = [torch.randn(7, generator=g), torch.randn(33, 3, generator=g)]
    grads = [[(0.5 + torch.rand(*v.shape, generator=g)) * torch.where(torch.rand(*v.shape, generator=g) < 0.5, -1.0, 1.0) for v in values] for _ in range(6)]
    assert all(bool((x != 0).all()) for step in grads for x in step)
    ps, opt = lazy_run(values, grads, torch.float64, lr=1e-2)
    qs = [torch.nn.Parameter(v.double().clone()) for v in values]
    ref = torch.optim.Adam(qs, foreach=False, lr=1e-2)
    for step in grads:
        for q, x in zip(qs, step):
            q.grad = x.double().clone()
        ref.step()
    for a, b in zip(_moments(ps, opt), _moments(qs, ref)):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_the_oracle_on_mixed_gradients_an_element_touched_on_steps_1_and_3_depends_on_those_two_gradients_alone():
    b1, b2, lr, eps = 0.9, 0.999, 1e-2, 1e-8
    g1, g3, p0 = 0.7, -0.2, 0.25

    def run(seed):
        g = torch.Generator().manual_seed(seed)
        grads = [torch.randn(5, generator=g).double() for _ in range(3)]        # the other elements: anything
        grads[0][2], grads[1][2], grads[2][2] = g1, 0.0, g3
        grads[1][4] = -0.0                                                      # and a negative zero is a zero
        ps, opt = lazy_run([torch.full((5,), p0)], [[x] for x in grads], torch.float64, lr=lr, betas=(b1, b2), eps=eps)
        return _moments(ps, opt)[0], grads
    (p, m, v), grads = run(1)
    (p_, m_, v_), _ = run(2)
    assert p[2] == p_[2] and m[2] == m_[2] and v[2] == v_[2]                    # whatever the neighbours saw
    m1, v1 = (1 - b1) * g1, (1 - b2) * g1 * g1
    x1 = p0 - lr / (1 - b1) * m1 / (v1 ** 0.5 / (1 - b2) ** 0.5 + eps)
    m3, v3 = b1 * m1 + (1 - b1) * g3, b2 * v1 + (1 - b2) * g3 * g3              # no decay for the skipped step 2 ...
    x3 = x1 - lr / (1 - b1 ** 3) * m3 / (v3 ** 0.5 / (1 - b2 ** 3) ** 0.5 + eps)  # ... and the bias corrections of the TENSOR's step 3
    for got, want in ((m[2], m3), (v[2], v3), (p[2], x3)):
        assert abs(float(got) - want) <= 1e-12 * abs(want), (float(got), want)
    # the element with the negative zero on step 2 moved on steps 1 and 3 only as well
    q = torch.nn.Parameter(torch.full((5,), p0, dtype=torch.float64))
    ref = torch.optim.Adam([q], foreach=False, lr=lr, betas=(b1, b2), eps=eps)
    for x in grads:
        q.grad = x.clone()
        ref.step()
    assert m[4] != ref.state[q]["exp_avg"][4] and m[0] == ref.state[q]["exp_avg"][0]   # plain Adam decayed it on step 2; an always-touched element agrees


def test_the_oracle_clamps_touched_elements_only_and_keeps_a_nan():
    values = [torch.tensor([-1.0, 0.5, -1.0, 0.0])]
    grads = [[torch.tensor([0.0, 1.0, 1.0, NAN])]]
    ps, _ = lazy_run(values, grads, torch.float64, clamp=0.0, lr=1.0)
    p = ps[0].detach()
    assert p[0] == -1.0 and p[1] == 0.0 and p[2] == 0.0 and bool(torch.isnan(p[3]))


# ---------------------------------------------------------------------------------------------------
# the entry
# ---------------------------------------------------------------------------------------------------
def test_the_lazy_entry_is_declared_bound_and_exported_at_abi_2(optim_lib):
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_optim.h")).read()
    assert "THE LAZY UPDATE" in hdr and "int mi_optim_adam_step_lazy(" in hdr
    assert optim_lib.ABI_VERSION == 2 and optim_lib.lib().mi_optim_abi_version() == 2
    assert "mi_optim_adam_step_lazy" in optim_lib.SIGNATURES
    assert "mi_optim_adam_step_lazy" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", optim_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T mi_optim_adam_step_lazy" in out


LAZY_GOOD = dict(GOOD, p_min=[0.0, -INF, 0.0], consume=1)
LAZY_REFUSALS = {
    "weight_decay 0.01": dict(wd=0.01),
    "consume 2": dict(consume=2),
    "consume negative": dict(consume=-1),
    "NaN p_min": dict(p_min=[0.0, NAN, 0.0]),
    "n 0": dict(n=0),
    "n negative": dict(n=-1),
    "NULL params array": dict(params=None),
    "NULL grads array": dict(grads=None),
    "NULL numel array": dict(numel=None),
    "NULL state_off array": dict(off=None),
    "NULL step array": dict(step=None),
    "NULL cfgs": dict(n_cfg=0),
    "NULL pointer inside grads": dict(grads=[None, 0x50004, 0x60000]),
    "NULL exp_avg": dict(m=None),
    "step 0": dict(step=[1, 0, 7]),
    "step negative": dict(step=[-3, 1, 7]),
    "moments outside the arenas": dict(state_numel=4104),
    "config size": dict(size=48),
}


def _call_lazy(mod, a):
    cfg = mod.AdamCfg(size=C.sizeof(mod.AdamCfg) if a["size"] is None else a["size"], decoupled=a["decoupled"], lr=a["lr"], beta1=a["beta1"],
                      beta2=a["beta2"], eps=a["eps"], weight_decay=a["wd"])
    cfgs = (mod.AdamCfg * 1)(cfg) if a["n_cfg"] else None
    rc = mod.lib().mi_optim_adam_step_lazy(a["n"], _arr(C.c_void_p, a["params"]), _arr(C.c_void_p, a["grads"]), _arr(C.c_int64, a["numel"]),
                                           _arr(C.c_int64, a["off"]), _arr(C.c_int64, a["step"]), a["m"], a["v"], a["state_numel"], cfgs, a["n_cfg"],
                                           _arr(C.c_int32, a["cfg_of"]), _arr(C.c_float, a["p_min"]), a["consume"], None)
    return rc, mod.last_error()


@pytest.mark.parametrize("case", sorted(LAZY_REFUSALS))
def test_lazy_refusals_answer_einval_with_a_message_before_any_hip_call(optim_lib, case):
    rc, msg = _call_lazy(optim_lib, dict(LAZY_GOOD, **LAZY_REFUSALS[case]))
    assert rc == EINVAL, (case, rc, msg)
    assert msg and "mi_optim_adam_step_lazy" in msg and "HIP error" not in msg, (case, msg)


def test_the_good_arguments_of_the_lazy_refusal_table_reach_the_device(optim_lib):
    """The base case, with and without a clamp array, is refused by nothing: it gets as far as its first launch, which fails here for want of a
    device -- so every refusal above is owed to its one override."""
    if torch.cuda.is_available():
        pytest.skip("made-up addresses must not reach a real device")
    for over in (dict(), dict(p_min=None), dict(consume=0)):
        rc, msg = _call_lazy(optim_lib, dict(LAZY_GOOD, **over))
        assert rc == 2 and "HIP error" in msg, (over, rc, msg)


def test_a_c99_program_links_against_the_lazy_entry_and_is_refused(tmp_path, optim_lib):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not found")
    pkg = os.path.dirname(optim_lib.LIB_PATH)
    exe = str(tmp_path / "optim_lazy_consumer")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "optim_lazy_consumer.c"), "-L", pkg, "-lmi_nerf_optim", f"-Wl,-rpath,{pkg}", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"optim lazy c_abi consumer ok: ABI {optim_lib.ABI_VERSION}" in run.stdout


# ---------------------------------------------------------------------------------------------------
# the class
# ---------------------------------------------------------------------------------------------------
def test_lazy_adam_refuses_host_tensors_and_weight_decay():
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    from nerf_pytorch_paeng_amd.optim import FusedAdam, LazyAdam
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(MiNerfError, match="LazyAdam.*HIP device"):
        LazyAdam([p]).step()
    for kw in (dict(weight_decay=0.1), dict(lr=-1.0), dict(betas=(0.9, 1.0)), dict(eps=float("inf")), dict(clamp_min=NAN), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(MiNerfError):
            LazyAdam([p], **kw)
    with pytest.raises(MiNerfError, match="weight_decay"):
        LazyAdam([dict(params=[p], weight_decay=0.1)])
    opt = LazyAdam([dict(params=[p], clamp_min=0.0)], lr=1e-2, clamp_min=None, consume=False)
    assert isinstance(opt, FusedAdam) and isinstance(opt, torch.optim.Optimizer) and opt.consume is False and not opt.guarded
    assert set(opt.param_groups[0]) == set(torch.optim.Adam([p]).param_groups[0]) | {"clamp_min"}   # a checkpoint's keys, and the clamp
    assert opt.param_groups[0]["clamp_min"] == 0.0 and LazyAdam([p]).param_groups[0]["clamp_min"] is None
    opt.param_groups[0]["weight_decay"] = 0.1
    with pytest.raises(MiNerfError, match="weight_decay"):
        opt.step()
