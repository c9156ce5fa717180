"""libmi_nerf_optim.so / include/mi_nerf_optim.h and nerf_pytorch_paeng_amd/optim.py without a GPU: the header, the ctypes table
(nerf_pytorch_paeng_amd/_optim.py) and the library's dynamic symbols name the same entries; the library exports nothing of the others and
stands alone; a C99 program links against it; every refusal answers MI_OPTIM_EINVAL with a message before any HIP call; FusedAdam refuses
host tensors; the schedule agrees with the sequences the reference's own scheduler produced (tests/golden/F13_lr_schedule.npz, written by
tools/gen_lr_fixture.py)."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1


@pytest.fixture(scope="module")
def optim_lib():
    """The library is built when the tree is fresh (a no-op when it is up to date), like tests/conftest.py does for libmi_nerf.so."""
    from nerf_pytorch_paeng_amd import _optim
    from nerf_pytorch_paeng_amd.build import build_optim_library
    build_optim_library()
    _optim.lib()
    return _optim


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def test_header_table_and_symbols_agree_and_only_mi_optim_is_exported(optim_lib):
    from nerf_pytorch_paeng_amd import _geo, _iqa, _lib, _mesh, _occ, _pose, _scene
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_optim.h")).read()
    declared = set(re.findall(r"\b(mi_optim_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(optim_lib.SIGNATURES), declared ^ set(optim_lib.SIGNATURES)
    new = _exports(optim_lib.LIB_PATH)
    assert {n for n in new if n.startswith("mi_")} == declared                             # the header's entries and no other mi_* name
    assert not [n for n in new if not n.startswith("mi_optim_") and not n.startswith("_Z")]   # beside them only the kernels' C++ launch stubs
    for other in (_lib, _geo, _iqa, _mesh, _occ, _pose, _scene):
        assert not set(optim_lib.SIGNATURES) & set(other.SIGNATURES)
    for other in ("mi_nerf.h", "mi_nerf_occ.h", "mi_nerf_iqa.h", "mi_nerf_scene.h", "mi_nerf_mesh.h", "mi_nerf_geo.h", "mi_nerf_pose.h"):
        assert "mi_optim_" not in open(os.path.join(ROOT, "include", other)).read()
    assert '#include "mi_nerf' not in hdr                                                  # the header stands alone
    assert optim_lib.lib().mi_optim_abi_version() == optim_lib.ABI_VERSION == int(re.search(r"#define MI_OPTIM_ABI_VERSION (\d+)", hdr).group(1))
    for name in ("MAX_TENSORS", "CHUNK", "CONTROL_WORDS", "TSTATE_WORDS"):
        assert getattr(optim_lib, name) == int(re.search(rf"#define MI_OPTIM_{name} (\d+)", hdr).group(1)), name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [n for n in sorted(declared) if n not in doc] == []


def test_the_library_stands_alone_and_is_in_the_build_table(optim_lib):
    from nerf_pytorch_paeng_amd import build
    assert build.LIBRARIES["optim"] == (["optim.hip"], [], False)
    dyn = subprocess.run(["readelf", "-d", optim_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libmi_nerf" not in dyn.replace("libmi_nerf_optim.so", "")
    und = subprocess.run(["nm", "-D", "--undefined-only", optim_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not [ln for ln in und.splitlines() if ln.split()[-1].startswith("mi_")]


def test_the_config_struct_of_the_binding_is_the_headers(optim_lib):
    """Field by field: the ctypes structure against the header's declaration, and its size against what a C compiler makes of it."""
    hdr = open(os.path.join(ROOT, "include", "mi_nerf_optim.h")).read()
    body = re.search(r"typedef struct mi_optim_adam_cfg \{(.*?)\} mi_optim_adam_cfg;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().split("[")[0] for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in optim_lib.AdamCfg._fields_], names
    assert C.sizeof(optim_lib.AdamCfg) == 56                                                # 2 x 4 + 5 x 8 + 2 x 4, no padding


def test_header_compiles_as_c99_and_the_library_links_and_answers(tmp_path, optim_lib):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not found")
    pkg = os.path.dirname(optim_lib.LIB_PATH)
    exe = str(tmp_path / "optim_consumer")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c_abi", "optim_consumer.c"), "-L", pkg, "-lmi_nerf_optim", f"-Wl,-rpath,{pkg}", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"optim c_abi consumer ok: ABI {optim_lib.ABI_VERSION}" in run.stdout


# made-up addresses that are never dereferenced: every call below is refused before the first HIP call (a call that got as far as one would
# answer MI_OPTIM_EHIP, "HIP error ... no ROCm-capable device", on a machine without a GPU)
GOOD = dict(n=3, params=[0x10000, 0x20000, 0x30004], grads=[0x40000, 0x50004, 0x60000], numel=[5, 0, 4097], off=[0, 8, 8], step=[1, 1, 7], m=0x100000,
            v=0x200000, state_numel=8 + 4100, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, decoupled=0, size=None, n_cfg=1, cfg_of=[0, 0, 0],
            slot=[0, 1, 2], n_slots=3, max_norm=1.0, skip=1, tstate=0x300000, control=0x400000, scratch=0x500000, scratch_bytes=None)
NAN, INF = float("nan"), float("inf")
# case -> (overrides, the entries it applies to: s plain step, g guarded step, t grad stats)
REFUSALS = {
    "n 0": (dict(n=0), "sgt"),
    "n negative": (dict(n=-1), "sgt"),
    "NULL params array": (dict(params=None), "sg"),
    "NULL grads array": (dict(grads=None), "sgt"),
    "NULL numel array": (dict(numel=None), "sgt"),
    "NULL state_off array": (dict(off=None), "sg"),
    "NULL step array": (dict(step=None), "s"),
    "NULL cfgs": (dict(n_cfg=0), "sgt"),
    "NULL slot array": (dict(slot=None), "gt"),
    "NULL pointer inside params": (dict(params=[None, 0x20000, 0x30004]), "sg"),
    "NULL pointer inside grads": (dict(grads=[None, 0x50004, 0x60000]), "sgt"),
    "negative numel": (dict(numel=[5, -1, 4097]), "sgt"),
    "param not 4-byte aligned": (dict(params=[0x10002, 0x20000, 0x30004]), "sg"),
    "grad not 4-byte aligned": (dict(grads=[0x40000, 0x50004, 0x60001]), "sgt"),
    "NULL exp_avg": (dict(m=None), "sg"),
    "exp_avg_sq not 4-byte aligned": (dict(v=0x200002), "sg"),
    "moments outside the arenas": (dict(state_numel=4104), "sg"),
    "negative state offset": (dict(off=[-4, 8, 8]), "sg"),
    "negative lr": (dict(lr=-1e-3), "sgt"),
    "NaN lr": (dict(lr=NAN), "sgt"),
    "infinite lr": (dict(lr=INF), "sgt"),
    "negative eps": (dict(eps=-1e-8), "sgt"),
    "NaN eps": (dict(eps=NAN), "sgt"),
    "negative weight_decay": (dict(wd=-0.1), "sgt"),
    "infinite weight_decay": (dict(wd=INF), "sgt"),
    "beta1 1": (dict(beta1=1.0), "sgt"),
    "beta1 negative": (dict(beta1=-0.1), "sgt"),
    "beta2 1": (dict(beta2=1.0), "sgt"),
    "beta2 NaN": (dict(beta2=NAN), "sgt"),
    "decoupled 2": (dict(decoupled=2), "sgt"),
    "config size": (dict(size=48), "sgt"),
    "cfg_of outside": (dict(cfg_of=[0, 1, 0]), "sgt"),
    "step 0": (dict(step=[1, 0, 7]), "s"),
    "max_norm 0": (dict(max_norm=0.0), "t"),
    "max_norm negative": (dict(max_norm=-1.0), "t"),
    "max_norm NaN": (dict(max_norm=NAN), "t"),
    "skip_nonfinite 2": (dict(skip=2), "t"),
    "slot outside": (dict(slot=[0, 1, 3]), "gt"),
    "NULL tstate": (dict(tstate=None), "gt"),
    "NULL control": (dict(control=None), "gt"),
    "control not 16-byte aligned": (dict(control=0x400004), "gt"),
    "NULL scratch": (dict(scratch=None), "t"),
    "scratch too small": (dict(scratch_bytes=-1), "t"),
    "scratch not 16-byte aligned": (dict(scratch=0x500008), "t"),
}


def _arr(ctype, values):
    return None if values is None else (ctype * len(values))(*values)


def _call(mod, entry, a):
    L = mod.lib()
    n = a["n"]
    cfg = mod.AdamCfg(size=C.sizeof(mod.AdamCfg) if a["size"] is None else a["size"], decoupled=a["decoupled"], lr=a["lr"], beta1=a["beta1"],
                      beta2=a["beta2"], eps=a["eps"], weight_decay=a["wd"])
    cfgs = (mod.AdamCfg * 1)(cfg) if a["n_cfg"] else None
    params, grads = _arr(C.c_void_p, a["params"]), _arr(C.c_void_p, a["grads"])
    numel, off, step = _arr(C.c_int64, a["numel"]), _arr(C.c_int64, a["off"]), _arr(C.c_int64, a["step"])
    cfg_of, slot = _arr(C.c_int32, a["cfg_of"]), _arr(C.c_int32, a["slot"])
    if entry == "s":
        rc = L.mi_optim_adam_step(n, params, grads, numel, off, step, a["m"], a["v"], a["state_numel"], cfgs, a["n_cfg"], cfg_of, None)
    elif entry == "g":
        rc = L.mi_optim_adam_step_guarded(n, params, grads, numel, off, a["m"], a["v"], a["state_numel"], cfgs, a["n_cfg"], cfg_of, slot, a["n_slots"],
                                          a["tstate"], a["control"], None)
    else:
        need = L.mi_optim_grad_stats_scratch_bytes(GOOD["n"], _arr(C.c_int64, GOOD["numel"]))
        nbytes = need if a["scratch_bytes"] is None else need + a["scratch_bytes"]
        rc = L.mi_optim_grad_stats(n, grads, numel, cfgs, a["n_cfg"], cfg_of, slot, a["n_slots"], a["max_norm"], a["skip"], a["tstate"], a["control"],
                                   a["scratch"], nbytes, None)
    return rc, mod.last_error()


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_answer_einval_with_a_message_before_any_hip_call(optim_lib, case):
    over, entries = REFUSALS[case]
    for entry in entries:
        rc, msg = _call(optim_lib, entry, dict(GOOD, **over))
        assert rc == EINVAL, (case, entry, rc, msg)
        assert msg and "HIP error" not in msg, (case, entry, msg)


def test_the_good_arguments_of_the_refusal_table_reach_the_device(optim_lib):
    """The table's base case is refused by nothing: each entry gets as far as its first launch, which fails here for want of a device
    (MI_OPTIM_EHIP) -- so every refusal above is owed to its one override."""
    if torch.cuda.is_available():
        pytest.skip("made-up addresses must not reach a real device")
    for entry in "sgt":
        rc, msg = _call(optim_lib, entry, dict(GOOD))
        assert rc == 2 and "HIP error" in msg, (entry, rc, msg)


def test_a_tensor_without_elements_may_have_null_pointers(optim_lib):
    """An empty torch tensor's data_ptr() is 0: the base case with NULL for its numel == 0 tensor is still refused by nothing (it reaches the
    launch, which fails here for want of a device)."""
    if torch.cuda.is_available():
        pytest.skip("made-up addresses must not reach a real device")
    a = dict(GOOD, params=[0x10000, None, 0x30004], grads=[0x40000, None, 0x60000])
    for entry in "sgt":
        rc, msg = _call(optim_lib, entry, a)
        assert rc == 2 and "HIP error" in msg, (entry, rc, msg)


def test_scratch_bytes_count_one_partial_per_chunk(optim_lib):
    L = optim_lib.lib()
    ch = optim_lib.CHUNK
    sizes = [0, 1, ch - 1, ch, ch + 1, 3 * ch + 1]
    assert L.mi_optim_grad_stats_scratch_bytes(len(sizes), _arr(C.c_int64, sizes)) == 16 * (0 + 1 + 1 + 1 + 2 + 4)
    assert L.mi_optim_grad_stats_scratch_bytes(1, _arr(C.c_int64, [0])) == 16
    assert L.mi_optim_grad_stats_scratch_bytes(0, _arr(C.c_int64, [1])) == 0
    assert L.mi_optim_grad_stats_scratch_bytes(1, _arr(C.c_int64, [-1])) == 0
    assert L.mi_optim_grad_stats_scratch_bytes(1, None) == 0


def test_the_per_tensor_table_travels_within_4_kb(optim_lib):
    """44 bytes of kernel arguments per tensor (two pointers, offset, size, prefix word, two floats or a slot and a float -- the source keeps
    slot and step size apart, 48) plus the scalars: MI_OPTIM_MAX_TENSORS is the largest multiple of 8 that keeps the table below 4 KB, and the
    source asserts the struct's size at compile time."""
    src = open(os.path.join(ROOT, "nerf_pytorch_paeng_amd", "csrc", "optim.hip")).read()
    assert "static_assert(sizeof(Table) <= 4096" in src and "static_assert(sizeof(FinishArgs) <= 4096" in src
    assert 48 * optim_lib.MAX_TENSORS + 4 + 96 <= 4096 < 48 * (optim_lib.MAX_TENSORS + 8) + 4 + 96


def test_fused_adam_refuses_what_it_does_not_run():
    from nerf_pytorch_paeng_amd._lib import MiNerfError
    from nerf_pytorch_paeng_amd.optim import FusedAdam
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(MiNerfError, match="HIP device"):
        FusedAdam([p]).step()
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(max_grad_norm=0.0), dict(max_grad_norm=float("nan")), dict(lr=-1.0), dict(betas=(0.9, 1.0)),
               dict(eps=float("inf")), dict(weight_decay=-1.0), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(MiNerfError):
            FusedAdam([p], **kw)
    opt = FusedAdam([p])
    assert set(opt.param_groups[0]) == set(torch.optim.Adam([p]).param_groups[0])           # the keys a checkpoint carries
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(MiNerfError, match="amsgrad"):
        opt.step()
    with pytest.raises(MiNerfError, match="guarded"):
        FusedAdam([p]).last_grad_norm


# ---------------------------------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------------------------------
ORDER = ("first_cycle_steps", "cycle_mult", "max_lr", "min_lr", "warmup_steps", "gamma")
BAR = 1e-12              # doubles through about ten operations: the margin over 1e-15 is not a measurement


def _case(golden, name):
    d = golden("F13_lr_schedule")
    a = d[name + "_args"]
    kw = dict(first_cycle_steps=int(a[0]), cycle_mult=float(a[1]), max_lr=float(a[2]), min_lr=float(a[3]), warmup_steps=int(a[4]), gamma=float(a[5]))
    return kw, d[name + "_lr"], d.get(name + "_epochs")


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b) / np.abs(b)))


@pytest.mark.parametrize("name, steps", [("recipe", 130), ("growing", 200), ("no_warmup", 60)])
def test_the_schedule_is_the_reference_schedulers_step_by_step(golden, name, steps):
    from nerf_pytorch_paeng_amd.optim import CosineAnnealingWarmupRestarts, lr_at
    kw, ref, _ = _case(golden, name)
    assert len(ref) == steps + 1
    pure = [lr_at(i, **kw) for i in range(steps + 1)]
    # the value the constructor leaves is min_lr in the reference; with warm-up that is lr_at(0), without it lr_at(0) is the peak
    first = 0 if kw["warmup_steps"] else 1
    assert ref[0] == kw["min_lr"] and (first == 0 or pure[0] == kw["max_lr"])
    assert _rel(pure[first:], ref[first:]) <= BAR, _rel(pure[first:], ref[first:])
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=1.0)
    sched = CosineAnnealingWarmupRestarts(opt, **kw)
    got = [opt.param_groups[0]["lr"]]
    for _ in range(steps):
        opt.step()
        sched.step()
        got.append(opt.param_groups[0]["lr"])
    assert _rel(got, ref) <= BAR, _rel(got, ref)
    assert sched.get_last_lr() == [got[-1]] and sched.last_epoch == steps


def test_the_fixture_crosses_restarts_and_decays_its_peaks(golden):
    kw, ref, _ = _case(golden, "recipe")
    assert [i for i in range(len(ref)) if ref[i] == kw["min_lr"]] == [0, 51, 102]            # two restarts in 130 steps of 51
    kw, ref, _ = _case(golden, "growing")
    peaks = [i for i in range(1, len(ref) - 1) if ref[i - 1] < ref[i] > ref[i + 1]]
    assert peaks == [5, 25, 60, 125] and [round(ref[i] / kw["max_lr"], 9) for i in peaks] == [1.0, 0.5, 0.25, 0.125]   # cycles of 20, 35, 65, 125


def test_explicit_epochs_agree_and_are_refused_when_the_cycles_grow(golden):
    from nerf_pytorch_paeng_amd.optim import CosineAnnealingWarmupRestarts
    kw, ref, epochs = _case(golden, "jumps")
    assert kw["cycle_mult"] == 1.0 and max(epochs) > 8 * kw["first_cycle_steps"]
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=1.0)                     # any torch.optim.Optimizer
    sched = CosineAnnealingWarmupRestarts(opt, **kw)
    got = [opt.param_groups[0]["lr"]]
    for e in epochs:
        sched.step(int(e))
        got.append(opt.param_groups[0]["lr"])
    assert _rel(got, ref) <= BAR, _rel(got, ref)
    sched = CosineAnnealingWarmupRestarts(opt, **dict(kw, cycle_mult=2.0))
    sched.step()
    with pytest.raises(ValueError, match="cycle_mult"):
        sched.step(30)
    with pytest.raises(ValueError, match="warmup_steps"):
        CosineAnnealingWarmupRestarts(opt, 10, warmup_steps=10)


def test_the_schedule_drives_every_group_and_survives_its_state_dict():
    from nerf_pytorch_paeng_amd.optim import CosineAnnealingWarmupRestarts, lr_at
    a, b = torch.zeros(1, requires_grad=True), torch.zeros(1, requires_grad=True)
    kw = dict(first_cycle_steps=9, cycle_mult=1.0, max_lr=1e-2, min_lr=1e-3, warmup_steps=2, gamma=0.5)
    opt = torch.optim.Adam([{"params": [a]}, {"params": [b], "lr": 5.0}], lr=1.0)
    sched = CosineAnnealingWarmupRestarts(opt, **kw)
    for _ in range(13):
        opt.step()
        sched.step()
    assert [g["lr"] for g in opt.param_groups] == [lr_at(13, **kw)] * 2
    opt2 = torch.optim.Adam([{"params": [a]}, {"params": [b]}], lr=1.0)
    sched2 = CosineAnnealingWarmupRestarts(opt2, **kw)
    sched2.load_state_dict(sched.state_dict())
    opt2.step()
    sched2.step()
    assert sched2.last_epoch == 14 and opt2.param_groups[0]["lr"] == lr_at(14, **kw)
    assert math.isclose(lr_at(9 + 2, **kw), 0.5e-2) and lr_at(9, **kw) == 1e-3                # second cycle: the peak halves, the start is min_lr


def test_the_optimizer_source_holds_no_preprocessor_conditional_and_no_ablation_macro():
    """tests/test_packing_cpu.py allows 14 conditionals in csrc/ and counts 12; this source adds none."""
    src = open(os.path.join(ROOT, "nerf_pytorch_paeng_amd", "csrc", "optim.hip")).read()
    assert not re.findall(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b", src, re.M) and "MN_" not in src
