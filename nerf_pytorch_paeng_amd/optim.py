"""The optimiser and the learning-rate schedule of the training loop (docs/design/20_optimizer.md).

``FusedAdam`` is a ``torch.optim.Optimizer`` over libmi_nerf_optim.so (include/mi_nerf_optim.h): Adam or AdamW over every parameter that has
a gradient in one library call (plain mode), or in two when the step is guarded -- gradient clipping by global norm and / or skipping a step
whose gradients are not finite, both decided on the device, without a host synchronisation.  Its ``state_dict()`` is ``torch.optim.Adam``'s,
in both directions.  There is no fallback: anything but contiguous fp32 tensors on a HIP device raises ``MiNerfError``.

``LazyAdam`` is its sparse counterpart for a large table that a step's gradient reaches in a few places (a radiance grid): it steps only the
elements whose gradient is not zero and leaves every other bit alone (docs/design/26_lazy_optimizer.md).

``CosineAnnealingWarmupRestarts`` is the schedule of the reference's training recipe, written from its definition on the pure function
``lr_at``; it drives any ``torch.optim.Optimizer``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional

import torch

from . import _optim
from ._lib import MiNerfError, stream_ptr

_GROUP_KEYS = ("lr", "betas", "eps", "weight_decay", "decoupled_weight_decay")


class FusedAdam(torch.optim.Optimizer):
    """Adam / AdamW in one launch per 80 tensors.  ``max_grad_norm``: clip the gradients of ALL groups by their global L2 norm
    (``torch.nn.utils.clip_grad_norm_``'s rule) inside the step, the gradients themselves stay as they are; ``skip_nonfinite``: leave
    parameters, moments and step counts untouched when any gradient element is inf or NaN.  Either makes the step *guarded*: the norm, the
    coefficient and the skip decision stay on the device; ``last_grad_norm`` and ``skipped_steps`` are device tensors, and reading them is
    the caller's synchronisation."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, decoupled_weight_decay=False, max_grad_norm=None,
                 skip_nonfinite=False, amsgrad=False, maximize=False):
        if amsgrad or maximize:
            raise MiNerfError("FusedAdam: amsgrad and maximize are not built")
        if max_grad_norm is not None and not (float(max_grad_norm) > 0.0):
            raise MiNerfError(f"FusedAdam: max_grad_norm={max_grad_norm} must be positive (None: no clipping)")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None, capturable=False,
                        differentiable=False, fused=None, decoupled_weight_decay=bool(decoupled_weight_decay))      # torch.optim.Adam's keys
        super().__init__(params, defaults)
        for group in self.param_groups:
            self._check_group(group)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        self._device: Optional[torch.device] = None
        self._slot: Dict[torch.Tensor, int] = {}
        self._key = None

    # ------------------------------------------------------------------------------------------------
    # checks
    # ------------------------------------------------------------------------------------------------
    @classmethod
    def _check_group(cls, group) -> None:
        if group.get("amsgrad") or group.get("maximize") or group.get("differentiable"):
            raise MiNerfError(f"{cls.__name__}: amsgrad, maximize and differentiable are not built")
        lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
        if isinstance(lr, torch.Tensor) or isinstance(b1, torch.Tensor) or isinstance(b2, torch.Tensor):
            raise MiNerfError(f"{cls.__name__}: lr and betas are Python numbers (the constants of the update are formed on the host)")
        if not (math.isfinite(lr) and lr >= 0.0 and math.isfinite(eps) and eps >= 0.0 and math.isfinite(wd) and wd >= 0.0):
            raise MiNerfError(f"{cls.__name__}: lr={lr}, eps={eps}, weight_decay={wd} must be finite and not negative")
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise MiNerfError(f"{cls.__name__}: betas {(b1, b2)} must lie in [0, 1)")

    @classmethod
    def _check_tensor(cls, t: torch.Tensor, what: str) -> None:
        if not t.is_cuda:
            raise MiNerfError(f"{cls.__name__}: {what} must live on a HIP device (got {t.device}); there is no CPU fallback")
        if t.is_sparse or t.layout != torch.strided:
            raise MiNerfError(f"{cls.__name__}: {what} is sparse; only dense tensors are built")
        if t.dtype != torch.float32:
            raise MiNerfError(f"{cls.__name__}: {what} must be torch.float32 (got {t.dtype})")
        if not t.is_contiguous():
            raise MiNerfError(f"{cls.__name__}: {what} must be contiguous")

    # ------------------------------------------------------------------------------------------------
    # the arenas: every parameter of every group owns a run of both, 16-byte aligned, from the first step on
    # ------------------------------------------------------------------------------------------------
    def _all_params(self) -> List[torch.Tensor]:
        return [p for group in self.param_groups for p in group["params"]]

    def _layout(self) -> None:
        """Size the arenas and the device words for the parameters as they stand (again after add_param_group: what was there is kept)."""
        params = self._all_params()
        if not params:
            raise MiNerfError(f"{type(self).__name__}: no parameters")
        for p in params:
            self._check_tensor(p, "a parameter")
        dev = params[0].device
        if any(p.device != dev for p in params):
            raise MiNerfError(f"{type(self).__name__}: all parameters must live on one device")
        kept = {p: (st["exp_avg"].clone(), st["exp_avg_sq"].clone()) for p, st in self.state.items() if "exp_avg" in st} if self._slot else {}
        old_rows = self._tstate[[self._slot[p] for p in kept]].clone() if kept else None
        old_steps = [self._steps[self._slot[p]] for p in kept]
        self._device = dev
        self._slot, self._off, total = {}, [], 0
        for i, p in enumerate(params):
            self._slot[p] = i
            self._off.append(total)
            total += (p.numel() + 3) // 4 * 4
        self._total = max(total, 4)
        self._exp_avg = torch.zeros(self._total, dtype=torch.float32, device=dev)
        self._exp_avg_sq = torch.zeros(self._total, dtype=torch.float32, device=dev)
        self._steps = [0] * len(params)                                      # plain mode: the step count of every slot, on the host
        self._tstate = torch.zeros(len(params), _optim.TSTATE_WORDS, dtype=torch.float32, device=dev)     # guarded mode: on the device
        if not hasattr(self, "_control"):
            self._control = torch.zeros(_optim.CONTROL_WORDS, dtype=torch.int32, device=dev)
        numel = (C.c_int64 * len(params))(*[p.numel() for p in params])
        self._scratch = torch.empty(max(_optim.lib().mi_optim_grad_stats_scratch_bytes(len(params), numel), 16), dtype=torch.uint8, device=dev)
        self._key = None
        for k, (p, (m, v)) in enumerate(kept.items()):
            st = self.state[p]
            st["exp_avg"], st["exp_avg_sq"] = self._views(p)
            st["exp_avg"].copy_(m)
            st["exp_avg_sq"].copy_(v)
            self._steps[self._slot[p]] = old_steps[k]
        if kept:
            self._tstate[[self._slot[p] for p in kept]] = old_rows

    def _views(self, p: torch.Tensor):
        off = self._off[self._slot[p]]
        return self._exp_avg[off:off + p.numel()].view_as(p), self._exp_avg_sq[off:off + p.numel()].view_as(p)

    def _ensure_layout(self) -> None:
        if self._device is None or len(self._slot) != sum(len(g["params"]) for g in self.param_groups):
            self._layout()

    # ------------------------------------------------------------------------------------------------
    # the step
    # ------------------------------------------------------------------------------------------------
    def _collect(self):
        """What a step hands to the library: the parameters that have a gradient, their slots, and the host arrays of the call (rebuilt only
        when an address moved).  -> (ps, slots, cfgs), or None when no parameter has a gradient."""
        for group in self.param_groups:
            self._check_group(group)
        self._ensure_layout()
        ps, gs, slots, cfg_of = [], [], [], []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                self._check_tensor(p, "a parameter")
                self._check_tensor(g, "a gradient")
                if g.device != self._device or p.device != self._device or g.shape != p.shape:
                    raise MiNerfError(f"{type(self).__name__}: a parameter or gradient moved or changed shape after the first step")
                ps.append(p)
                gs.append(g)
                slots.append(self._slot[p])
                cfg_of.append(gi)
        n = len(ps)
        if n == 0:
            return None
        key = (tuple(p.data_ptr() for p in ps), tuple(g.data_ptr() for g in gs), tuple(slots), tuple(cfg_of))
        if key != self._key:                                                 # the host arrays of the call, rebuilt only when an address moved
            self._arr = ((C.c_void_p * n)(*key[0]), (C.c_void_p * n)(*key[1]), (C.c_int64 * n)(*[p.numel() for p in ps]),
                         (C.c_int64 * n)(*[self._off[s] for s in slots]), (C.c_int32 * n)(*cfg_of), (C.c_int32 * n)(*slots), (C.c_int64 * n)())
            self._key = key
            for p in ps:
                if "exp_avg" not in self.state[p]:
                    st = self.state[p]
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"], st["exp_avg_sq"] = self._views(p)
        n_cfg = len(self.param_groups)
        cfgs = (_optim.AdamCfg * n_cfg)()
        for c, group in zip(cfgs, self.param_groups):
            c.size, c.decoupled = C.sizeof(_optim.AdamCfg), int(bool(group.get("decoupled_weight_decay", False)))
            c.lr, (c.beta1, c.beta2), c.eps, c.weight_decay = group["lr"], group["betas"], group["eps"], group["weight_decay"]
        return ps, slots, cfgs

    def _count_steps(self, slots):
        """Plain mode's bookkeeping: every slot that steps is one step further, and the call's step array says so."""
        steps, a_step = self._steps, self._arr[6]
        for i, s in enumerate(slots):
            steps[s] += 1
            a_step[i] = steps[s]
        return a_step

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        got = self._collect()
        if got is None:
            return loss
        ps, slots, cfgs = got
        n, n_cfg = len(ps), len(cfgs)
        a_p, a_g, a_numel, a_off, a_cfg, a_slot, a_step = self._arr
        L, dev = _optim.lib(), self._device
        m, v = self._exp_avg.data_ptr(), self._exp_avg_sq.data_ptr()
        with torch.cuda.device(dev):
            stream = stream_ptr(dev)
            if self.guarded:
                max_norm = math.inf if self.max_grad_norm is None else self.max_grad_norm
                ts, ctl = self._tstate.data_ptr(), self._control.data_ptr()
                _optim.check(L.mi_optim_grad_stats(n, a_g, a_numel, cfgs, n_cfg, a_cfg, a_slot, len(self._slot), max_norm, int(self.skip_nonfinite), ts, ctl,
                                                   self._scratch.data_ptr(), self._scratch.numel(), stream), "mi_optim_grad_stats")
                _optim.check(L.mi_optim_adam_step_guarded(n, a_p, a_g, a_numel, a_off, m, v, self._total, cfgs, n_cfg, a_cfg, a_slot, len(self._slot), ts, ctl,
                                                          stream), "mi_optim_adam_step_guarded")
            else:
                a_step = self._count_steps(slots)
                _optim.check(L.mi_optim_adam_step(n, a_p, a_g, a_numel, a_off, a_step, m, v, self._total, cfgs, n_cfg, a_cfg, stream), "mi_optim_adam_step")
        torch.autograd.graph.increment_version(ps)                           # the kernel wrote behind autograd's back: caches keyed on _version must see it
        return loss

    @property
    def last_grad_norm(self) -> torch.Tensor:
        """The global gradient norm of the last guarded step, a 0-dim fp32 DEVICE tensor (a view: the next step overwrites it)."""
        return self._guarded_words().view(torch.float32)[0]

    @property
    def skipped_steps(self) -> torch.Tensor:
        """How many guarded steps were skipped so far, a 0-dim int32 DEVICE tensor (a view)."""
        return self._guarded_words()[4]

    def _guarded_words(self) -> torch.Tensor:
        if not self.guarded:
            raise MiNerfError("FusedAdam: last_grad_norm / skipped_steps exist in guarded mode (max_grad_norm= or skip_nonfinite=)")
        self._ensure_layout()
        return self._control

    # ------------------------------------------------------------------------------------------------
    # torch.optim.Adam's state_dict, both ways
    # ------------------------------------------------------------------------------------------------
    def _refresh_steps(self) -> None:
        """state[p]["step"] as torch.optim.Adam keeps it (a 0-dim fp32 CPU tensor); in guarded mode this reads the device steps."""
        if self._device is None:
            return
        dev_steps = self._tstate[:, 0].cpu().tolist() if self.guarded else None
        for p, st in self.state.items():
            if "exp_avg" in st:
                s = self._slot[p]
                st["step"] = torch.tensor(float(dev_steps[s] if self.guarded else self._steps[s]), dtype=torch.float32)

    def state_dict(self):
        """``torch.optim.Adam``'s layout with CLONES of the moments (a view would drag the whole arena into ``torch.save`` once per tensor)."""
        self._refresh_steps()
        sd = super().state_dict()
        sd["state"] = {k: {kk: (vv.clone() if isinstance(vv, torch.Tensor) else vv) for kk, vv in st.items()} for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict) -> None:
        """A state dict of ``torch.optim.Adam`` / ``AdamW`` (or of this class): the moments are copied into the arenas."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_group(group)
        loaded = {p: dict(st) for p, st in self.state.items()}
        self._device = None                                                  # a fresh layout: nothing of the old state survives a load
        self._slot = {}
        self._layout()
        rows = torch.zeros(len(self._slot), _optim.TSTATE_WORDS, dtype=torch.float32)
        for p, st in loaded.items():
            if not {"step", "exp_avg", "exp_avg_sq"} <= set(st):
                raise MiNerfError(f"{type(self).__name__}.load_state_dict: a parameter's state has the keys {sorted(st)}, expected step, exp_avg, exp_avg_sq")
            if "max_exp_avg_sq" in st:
                raise MiNerfError(f"{type(self).__name__}.load_state_dict: the checkpoint was written with amsgrad, which is not built")
            m, v = self._views(p)
            m.copy_(st["exp_avg"])
            v.copy_(st["exp_avg_sq"])
            step = int(st["step"])
            self._steps[self._slot[p]] = step
            rows[self._slot[p], 0] = float(step)
            self.state[p] = {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": m, "exp_avg_sq": v}
        self._tstate.copy_(rows)


class LazyAdam(FusedAdam):
    """Adam that steps only where a gradient arrived (THE LAZY UPDATE of include/mi_nerf_optim.h, docs/design/26_lazy_optimizer.md): an
    element whose gradient is zero (``g != 0`` is false; -0.0 counts as zero) keeps the bits of its parameter and of both moments, and
    nothing catches up later.  Made for a table of which a step's gradient reaches a few per cent, a radiance grid's records; the bias
    corrections come from the tensor's step count.  ``clamp_min`` (per group; None: no clamp) is applied to the touched elements after the
    update.  ``consume=True`` overwrites every touched gradient element with +0 in the same pass: ``p.grad`` is then a persistent
    accumulator that the next backward adds into, and ``zero_grad`` is not needed (``zero_grad(set_to_none=True)`` would discard the
    buffer).  Arenas, step bookkeeping and ``state_dict`` are ``FusedAdam``'s: a checkpoint moves between this class, ``FusedAdam`` and
    ``torch.optim.Adam``.  A weight decay is refused: a lazy decay has more than one meaning and none is chosen here."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, *, clamp_min=None, consume=True, weight_decay=0):
        if weight_decay != 0:
            raise MiNerfError(f"LazyAdam: weight_decay={weight_decay} is refused (a lazy weight decay is not defined)")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=0)
        self.consume = bool(consume)
        self.defaults["clamp_min"] = clamp_min                               # what add_param_group gives a group that names none
        for group in self.param_groups:
            group.setdefault("clamp_min", clamp_min)
            self._check_group(group)

    @classmethod
    def _check_group(cls, group) -> None:
        super()._check_group(group)
        if group["weight_decay"] != 0:
            raise MiNerfError(f"{cls.__name__}: weight_decay={group['weight_decay']} is refused (a lazy weight decay is not defined)")
        lo = group.get("clamp_min")
        if lo is not None and (isinstance(lo, torch.Tensor) or math.isnan(lo)):
            raise MiNerfError(f"{cls.__name__}: clamp_min={lo} must be a Python number, not NaN (None: no clamp)")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        got = self._collect()
        if got is None:
            return loss
        ps, slots, cfgs = got
        n, n_cfg = len(ps), len(cfgs)
        a_p, a_g, a_numel, a_off, a_cfg, _, _ = self._arr
        lows = [self.param_groups[gi].get("clamp_min") for gi in a_cfg]
        p_min = None if all(lo is None for lo in lows) else (C.c_float * n)(*[-math.inf if lo is None else float(lo) for lo in lows])
        a_step = self._count_steps(slots)
        dev = self._device
        with torch.cuda.device(dev):
            _optim.check(_optim.lib().mi_optim_adam_step_lazy(n, a_p, a_g, a_numel, a_off, a_step, self._exp_avg.data_ptr(), self._exp_avg_sq.data_ptr(),
                                                              self._total, cfgs, n_cfg, a_cfg, p_min, int(self.consume), stream_ptr(dev)),
                         "mi_optim_adam_step_lazy")
        torch.autograd.graph.increment_version(ps)
        return loss

    def load_state_dict(self, state_dict) -> None:
        """As ``FusedAdam.load_state_dict``; a group of a checkpoint that names no ``clamp_min`` (one written by ``torch.optim.Adam`` or
        ``FusedAdam``) keeps the one this optimiser's group had."""
        lows = [group.get("clamp_min") for group in self.param_groups]
        super().load_state_dict(state_dict)
        for group, lo in zip(self.param_groups, lows):
            group.setdefault("clamp_min", lo)


# ---------------------------------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------------------------------
def lr_at(step, first_cycle_steps, cycle_mult=1.0, max_lr=0.1, min_lr=0.001, warmup_steps=0, gamma=1.0) -> float:
    """The learning rate at ``step`` (0 is the first).  Cycle 0 lasts ``first_cycle_steps``; each later cycle lasts ``warmup_steps`` plus
    ``cycle_mult`` times what the one before had left after its warm-up (rounded down), and peaks at ``max_lr * gamma ** cycle``.  Inside a
    cycle the rate rises linearly from ``min_lr`` to the peak over ``warmup_steps``, then follows half a cosine back down to ``min_lr`` at the
    cycle's end."""
    if step < 0:
        return float(min_lr)
    if not 0 <= warmup_steps < first_cycle_steps:
        raise ValueError(f"warmup_steps={warmup_steps} must be below first_cycle_steps={first_cycle_steps}")
    length, cycle, pos = first_cycle_steps, 0, step
    if cycle_mult == 1.0:
        cycle, pos = int(step // first_cycle_steps), step % first_cycle_steps
    else:
        while pos >= length:
            pos -= length
            cycle += 1
            length = int((length - warmup_steps) * cycle_mult) + warmup_steps
            if length <= warmup_steps:
                raise ValueError(f"cycle {cycle} has no steps left after its warm-up (cycle_mult={cycle_mult})")
    peak = max_lr * gamma ** cycle
    if pos < warmup_steps:
        return min_lr + (peak - min_lr) * pos / warmup_steps
    return min_lr + (peak - min_lr) * (1.0 + math.cos(math.pi * (pos - warmup_steps) / (length - warmup_steps))) / 2.0


class CosineAnnealingWarmupRestarts(torch.optim.lr_scheduler.LRScheduler):
    """``lr_at`` behind the scheduler protocol: the constructor puts every group at ``min_lr``, each ``step()`` moves one step on and
    writes ``lr_at`` of it into every group of the optimizer.  ``step(epoch)`` jumps to ``epoch``; with ``cycle_mult != 1`` that call is
    refused (the closed form in use elsewhere for it disagrees with the step-by-step cycle lengths and yields fractional ones)."""

    def __init__(self, optimizer, first_cycle_steps, cycle_mult=1., max_lr=.1, min_lr=.001, warmup_steps=0, gamma=1., last_epoch=-1):
        if not 0 <= warmup_steps < first_cycle_steps:
            raise ValueError(f"warmup_steps={warmup_steps} must be below first_cycle_steps={first_cycle_steps}")
        self.first_cycle_steps, self.cycle_mult, self.max_lr, self.min_lr = first_cycle_steps, cycle_mult, max_lr, min_lr
        self.warmup_steps, self.gamma = warmup_steps, gamma
        for group in optimizer.param_groups:
            group["lr"] = min_lr
            if last_epoch != -1:
                group.setdefault("initial_lr", min_lr)
        super().__init__(optimizer, last_epoch)
        if last_epoch == -1:                                                 # a fresh schedule starts at min_lr, also when warmup_steps == 0
            for group in optimizer.param_groups:                             # (there lr_at(0) is the peak): the first rate of the reference's recipe
                group["lr"] = min_lr
            self._last_lr = [min_lr] * len(optimizer.param_groups)

    def lr(self, step) -> float:
        return lr_at(step, self.first_cycle_steps, self.cycle_mult, self.max_lr, self.min_lr, self.warmup_steps, self.gamma)

    def get_lr(self):
        return [self.lr(self.last_epoch)] * len(self.optimizer.param_groups)

    def step(self, epoch=None):
        if epoch is None:
            epoch = self.last_epoch + 1
        elif self.cycle_mult != 1.0:
            raise ValueError("CosineAnnealingWarmupRestarts.step(epoch) with cycle_mult != 1 is refused: call step() once per step")
        rate = self.lr(epoch)
        self.last_epoch = math.floor(epoch)
        self._step_count = getattr(self, "_step_count", 0) + 1
        for group in self.optimizer.param_groups:
            group["lr"] = rate
        self._last_lr = [rate] * len(self.optimizer.param_groups)
