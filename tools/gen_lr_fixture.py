#!/usr/bin/env python
"""Write tests/golden/F13_lr_schedule.npz: learning-rate sequences produced by the reference project's own scheduler under a CPU
torch.optim.Adam, which tests/test_optim_cpu.py holds nerf_pytorch_paeng_amd.optim.lr_at against.

    python tools/gen_lr_fixture.py /path/to/reference [out.npz]

The reference's scheduler.py is imported by path and only run; nothing of it is written here.  Per case the file holds `<name>_args` (first_cycle_steps,
cycle_mult, max_lr, min_lr, warmup_steps, gamma as doubles), `<name>_lr` (the rate of group 0 after the constructor and after every step()
call) and, for the case that jumps, `<name>_epochs` (the argument of every step(epoch) call).  The explicit-epoch branch with cycle_mult != 1
yields fractional cycle lengths in the reference and is left out: the package refuses that call.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

CASES = {
    # the reference recipe's shape, scaled down: crosses two restarts
    "recipe": (dict(first_cycle_steps=51, cycle_mult=1.0, max_lr=5e-4, min_lr=5e-5, warmup_steps=10, gamma=1.0), 130),
    "growing": (dict(first_cycle_steps=20, cycle_mult=2.0, max_lr=1e-2, min_lr=1e-4, warmup_steps=5, gamma=0.5), 200),
    "no_warmup": (dict(first_cycle_steps=17, cycle_mult=1.0, max_lr=1e-3, min_lr=1e-5, warmup_steps=0, gamma=0.9), 60),
}
JUMPS = ("jumps", dict(first_cycle_steps=12, cycle_mult=1.0, max_lr=2e-3, min_lr=1e-4, warmup_steps=3, gamma=0.7), [0, 5, 11, 12, 13, 30, 47, 48, 100, 101])
ORDER = ("first_cycle_steps", "cycle_mult", "max_lr", "min_lr", "warmup_steps", "gamma")


def main():
    ref = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "F13_lr_schedule.npz")
    spec = importlib.util.spec_from_file_location("reference_scheduler", os.path.join(ref, "scheduler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def fresh(kw):
        opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=1.0)
        return opt, mod.CosineAnnealingWarmupRestarts(opt, **kw)

    data = {}
    for name, (kw, steps) in CASES.items():
        opt, sched = fresh(kw)
        lrs = [opt.param_groups[0]["lr"]]
        for _ in range(steps):
            opt.step()
            sched.step()
            lrs.append(opt.param_groups[0]["lr"])
        data[name + "_args"] = np.array([kw[k] for k in ORDER], dtype=np.float64)
        data[name + "_lr"] = np.array(lrs, dtype=np.float64)
    name, kw, epochs = JUMPS
    opt, sched = fresh(kw)
    lrs = [opt.param_groups[0]["lr"]]
    for e in epochs:
        sched.step(e)
        lrs.append(opt.param_groups[0]["lr"])
    data[name + "_args"] = np.array([kw[k] for k in ORDER], dtype=np.float64)
    data[name + "_lr"] = np.array(lrs, dtype=np.float64)
    data[name + "_epochs"] = np.array(epochs, dtype=np.int64)
    np.savez(out, **data)
    print(f"wrote {out}: " + ", ".join(f"{k} {v.shape}" for k, v in data.items()))


if __name__ == "__main__":
    main()
