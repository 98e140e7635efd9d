#!/usr/bin/env python3
"""Golden LARS trajectories for the linear probe -> tests/golden/linprobe.npz.

Runs only where the reference checkout is present (never on the GPU box): it imports the reference's own VMAE/util/lars.py and steps it in
f64 on a 2-D weight and a 1-D bias.  Only inputs and results are stored (no reference source text).  Every input is f32-representable, so a
f32 kernel starts from exactly the stored values.  Cases (each: `<case>_p0_w`, `_p0_b`, `_gw` [steps, ...], `_gb`, `_lr` [steps], `_hp` =
(weight_decay, momentum, trust), results `_w` / `_b` / `_mu_w` / `_mu_b` [steps, ...]):
    main         five steps, seeded gradients, weight decay 1/16
    zero_p       the weight starts at zero: |p| = 0, the trust ratio is 1 on the first step
    zero_update  zero gradients and no weight decay on the first step: |dp| = 0, the trust ratio is 1 and nothing moves; then two ordinary steps
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("LDMAE_REFERENCE", "/root/reference")


def reference_lars():
    spec = importlib.util.spec_from_file_location("ref_lars", os.path.join(REF, "VMAE", "util", "lars.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.LARS


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def run_case(LARS, p0_w, p0_b, gw, gb, lrs, wd, momentum, trust):
    w = torch.tensor(p0_w, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(p0_b, dtype=torch.float64, requires_grad=True)
    opt = LARS([w, b], lr=0.0, weight_decay=wd, momentum=momentum, trust_coefficient=trust)
    out = {k: [] for k in ("w", "b", "mu_w", "mu_b")}
    for s, lr in enumerate(lrs):
        for grp in opt.param_groups:
            grp["lr"] = float(lr)
        w.grad, b.grad = torch.tensor(gw[s], dtype=torch.float64), torch.tensor(gb[s], dtype=torch.float64)
        opt.step()
        out["w"].append(w.detach().numpy().copy()), out["b"].append(b.detach().numpy().copy())
        out["mu_w"].append(opt.state[w]["mu"].numpy().copy()), out["mu_b"].append(opt.state[b]["mu"].numpy().copy())
    return {k: np.stack(v) for k, v in out.items()}


def main():
    LARS = reference_lars()
    rng = np.random.default_rng(20240611)
    C, D = 6, 8
    cases = {}
    momentum, trust = 0.9, 0.001

    def grads(steps):
        return f32(rng.normal(0, 0.3, (steps, C, D))), f32(rng.normal(0, 0.3, (steps, C)))

    gw, gb = grads(5)
    cases["main"] = (f32(rng.normal(0, 0.01, (C, D))), f32(np.zeros(C)), gw, gb, f32([0.5, 1.0, 1.5, 1.25, 0.75]), 0.0625)
    gw, gb = grads(5)
    cases["zero_p"] = (np.zeros((C, D)), f32(rng.normal(0, 0.1, C)), gw, gb, f32([0.5, 1.0, 1.5, 1.25, 0.75]), 0.0)
    gw, gb = grads(3)
    gw[0], gb[0] = 0.0, 0.0
    cases["zero_update"] = (f32(rng.normal(0, 0.01, (C, D))), f32(np.zeros(C)), gw, gb, f32([1.0, 1.0, 0.5]), 0.0)
    store = {}
    for name, (p0_w, p0_b, gw, gb, lrs, wd) in cases.items():
        res = run_case(LARS, p0_w, p0_b, gw, gb, lrs, wd, momentum, trust)
        store.update({f"{name}_p0_w": p0_w, f"{name}_p0_b": p0_b, f"{name}_gw": gw, f"{name}_gb": gb, f"{name}_lr": lrs,
                      f"{name}_hp": np.array([wd, momentum, trust], dtype=np.float64)})
        store.update({f"{name}_{k}": v for k, v in res.items()})
    np.savez(os.path.join(HERE, "linprobe.npz"), **store)
    print("wrote linprobe.npz:", {k: v.shape for k, v in store.items()})


if __name__ == "__main__":
    main()
