#!/usr/bin/env python3
"""One drift evaluation of likelihood evaluation on LightningDiT-B/1 at batch 64: forward + vector-Jacobian product, with the input-gradient-only
backward (LightningDiT.input_grad_only) ON and OFF in alternation in one process, f32 and bf16 autocast, every repetition listed; plus the two
per-evaluation kernels of csrc/ode.hip (the Rademacher draw and the row dot product) between two HIP events with the bytes they move.  Weights
seeded as tools/bench_dopri5.py seeds them.  Writes profiles/likelihood_bench.txt line by line.

OFF = the existing full backward with the parameters requiring grad (what a caller had before the mode existed: every weight gradient is
computed and dropped with the graph).  The report states times; it draws no conclusion.

Needs an MI355X; there is no CPU path.  usage: python tools/bench_likelihood.py [--batch 64] [--reps 5] [--iters 10] [--out FILE]"""
import argparse
import os
import sys

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10, help="drift evaluations per timed repetition")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "likelihood_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_likelihood needs an MI355X"
    from ldmae_amd import ops
    from ldmae_amd.train_accum import build_model
    device = torch.device("cuda", 0)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "ldmae_amd/configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml")))
    model = build_model(cfg)
    gsd = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for nm, p in model.named_parameters():
            if "adaLN_modulation" in nm or nm.startswith("final_layer.linear"):
                p.copy_(torch.randn(p.shape, generator=gsd) * 0.02)
    model = model.to(device).eval()
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    size = model.x_embedder.img_size[0]
    g = torch.Generator().manual_seed(1)
    x = torch.randn(a.batch, model.in_channels, size, size, generator=g).to(device)
    t = torch.rand(a.batch, generator=g).to(device)
    y = torch.randint(0, cfg["data"]["num_classes"], (a.batch,), generator=g).to(device)
    eps = ops.rademacher(x.shape, 0, 0, device)
    say(f"# tools/bench_likelihood.py: LightningDiT-B/1, batch {a.batch}, latent {tuple(x.shape[1:])}, {torch.cuda.get_device_name(0)}")
    say(f"# one drift evaluation = forward + vector-Jacobian product; {a.iters} evaluations per repetition, {a.reps} repetitions, ON / OFF alternating")

    def drift(on):
        xg = x.detach().requires_grad_(True)
        if on:
            with model.input_grad_only():
                v = model(xg, t, y)
        else:
            v = model(xg, t, y)
        (vjp,) = torch.autograd.grad(v, xg, eps)
        return vjp

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    for prec in ("bf16", "f32"):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec == "bf16"):
            same = torch.equal(drift(True), drift(False))           # also the warm-up of both
            drift(True), drift(False)
            ts = {True: [], False: []}
            for _ in range(a.reps):
                for on in (True, False):
                    ts[on].append(timed(lambda: drift(on)))
        med = {on: sorted(v)[len(v) // 2] for on, v in ts.items()}
        say(f"{prec}: input-only ON  ms / evaluation: " + " ".join(f"{v:.3f}" for v in ts[True]) + f"  (median {med[True]:.3f})")
        say(f"{prec}: input-only OFF ms / evaluation: " + " ".join(f"{v:.3f}" for v in ts[False]) + f"  (median {med[False]:.3f})")
        say(f"{prec}: dx bitwise equal ON / OFF: {same}")

    n = x.numel()
    vjp = torch.randn_like(x)
    for name, fn, nbytes in (("rademacher", lambda: ops.rademacher(x.shape, 0, 1, device), 4 * n),
                             ("rowdot", lambda: ops.rowdot(vjp, eps), 8 * n)):
        fn()
        ms = sorted(timed(fn) for _ in range(a.reps))[a.reps // 2]
        say(f"{name}: n = {n}: {ms * 1e3:.1f} us per call (median of {a.reps} x {a.iters}, launch and allocation included), {nbytes} B moved")


if __name__ == "__main__":
    main()
