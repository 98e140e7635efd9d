#!/usr/bin/env python3
"""The SDE sampler on LightningDiT-B/1 at batch 64 (bf16 autocast): (1) the solver's kernels of csrc/ode.hip per step -- the Euler-Maruyama launch
with the draw generated in the kernel, the same step with a stored draw (ldmae_normal_f32 + the tensor form), Heun's three launches -- between two
HIP events, with the bytes they move, against one model forward; (2) Sampler.sample_sde's loop (one model call per drift evaluation) against a
two-call restatement of the same steps in torch (the SDE drift assembled as the reference assembles it, v from one model call and the score from a
second one, th.randn for the noise), alternating in one process, every repetition listed.  Weights seeded as tools/bench_dopri5.py seeds them.
Writes profiles/sde_bench.txt line by line.  The report states times; it draws no conclusion.

Needs an MI355X; there is no CPU path.  usage: python tools/bench_sde.py [--batch 64] [--steps 20] [--reps 5] [--iters 200] [--out FILE]"""
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
    ap.add_argument("--steps", type=int, default=20, help="num_steps of the timed sampling loops")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200, help="kernel launches per timed repetition")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sde_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sde needs an MI355X"
    from ldmae_amd import ops
    from ldmae_amd.train_accum import build_model
    from ldmae_amd.transport import Sampler, create_transport, path
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
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    size = model.x_embedder.img_size[0]
    g = torch.Generator().manual_seed(1)
    x = torch.randn(a.batch, model.in_channels, size, size, generator=g).to(device)
    y = torch.randint(0, cfg["data"]["num_classes"], (a.batch,), generator=g).to(device)
    tvec = torch.full((a.batch,), 0.5, device=device)
    n = x.numel()
    say(f"# tools/bench_sde.py: LightningDiT-B/1, bf16 autocast, batch {a.batch}, latent {tuple(x.shape[1:])}, n = {n} state elements, {torch.cuda.get_device_name(0)}")

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    # ---- (1) the solver's kernels, per launch (enqueue from Python included: what the loop pays)
    v, v2, xp, out, z = (torch.randn_like(x) for _ in range(5))
    kernels = (
        ("Euler step, draw in the kernel   (2 in + 1 out)", 12 * n, lambda: ops.sde_combine((x, v), (0.9, 0.05), out, noise_coef=0.3, seed=1, counter=3, t_next=0.5, t_out=tvec)),
        ("Euler step, stored draw          (3 in + 1 out)", 16 * n, lambda: ops.sde_combine((x, v), (0.9, 0.05), out, noise_coef=0.3, z=z, t_next=0.5, t_out=tvec)),
        ("normal draw alone                (1 out)", 4 * n, lambda: ops.normal(None, 1, 3, device, out=z)),
        ("Heun xhat = x + c z, in kernel   (1 in + 1 out)", 8 * n, lambda: ops.sde_combine((x,), (1.0,), out, noise_coef=0.3, seed=1, counter=3)),
        ("Heun predictor                   (2 in + 1 out)", 12 * n, lambda: ops.sde_combine((x, v), (0.9, 0.05), xp, t_next=0.5, t_out=tvec)),
        ("Heun corrector                   (4 in + 1 out)", 20 * n, lambda: ops.sde_combine((x, v, xp, v2), (0.9, 0.05, -0.02, 0.03), out, t_next=0.5, t_out=tvec)))
    say(f"# kernels: median of {a.reps} repetitions of {a.iters} launches, us per launch; bytes = what the algorithm needs")
    for name, nbytes, fn in kernels:
        fn()
        ts = sorted(timed(fn, a.iters) for _ in range(a.reps))
        us = ts[a.reps // 2] * 1e3
        say(f"{name}: {us:8.1f} us  (min {ts[0] * 1e3:.1f}, max {ts[-1] * 1e3:.1f}); {nbytes} B -> {nbytes / us * 1e-6:.2f} TB/s")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        model(x, tvec, y)
        ts = sorted(timed(lambda: model(x, tvec, y), 10) for _ in range(a.reps))
    fwd = ts[a.reps // 2]
    say(f"one model forward: {fwd:.3f} ms (median of {a.reps} x 10; min {ts[0]:.3f}, max {ts[-1]:.3f})")

    # ---- (2) the loop: one model call per drift evaluation against the two-call restatement
    form, norm, last_size = "sigma", 1.0, 0.04
    smp = Sampler(create_transport())

    def two_call(method):
        """The steps of integrators.sde with the drift the way the reference builds it: drift(x, t) + w(t) * score(x, t), each of the two terms
        from its own model call; torch elementwise arithmetic, th.randn."""
        t = torch.linspace(0, 1 - last_size, a.steps)
        dt = float(t[1] - t[0])

        def sde_drift(xx, tt):
            tv = torch.full((a.batch,), tt, device=device)
            sa, sb = path.score_from_velocity(tt)
            return model(xx, tv, y).float() + path.diffusion(tt, form, norm) * (sa * model(xx, tv, y).float() + sb * xx)

        def run():
            xx = x
            for k in range(a.steps - 1):
                tk = float(t[k])
                w = path.diffusion(tk, form, norm)
                if method == "Euler":
                    xx = xx + dt * sde_drift(xx, tk) + (2 * w * dt) ** 0.5 * torch.randn_like(xx)
                else:
                    xh = xx + (2 * w * dt) ** 0.5 * torch.randn_like(xx)
                    k1 = sde_drift(xh, tk)
                    xx = xh + 0.5 * dt * (k1 + sde_drift(xh + dt * k1, tk + dt))
            return xx + last_size * sde_drift(xx, float(t[-1]))
        return run

    for method in ("Euler", "Heun"):
        fn = smp.sample_sde(sampling_method=method, diffusion_form=form, diffusion_norm=norm, last_step="Mean", last_step_size=last_size,
                            num_steps=a.steps, seed=0, keep_trajectory=False)
        one, two = (lambda: fn(x, model.forward, y=y)[-1]), two_call(method)
        ts = {"one": [], "two": []}
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            fin = bool(torch.isfinite(one()).all()) and bool(torch.isfinite(two()).all())        # also the warm-up of both
            for _ in range(a.reps):
                ts["one"].append(timed(one, 1))
                ts["two"].append(timed(two, 1))
        calls2 = 2 * fn.model_calls
        for key, label, calls in (("one", "sample_sde (one call per evaluation)", fn.model_calls), ("two", "two-call restatement in torch   ", calls2)):
            med = sorted(ts[key])[a.reps // 2]
            say(f"{method}, {a.steps} steps, {label}: {calls} model calls, ms per sample batch: " + " ".join(f"{v:.1f}" for v in ts[key])
                + f"  (median {med:.1f}; {med / calls:.3f} ms per model call)")
        say(f"{method}: both loops finite: {fin}")


if __name__ == "__main__":
    main()
