#!/usr/bin/env python3
"""dopri5 against euler-250 on LightningDiT-B/1 with CFG, batch 64 (doubled to 128), bf16 autocast: model and noise seeded as
`bench.py --workload do_sample` builds them.  Writes profiles/ode_dopri5.txt:

  * nfe / accepted / rejected of dopri5 at the shipped atol / rtol;
  * wall time per sample batch, euler-250 and dopri5 alternating in one process (after a warm-up of each), every repetition listed;
  * the solver's own kernels of one attempted step (6 stages, finish + fold, controller) between two HIP events, against the six model
    evaluations of the same step, and the bytes those kernels move over the time (share of the HBM peak);
  * max|x_dopri5 - x_euler250| / max|x_euler250| on the final latents.

Needs an MI355X; there is no CPU path.  usage: python tools/bench_dopri5.py [--batch 64] [--reps 3] [--out profiles/ode_dopri5.txt]"""
import argparse
import copy
import os
import sys
import time

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12          # B/s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-steps", type=int, default=2000, help="cap on attempted dopri5 steps per grid point (the run fails beyond it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ode_dopri5.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dopri5 needs an MI355X"
    from ldmae_amd import inference as inf, ops
    from ldmae_amd.train_accum import build_model
    from ldmae_amd.transport import integrators as I
    device = torch.device("cuda", 0)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "ldmae_amd/configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml")))
    model = build_model(cfg)
    gsd = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for nm, p in model.named_parameters():
            if "adaLN_modulation" in nm or nm.startswith("final_layer.linear"):
                p.copy_(torch.randn(p.shape, generator=gsd) * 0.02)
    model = model.to(device).eval()
    s = cfg["sample"]
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    fns = {}
    for method in ("euler", "dopri5"):
        c = copy.deepcopy(cfg)
        c["sample"]["sampling_method"] = method
        fns[method] = inf.build_sampler(c)
    fns["dopri5"].__self__.max_num_steps = a.max_steps

    def run(method):
        gen = torch.Generator(device=device).manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            lat, _ = inf.sample_latents(model, fns[method], a.batch, s["cfg_scale"], s.get("cfg_interval_start", 0), device, cfg["data"]["num_classes"], generator=gen)
        torch.cuda.synchronize()
        return lat, time.perf_counter() - t0

    say(f"# tools/bench_dopri5.py: LightningDiT-B/1, batch {a.batch} (CFG: {2 * a.batch}), bf16 autocast, cfg {s['cfg_scale']}, interval start "
        f"{s.get('cfg_interval_start', 0)}, timestep_shift {s.get('timestep_shift', 0)}, atol {s['atol']}, rtol {s['rtol']}, grid {s['num_sampling_steps']}")
    lat = {}
    for method in ("euler", "dopri5"):               # warm-up of every shape
        lat[method], sec = run(method)
        say(f"warm-up {method}: {sec:.3f} s")
    o = fns["dopri5"].__self__
    say(f"dopri5: nfe {o.nfe}, accepted {o.accepted}, rejected {o.rejected}")
    for r in range(a.reps):
        for method in ("euler", "dopri5"):
            out, sec = run(method)
            assert torch.equal(out, lat[method]), method + ": not reproducible"
            say(f"rep {r} {method}: {sec:.3f} s per sample batch")
    d = float((lat["dopri5"] - lat["euler"]).abs().max() / lat["euler"].abs().max())
    say(f"max|x_dopri5 - x_euler250| / max|x_euler250| = {d:.4e}")

    # one attempted step: the solver's kernels against its six model evaluations
    shape = (2 * a.batch, model.in_channels) + tuple(model.x_embedder.img_size)
    n = 1
    for v in shape:
        n *= v
    ld = ops.ode_slab_ld(n)
    k = torch.randn(7, ld, device=device)
    yb = torch.randn(3, ld, device=device)
    y, y1, yt = (yb[i, :n] for i in range(3))
    st = torch.tensor([0.3, 0.01, 0.0] + [0.0] * 6, device=device)
    partial = torch.empty(ops.ode_partials(n), device=device)
    tvec = torch.zeros(shape[0], device=device)
    labels = torch.cat([torch.zeros(a.batch, dtype=torch.long), torch.full((a.batch,), cfg["data"]["num_classes"])]).to(device)

    reset = st[0:2].clone()

    def solver_step():
        st[0:2].copy_(reset)                       # the controller moves t and h: every repetition starts from the same scalars
        for sidx in range(1, 7):
            ops.rk_stage(y, k, I.DP_A[sidx], st[1:2], yt, st[0:1], I.DP_C[sidx], tvec)
        ops.dopri5_finish(y, k, st[1:2], s["atol"], s["rtol"], y1, partial, st[2:3])
        ops.dopri5_advance(st[2:3], st[1:2], st[0:1], st[3:9])

    def model_step():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            for sidx in range(6):
                k[sidx + 1, :n].view(shape).copy_(model.forward_with_cfg(yt.view(shape), tvec, labels, s["cfg_scale"], True, s.get("cfg_interval_start", 0)))

    def timed(fn, reps):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    ms_solver, ms_model = timed(solver_step, 20), timed(model_step, 3)
    nbytes = 4 * n * (sum(m + 2 for m in range(1, 7)) + 8)
    say(f"one attempted step, state {shape} = {4 * n / 1e6:.1f} MB: solver kernels {ms_solver:.3f} ms ({nbytes / 1e6:.0f} MB moved, "
        f"{nbytes / ms_solver / 1e9:.2f} TB/s = {100 * nbytes / (ms_solver * 1e-3) / HBM_PEAK:.0f} % of the HBM peak), six model evaluations with their "
        f"copies into the slab {ms_model:.1f} ms: the solver is {100 * ms_solver / (ms_solver + ms_model):.2f} % of the step")


if __name__ == "__main__":
    main()
