#!/usr/bin/env python3
"""Cost of the guidance rules on one MI355X: the one launch of csrc/guidance.hip for each rule at the shipped sampling shape (256 x 16 x 32 x
32, f32 model outputs) against the torch chain of LightningDiT.forward_with_cfg (slice, split, sub, mul, add, two cats) on the same operands, in
alternating rounds, and the share of one guided step the rule takes next to the model forward on the doubled batch.  Writes
profiles/guidance_bench.txt (or --out).
      python tools/bench_guidance.py [--batch 256] [--rounds 7] [--iters 20]

By the bytes, per guided element: cfg reads p and q and writes g (12 B); rescale reads p and q twice (the second time from L2 / MALL when the
sample fits) and writes g (20 B issued, 12 B from HBM at best); apg reads p, q and x twice and writes g (28 B issued, 16 B at best), plus 8 B
(read) + 4 B (write) with a momentum buffer.  Pass-through channels cost 8 B each.  The figures below use the bytes that must cross HBM at
least once."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ldmae_amd import ops                                          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--channels", type=int, default=16)
ap.add_argument("--side", type=int, default=32)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20, help="calls per timed window of the kernel measurements")
ap.add_argument("--model-iters", type=int, default=3, help="calls per timed window of the model measurements")
ap.add_argument("--skip-model", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_bench.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
B, C, S = a.batch, a.channels, a.side
g = torch.Generator(device="cuda").manual_seed(0)
both = torch.randn(2 * B, C, S, S, device="cuda", generator=g)      # the model's output on the doubled batch
pos, neg = both[:B], both[B:]
x = torch.randn(B, C, S, S, device="cuda", generator=g)
t = torch.rand(B, device="cuda", generator=g) * 0.8 + 0.1
mom = torch.zeros(B, C * S * S, device="cuda")
out = torch.empty(B, C, S, S, device="cuda")
hold = {}
SCALE = 10.0


def torch_chain():
    """forward_with_cfg after the model call, verbatim: guidance on the first three channels of the doubled output."""
    eps, rest = both[:, :3], both[:, 3:]
    cond_eps, uncond_eps = torch.split(eps, len(eps) // 2, dim=0)
    half_eps = uncond_eps + SCALE * (cond_eps - uncond_eps)
    eps = torch.cat([half_eps, half_eps], dim=0)
    hold["o"] = torch.cat([eps, rest], dim=1)


def torch_chain_all():
    """The same expression on all channels: what an all-channel CFG costs in torch (sub, mul, add)."""
    hold["o"] = neg + SCALE * (pos - neg)


def kernel(rule, k, m=None):
    return lambda: ops.guidance_combine(rule, pos, neg, SCALE, k=k, x=x, t=t, phi=0.7, eta=0.0, norm_threshold=2.5,
                                        momentum=-0.5 if m is not None else 0.0, mom=m, out=out)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def rounds(fns, iters):
    """Alternating rounds: drift of the clocks or of a neighbour's load hits every variant alike.  Median, min, max per variant (ms)."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(a.rounds):
        for k, fn in enumerate(fns):
            ts[k].append(timed(fn, iters))
    return [(statistics.median(v), min(v), max(v)) for v in ts]


n = B * C * S * S
n3 = B * 3 * S * S
# (label, function, bytes that must cross HBM)
cases = [("torch chain of forward_with_cfg, k = 3 (7 launches)", torch_chain, None),
         ("torch q + s (p - q) on all channels (3 launches)", torch_chain_all, None),
         ("kernel cfg, k = 3", kernel("cfg", 3), 12 * n),
         ("kernel cfg, k = all", kernel("cfg", C), 12 * n),
         ("kernel rescale, k = 3", kernel("rescale", 3), 12 * n),
         ("kernel rescale, k = all", kernel("rescale", C), 12 * n),
         ("kernel apg, k = 3", kernel("apg", 3), 12 * n + 4 * n3),
         ("kernel apg, k = all", kernel("apg", C), 16 * n),
         ("kernel apg, k = all, momentum", kernel("apg", C, mom), 24 * n)]
res = rounds([c[1] for c in cases], a.iters)
prop = torch.cuda.get_device_properties(0)
lines = [f"guidance rules on {prop.name} ({prop.gcnArchName}, {prop.multi_processor_count} CUs): B {B}, C {C}, H x W {S} x {S}, f32 ({n} elements per "
         f"tensor); {a.rounds} alternating rounds of {a.iters} calls, device events; one launch per kernel call",
         f"  the operands of a call ({12 * n / 1e6:.0f} to {24 * n / 1e6:.0f} MB) fit in the 256 MB Infinity Cache and every call reads the same ones, as a "
         "sampler reads the output the model has just written: the rates below are cache-warm rates, not HBM rates"]
for (label, _, nbytes), r in zip(cases, res):
    line = f"  {label:58s}: median {r[0] * 1e3:7.1f} us (min {r[1] * 1e3:.1f} .. max {r[2] * 1e3:.1f})"
    if nbytes:
        line += f"; {nbytes / 1e6:.1f} MB at least -> {nbytes / r[0] / 1e9:.2f} TB/s"
    lines.append(line)
lines.append(f"  cfg k = 3: the kernel takes {res[2][0] / res[0][0]:.2f} x the time of the torch chain it stands in for; all channels: "
             f"{res[3][0] / res[1][0]:.2f} x of the three torch launches")

if not a.skip_model:
    import yaml                                                    # noqa: E402
    from ldmae_amd.train_accum import build_model                  # noqa: E402
    with open(os.path.join(ROOT, "ldmae_amd/configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml")) as f:
        model = build_model(yaml.safe_load(f))
    assert model.in_channels == C and model.x_embedder.img_size[0] == S, "the step measurement runs at the shipped configuration"
    with torch.no_grad():                                          # an untrained final layer is zero: give the output ordinary values
        for nm, p in model.named_parameters():
            if "adaLN_modulation" in nm or nm.startswith("final_layer.linear"):
                p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(1)) * 0.02)
    model = model.cuda().eval().requires_grad_(False)
    y = torch.randint(0, 1000, (B,), device="cuda", generator=g)
    x2, t2, y2 = torch.cat([x, x]), torch.cat([t, t]), torch.cat([y, torch.full_like(y, 1000)])

    def fwd():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            hold["v"] = model(x2, t2, y2)

    def step(rule):
        def run():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                v = model(x2, t2, y2)
            ops.guidance_combine(rule, v[:B], v[B:], SCALE, k=C, x=x, t=t, norm_threshold=2.5, out=out)
        return run

    def old_step():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            hold["v"] = model.forward_with_cfg(x2, t2, y2, SCALE, True, 0.1)

    mres = rounds([fwd, old_step, step("cfg"), step("rescale"), step("apg")], a.model_iters)
    lines.append(f"  one guided evaluation on LightningDiT-B/1, doubled batch {2 * B} (bf16 autocast, eval, no_grad; {a.rounds} rounds of {a.model_iters} "
                 f"calls; the rule's time includes the copy of the model's permuted output view):")
    names = ["model forward alone", "forward_with_cfg (k = 3, torch chain)", "forward + kernel cfg, all channels", "forward + kernel rescale, all channels",
             "forward + kernel apg, all channels"]
    for nm, r in zip(names, mres):
        share = "" if nm == names[0] else f"; {100 * (r[0] - mres[0][0]) / r[0]:.2f} % of it beyond the forward"
        lines.append(f"    {nm:42s}: median {r[0]:8.3f} ms (min {r[1]:.3f} .. max {r[2]:.3f}){share}")
lines.append("  not measured: the effect of any rule on FID (no trained checkpoint is available); a guide model smaller than the main one; a multi-rank "
             "run")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
