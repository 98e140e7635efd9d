#!/usr/bin/env python3
"""Cost of the validation objective on one MI355X: the two kernels of csrc/fm_valid.hip at B 256, C 16, HW 1024 against the torch chain they
replace (two randn, the prologue kernel, ICPlan.plan, mean_flat((out - ut) ** 2)), in alternating rounds, and one whole validation batch
on LightningDiT-B/1 with the share of it the objective takes.  Writes profiles/validate_bench.txt (or --out).
      python tools/bench_validate.py [--batch 256] [--model-batch 64] [--rounds 7] [--iters 20]

By the bytes: the plan reads the stored moments (8 B per output element: mean and logvar) and writes xt and ut (8 B); the loss reads the model
output and ut (8 B, or 6 B for a bf16 output).  Both draws are generated in registers (two Philox blocks and four Box-Muller pairs per four
elements), so the plan may be bound by the vector units instead of HBM: the figure below says which."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ldmae_amd import ops                                          # noqa: E402
from ldmae_amd.transport.path import ICPlan                        # noqa: E402
from ldmae_amd.transport.utils import mean_flat                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--channels", type=int, default=16)
ap.add_argument("--hw", type=int, default=1024)
ap.add_argument("--model-batch", type=int, default=64, help="batch of the whole-batch measurement on LightningDiT-B/1")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20, help="calls per timed window of the kernel measurements")
ap.add_argument("--model-iters", type=int, default=10, help="calls per timed window of the whole-batch measurement")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validate_bench.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
B, C, HW = a.batch, a.channels, a.hw
side = int(round(HW ** 0.5))
assert side * side == HW
g = torch.Generator(device="cuda").manual_seed(0)
stored = torch.randn(B, 2 * C, side, side, device="cuda", generator=g)
mean, std = torch.randn(C, device="cuda", generator=g) * 0.1, torch.rand(C, device="cuda", generator=g) + 0.5
idx = torch.arange(B, device="cuda", dtype=torch.int64)
t = torch.rand(B, device="cuda", generator=g)
out = torch.randn(B, C, side, side, device="cuda", generator=g)
plan = ICPlan()
hold = {}


def k_plan():
    hold["xt"], hold["ut"] = ops.fm_valid_plan(stored, idx, t, mean, std, 1.0, True, 0)


def t_plan():
    z, x0 = torch.randn(B, C, side, side, device="cuda"), torch.randn(B, C, side, side, device="cuda")
    x1 = ops.latent_prologue(stored, z, mean, std, 1.0, True)
    _, hold["xt"], hold["ut"] = plan.plan(t, x0, x1)


def k_loss():
    hold["loss"] = ops.row_mse(out, hold["ut"])


def t_loss():
    hold["loss"] = mean_flat((out - hold["ut"]) ** 2)


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
    return [(statistics.median(x), min(x), max(x)) for x in ts]


n = B * C * HW
(kp, tp, kl, tl) = rounds([k_plan, t_plan, k_loss, t_loss], a.iters)
lines = [f"validation objective on {torch.cuda.get_device_name(0)}: B {B}, C {C}, HW {HW} ({n} elements per tensor); {a.rounds} alternating rounds of "
         f"{a.iters} calls, device events"]
fmt = lambda x: f"median {x[0] * 1e3:.1f} us (min {x[1] * 1e3:.1f} .. max {x[2] * 1e3:.1f})"          # noqa: E731
lines.append(f"  plan, ldmae_fm_valid_plan_f32 (1 launch)                      : {fmt(kp)}; 16 B per element = {16 * n / 1e6:.1f} MB -> "
             f"{16 * n / kp[0] / 1e9:.2f} TB/s")
lines.append(f"  plan, torch chain (2 randn, prologue kernel, ICPlan.plan)      : {fmt(tp)}")
lines.append(f"  loss, ldmae_row_mse f32 (2 launches)                          : {fmt(kl)}; 8 B per element = {8 * n / 1e6:.1f} MB -> "
             f"{8 * n / kl[0] / 1e9:.2f} TB/s")
lines.append(f"  loss, torch chain (sub, square, mean over dims 1..3)           : {fmt(tl)}")
lines.append(f"  both kernels {(kp[0] + kl[0]) * 1e3:.1f} us against {(tp[0] + tl[0]) * 1e3:.1f} us for the chains they replace "
             f"({(tp[0] + tl[0]) / (kp[0] + kl[0]):.2f} x); the chain's draws come from torch's generator and are not named")

# one whole validation batch on LightningDiT-B/1 (bf16 autocast, eval, no_grad): objective + forward + loss, and the objective's share
import yaml                                                        # noqa: E402
from ldmae_amd.train_accum import build_model                      # noqa: E402
Bm = a.model_batch
with open(os.path.join(ROOT, "ldmae_amd/configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml")) as f:
    model = build_model(yaml.safe_load(f))
assert model.in_channels == C and model.x_embedder.img_size[0] == side, "the whole-batch measurement runs at the shipped configuration: C 16, HW 1024"
with torch.no_grad():                                              # an untrained final layer is zero: give the output ordinary values
    for nm, p in model.named_parameters():
        if "adaLN_modulation" in nm or nm.startswith("final_layer.linear"):
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(1)) * 0.02)
model = model.cuda().eval().requires_grad_(False)
y = torch.randint(0, 1000, (Bm,), device="cuda", generator=g)
st_m, idx_m, t_m = stored[:Bm].contiguous(), idx[:Bm].contiguous(), t[:Bm].contiguous()
xt_m, ut_m = ops.fm_valid_plan(st_m, idx_m, t_m, mean, std, 1.0, True, 0)


def fwd():
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        hold["out"] = model(xt_m, t_m, y=y)


def objective():
    xt, ut = ops.fm_valid_plan(st_m, idx_m, t_m, mean, std, 1.0, True, 0)
    hold["l"] = ops.row_mse(hold["out"], ut)


def whole():
    xt, ut = ops.fm_valid_plan(st_m, idx_m, t_m, mean, std, 1.0, True, 0)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        o = model(xt, t_m, y=y)
    hold["l"] = ops.row_mse(o, ut)


fwd()
(tf, to, tw) = rounds([fwd, objective, whole], a.model_iters)
lines.append(f"  a validation batch of {Bm} on LightningDiT-B/1 (bf16 autocast, eval, no_grad; {a.rounds} rounds of {a.model_iters} calls; shard reads and the "
             f"host-to-device copy not included; the loss includes the copy of the model's permuted output view):")
lines.append(f"    forward alone            : median {tf[0]:.3f} ms (min {tf[1]:.3f} .. max {tf[2]:.3f})")
lines.append(f"    plan + loss alone        : median {to[0]:.3f} ms (min {to[1]:.3f} .. max {to[2]:.3f})")
lines.append(f"    plan + forward + loss    : median {tw[0]:.3f} ms (min {tw[1]:.3f} .. max {tw[2]:.3f}); the objective is {100 * to[0] / tw[0]:.1f} % of the batch")
lines.append("  not measured: whether the held-out loss ranks EMA widths as FID does (needs a trained run); the shard reads of a real validation set; "
             "a multi-rank run")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
