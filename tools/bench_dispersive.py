#!/usr/bin/env python3
"""Cost of the Dispersive Loss on one MI355X at the bench shape (B = 256 samples x K = 1024 tokens x 768 = 786 432 features, f32: 805 MB):
the two kernels of csrc/dispersive.hip against a torch restatement on the same z (z @ z.T in f32 plus the elementwise chain; C @ z), in
alternating rounds, and the bf16 train step of bench.py's model with and without train.dispersive, alternating.  The step without the key
is the parent's.  Writes profiles/dispersive_bench.txt (or --out).
      python tools/bench_dispersive.py [--batch 256] [--rounds 7] [--iters 10] [--step-iters 3]

By the shapes: each product is 2 B^2 K = 103 GFLOP (the forward computes the 10 of 16 64 x 64 tiles on or above the diagonal of a 256 x 256 G: 64 GFLOP);
the forward must read z once (805 MB) and writes slabs x B^2 x 4 bytes of partial tiles; the backward reads z and writes dz (1.61 GB).  The
least time of a kernel is the larger of FLOP / 157.3 TF/s (f32 MFMA peak) and bytes / 8 TB/s (HBM peak)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                       # noqa: E402
from ldmae_amd import _lib, ops                                    # noqa: E402
from ldmae_amd.transport import create_transport                   # noqa: E402
from ldmae_amd.transport.transport import dispersive_options       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--features", type=int, default=1024 * 768)
ap.add_argument("--tau", type=float, default=0.5)
ap.add_argument("--weight", type=float, default=0.5)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=10, help="calls per timed window of the kernel measurements")
ap.add_argument("--step-iters", type=int, default=3, help="steps per timed window of the train-step measurement")
ap.add_argument("--skip-step", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dispersive_bench.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
B, K, TAU = a.batch, a.features, a.tau
PEAK_TF, PEAK_TBS = 157.3, 8.0
g = torch.Generator(device="cuda").manual_seed(0)
z = torch.randn(B, K, device="cuda", generator=g)
dz = torch.empty_like(z)
hold = {}


def torch_fwd():
    G = z @ z.T
    n = torch.diagonal(G)
    d = (n[:, None] + n[None, :] - 2 * G).clamp_min(0)
    d.fill_diagonal_(0)
    e = torch.exp(-d / (K * TAU))
    r = e.sum(1)
    S = r.sum()
    hold["L"] = torch.log(S) - 2 * torch.log(torch.tensor(float(B), device="cuda"))
    hold["C"] = 4 / (S * K * TAU) * (e - torch.diag(r))


def torch_bwd():
    hold["dz"] = a.weight * (hold["Ct"] @ z)


def hip_fwd():
    hold["loss"], hold["Ck"] = ops.dispersive_fwd(z, TAU)


def hip_bwd():
    ops.dispersive_bwd(hold["Ck"], z, a.weight, out=dz)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def rounds(fns, iters, warm=3):
    """Alternating rounds: drift of the clocks or of a neighbour's load hits every variant alike.  Median, min, max per variant (ms)."""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(a.rounds):
        for k, fn in enumerate(fns):
            ts[k].append(timed(fn, iters))
    return [(statistics.median(v), min(v), max(v)) for v in ts]


torch_fwd()
hip_fwd()
hold["Ct"] = hold["C"].clone()
torch.cuda.synchronize()
slabs = _lib.load().ldmae_dispersive_slabs(B, K)
ws = _lib.load().ldmae_dispersive_workspace_bytes(B, K)
t64 = -(-B // 64)
tiles = t64 * (t64 + 1) // 2
flop_f = 2.0 * tiles * 64 * 64 * K
flop_b = 2.0 * B * B * K
bytes_f = 4.0 * B * K + 4.0 * slabs * B * B
bytes_b = 8.0 * B * K
cases = [("torch forward: z @ z.T (f32) + elementwise chain", torch_fwd, None, None),
         ("kernel forward: ldmae_dispersive_fwd (4 launches)", hip_fwd, flop_f, bytes_f),
         ("torch backward: weight * (C @ z)", torch_bwd, None, None),
         ("kernel backward: ldmae_dispersive_bwd (1 launch)", hip_bwd, flop_b, bytes_b)]
res = rounds([c[1] for c in cases], a.iters)
prop = torch.cuda.get_device_properties(0)
dL = abs(float(hold["loss"]) - float(hold["L"]))
dC = float((hold["Ck"] - hold["C"]).abs().max() / hold["C"].abs().max())
lines = [f"Dispersive Loss on {prop.name} ({prop.gcnArchName}, {prop.multi_processor_count} CUs): z [{B}, {K}] f32 ({4 * B * K / 1e6:.0f} MB), N(0, 1) values, "
         f"tau {TAU}; {a.rounds} alternating rounds of {a.iters} calls, device events",
         f"  split plan: {slabs} K-slabs, workspace {ws / 1e6:.1f} MB; kernel against torch on this z: |L - L_torch| = {dL:.2e}, "
         f"max |C - C_torch| / max |C| = {dC:.2e}"]
for (label, _, flop, nbytes), r in zip(cases, res):
    line = f"  {label:52s}: median {r[0]:7.3f} ms (min {r[1]:.3f} .. max {r[2]:.3f})"
    if flop:
        least = max(flop / (PEAK_TF * 1e12), nbytes / (PEAK_TBS * 1e12)) * 1e3
        by = "MFMA" if flop / (PEAK_TF * 1e12) > nbytes / (PEAK_TBS * 1e12) else "HBM"
        line += (f"; {flop / 1e9:.0f} GFLOP -> {flop / r[0] / 1e9:.1f} TF/s, {nbytes / 1e6:.0f} MB -> {nbytes / r[0] / 1e9:.2f} TB/s; least time {least:.3f} ms "
                 f"({by}-bound): {100 * least / r[0]:.0f} % of it")
    lines.append(line)
lines.append(f"  forward: the kernel takes {res[1][0] / res[0][0]:.2f} x the time of the torch restatement; backward: {res[3][0] / res[2][0]:.2f} x")

if not a.skip_step:
    del dz
    hold.clear()
    torch.cuda.empty_cache()
    model, opt, reducer, transport = bench.build(torch.device("cuda"), B)
    depth = len(model.blocks)
    disp = dispersive_options({"weight": a.weight, "tau": TAU}, depth, per_gpu_batch=B)
    tapped = create_transport("Linear", "velocity", None, None, None, use_cosine_loss=False, use_lognorm=True, dispersive=disp)
    x = torch.randn(B, 16, 32, 32, device="cuda", generator=g)
    y = torch.randint(0, 1000, (B,), device="cuda", generator=g)

    def step_parent():
        hold["loss"] = bench.train_step(model, opt, reducer, transport, x, y)

    def step_disp():                                               # train_accum.py's loss with the key set
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            terms = tapped.training_losses(model, x, dict(y=y))
        loss = terms["loss"].mean() + disp["weight"] * terms["disp_loss"]
        loss.backward()
        opt.step(grad_scale=reducer.finish())
        hold["disp"] = terms["disp_loss"].detach()

    sres = rounds([step_parent, step_disp], a.step_iters, warm=4)
    over = sres[1][0] - sres[0][0]
    lines.append(f"  bf16 train step of bench.py's model (LightningDiT-B/1, batch {B}, fwd + bwd + AdamW + EMA), block {disp['block']} of {depth} tapped, "
                 f"weight {a.weight}; {a.rounds} alternating rounds of {a.step_iters} steps:")
    lines.append(f"    without train.dispersive (the parent's step): median {sres[0][0]:8.3f} ms (min {sres[0][1]:.3f} .. max {sres[0][2]:.3f})")
    lines.append(f"    with train.dispersive                       : median {sres[1][0]:8.3f} ms (min {sres[1][1]:.3f} .. max {sres[1][2]:.3f}); "
                 f"{over:+.3f} ms = {100 * over / sres[0][0]:+.2f} %; the two kernels alone are {res[1][0] + res[3][0]:.3f} ms of it; the rest is "
                 f"block {disp['block']}'s private gradient copy and own gate backward, block {disp['block'] + 1}'s unfused norm backward, autograd's add of dz "
                 f"and the host read of the upstream factor")
    lines.append(f"    last Dispersive Loss {float(hold['disp']):.4f} (in [-log B, 0] = [{-torch.log(torch.tensor(float(B))).item():.4f}, 0])")
lines.append("  not measured: the effect of the term on FID (no trained checkpoint is available); other batch sizes; a multi-rank run")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
