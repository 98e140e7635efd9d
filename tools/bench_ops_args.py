#!/usr/bin/env python3
"""Host cost of the argument checks of ldmae_amd/ops.py against another revision of that file, where host time is not hidden behind the GPU.

  python tools/bench_ops_args.py wrappers --other OPS.py    host microseconds per call of the training path's wrappers at one-tile shapes: this
                                                            tree's ops.py and OPS.py (a copy of another revision's file, loaded beside it under
                                                            another module name) in ONE process, called alternately in blocks, 5 repeats each
  python tools/bench_ops_args.py steps [--ops OPS.py]       the launch-bound train steps -- the tiny DiT of tests/test_gpu_dit.py (bf16, batch 4)
                                                            and a depth-2 VMAE (128 px, batch 2): forward, backward, optimizer step -- ms per
                                                            step over 200 steps after warm-up, 5 repeats.  --ops: that file takes the place of
                                                            ldmae_amd.ops in this process (run once with, once without, and compare the spreads)
  python tools/bench_ops_args.py bench --ops OPS.py -- <bench.py arguments>
                                                            bench.py itself, unchanged, with OPS.py in the place of ldmae_amd.ops: one JSON line per
                                                            run; run it five times per revision, alternating, for the spread of the step figures
profiles/ops_args_host.txt holds the three sets of figures."""
import argparse
import importlib.util
import os
import runpy
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF16, F32 = torch.bfloat16, torch.float32


def load_ops(path, name):
    """Another revision's ops.py as the module ldmae_amd.<name> (its relative imports resolve against this tree's package)."""
    import ldmae_amd  # noqa: F401
    spec = importlib.util.spec_from_file_location("ldmae_amd." + name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def wrapper_cases():
    """name -> call(ops): well-formed calls as the DiT / VMAE train steps make them; M = 256 rows of D = 192, B = 2 samples of N = 128 tokens."""
    g = torch.Generator(device="cuda").manual_seed(0)
    rf = lambda *s: torch.randn(*s, device="cuda", generator=g)      # noqa: E731
    rb = lambda *s: rf(*s).to(BF16)                                   # noqa: E731
    M, D, B, N, H, hd = 256, 192, 2, 128, 3, 64
    x, dx, w, rstd = rf(M, D), rf(M, D), rf(D), torch.rand(M, device="cuda") + 0.5
    mod, dmod = rf(B, 6 * D) * 0.1, torch.empty(B, 6 * D, device="cuda")
    sh, sc, gt, dsh, dsc, dgt = mod[:, :D], mod[:, D:2 * D], mod[:, 2 * D:3 * D], dmod[:, :D], dmod[:, D:2 * D], dmod[:, 2 * D:3 * D]
    ya, dout, a, wqkv, bqkv = rb(M, D), rb(M, D), rb(M, D), rb(3 * D, D), rf(3 * D)
    qkv, wq, wk, cos, sin = rb(M, 3 * D), rf(hd), rf(hd), torch.rand(N, hd, device="cuda"), torch.rand(N, hd, device="cuda")
    import ldmae_amd.ops as ops0
    q, k, _ = ops0.qknorm_rope_fwd(qkv, wq, wk, cos, sin, B, N, H, hd, copy_v=False)
    o, lse = ops0.attention_fwd_pv(q, k, qkv, hd ** -0.5)
    do, bound = rb(B, N, D), ops0.qk_score_bound(wq, wk, hd, hd ** -0.5)
    qkv16 = rb(M, 3 * D)                                              # the VMAE blocks: 12 heads of 16
    o16, lse16 = ops0.attention_fwd_qkv(qkv16, B, N, 12, 16, 0.25)
    mean, t, y, table = rf(M), torch.rand(B, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda"), rf(11, D)
    p, gr, m1, v1, ema = (rf(4096) for _ in range(5))
    v1.abs_()
    ids, xt = torch.stack([torch.randperm(N, device="cuda")[:32] for _ in range(B)]), rf(B, N, D)
    dsts, srcs = [rf(D) for _ in range(8)], [rf(D) for _ in range(8)]
    return {
        "rmsnorm_modulate_fwd": lambda o_: o_.rmsnorm_modulate_fwd(x, w, sh, sc, N, BF16),
        "res_rmsnorm_modulate_fwd": lambda o_: o_.res_rmsnorm_modulate_fwd(x, ya, gt, None, None, w, sh, sc, N),
        "rmsnorm_modulate_bwd": lambda o_: o_.rmsnorm_modulate_bwd(dout, x, w, sc, rstd, dx, dsh, dsc, N),
        "rmsnorm_modulate_bwd_gate": lambda o_: o_.rmsnorm_modulate_bwd_gate(dout, x, w, sc, rstd, dx, dsh, dsc, ya, gt, dgt, N, BF16),
        "gate_bwd": lambda o_: o_.gate_bwd(dx, ya, gt, dgt, N, BF16, with_bias=True),
        "gemm_nt": lambda o_: o_.gemm_nt(a, wqkv, bqkv),
        "qknorm_rope_fwd": lambda o_: o_.qknorm_rope_fwd(qkv, wq, wk, cos, sin, B, N, H, hd, copy_v=False),
        "attention_fwd_pv[bound]": lambda o_: o_.attention_fwd_pv(q, k, qkv, hd ** -0.5, bound=bound),
        "attention_bwd_pv_qknorm": lambda o_: o_.attention_bwd_pv_qknorm(q, k, qkv, o, do, lse, hd ** -0.5, wq, wk, cos, sin),
        "attention_fwd_qkv": lambda o_: o_.attention_fwd_qkv(qkv16, B, N, 12, 16, 0.25),
        "attention_bwd_qkv": lambda o_: o_.attention_bwd_qkv(qkv16, o16, do, lse16, B, N, 12, 16, 0.25),
        "layernorm_fwd": lambda o_: o_.layernorm_fwd(x, w, w, BF16),
        "layernorm_bwd[cast]": lambda o_: o_.layernorm_bwd(dout, x, w, mean, rstd, dx, cast=True),
        "gelu_bwd": lambda o_: o_.gelu_bwd(dout, ya),
        "cast": lambda o_: o_.cast(x, BF16),
        "silu_fwd": lambda o_: o_.silu_fwd(mod),
        "silu_bwd": lambda o_: o_.silu_bwd(dmod, mod),
        "timestep_embedding": lambda o_: o_.timestep_embedding(t),
        "label_embed_fwd": lambda o_: o_.label_embed_fwd(table, y, None, 10),
        "gather_rows": lambda o_: o_.gather_rows(xt, ids),
        "multi_add_": lambda o_: o_.multi_add_(dsts, srcs),
        "adamw_ema": lambda o_: o_.adamw_ema(p, gr, m1, v1, ema, 1, 1e-4, 0.9, 0.95, 1e-8, 0.0, 0.9999),
    }


def bench_wrappers(other_path, calls=300, repeats=5):
    import ldmae_amd.ops as new
    sides = (("other", load_ops(other_path, "_ops_other")), ("this", new))
    print(f"host microseconds per call (enqueue only; {calls} calls per block, blocks alternate, min .. max of {repeats} blocks); "
          f"other = {os.path.basename(other_path)}")
    for name, fn in wrapper_cases().items():
        us = {s: [] for s, _ in sides}
        try:
            for _, mod in sides:
                for _ in range(20):
                    fn(mod)
        except RuntimeError as e:                     # a shape the library refuses: said, not timed
            print(f"  {name:28s} not timed: {e}")
            continue
        for _ in range(repeats):
            for s, mod in sides:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn(mod)
                us[s].append((time.perf_counter() - t0) / calls * 1e6)
        torch.cuda.synchronize()
        d = statistics.median(us["this"]) - statistics.median(us["other"])
        out = min(us["this"]) > max(us["other"])
        print(f"  {name:28s} other {min(us['other']):6.2f} .. {max(us['other']):6.2f}   this {min(us['this']):6.2f} .. {max(us['this']):6.2f}   "
              f"median {d:+5.2f} us{'   <- above the whole spread of the other' if out else ''}")


def tiny_dit_step():
    from ldmae_amd.models.lightningdit import LightningDiT
    from ldmae_amd.optim import AdamWEMA
    torch.manual_seed(0)
    m = LightningDiT(input_size=8, patch_size=1, in_channels=16, hidden_size=192, depth=2, num_heads=3, num_classes=10, class_dropout_prob=0.5,
                     use_qknorm=True, use_swiglu=True, use_rope=True, use_rmsnorm=True).cuda().train()
    m.set_precision(BF16)
    opt = AdamWEMA(m, lr=1e-4)
    x, u, t, y = torch.randn(4, 16, 8, 8, device="cuda"), torch.randn(4, 16, 8, 8, device="cuda"), torch.rand(4, device="cuda"), torch.arange(4, device="cuda")

    def step():
        opt.zero_grad()
        ((m(x, t, y) - u) ** 2).mean().backward()
        opt.step()
    return step


def vmae2_step():
    from ldmae_amd.tokenizer import models_mae
    torch.manual_seed(0)
    m = models_mae.MaskedAutoencoderViT(img_size=128, patch_size=8, embed_dim=192, depth=2, num_heads=12, decoder_embed_dim=192, decoder_depth=2,
                                        decoder_num_heads=12, mlp_ratio=4, norm_layer=models_mae._ln(), latent_dim=16, no_cls=True, kl_loss_weight=1e-3,
                                        smooth_output=True).cuda().train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4)
    imgs = torch.rand(2, 3, 128, 128, device="cuda") * 2 - 1

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=BF16):
            loss = m(imgs, 0.75, 0.5)[0]
        loss.backward()
        opt.step()
    return step


def install_ops(ops_path):
    """OPS.py takes the place of ldmae_amd.ops for everything imported afterwards."""
    import ldmae_amd
    ldmae_amd.ops = load_ops(ops_path, "ops")


def bench_steps(ops_path, steps=200, warmup=30, repeats=5):
    if ops_path:
        install_ops(ops_path)
    print(f"launch-bound train steps with ops = {os.path.basename(ops_path) if ops_path else 'this tree'}: ms per step over {steps} steps, {repeats} repeats")
    for name, make in (("tiny DiT (depth 2, 192 wide, 64 tokens, batch 4, bf16)", tiny_dit_step), ("VMAE depth 2 + 2 (128 px, batch 2, bf16 autocast)", vmae2_step)):
        step = make()
        for _ in range(warmup):
            step()
        ms = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / steps * 1e3)
        print(f"  {name}: {min(ms):.3f} .. {max(ms):.3f} ms (median {statistics.median(ms):.3f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["wrappers", "steps", "bench"])
    ap.add_argument("--other", help="wrappers: the ops.py of the revision to compare with")
    ap.add_argument("--ops", help="steps / bench: run with this ops.py in place of the tree's")
    args, rest = ap.parse_known_args()                      # bench: what is left over goes to bench.py
    if rest and args.mode != "bench":
        ap.error(f"unrecognised arguments: {rest}")
    if args.mode == "bench":
        if args.ops:
            install_ops(args.ops)
        sys.argv = [os.path.join(ROOT, "bench.py")] + [a for a in rest if a != "--"]
        runpy.run_path(sys.argv[0], run_name="__main__")
        sys.exit(0)
    if args.mode == "wrappers":
        if not args.other:
            ap.error("wrappers needs --other OPS.py")
        bench_wrappers(args.other)
    else:
        bench_steps(args.ops)
