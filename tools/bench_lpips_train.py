"""Cost of the LPIPS perceptual loss in the stage-3 decoder tuning on one MI355X, random weights, per LPIPS precision (models/lpips.py: "f32" =
exact f32, "fp16" = fp16 VGG forward + bf16 data gradient).  The precisions ALTERNATE inside one process, round by round, so that a difference
between them is measured against the spread of the same process; every figure is the median over the rounds with (min .. max):
  - every conv geometry of the VGG16: forward conv and data gradient (ReLU mask in the gather), ms and TF/s;
  - LPIPS forward + backward with the gradient to the target only (what stage 3 asks for) at B = 16, 256 x 256, against the forward-only call;
  - one stage-3 step (vmae_pretrain's model at --batch_size 16, bf16 and fp16 autocast), the share LPIPS forward + backward takes of it, and
    torch.cuda.max_memory_allocated of the step.

    python tools/bench_lpips_train.py [--batch 16] [--iters 5] [--rounds 5] [--precisions f32,fp16] [--out profiles/lpips_train_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ldmae_amd.models.lpips import CONVS, LPIPS, PRECISIONS, random_state_dict  # noqa: E402


def timed(fn, iters, warmup=0):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def alternate(fns, iters, rounds):
    """fns {key: callable} -> {key: [seconds per call, one per round]}; every callable is warmed up first, then the keys take turns round by round."""
    for fn in fns.values():
        timed(fn, 2)
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, iters))
    return out


def med(ts):
    return statistics.median(ts)


def ms(ts):
    return f"{med(ts) * 1e3:.3f} ({min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precisions", default="f32,fp16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_train_bench.txt"))
    a = ap.parse_args()
    precs = a.precisions.split(",")
    if not precs or any(p not in PRECISIONS for p in precs):
        ap.error(f"--precisions: a comma-separated subset of {PRECISIONS}")
    B, S = a.batch, 256
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    torch.manual_seed(0)
    sd = random_state_dict(0)
    lps = {p: LPIPS(state_dict=sd, device="cuda", differentiable=True, precision=p) for p in precs}
    x = torch.rand(B, 3, S, S, device="cuda") * 2 - 1
    y = (x + 0.1 * torch.randn_like(x)).clamp(-1, 1)

    say(f"precisions {precs} alternating in one process; {a.rounds} rounds of {a.iters} calls; ms = median (min .. max) over the rounds")
    say(f"forward conv and conv data gradient (ReLU mask in the gather), one half = {B} images of {S} x {S}; TF/s by the layer's real Cin (3 for conv1_1)")
    say(f"{'layer':>8} {'H x W':>9} {'Cin':>4} {'Cout':>4} {'prec':>5} {'fwd ms':>24} {'fwd TF/s':>8} {'dgrad ms':>24} {'dgrad TF/s':>10}")
    h, prev = S, 1
    tot = {p: [0.0, 0.0] for p in precs}
    for j, (i, s, cin, cout) in enumerate(CONVS):
        if s != prev:
            h, prev = h // 2, s
        flops = 2.0 * B * h * h * cout * 9 * cin
        fwd, bwd = {}, {}
        keep = []
        for p in precs:
            lp = lps[p]
            w, b, _ = lp.convs[j]
            xin = torch.randn(B, h, h, w.shape[3], device="cuda").to(lp._k.act_dtype)      # 4 (f32) or 8 (fp16) channels for conv1_1 (padded)
            yout = lp._k.conv(xin, w, b)
            dy = torch.randn(yout.shape, device="cuda")
            dx = torch.empty(xin.shape, dtype=torch.float32, device="cuda")
            keep.append((xin, yout, dy, dx))
            fwd[p] = lambda lp=lp, xin=xin, w=w, b=b, yout=yout: lp._k.conv(xin, w, b, out=yout)
            bwd[p] = lambda lp=lp, dy=dy, yout=yout, j=j, dx=dx: lp._k.dgrad(dy, yout, lp.wrot[j], out=dx)
        tf, td = alternate(fwd, a.iters, a.rounds), alternate(bwd, a.iters, a.rounds)
        for p in precs:
            tot[p][0] += med(tf[p])
            tot[p][1] += med(td[p])
            say(f"{'conv' + str(s) + '_' + str(j):>8} {h:>4}x{h:<4} {cin:>4} {cout:>4} {p:>5} {ms(tf[p]):>24} {flops / med(tf[p]) / 1e12:>8.1f} {ms(td[p]):>24} "
                f"{flops / med(td[p]) / 1e12:>10.1f}")
        del keep
    for p in precs:
        say(f"sum of the 13 layers' medians, {p}: forward {tot[p][0] * 1e3:.2f} ms, data gradient {tot[p][1] * 1e3:.2f} ms")

    def fwd_only(lp):
        with torch.no_grad():
            lp(x, y)

    def fwd_bwd(lp):
        yg = y.clone().requires_grad_()
        lp(x, yg).mean().backward()
    t_fwd = alternate({p: (lambda lp=lps[p]: fwd_only(lp)) for p in precs}, a.iters, a.rounds)
    t_fb = alternate({p: (lambda lp=lps[p]: fwd_bwd(lp)) for p in precs}, a.iters, a.rounds)
    for p in precs:
        say(f"LPIPS {p} B = {B}, {S}^2: forward only {ms(t_fwd[p])} ms; forward + backward to the target {ms(t_fb[p])} ms = {med(t_fb[p]) / med(t_fwd[p]):.2f} x")

    from ldmae_amd.tokenizer import models_mae
    torch.manual_seed(0)
    model = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, smooth_output=True, kl_loss_weight=0.0, img_size=S, perceptual_loss=lps[precs[0]],
                                                perceptual_loss_ratio=10.0).cuda()
    for prec, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        def step(lp):
            model.perceptual_loss = lp
            with torch.autocast("cuda", dtype=dt):
                loss = model(x, mask_ratio=0.0)[0]
            loss.backward()
            model.zero_grad(set_to_none=True)
        fns = {p: (lambda lp=lps[p]: step(lp)) for p in precs}
        fns["none"] = lambda: step(None)
        t = alternate(fns, a.iters, a.rounds)
        peak = {}
        for k, fn in fns.items():                                                   # the step's own peak, one call each after the timing
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() / 2 ** 30
        model.perceptual_loss = lps[precs[0]]
        say(f"stage-3 step (forward + backward, batch {B}, {prec} autocast, mask_ratio 0.0) without LPIPS: {ms(t['none'])} ms; peak memory {peak['none']:.2f} GiB")
        for p in precs:
            say(f"stage-3 step, {prec} autocast, LPIPS {p}: {ms(t[p])} ms; LPIPS share {100 * (med(t[p]) - med(t['none'])) / med(t[p]):.1f} %; "
                f"peak memory {peak[p]:.2f} GiB")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
