"""Cost of the LPIPS perceptual loss in the stage-3 decoder tuning on one MI355X, random weights:
  - every conv data-gradient geometry of the VGG16 backward (ops.conv3x3_relu_dgrad_nhwc) next to the forward conv of the same layer: ms and TF/s;
  - LPIPS forward + backward with the gradient to the target only (what stage 3 asks for) at B = 16, 256 x 256, against the forward-only call;
  - one stage-3 step (vmae_pretrain's model at --batch_size 16, bf16 and fp16 autocast) and the share LPIPS forward + backward takes of it.

    python tools/bench_lpips_train.py [--batch 16] [--iters 5] [--out profiles/lpips_train_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ldmae_amd import ops  # noqa: E402
from ldmae_amd.models.lpips import CONVS, LPIPS, random_state_dict  # noqa: E402


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_train_bench.txt"))
    a = ap.parse_args()
    B, S = a.batch, 256
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    torch.manual_seed(0)
    lp = LPIPS(state_dict=random_state_dict(0), device="cuda", differentiable=True)
    x = torch.rand(B, 3, S, S, device="cuda") * 2 - 1
    y = (x + 0.1 * torch.randn_like(x)).clamp(-1, 1)

    say(f"conv data gradient (ReLU mask in the gather) vs the forward conv, one half = {B} images of {S} x {S}, f32")
    say(f"{'layer':>8} {'H x W':>9} {'Cin':>4} {'Cout':>4} {'fwd ms':>8} {'fwd TF/s':>8} {'dgrad ms':>8} {'dgrad TF/s':>10} {'ratio':>6}")
    h, prev, tot_f, tot_d = S, 1, 0.0, 0.0
    for j, (i, s, cin, cout) in enumerate(CONVS):
        if s != prev:
            h, prev = h // 2, s
        w, b, _ = lp.convs[j]
        cx = w.shape[3]                                              # 4 for conv1_1 (padded)
        xin = torch.randn(B, h, h, cx, device="cuda")
        yout = ops.conv2d_nhwc(xin, w, b, (1, 1), (1, 1), True)
        dy = torch.randn_like(yout)
        flops = 2.0 * B * h * h * cout * 9 * cx
        tf = timed(lambda: ops.conv2d_nhwc(xin, w, b, (1, 1), (1, 1), True, out=yout), a.iters)
        dx = torch.empty_like(xin)
        td = timed(lambda: ops.conv3x3_relu_dgrad_nhwc(dy, yout, lp.wrot[j], out=dx), a.iters)
        tot_f, tot_d = tot_f + tf, tot_d + td
        say(f"{'conv' + str(s) + '_' + str(j):>8} {h:>4}x{h:<4} {cx:>4} {cout:>4} {tf * 1e3:>8.3f} {flops / tf / 1e12:>8.1f} {td * 1e3:>8.3f} {flops / td / 1e12:>10.1f} "
            f"{tf / td:>6.2f}")
    say(f"sum over the 13 layers: forward {tot_f * 1e3:.2f} ms, data gradient {tot_d * 1e3:.2f} ms (ratio = dgrad TF/s over forward TF/s)")

    with torch.no_grad():
        t_fwd = timed(lambda: lp(x, y), a.iters)

    def fwd_bwd():
        yg = y.clone().requires_grad_()
        lp(x, yg).mean().backward()
    t_fb = timed(fwd_bwd, a.iters)
    say(f"LPIPS B = {B}, {S}^2: forward only {t_fwd * 1e3:.2f} ms; forward + backward to the target {t_fb * 1e3:.2f} ms = {t_fb / t_fwd:.2f} x "
        f"(by FLOP count 1.5 x: the backward of one half costs one half's forward convs)")

    from ldmae_amd.tokenizer import models_mae
    torch.manual_seed(0)
    model = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, smooth_output=True, kl_loss_weight=0.0, img_size=S, perceptual_loss=lp,
                                                perceptual_loss_ratio=10.0).cuda()
    for prec, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        def step(with_lpips=True):
            model.perceptual_loss = lp if with_lpips else None
            with torch.autocast("cuda", dtype=dt):
                loss = model(x, mask_ratio=0.0)[0]
            loss.backward()
            model.zero_grad(set_to_none=True)
        t_step = timed(step, a.iters)
        t_bare = timed(lambda: step(False), a.iters)
        model.perceptual_loss = lp
        say(f"stage-3 step (forward + backward, batch {B}, {prec}, mask_ratio 0.0): {t_step * 1e3:.2f} ms; without LPIPS {t_bare * 1e3:.2f} ms; "
            f"LPIPS share {100 * (t_step - t_bare) / t_step:.1f} %")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
