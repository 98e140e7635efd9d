"""Throughput of the tokenizer evaluation on one MI355X, random weights, batch 64 of 256 x 256 images:
  - LPIPS pairs/s and the achieved TF/s of its VGG16 part (ldmae_amd.models.lpips.conv_flops_per_image: 40.1 GFLOP per image, 2 per pair);
  - the time of the ScalingLayer prep, the five heads, SSIM and the quantisation + PSNR apart from the convolutions, and their share of
    the VGG time;
  - end-to-end images/s of encode, decode, the metrics, the device-to-host copy and the PNG encode (the driver's loop, no disk reads).

Per LPIPS precision (models/lpips.py: "f32" exact, "fp16" the 16-bit VGG): the LPIPS call of the precisions ALTERNATES round by round inside one
process (the figure is the median over the rounds), then the pieces and the end-to-end loop are timed per precision; one JSON line each.

    python tools/bench_tokenizer_eval.py [--batch 64] [--iters 5] [--rounds 3] [--precisions f32,fp16] [--no-e2e]
"""
import argparse
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ldmae_amd import ops  # noqa: E402
from ldmae_amd.metrics import psnr_from_sse, ssim  # noqa: E402
from ldmae_amd.models.lpips import LPIPS, PRECISIONS, conv_flops_per_image, random_state_dict  # noqa: E402


def timed(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def _png(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="png")
    return len(buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precisions", default="f32,fp16")
    ap.add_argument("--no-e2e", action="store_true")
    a = ap.parse_args()
    precs = a.precisions.split(",")
    if not precs or any(p not in PRECISIONS for p in precs):
        ap.error(f"--precisions: a comma-separated subset of {PRECISIONS}")
    B, S = a.batch, 256
    torch.manual_seed(0)
    sd = random_state_dict(0)
    lps = {p: LPIPS(state_dict=sd, device="cuda", precision=p) for p in precs}
    x = torch.rand(B, 3, S, S, device="cuda") * 2 - 1
    y = (x + 0.1 * torch.randn_like(x)).clamp(-1, 1)
    t_rounds = {p: [] for p in precs}
    for p in precs:
        timed(lambda: lps[p](x, y), 1)
    for _ in range(a.rounds):                                   # the precisions take turns: a difference is seen against this process's own spread
        for p in precs:
            t_rounds[p].append(timed(lambda: lps[p](x, y), a.iters, warmup=0))
    for p in precs:
        bench_one(a, p, lps[p], x, y, t_rounds[p])


def bench_one(a, prec, lp, x, y, t_rounds):
    B, S = a.batch, 256
    k_ = lp._k
    res = {"batch": B, "size": S, "lpips_precision": prec}
    t_lpips = statistics.median(t_rounds)
    vgg_flops = 2 * B * conv_flops_per_image(S, S)
    # the pieces apart from the convolutions, on the tensors the forward really sees
    taps, h, prev = [], k_.prep(x, y), 1
    for w, b, s in lp.convs:
        if s != prev:
            taps.append(h)
            h = k_.pool(h)
            prev = s
        h = k_.conv(h, w, b)
    taps.append(h)
    out = torch.zeros(B, device="cuda")
    t_prep = timed(lambda: k_.prep(x, y), a.iters)
    t_heads = timed(lambda: [k_.head(t, lp.lins[k], out) for k, t in enumerate(taps)], a.iters)
    t_pool = timed(lambda: [k_.pool(t) for t in taps[:4]], a.iters)
    t_ssim = timed(lambda: ssim(x, y, reduction="none"), a.iters)
    t_quant = timed(lambda: ops.recon_quantize_sse(x, y), a.iters)
    t_vgg = t_lpips - t_prep - t_heads
    res.update({
        "lpips_ms": t_lpips * 1e3, "lpips_ms_min": min(t_rounds) * 1e3, "lpips_ms_max": max(t_rounds) * 1e3, "lpips_pairs_per_s": B / t_lpips,
        "vgg_ms": t_vgg * 1e3, "vgg_tflops": vgg_flops / t_vgg / 1e12, "pool_ms": t_pool * 1e3,
        "prep_ms": t_prep * 1e3, "heads_ms": t_heads * 1e3, "ssim_ms": t_ssim * 1e3, "quantize_psnr_ms": t_quant * 1e3,
        "non_conv_share_of_vgg": (t_prep + t_heads + t_ssim + t_quant) / t_vgg,
    })
    print(f"LPIPS {prec}  batch {B} pairs of {S}^2: {t_lpips * 1e3:.1f} ms ({min(t_rounds) * 1e3:.1f} .. {max(t_rounds) * 1e3:.1f}) = {B / t_lpips:.0f} pairs/s; "
          f"VGG part (LPIPS minus prep and heads) {t_vgg * 1e3:.1f} ms = {vgg_flops / t_vgg / 1e12:.1f} TF/s (pools included: {t_pool * 1e3:.2f} ms)")
    print(f"apart from the convs: prep {t_prep * 1e3:.2f} ms, five heads {t_heads * 1e3:.2f} ms, SSIM {t_ssim * 1e3:.2f} ms, "
          f"quantise + PSNR {t_quant * 1e3:.2f} ms = {100 * res['non_conv_share_of_vgg']:.1f} % of the VGG time")

    if not a.no_e2e:
        from ldmae_amd.tokenizer import models_mae
        model = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, kl_loss_weight=True, smooth_output=True, img_size=S).cuda().eval()
        pool = ThreadPoolExecutor(max_workers=16)

        def step():
            with torch.no_grad():
                z = model.encode(x).latent_dist.mode().float()
                d = model.decode(z).sample.float().contiguous()
                lv = lp(d, x).mean()
                sv = ssim(d, x)
                d8, r8, sse = ops.recon_quantize_sse(d, x)
                p = psnr_from_sse(sse, 3 * S * S)
                host = d8.cpu().numpy()
                list(pool.map(_png, list(host)))
                return lv, sv, p

        with torch.no_grad():
            t_enc = timed(lambda: model.decode(model.encode(x).latent_dist.mode().float()), a.iters)
        t_e2e = timed(step, a.iters)
        pool.shutdown()
        res.update({"encode_decode_ms": t_enc * 1e3, "e2e_ms": t_e2e * 1e3, "e2e_images_per_s": B / t_e2e})
        print(f"end to end (encode, decode, LPIPS, SSIM, quantise + PSNR, copy, PNG encode on 16 threads): {t_e2e * 1e3:.1f} ms per {B} "
              f"images = {B / t_e2e:.0f} images/s (encode + decode alone {t_enc * 1e3:.1f} ms)")
    print(json.dumps({"metric": "bench_tokenizer_eval", **{k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}}))


if __name__ == "__main__":
    main()
