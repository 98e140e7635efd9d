"""Timings of the linear probe / k-NN evaluation on one MI355X (ldmae_amd/linear_probe.py, csrc/linprobe.hip), on random weights and data:
  - feature images/s of the frozen f8d16 tokenizer at 256 px, batch 256, per --features and --pool (encoder forward + pooling), fp32 and bf16;
  - the head's training step (BatchNorm -> Linear -> cross-entropy -> weight / bias gradients -> LARS) at batch 1024, 1000 classes, for
    feature widths 16 (latent, mean), 192 (encoder, mean) and 16 384 (latent, flatten), and its cross-entropy + rank kernel alone;
  - k-NN: seconds per 1 000 queries against the bank size (similarities + top-k merge + vote, k = 20, width 16);
  - as a YARDSTICK ONLY (not part of the package): torch's own cross_entropy (forward + backward) + topk(5) on the same logits.

    python tools/bench_linprobe.py [--iters 20] [--out profiles/linprobe_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ldmae_amd import linear_probe as lp, ops  # noqa: E402


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linprobe_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"linear probe / k-NN timings, {torch.cuda.get_device_name(0)}, torch {torch.__version__}, iters {args.iters} (host clock around a "
             f"device synchronise, after 2 warm-up calls)"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- features
    from ldmae_amd.tokenizer import models_mae
    torch.manual_seed(0)
    model = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, kl_loss_weight=True, smooth_output=True, img_size=256).to(dev).eval()
    images = torch.randn(256, 3, 256, 256, device=dev)
    feat_rate = {}
    for prec, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        model.set_precision(dtype)
        for features in lp.FEATURES:
            for pool in lp.POOLS:
                t = timed(lambda: lp.pool_features(model, images, features, pool), max(3, args.iters // 4))
                feat_rate[(prec, features, pool)] = 256 / t
                say(f"features  {prec}  --features {features:7s} --pool {pool:7s}  width {lp.feature_width(model, features, pool):6d}  "
                    f"{t * 1e3:8.2f} ms / 256 images  {256 / t:9.0f} images/s")
    model.set_precision(torch.float32)
    del images

    # ---- the head's step
    B, C = 1024, 1000
    labels = ops.check_labels(torch.randint(0, C, (B,)), C, dev)
    step_ms = {}
    for D in (16, 192, 16384):
        head = lp.ProbeHead(D, C, dev, "bn", 0)
        x = torch.randn(B, D, device=dev)

        def step():
            head.accumulate(x, labels, 1.0 / B, True)
            head.step(0.4, 0.0, 0.9, 0.001)
        t = timed(step, args.iters)
        step_ms[D] = t * 1e3
        say(f"head step  batch {B}  classes {C}  width {D:6d}  {t * 1e3:8.3f} ms  ({B / t:10.0f} images/s)")
        del head, x
    logits = torch.randn(B, 1008, device=dev)
    dl = torch.zeros(B, 1008, device=dev)
    t_own = timed(lambda: ops.softmax_xent(logits, labels, C, grad_scale=1.0 / B, dlogits=dl), args.iters * 5)
    say(f"softmax_xent (loss + dlogits + rank, one kernel)  [{B}, {C}]  {t_own * 1e6:8.1f} us")
    lt = logits[:, :C].clone().requires_grad_(True)

    def torch_xent():
        lt.grad = None
        torch.nn.functional.cross_entropy(lt, labels).backward()
        return lt.detach().topk(5, dim=1)
    t_torch = timed(torch_xent, args.iters * 5)
    say(f"YARDSTICK torch cross_entropy fwd + bwd + topk(5)  [{B}, {C}]  {t_torch * 1e6:8.1f} us")

    # ---- k-NN
    D, k, nq = 16, 20, 1000
    q = ops.l2_normalize(torch.randn(nq, D, device=dev))
    ql = torch.randint(0, C, (nq,))
    for nbank in (10000, 100000, 1281167):
        bank = ops.l2_normalize(torch.randn(nbank, D, device=dev))
        bl, qld = ops.check_labels(torch.randint(0, C, (nbank,)), C, dev), ops.check_labels(ql, C, dev)

        def knn():
            vals, idx = ops.topk_empty(nq, k, dev)
            for b0 in range(0, nbank, lp.KNN_BANK_CHUNK):
                ops.topk_merge(ops.pairwise_logits(q, bank[b0:b0 + lp.KNN_BANK_CHUNK]), b0, vals, idx)
            return ops.knn_vote(vals, idx, bl, qld, C, 0.07)
        t = timed(knn, max(2, args.iters // 10), warmup=1)
        say(f"k-NN  k {k}  width {D}  bank {nbank:8d}  {t:8.4f} s / {nq} queries")
        del bank

    # ---- which pass bounds an rrc epoch
    for (prec, features, pool), rate in feat_rate.items():
        Dw = lp.feature_width(model, features, pool)
        if Dw in step_ms:
            feat_ms = 1024 / rate * 1e3
            say(f"rrc epoch, {prec} {features}/{pool}: features {feat_ms:8.2f} ms per 1024 images, head step {step_ms[Dw]:8.3f} ms -> bound by the "
                f"{'feature pass' if feat_ms > step_ms[Dw] else 'head'} ({feat_ms / step_ms[Dw]:.1f} x)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
