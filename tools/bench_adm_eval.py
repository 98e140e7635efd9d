"""Timings of the ADM evaluator's metric arithmetic on one MI355X, on synthetic features (no Inception weights needed):
  - manifold_radii (k-NN radii, nhood (3,)) at N = 10 000 and 50 000, D = 2048: ms and TF/s at 2 N^2 D FLOP per pass;
  - evaluate_pr for 10 000 reference x 50 000 sample features: ms and TF/s at 2 N1 N2 D FLOP;
  - the softmax / Inception Score path for 50 000 rows (logits GEMM against a [1008, 2048] weight + softmax sums);
  - images/s of InceptionFID.adm_features at batch 250 (random weights in the real layout, 256 x 256 uint8 images);
  - KID: ops.kid_sums for 100 subsets of 1000 rows at D = 2048 (one launch); density / coverage: ops.ball_counts for 10 000 x 50 000;
  - as a YARDSTICK ONLY (not part of the package): the same radii with torch.cdist + kthvalue on the GPU, in row blocks; the KID sums with
    torch's gather + matmul in f32 and the ball counts with torch.cdist.

    python tools/bench_adm_eval.py [--iters 3] [--no-torch] [--json OUT]

profiles/kid_dc_bench.txt holds the KID and density / coverage lines of one run.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ldmae_amd import evaluator as ev, fid, ops  # noqa: E402


def timed(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def features(n, d, seed):
    """Post-ReLU-like clustered features on the device; every set shares the same 256 cluster centres."""
    centers = torch.rand(256, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(12345))
    g = torch.Generator(device="cuda").manual_seed(seed)
    idx = torch.randint(0, 256, (n,), device="cuda", generator=g)
    return (centers[idx] + 0.3 * torch.rand(n, d, device="cuda", generator=g)).contiguous()


def torch_radii(x, k=3, rows=2048):
    out = torch.empty(x.shape[0], device=x.device)
    for i in range(0, x.shape[0], rows):
        d = torch.cdist(x[i:i + rows], x).square_()
        out[i:i + rows] = d.kthvalue(k + 1, dim=1).values
    return out


def torch_kid(a, b, idx1, idx2, gamma, coef0=1.0):
    """f32 restatement with torch's own kernels: gather the subsets, three batched products, cube, f64 sums -> [S, 3]."""
    i1, i2 = torch.as_tensor(idx1, device=a.device).long(), torch.as_tensor(idx2, device=a.device).long()
    out = torch.empty(i1.shape[0], 3, dtype=torch.float64, device=a.device)
    for s in range(i1.shape[0]):
        x, y = a[i1[s]], b[i2[s]]
        kxx, kyy, kxy = (gamma * (x @ x.T) + coef0) ** 3, (gamma * (y @ y.T) + coef0) ** 3, (gamma * (x @ y.T) + coef0) ** 3
        out[s, 0] = kxx.double().sum() - kxx.diagonal().double().sum()
        out[s, 1] = kyy.double().sum() - kyy.diagonal().double().sum()
        out[s, 2] = kxy.double().sum()
    return out


def torch_ball_counts(u, ru, v, rows=2048):
    out = torch.empty(u.shape[0], dtype=torch.int32, device=u.device)
    for i in range(0, u.shape[0], rows):
        d = torch.cdist(u[i:i + rows], v).square_()
        out[i:i + rows] = (d < ru[i:i + rows, None]).sum(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    D = 2048
    res = {"device": torch.cuda.get_device_name(0)}

    def say(s):
        print(s, flush=True)

    f10, f50 = features(10_000, D, 0), features(50_000, D, 1)
    for name, x in (("10k", f10), ("50k", f50)):
        n = x.shape[0]
        t = timed(lambda: ops.knn_radii(x, (3,)), a.iters)
        tf = 2.0 * n * n * D / t / 1e12
        res[f"radii_{name}_ms"], res[f"radii_{name}_tflops"] = t * 1e3, tf
        say(f"manifold_radii N={n:6d} D={D}: {t * 1e3:9.2f} ms  {tf:6.1f} TF/s  (nsplit {ops.default_col_splits(n, n)})")
    r10, r50 = ops.knn_radii(f10, (3,)), ops.knn_radii(f50, (3,))
    t = timed(lambda: ops.pr_flags(f10, r10, f50, r50), a.iters)
    tf = 2.0 * 10_000 * 50_000 * D / t / 1e12
    res["pr_10k_50k_ms"], res["pr_10k_50k_tflops"] = t * 1e3, tf
    say(f"evaluate_pr 10000 x 50000 D={D}: {t * 1e3:9.2f} ms  {tf:6.1f} TF/s")
    in1, in2 = ops.pr_flags(f10, r10, f50, r50)
    say(f"  (synthetic precision {float(in2.float().mean()):.4f}, recall {float(in1.float().mean()):.4f})")

    w = (torch.randn(1008, D, device="cuda") * 0.02).contiguous()

    def is_path():
        h, S = ops.adm_softmax_is(ops.pairwise_logits(f50, w), 5000)
        return ev.inception_score_from_sums(h.cpu().numpy(), S.cpu().numpy(), f50.shape[0], 5000)
    t = timed(is_path, a.iters)
    tl = timed(lambda: ops.pairwise_logits(f50, w), a.iters)
    res["is_50k_ms"], res["logits_50k_ms"] = t * 1e3, tl * 1e3
    say(f"softmax / IS path 50000 rows: {t * 1e3:9.2f} ms  (logits GEMM {tl * 1e3:.2f} ms, {2.0 * 50_000 * 1008 * D / tl / 1e12:.1f} TF/s)")

    sd = fid.random_state_dict(0)
    sd["fc.weight"] = torch.randn(1008, D) * 0.02
    model = fid.InceptionFID(dims=2048, state_dict=sd)
    imgs = torch.randint(0, 256, (250, 256, 256, 3), dtype=torch.uint8, device="cuda")
    t = timed(lambda: model.adm_features(imgs), a.iters)
    res["adm_features_img_s"] = 250 / t
    say(f"adm_features batch 250 (256x256 -> 299): {250 / t:8.0f} images/s")

    total = res["radii_10k_ms"] + res["radii_50k_ms"] + res["pr_10k_50k_ms"] + res["is_50k_ms"]
    res["metrics_50k_vs_10k_ms"] = total
    say(f"metric arithmetic of a 50k-sample / 10k-reference evaluation (2 radii passes + PR + IS): {total:.1f} ms")

    # KID: 100 subsets of 1000 rows (the defaults of --kid) from the 10k reference and the 50k sample features, one launch
    idx1, idx2 = ev.kid_subset_indices(f10.shape[0], f50.shape[0], 100, 1000, 2020)
    t = timed(lambda: ops.kid_sums(f10, f50, idx1, idx2, 1.0 / D), a.iters)
    tf = 2.0 * 3 * 100 * 1000 * 1000 * D / t / 1e12
    res["kid_100x1000_ms"], res["kid_100x1000_tflops"] = t * 1e3, tf
    say(f"kid_sums 100 subsets x 1000 rows D={D}: {t * 1e3:9.2f} ms  {tf:6.1f} TF/s  (host index check and upload included)")
    mean, std = ev.kid_from_sums(ops.kid_sums(f10, f50, idx1, idx2, 1.0 / D).cpu().numpy(), 1000)
    say(f"  (synthetic KID {mean:.6g} +- {std:.3g})")
    # density / coverage: one ball-count pass, 10k real x 50k fake, radii of nearest_k = 5
    r5 = ops.knn_radii(f10, (5,))[:, 0].contiguous()
    n10, n50 = ops.row_sqnorms(f10), ops.row_sqnorms(f50)
    t = timed(lambda: ops.ball_counts(f10, r5, f50, nu=n10, nv=n50), a.iters)
    tf = 2.0 * 10_000 * 50_000 * D / t / 1e12
    res["ball_counts_10k_50k_ms"], res["ball_counts_10k_50k_tflops"] = t * 1e3, tf
    say(f"ball_counts 10000 x 50000 D={D}: {t * 1e3:9.2f} ms  {tf:6.1f} TF/s")
    counts = ops.ball_counts(f10, r5, f50, nu=n10, nv=n50)
    say(f"  (synthetic density {float(counts.sum()) / (5 * 50_000):.4f}, coverage {float((counts > 0).float().mean()):.4f})")

    if not a.no_torch:
        try:
            t = timed(lambda: torch_kid(f10, f50, idx1, idx2, 1.0 / D), a.iters)
            tm, _ = ev.kid_from_sums(torch_kid(f10, f50, idx1, idx2, 1.0 / D).cpu().numpy(), 1000)
            res["yardstick_torch_kid_100x1000_ms"] = t * 1e3
            say(f"[yardstick only] torch f32 gather + matmul KID sums, 100 x 1000: {t * 1e3:9.2f} ms  (KID {tm:.6g}, ours {mean:.6g})")
            t = timed(lambda: torch_ball_counts(f10, r5, f50), a.iters)
            same = float((torch_ball_counts(f10, r5, f50) == counts).float().mean())
            res["yardstick_torch_ball_counts_10k_50k_ms"] = t * 1e3
            say(f"[yardstick only] torch.cdist ball counts 10000 x 50000: {t * 1e3:9.2f} ms  (rows with the same count: {same:.4f})")
        except RuntimeError as e:
            say(f"[yardstick only] torch KID / ball counts not run: {e}")
        try:
            t = timed(lambda: torch_radii(f10), a.iters)
            ok = bool(torch.allclose(torch_radii(f10), ops.knn_radii(f10, (3,))[:, 0], rtol=1e-3, atol=1e-3))
            res["yardstick_torch_cdist_kthvalue_10k_ms"] = t * 1e3
            say(f"[yardstick only] torch.cdist + kthvalue radii N=10000: {t * 1e3:9.2f} ms  (agrees to 1e-3: {ok})")
        except RuntimeError as e:          # the yardstick is optional: torch's own kernels may be missing on this machine
            say(f"[yardstick only] torch.cdist + kthvalue not run: {e}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
