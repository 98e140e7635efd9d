"""Throughput of the FID feature extractor (ldmae_amd.fid.InceptionFID) on one MI355X: random weights in the real layout, batch 250 of
299 x 299-sized uint8 images.  Prints images/s and achieved TF/s (11.42 GFLOP of convolutions per image, counted by
ldmae_amd.fid.conv_flops_per_image), a per-layer table of the 43 conv geometries (device events around each conv call), and, as an optional
yardstick, torch's own f32 NCHW conv stack on the same input when it runs on this machine.

    python tools/bench_fid.py [--batch 250] [--iters 10] [--dims 2048] [--no-torch] [--unfused]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ldmae_amd import fid, ops  # noqa: E402


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def per_layer(model, imgs):
    """Wrap ops.conv2d_nhwc with device events for one forward; return name -> ms, grouped later by geometry."""
    geo_of = {}
    for name, g in fid.conv_geometries().items():
        geo_of[id(model.params[name][0])] = (name, g)
    for blk, (a, b) in fid.FUSED_1X1.items():
        k = f"{blk}.fused_1x1"
        if k in model.params:
            ga = fid.conv_geometries()[a]
            geo_of[id(model.params[k][0])] = (k, ga[:3] + (model.params[k][0].shape[0],) + ga[4:])
    rec = []
    orig = ops.conv2d_nhwc

    def wrapped(x, w, *a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = orig(x, w, *a, **k)
        e1.record()
        rec.append((geo_of[id(w)], e0, e1))
        return r
    ops.conv2d_nhwc = wrapped
    try:
        model.features(imgs)
        torch.cuda.synchronize()
    finally:
        ops.conv2d_nhwc = orig
    return [(name, g, e0.elapsed_time(e1)) for (name, g), e0, e1 in rec]


def torch_stack(sd, x_nchw):
    """torch's f32 conv (+ folded BN) / pool stack on the device: the yardstick, NCHW, TF32 off."""
    import torch.nn.functional as F
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    folded = {k: (w.permute(0, 3, 1, 2).contiguous().cuda(), b.cuda()) for k, (w, b) in fid.fold_bn(sd).items()}

    def c(name, x):
        _, _, _, _, s, ph, pw = fid.LAYERS[name]
        w, b = folded[name]
        return F.relu(F.conv2d(x, w, b, stride=s, padding=(ph, pw)))

    def run():
        x = c("Conv2d_2b_3x3", c("Conv2d_2a_3x3", c("Conv2d_1a_3x3", x_nchw)))
        x = F.max_pool2d(c("Conv2d_4a_3x3", c("Conv2d_3b_1x1", F.max_pool2d(x, 3, 2))), 3, 2)
        for p in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            x = torch.cat([c(f"{p}.branch1x1", x), c(f"{p}.branch5x5_2", c(f"{p}.branch5x5_1", x)),
                           c(f"{p}.branch3x3dbl_3", c(f"{p}.branch3x3dbl_2", c(f"{p}.branch3x3dbl_1", x))),
                           c(f"{p}.branch_pool", F.avg_pool2d(x, 3, 1, 1, count_include_pad=False))], 1)
        x = torch.cat([c("Mixed_6a.branch3x3", x), c("Mixed_6a.branch3x3dbl_3", c("Mixed_6a.branch3x3dbl_2", c("Mixed_6a.branch3x3dbl_1", x))),
                       F.max_pool2d(x, 3, 2)], 1)
        for p in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            d = c(f"{p}.branch7x7dbl_1", x)
            for i in (2, 3, 4, 5):
                d = c(f"{p}.branch7x7dbl_{i}", d)
            x = torch.cat([c(f"{p}.branch1x1", x), c(f"{p}.branch7x7_3", c(f"{p}.branch7x7_2", c(f"{p}.branch7x7_1", x))), d,
                           c(f"{p}.branch_pool", F.avg_pool2d(x, 3, 1, 1, count_include_pad=False))], 1)
        d = c("Mixed_7a.branch7x7x3_1", x)
        for i in (2, 3, 4):
            d = c(f"Mixed_7a.branch7x7x3_{i}", d)
        x = torch.cat([c("Mixed_7a.branch3x3_2", c("Mixed_7a.branch3x3_1", x)), d, F.max_pool2d(x, 3, 2)], 1)
        for p, pool in (("Mixed_7b", lambda t: F.avg_pool2d(t, 3, 1, 1, count_include_pad=False)), ("Mixed_7c", lambda t: F.max_pool2d(t, 3, 1, 1))):
            t = c(f"{p}.branch3x3_1", x)
            d = c(f"{p}.branch3x3dbl_2", c(f"{p}.branch3x3dbl_1", x))
            x = torch.cat([c(f"{p}.branch1x1", x), c(f"{p}.branch3x3_2a", t), c(f"{p}.branch3x3_2b", t), c(f"{p}.branch3x3dbl_3a", d),
                           c(f"{p}.branch3x3dbl_3b", d), c(f"{p}.branch_pool", pool(x))], 1)
        return x.mean((2, 3))
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dims", type=int, default=2048)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch conv-stack yardstick")
    ap.add_argument("--unfused", action="store_true", help="also time the shared-input 1x1 convs as separate GEMMs")
    a = ap.parse_args()
    torch.manual_seed(0)
    sd = fid.random_state_dict(0)
    imgs = torch.randint(0, 256, (a.batch, 299, 299, 3), dtype=torch.uint8).cuda()
    flops = fid.conv_flops_per_image()
    res = {"batch": a.batch, "dims": a.dims, "gflop_per_image": round(flops / 1e9, 3)}
    variants = [("fused", True)] + ([("unfused", False)] if a.unfused else [])
    for tag, fuse in variants:
        model = fid.InceptionFID(dims=a.dims, state_dict=sd, fuse_1x1=fuse)
        t = timed(lambda: model.features(imgs), a.iters)
        res[f"{tag}_ms_per_batch"] = round(t * 1e3, 2)
        res[f"{tag}_images_per_s"] = round(a.batch / t, 1)
        res[f"{tag}_tflops"] = round(flops * a.batch / t / 1e12, 2)
        print(f"[{tag}] {a.batch / t:.1f} images/s, {flops * a.batch / t / 1e12:.2f} TF/s (conv FLOPs only), {t * 1e3:.1f} ms / batch of {a.batch}")
        if tag == "fused":
            rows = per_layer(model, imgs)
            by_geo = {}
            for name, g, ms in rows:
                key = g[:9]
                e = by_geo.setdefault(key, [0.0, 0, name])
                e[0] += ms
                e[1] += 1
            print(f"\nper-layer (one forward, batch {a.batch}; device events; fused 1x1 pairs as their own rows)")
            print(f"{'H':>4} {'W':>4} {'Cin':>5} {'Cout':>5} {'k':>5} {'s':>2} {'pad':>5} {'n':>3} {'ms':>8} {'TF/s':>7}  first layer")
            total = 0.0
            table = []
            for key, (ms, n, name) in sorted(by_geo.items(), key=lambda kv: -kv[1][0]):
                h, w, cin, cout, kh, kw, s, ph, pw = key
                ho, wo = (h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1
                f = 2.0 * a.batch * ho * wo * cout * kh * kw * cin * n
                total += ms
                table.append({"geom": key, "layers": n, "ms": round(ms, 3), "tflops": round(f / ms / 1e9, 2), "first": name})
                print(f"{h:4d} {w:4d} {cin:5d} {cout:5d} {kh}x{kw:<3d} {s:2d} {ph},{pw:<3d} {n:3d} {ms:8.3f} {f / ms / 1e9:7.2f}  {name}")
            print(f"convs {total:.2f} ms of {t * 1e3:.2f} ms per batch")
            res["per_geometry"] = table
            res["conv_ms"] = round(total, 2)
    if not a.no_torch:
        try:
            x = ops.fid_preprocess(imgs).permute(0, 3, 1, 2).contiguous()
            run = torch_stack(sd, x)
            t = timed(run, max(2, a.iters // 2), warmup=1)
            res["torch_ms_per_batch"] = round(t * 1e3, 2)
            res["torch_images_per_s"] = round(a.batch / t, 1)
            print(f"[torch f32 conv stack] {a.batch / t:.1f} images/s, {flops * a.batch / t / 1e12:.2f} TF/s")
        except Exception as e:             # the yardstick is optional: MIOpen may be absent or refuse a shape
            res["torch_error"] = f"{type(e).__name__}: {str(e)[:200]}"
            print(f"[torch f32 conv stack] not available: {res['torch_error']}")
    print(json.dumps({k: v for k, v in res.items() if k != "per_geometry"}))
    out = os.environ.get("BENCH_FID_JSON")
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
