#!/usr/bin/env python3
"""Throughput of the convolutional KL-VAE tokenizer on the HIP kernels at the product shape (the reference drivers' Diffusers_AutoencoderKL:
block widths (128, 256, 512, 512), two layers per block, 16 latent channels, 256 x 256 images, batch 16):

  - encode and decode images/s and TF/s (operations counted from the shapes of every convolution and GEMM call, over event time);
  - a per-call table (op, shape, GFLOP, ms, TF/s), calls of one op and shape added up;
  - the same network in torch (F.group_norm / F.silu / F.conv2d, f32, NCHW, TF32 off) on the same weights and input as yardstick;
  - the fused norm-act gather against "normalise kernel, then plain convolution" on the 256 x 256 x 128 layer, alternating;
  - all of it per --precision: "f32" (the exact-f32 MFMA) and "tf32" (operands rounded once to fp16, f32 accumulation; set_precision), and
    for tf32 the fused / two-pass comparison on the 256 x 256 x 128 and the 32 x 32 x 512 layer plus each layer class against its f32 kernel,
    alternating in one process.

    python tools/bench_conv_vae.py [--batch 16] [--size 256] [--iters 5] [--precision f32,tf32] [--no-torch] [--out profiles/conv_vae_bench.txt]
"""
import argparse
import os
import sys
from collections import OrderedDict

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ldmae_amd import ops  # noqa: E402
from ldmae_amd.tokenizer import autoencoder as ae  # noqa: E402
from ldmae_amd.tokenizer.sdvae import Diffusers_AutoencoderKL  # noqa: E402

OUT = None


def say(s=""):
    print(s, flush=True)
    if OUT is not None:                 # line by line: a run that is cut short keeps what it measured
        OUT.write(s + "\n")
        OUT.flush()


def timed(fn, iters, warmup=2):
    """Median milliseconds of `iters` timed calls (device events) after `warmup` untimed ones."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


# ---------------------------------------------------------------------------------------------------- operation counts and the per-call table
class Ledger:
    """Wraps the op-level entry points: counts 2 M N K per call and, when `events` is on, brackets each call with device events."""
    OPS = ("conv3x3_vae_nhwc", "conv2d_nhwc", "conv1x1_res_nhwc", "gemm_nt", "groupnorm_stats_nhwc", "groupnorm_apply_nhwc", "softmax_rows_")

    def __init__(self):
        self.rows, self.events, self.saved = OrderedDict(), False, {}

    def flops(self, name, args, kwargs, out):
        if name == "conv3x3_vae_nhwc":
            return 2.0 * out.numel() * 9 * args[0].shape[3], f"{tuple(args[0].shape)} -> {out.shape[3]} mode {kwargs.get('mode', 0)}"
        if name == "conv2d_nhwc":
            w = args[1]
            return 2.0 * out.numel() * w.shape[1] * w.shape[2] * w.shape[3], f"{tuple(args[0].shape)} -> {out.shape[3]} k{w.shape[1]}"
        if name == "conv1x1_res_nhwc":
            return 2.0 * out.numel() * args[0].shape[-1], f"{tuple(args[0].shape)} -> {out.shape[-1]}"
        if name == "gemm_nt":
            return 2.0 * args[0].shape[0] * args[1].shape[0] * args[0].shape[1], f"{tuple(args[0].shape)} x {tuple(args[1].shape)}^T"
        return 0.0, f"{tuple(args[0].shape)}"

    def __enter__(self):
        for name in self.OPS:
            self.saved[name] = getattr(ops, name)
            setattr(ops, name, self.wrap(name, self.saved[name]))
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(ops, name, fn)

    def wrap(self, name, fn):
        def inner(*args, **kwargs):
            if self.events:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
            out = fn(*args, **kwargs)
            fl, shape = self.flops(name, args, kwargs, out if torch.is_tensor(out) else args[0])
            row = self.rows.setdefault((name, shape), [0, 0.0, []])
            row[0] += 1
            row[1] += fl
            if self.events:
                b.record()
                row[2].append((a, b))
            return out
        return inner

    def total(self):
        return sum(r[1] for r in self.rows.values())

    def table(self, title):
        torch.cuda.synchronize()
        say(f"{title}: per call (calls of one op and shape added up; event time includes the launch gap after the previous call)")
        say(f"  {'op':22s} {'shape':44s} {'calls':>5s} {'GFLOP':>9s} {'ms':>8s} {'TF/s':>7s}")
        for (name, shape), (n, fl, evs) in self.rows.items():
            ms = sum(a.elapsed_time(b) for a, b in evs)
            say(f"  {name:22s} {shape:44s} {n:5d} {fl / 1e9:9.2f} {ms:8.3f} {fl / ms / 1e9 if fl and ms else 0:7.1f}")


# ---------------------------------------------------------------------------------------------------- the torch yardstick
def t_norm(n, x, act=True):
    y = F.group_norm(x, n.num_groups, n.weight, n.bias, n.eps)
    return F.silu(y) if act else y


def t_res(b, x):
    h = F.conv2d(t_norm(b.norm1, x), b.conv1.weight, b.conv1.bias, padding=1)
    h = F.conv2d(t_norm(b.norm2, h), b.conv2.weight, b.conv2.bias, padding=1)
    if b.in_channels != b.out_channels:
        x = F.conv2d(x, b.nin_shortcut.weight, b.nin_shortcut.bias)
    return x + h


def t_attn(a, x):
    h = t_norm(a.norm, x, act=False)
    q, k, v = (F.conv2d(h, m.weight, m.bias) for m in (a.q, a.k, a.v))
    B, C, H, W = q.shape
    w = torch.softmax(torch.bmm(q.reshape(B, C, H * W).permute(0, 2, 1), k.reshape(B, C, H * W)) * (int(C) ** -0.5), dim=2)
    h = torch.bmm(v.reshape(B, C, H * W), w.permute(0, 2, 1)).reshape(B, C, H, W)
    return x + F.conv2d(h, a.proj_out.weight, a.proj_out.bias)


def t_mid(m, h):
    return t_res(m.mid.block_2, t_attn(m.mid.attn_1, t_res(m.mid.block_1, h)))


def t_encoder(e, x):
    h = F.conv2d(x, e.conv_in.weight, e.conv_in.bias, padding=1)
    for i in range(e.num_resolutions):
        for j in range(e.num_res_blocks):
            h = t_res(e.down[i].block[j], h)
        if i != e.num_resolutions - 1:
            c = e.down[i].downsample.conv
            h = F.conv2d(F.pad(h, (0, 1, 0, 1)), c.weight, c.bias, stride=2)
    return F.conv2d(t_norm(e.norm_out, t_mid(e, h)), e.conv_out.weight, e.conv_out.bias, padding=1)


def t_decoder(d, z):
    h = t_mid(d, F.conv2d(z, d.conv_in.weight, d.conv_in.bias, padding=1))
    for i in reversed(range(d.num_resolutions)):
        for j in range(d.num_res_blocks + 1):
            h = t_res(d.up[i].block[j], h)
        if i != 0:
            c = d.up[i].upsample.conv
            h = F.conv2d(F.interpolate(h, scale_factor=2.0, mode="nearest"), c.weight, c.bias, padding=1)
    return F.conv2d(t_norm(d.norm_out, h), d.conv_out.weight, d.conv_out.bias, padding=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_vae_bench.txt"))
    ap.add_argument("--precision", default="f32,tf32", help="comma-separated: f32, tf32 (default both, so that each is timed against the other)")
    ap.add_argument("--no-torch", action="store_true", help="leave the torch yardstick out (its first call per shape pays MIOpen's kernel search)")
    args = ap.parse_args()
    precisions = [ae.check_precision(p) for p in args.precision.split(",")]
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_vae needs a GPU: nothing is measured without one")
    global OUT
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    OUT = open(args.out, "w")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(0)
    B, S = args.batch, args.size
    vae = Diffusers_AutoencoderKL(img_size=S, layers_per_block=2, latent_channels=16, block_out_channels=(128, 256, 512, 512),
                                  use_quant_conv=False, use_post_quant_conv=False).cuda().eval()
    x = torch.rand(B, 3, S, S, device="cuda") * 2 - 1
    say(f"conv KL-VAE (128, 256, 512, 512), latent 16, batch {B}, {S} x {S}, precision {' and '.join(precisions)}; {torch.cuda.get_device_name(0)}; median of {args.iters}")

    # ---- fused gather against two passes, alternating: the widest-image layer and (tf32) the deepest one; each precision against the other
    blk = vae.decoder.up[0].block[1]
    deep = vae.decoder.mid.block_1
    f16 = torch.float16
    for (hh, C, rb) in ((S, 128, blk), (S // 8, 512, deep)):
        h = torch.randn(B, hh, hh, C, device="cuda")
        w, bias, ga, be = ae._packed(rb.conv1), ae._f32(rb.conv1.bias), ae._f32(rb.norm1.weight), ae._f32(rb.norm1.bias)
        w16 = ae._packed_f16(rb.conv1)
        st = ops.groupnorm_stats_nhwc(h)
        fl = 2.0 * B * hh * hh * C * 9 * C
        forms = OrderedDict()
        if "f32" in precisions:
            forms["f32 fused"] = lambda: ops.conv3x3_vae_nhwc(h, w, bias, mode=ops.VAE_NORM_ACT, stats=st, gamma=ga, beta=be)
            forms["f32 two-pass"] = lambda: ops.conv3x3_vae_nhwc(ops.groupnorm_apply_nhwc(h, st, ga, be, silu=True), w, bias)
            forms["f32 plain conv"] = lambda: ops.conv3x3_vae_nhwc(h, w, bias)
        if "tf32" in precisions:
            forms["tf32 fused"] = lambda: ops.conv3x3_vae_nhwc(h, w16, bias, mode=ops.VAE_NORM_ACT, stats=st, gamma=ga, beta=be, precision="tf32")
            forms["tf32 two-pass"] = lambda: ops.conv3x3_vae_nhwc(ops.groupnorm_apply_nhwc(h, st, ga, be, silu=True, out_dtype=f16), w16, bias,
                                                                  precision="tf32")
            forms["tf32 plain conv"] = lambda: ops.conv3x3_vae_nhwc(h, w16, bias, precision="tf32")
        say(f"norm-act on [{B}, {hh}, {hh}, {C}] -> {C} ({fl / 1e9:.1f} GFLOP), alternating, ms:")
        res = {k: [] for k in forms}
        for _ in range(3):
            for k, fn in forms.items():
                res[k].append(timed(fn, args.iters))
        for k, v in res.items():
            say(f"  {k:15s} {' '.join(f'{t:8.3f}' for t in v)}   best {min(v):8.3f} ms  {fl / min(v) / 1e9:6.1f} TF/s")
        say(f"  statistics {timed(lambda: ops.groupnorm_stats_nhwc(h), args.iters):8.3f} ms; normalise+SiLU pass to f32 "
            f"{timed(lambda: ops.groupnorm_apply_nhwc(h, st, ga, be, silu=True), args.iters):8.3f} ms, to fp16 "
            f"{timed(lambda: ops.groupnorm_apply_nhwc(h, st, ga, be, silu=True, out_dtype=f16), args.iters):8.3f} ms")
        for prec, knob in (("f32", ae.FUSED_NORM_ACT), ("tf32", ae.TF32_FUSED_NORM_ACT)):
            if prec in precisions:
                say(f"  {prec}: shipped {'fused gather' if knob else 'two-pass'}; faster here: "
                    f"{'fused gather' if min(res[prec + ' fused']) < min(res[prec + ' two-pass']) else 'two-pass'}")
        del h, forms
    if len(precisions) == 2:
        # the other layer classes, tf32 against f32, alternating: down, up, the 3-channel head, the residual 1x1
        say("layer classes, f32 / tf32 alternating, best of 3 medians, ms:")
        cases = []
        for name, shape, mod, mode in (("down 256x256x128", (B, S, S, 128), vae.encoder.down[0].downsample.conv, ops.VAE_DOWN),
                                       ("up 128x128x256", (B, S // 2, S // 2, 256), vae.decoder.up[1].upsample.conv, ops.VAE_UP),
                                       ("conv_out 256x256x128 -> 3", (B, S, S, 128), vae.decoder.conv_out, ops.VAE_PLAIN)):
            h = torch.randn(*shape, device="cuda")
            w, w16, bias = ae._packed(mod), ae._packed_f16(mod), ae._f32(mod.bias)
            cases.append((name, (lambda h=h, w=w, bias=bias, mode=mode: ops.conv3x3_vae_nhwc(h, w, bias, mode=mode)),
                          (lambda h=h, w16=w16, bias=bias, mode=mode: ops.conv3x3_vae_nhwc(h, w16, bias, mode=mode, precision="tf32"))))
        h1 = torch.randn(B, S // 8, S // 8, 512, device="cuda")
        w1 = torch.randn(512, 512, device="cuda") / 23
        w1h = ops.cast(w1, f16)
        cases.append(("1x1 + residual 32x32x512", lambda: ops.conv1x1_res_nhwc(h1, w1, res=h1), lambda: ops.conv1x1_res_nhwc(h1, w1h, res=h1, precision="tf32")))
        for name, f32fn, tf32fn in cases:
            a, b = [], []
            for _ in range(3):
                a.append(timed(f32fn, args.iters))
                b.append(timed(tf32fn, args.iters))
            say(f"  {name:28s} f32 {min(a):8.3f}   tf32 {min(b):8.3f}   x{min(a) / min(b):.2f}")
        del cases, h1

    # ---- the whole encoder and decoder, per precision, in both forms of norm-act; the per-call table is taken in the shipped form
    knob = {"f32": "FUSED_NORM_ACT", "tf32": "TF32_FUSED_NORM_ACT"}
    with torch.no_grad():
        z = vae.encode_images(x)
        for name, fn, tfn in (("encode", lambda: vae.encode_images(x), lambda: t_encoder(vae.encoder, x)),
                              ("decode", lambda: vae.decode(z).sample, lambda: t_decoder(vae.decoder, z))):
            outs, f32_out = [], None
            for prec in precisions:
                vae.set_precision(prec)
                shipped = getattr(ae, knob[prec])
                for form in (False, True):
                    setattr(ae, knob[prec], form)
                    with Ledger() as led:
                        out = fn()
                        flops = led.total()
                    ms = timed(fn, args.iters)
                    outs.append((prec, form, ms, out))
                    say(f"{name} [{prec}, {'fused gather' if form else 'two-pass'}{', shipped' if form == shipped else ''}]: {ms:9.2f} ms  "
                        f"{B / ms * 1e3:8.1f} img/s  {flops / ms / 1e9:6.1f} TF/s ({flops / B / 1e9:.1f} GFLOP per image)")
                    if prec == "f32" and form == shipped:
                        f32_out = out
                    elif prec == "tf32" and f32_out is not None:
                        say(f"  max|tf32 - f32| / max|f32| {float((out - f32_out).abs().max() / f32_out.abs().max()):.2e}")
                setattr(ae, knob[prec], shipped)
                with Ledger() as led:
                    led.events = True
                    fn()
                    led.table(f"{name} [{prec}, {'fused gather' if shipped else 'two-pass'}]")
            vae.set_precision("f32")
            if not args.no_torch:          # last: the first torch call of every shape pays MIOpen's kernel search
                ref = tfn()
                tms = timed(tfn, args.iters)
                say(f"{name} [torch f32, F.conv2d / group_norm / silu]: {tms:9.2f} ms  {B / tms * 1e3:8.1f} img/s  {flops / tms / 1e9:6.1f} TF/s (our operation count)")
                for prec, form, ms, out in outs:
                    err = float((out - ref).abs().max() / ref.abs().max())
                    say(f"  {prec} {'fused gather' if form else 'two-pass'}: x{tms / ms:.2f} of torch, max|diff|/max against torch {err:.1e}")
                del ref
            del out, outs, f32_out
    OUT.close()


if __name__ == "__main__":
    main()
