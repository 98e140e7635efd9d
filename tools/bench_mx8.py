#!/usr/bin/env python3
"""The MXFP8 sampling mode against the bf16 path, in one process, alternating the two with a warm-up, device events and at least 0.5 s per
timed window:
  * the four block GEMMs with their real epilogues at B/1 (CFG batch 512: M = 524 288) and XL/1 (hidden 1152) against gemm_nt_lines_kernel:
    time and algorithmic TF/s (2 M N K);
  * the two stand-alone quantise passes (o, hid) and the fused norm + quantise against the plain norm: time and bytes/s;
  * forward_with_cfg of B/1 at batch 512 and XL/1 at batch 128, both modes;
  * drift: relative L2 of bf16 and of mxfp8 against the f32 kernels for one forward and for the end of a 10-step Euler trajectory, on a
    seeded randomised B/1.
  * --probe: the worst error of ONE scaled MFMA against f64 (the constant of tests/mx8_check.py's bound).
    python tools/bench_mx8.py [--out profiles/mx8_bench.txt] [--rows 524288] [--skip-forward] [--skip-drift] [--probe]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldmae_amd import ops                                              # noqa: E402
from ldmae_amd.models.lightningdit import LightningDiT_models          # noqa: E402

BF16 = torch.bfloat16
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def window(fn, min_ms=500.0):
    """ms per call over a window of at least min_ms (device events), after a warm-up call."""
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    n = max(2, int(min_ms / max(a.elapsed_time(b), 1e-3)) + 1)
    a.record()
    for _ in range(n):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def ab(f16, f8, rounds=2):
    """alternate the two, keep the best window of each"""
    t16, t8 = [], []
    for _ in range(rounds):
        t16.append(window(f16)); t8.append(window(f8))
    return min(t16), min(t8)


def gemms(tag, M, D, Hs, tokens):
    g = torch.Generator(device="cuda").manual_seed(0)
    rb = lambda *s: torch.randn(*s, device="cuda", generator=g).to(BF16)
    rf = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x, hid = rb(M, D), rb(M, Hs)
    w = {"qkv": rf(3 * D, D) * D ** -0.5, "proj": rf(D, D) * D ** -0.5, "w12": rf(2 * Hs, D) * D ** -0.5, "w3": rf(D, Hs) * Hs ** -0.5}
    wb = {k: v.to(BF16) for k, v in w.items()}
    wq = {k: ops.mx8_quantize(v) for k, v in w.items()}
    xq, hq = ops.mx8_quantize(x), ops.mx8_quantize(hid)
    bq, bp, b12, b3 = rf(3 * D), rf(D), rf(2 * Hs), rf(D)
    xin, gate = rf(M, D), rf(M // tokens, D)
    cases = [
        (f"qkv  bias     N={3 * D} K={D}", 3 * D, D, lambda: ops.gemm_nt(x, wb["qkv"], bq), lambda: ops.gemm_nt_mx8(*xq, *wq["qkv"], bq)),
        (f"proj gate_res N={D} K={D}", D, D, lambda: ops.gemm_nt_gate_res(x, wb["proj"], bp, xin, gate, tokens, save_y=False),
         lambda: ops.gemm_nt_gate_res_mx8(*xq, *wq["proj"], bp, xin, gate, tokens)),
        (f"w12  swiglu   N={2 * Hs} K={D}", 2 * Hs, D, lambda: ops.gemm_nt_swiglu(x, wb["w12"], b12, save_h12=False), lambda: ops.gemm_nt_swiglu_mx8(*xq, *wq["w12"], b12)),
        (f"w3   gate_res N={D} K={Hs}", D, Hs, lambda: ops.gemm_nt_gate_res(hid, wb["w3"], b3, xin, gate, tokens, save_y=False),
         lambda: ops.gemm_nt_gate_res_mx8(*hq, *wq["w3"], b3, xin, gate, tokens)),
    ]
    say(f"-- block GEMMs, {tag}: M = {M}, forward-only epilogues; bf16 = gemm_nt_lines_kernel")
    s16 = s8 = 0.0
    for name, N, K, f16, f8 in cases:
        t16, t8 = ab(f16, f8)
        fl = 2.0 * M * N * K
        s16 += t16; s8 += t8
        say(f"   {name:34s} bf16 {t16:8.3f} ms {fl / t16 / 1e9:7.1f} TF/s | mxfp8 {t8:8.3f} ms {fl / t8 / 1e9:7.1f} TF/s | mxfp8 / bf16 time {t8 / t16:.3f}")
    say(f"   {'sum of the four':34s} bf16 {s16:8.3f} ms              | mxfp8 {s8:8.3f} ms              | mxfp8 / bf16 time {s8 / s16:.3f}")
    # passes
    say(f"-- quantise passes, {tag}")
    o = rb(M, D)
    for name, t, K in (("quantize(o)", o, D), ("quantize(hid)", hid, Hs)):
        ms = window(lambda: ops.mx8_quantize(t))
        by = M * K * (2 + 1 + 1 / 32)
        say(f"   {name:34s} {ms:8.3f} ms  {by / ms / 1e6:8.1f} GB/s  ({by / 1e6:.0f} MB read + written)")
    xf, nw, mod = rf(M, D), rf(D), rf(M // tokens, 6 * D)
    t_plain = window(lambda: ops.rmsnorm_modulate_fwd(xf, nw, mod[:, :D], mod[:, D:2 * D], tokens, BF16))
    t_fused = window(lambda: ops.rmsnorm_modulate_fwd_mx8(xf, nw, mod[:, :D], mod[:, D:2 * D], tokens))
    b_plain, b_fused = M * D * (4 + 2), M * D * (4 + 1 + 1 / 32)
    say(f"   {'rmsnorm_modulate_fwd (bf16 out)':34s} {t_plain:8.3f} ms  {b_plain / t_plain / 1e6:8.1f} GB/s")
    say(f"   {'rmsnorm_modulate_fwd_mx8':34s} {t_fused:8.3f} ms  {b_fused / t_fused / 1e6:8.1f} GB/s  (fused / plain time {t_fused / t_plain:.3f})")


def randomise(m, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "adaLN_modulation" in n or n.startswith("final_layer.linear"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    return m


def model(name, latent=32):
    torch.manual_seed(0)
    m = LightningDiT_models[name](input_size=latent, num_classes=1000, use_qknorm=True, use_swiglu=True, use_rope=True, use_rmsnorm=True,
                                  wo_shift=False, in_channels=16, use_checkpoint=False, class_dropout_prob=0.1)
    return randomise(m).cuda().eval()


def forward(name, batch):
    m = model(name)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(batch, 16, 32, 32, device="cuda", generator=g)
    t = torch.full((batch,), 0.4, device="cuda")
    y = torch.cat([torch.randint(0, 1000, (batch // 2,), device="cuda", generator=g), torch.full((batch // 2,), 1000, device="cuda")])

    def run(mode):
        m.set_gemm_precision(mode)
        with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
            return m.forward_with_cfg(x, t, y, 4.0)
    t16, t8 = ab(lambda: run(None), lambda: run("mxfp8"))
    m.set_gemm_precision(None)
    say(f"-- forward_with_cfg {name} batch {batch}: bf16 {t16:8.2f} ms | mxfp8 {t8:8.2f} ms | mxfp8 / bf16 time {t8 / t16:.3f}")
    del m
    torch.cuda.empty_cache()


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def drift(batch=8, steps=10):
    m = model("LightningDiT-B/1")
    g = torch.Generator(device="cuda").manual_seed(2)
    x0 = torch.randn(batch, 16, 32, 32, device="cuda", generator=g)
    y = torch.cat([torch.randint(0, 1000, (batch // 2,), device="cuda", generator=g), torch.full((batch // 2,), 1000, device="cuda")])

    def traj(mode, dtype):
        m.set_gemm_precision(mode)
        x, first = x0.clone(), None
        with torch.no_grad(), torch.autocast("cuda", dtype=BF16, enabled=dtype == BF16):
            for i in range(steps):                                  # plain Euler on the model output as the velocity, t from 0 to 1
                t = torch.full((batch,), i / steps, device="cuda")
                v = m.forward_with_cfg(x, t, y, 4.0).float()
                first = v if first is None else first
                x = x + v / steps
        m.set_gemm_precision(None)
        return first, x
    f32 = traj(None, torch.float32)
    b16 = traj(None, BF16)
    mx8 = traj("mxfp8", BF16)
    say(f"-- drift on a seeded randomised B/1 (batch {batch}, CFG 4), relative L2 against the f32 kernels")
    say(f"   one forward:                bf16 {rel(b16[0], f32[0]):.3e} | mxfp8 {rel(mx8[0], f32[0]):.3e}")
    say(f"   end of a {steps}-step Euler path: bf16 {rel(b16[1], f32[1]):.3e} | mxfp8 {rel(mx8[1], f32[1]):.3e}")


def probe(draws=4):
    """One-instruction probe of the scaled MFMA: gemm_nt_mx8 at K = 128 without bias and with f32 output is one instruction per output element
    on a zero accumulator.  Random e4m3 codes (NaN codes excluded) and random E8M0 scales; worst |got - f64| / sum |a| |w|."""
    def deq(q, s):
        v = q.view(torch.float8_e4m3fn).float().double().reshape(q.shape[0], -1, 32)
        return (v * torch.exp2((s.double() - 127)).unsqueeze(-1)).reshape(q.shape)
    g = torch.Generator().manual_seed(0)
    worst = 0.0
    say("-- one-instruction probe of v_mfma_scale_f32_16x16x128_f8f6f4 (K = 128, zero accumulator), 256 x 256 outputs per draw")
    for spread in (0, 3, 7, 20):
        w_s = 0.0
        for _ in range(draws):
            code = lambda: torch.randint(0, 127, (256, 128), generator=g).to(torch.uint8) | (torch.randint(0, 2, (256, 128), generator=g).to(torch.uint8) << 7)
            sc = lambda: (127 + torch.randint(-spread, spread + 1, (256, 4), generator=g)).to(torch.uint8)
            aq, asc, wq, wsc = code(), sc(), code(), sc()
            o = ops.gemm_nt_mx8(aq.cuda(), asc.cuda(), wq.cuda(), wsc.cuda(), None, out_dtype=torch.float32).cpu().double()
            a, w = deq(aq, asc), deq(wq, wsc)
            w_s = max(w_s, float(((o - a @ w.T).abs() / (a.abs() @ w.abs().T)).max()))
        say(f"   scale exponents within +-{spread:2d}: worst |err| / S = {w_s:.4e}")
        worst = max(worst, w_s)
    say(f"   worst of all: {worst:.4e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=524288)
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--skip-drift", action="store_true")
    ap.add_argument("--probe", action="store_true", help="only the one-instruction error probe of the scaled MFMA")
    a = ap.parse_args()
    say(f"bench_mx8: {torch.cuda.get_device_name(0)}; windows >= 0.5 s, device events, bf16 and mxfp8 alternated, best of 2")
    probe()
    if a.probe:
        return
    gemms("B/1", a.rows, 768, 2048, 1024)
    gemms("XL/1", a.rows // 4, 1152, 3072, 1024)
    if not a.skip_forward:
        forward("LightningDiT-B/1", 512)
        forward("LightningDiT-XL/1", 128)
    if not a.skip_drift:
        drift()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
