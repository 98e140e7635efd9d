#!/usr/bin/env python3
"""Records the output bits of the flat f32 kernels and of every kernel with a 256-thread block sum: tests/golden/flat_bits.json.

    python tests/golden/make_golden_flat_bits.py <commit hash of the tree it runs in>       (on an MI355X; FLAT_BITS_OUT=path: write there)

The file is a record of behaviour that must not change, so it is generated from a build of the commit BEFORE the change under test (the
whole tree of that commit: its library and its ops.py), never from the code a test then checks against it.  One SHA-256 per named case,
over the raw bytes of the case's outputs in order.  tests/test_gpu_flat_bits.py recomputes every case with cases() below and compares.

Inputs come from a closed-form integer hash (values(): a function of the element index and a salt), never from a random generator, so the
file does not depend on a generator's version.  The shapes are the smallest at which the walker, its tail and the chunk map of the row
reduction can go wrong, not sampler shapes:
  flat kernels     n in 1, 3, 4, 5, 4095, 4096, 4097, 4099, 8193 (4096 elements = 1024 float4 items = one block; 8193 leaves a block that
                   holds the tail alone); the two draws once more at n = 4099 into a view one element off a 16-byte boundary (the scalar
                   store path); the time-vector side output with nt = 3
  row reductions   (B, m) in (1, 1), (1, 4097), (3, 5), (3, 4096), (3, 4099), (2, 8196): B > 1 with m % 4 != 0 takes the scalar map, the
                   others the vector map; (1, 4097) also from a view one element off (scalar map)
  block sums       one or two small cases per kernel whose block sum is the shared one
"""
import hashlib
import json
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "flat_bits.json")
FLAT_N = (1, 3, 4, 5, 4095, 4096, 4097, 4099, 8193)
ROWS = ((1, 1), (1, 4097), (3, 5), (3, 4096), (3, 4099), (2, 8196))
SEED, COUNTER = 0x1234567890ABCDEF, 2 ** 33 + 5            # both words of the key and of the counter in use


def hash32(n, salt):
    """n 32-bit words, word i a function of (i, salt) alone (two rounds of a multiply-xorshift mixer, in 64-bit integers)."""
    x = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503) + np.uint64(1)) & np.uint64(0xffffffff)
    for _ in range(2):
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(0x45d9f3b)) & np.uint64(0xffffffff)
    return x ^ (x >> np.uint64(16))


def values(n, salt):
    """n f32 values in [-2, 2)."""
    return ((hash32(n, salt).astype(np.float64) / 2.0 ** 32 - 0.5) * 4.0).astype(np.float32)


def cases(ops, torch):
    """Yields (name, [output tensors]) for every case; the same code serves the generator and the test."""
    dev = "cuda"

    def f(shape, salt, offset=0):
        n = int(np.prod(shape))
        buf = torch.from_numpy(values(n + offset, salt)).to(dev)
        return buf[offset:].view(shape)

    def empty(n, offset=0, dtype=torch.float32):
        return torch.full((n + offset,), -7.0, dtype=dtype, device=dev)[offset:]

    h_dev = torch.tensor([0.0375], dtype=torch.float32, device=dev)
    t_dev = torch.tensor([0.25], dtype=torch.float32, device=dev)
    coef7 = [0.2, -0.3, 0.975, 2.0 / 3.0, -1.0 / 7.0, 0.0625, 1.3]
    for n in FLAT_N:
        ld = ops.ode_slab_ld(n)
        k = torch.zeros(7, ld, dtype=torch.float32, device=dev)
        k[:, :n] = f((7, n), 1)
        y, y1, ym = f((n,), 2), f((n,), 3), f((n,), 4)
        for m in (1, 7):
            out, t_out = empty(n), empty(3)
            ops.rk_stage(y, k, coef7[:m], h_dev, out, t_dev=t_dev, ct=0.3, t_out=t_out)
            yield f"rk_stage-m{m}-n{n}", [out, t_out]
        out, partial, ratio = empty(n), empty(ops.ode_partials(n)), empty(1)
        ops.dopri5_finish(y, k, h_dev, 1e-3, 1e-2, out, partial, ratio)
        yield f"dopri5_finish-n{n}", [out, partial, ratio]
        partial, norm = empty(ops.ode_partials(n)), empty(1)
        ops.rms_norm_scaled(y1, y, 1e-3, 1e-2, partial, norm)
        yield f"rms_norm_scaled-n{n}", [partial, norm]
        out = empty(n)
        ops.dopri5_interp(y, y1, ym, k, h_dev, t_dev, 0.26, out)
        yield f"dopri5_interp-n{n}", [out]
        yield f"rademacher-n{n}", [ops.rademacher((n,), SEED, COUNTER, dev)]
        yield f"normal-n{n}", [ops.normal((n,), SEED, COUNTER, dev)]
        ins = [y, y1, ym, f((n,), 5)]
        for m in (1, 4):
            for mode in ("none", "tensor", "philox"):
                out, mean, t_out = empty(n), empty(n), empty(3)
                ops.sde_combine(ins[:m], coef7[:m], out, noise_coef=0.0 if mode == "none" else 0.7, z=f((n,), 6) if mode == "tensor" else None,
                                seed=SEED if mode == "philox" else None, counter=COUNTER, mean_out=mean, t_next=0.4375, t_out=t_out)
                yield f"sde_combine-m{m}-{mode}-n{n}", [out, mean, t_out]
    out = empty(4099, offset=1)
    ops.call("ldmae_rademacher_f32", ops.ptr(out), 4099, SEED, COUNTER, ops.stream())
    yield "rademacher-n4099-offset", [out]
    yield "normal-n4099-offset", [ops.normal((4099,), SEED, COUNTER, dev, out=empty(4099, offset=1))]

    for B, m in ROWS:
        for off in ((0, 1) if (B, m) == (1, 4097) else (0,)):
            tag = f"B{B}-m{m}" + ("-offset" if off else "")
            a, b = f((B, m), 7, off), f((B, m), 8, off)
            yield f"rowdot-{tag}", [ops.rowdot(a, b)]
            yield f"row_mse-f32-{tag}", [ops.row_mse(a, b)]
            a16 = torch.from_numpy(values(B * m + off, 7)).to(dev).to(torch.bfloat16)[off:].view(B, m)
            yield f"row_mse-bf16-{tag}", [ops.row_mse(a16, b)]

    for C in (32, 128):                                     # one channel per group (scalar loads), four (16-byte loads)
        yield f"gn_stats-C{C}", list(ops.groupnorm_stats_nhwc(f((1, 2, 2, C), 9)))
    for ld, cols in ((16, 5), (304, 300)):
        yield f"softmax_rows-cols{cols}", [ops.softmax_rows_(f((2, ld), 10).clone(), cols, 0.5)]
    yield "is_softmax-C1008", list(ops.adm_softmax_is(f((3, 1008), 11)))
    for C in (10, 1000, 4097):                              # registers (1 and 4 values per thread), and beyond the register path
        yield f"softmax_xent-C{C}", list(ops.softmax_xent(f((3, C), 12), [0, C - 1, C // 2], grad_scale=0.5))
    for n in (1, 4097):
        yield f"lars_norms-n{n}", [ops.lars_norms(f((n,), 13), f((n,), 14), 0.1)]
    for M, D in ((5, 3), (2, 130)):
        yield f"row_sqnorms-M{M}-D{D}", [ops.row_sqnorms(f((M, D), 15))]
    dec8, ref8, sse = ops.recon_quantize_sse(f((2, 3, 5, 7), 16), f((2, 3, 5, 7), 17))
    yield "recon_quantize_sse", [dec8, ref8, sse]
    yield "sse_u8", [ops.sse_u8(dec8, ref8)]
    yield "lpips_layer-f32-C64", [ops.lpips_layer(f((2, 2, 2, 64), 18), f((64,), 19).abs(), torch.zeros(1, dtype=torch.float32, device=dev))]
    yield "ssim-one_tile", [ops.ssim(f((1, 1, 16, 16), 20), f((1, 1, 16, 16), 21))]
    mask = torch.tensor([[1.0, 0.0, 0.0, 1.0]], dtype=torch.float32, device=dev)
    yield "mae_loss_fwd", [ops.mae_loss_fwd(f((1, 3, 8, 8), 22), f((1, 3, 8, 8), 23), mask, 4)]
    yield "conv3x3_bwd", list(ops.conv3x3_bwd(f((1, 3, 4, 4), 24), f((1, 3, 4, 4), 25), f((3, 3, 3, 3), 26)))
    for C, kk, H, W in ((2, 1, 1, 2), (2, 1, 1, 7), (4, 4, 32, 32)):       # k * H * W = 2, 7, 4096
        pos, neg, x = f((2, C, H, W), 27), f((2, C, H, W), 28), f((2, C, H, W), 29)
        t = torch.tensor([0.25, 0.875], dtype=torch.float32, device=dev)
        yield f"guidance-rescale-{kk * H * W}", [ops.guidance_combine("rescale", pos, neg, 2.5, k=kk, phi=0.7)]
        mom = f((2, kk * H * W), 30).clone()
        out = ops.guidance_combine("apg", pos, neg, 2.5, k=kk, x=x, t=t, eta=0.5, norm_threshold=2.5, momentum=-0.5, mom=mom)
        yield f"guidance-apg-{kk * H * W}", [out, mom]
    idx = (hash32(2 * 33, 31) % 40).astype(np.int32).reshape(2, 33)
    yield "kid_sums", [ops.kid_sums(f((40, 16), 32), f((40, 16), 33), idx, idx[::-1].copy(), 1.0 / 16.0)]
    vals, nidx = f((3, 5), 34), torch.from_numpy((hash32(15, 35) % 20).astype(np.int32).reshape(3, 5)).to(dev)
    yield "knn_vote", [ops.knn_vote(vals, nidx, (hash32(20, 36) % 7).astype(np.int64), [0, 3, 6], 7)]


def digest(outputs):
    h = hashlib.sha256()
    for t in outputs:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    import torch
    from ldmae_amd import _lib, ops
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    assert _lib.load().ldmae_arch() == b"gfx950"
    out = {name: digest(outputs) for name, outputs in cases(ops, torch)}
    torch.cuda.synchronize()
    head = ("Recorded by tests/golden/make_golden_flat_bits.py on an MI355X from the tree of the commit named here, BEFORE the flat kernels "
            "moved onto csrc/flat_common.h and the block sums onto csrc/common.h: the old behaviour, never the code under test.")
    path = os.environ.get("FLAT_BITS_OUT", OUT)
    with open(path, "w") as fh:
        json.dump({"_comment": head, "commit": sys.argv[1], "sha256": out}, fh, indent=1)
        fh.write("\n")
    print(f"{len(out)} cases from {_lib.LIB_PATH} -> {path}")


if __name__ == "__main__":
    main()
