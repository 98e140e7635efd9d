#!/usr/bin/env python3
"""A/B of the operand-fragment prefetch in the head-dim-16 attention backward pair (the VMAE heads at 256 images; template parameter PF
of the backward kernels, tune key 25: 1 = PF 1, 3 = none; shipped at head dim 16: none): timing and bitwise equality, same process, same
data.  Neutral, not shipped (csrc/attention.hip, attn_pf).
    make -C ldmae_amd/csrc diag && LDMAE_HIP_LIB=ldmae_amd/libldmae_hip_diag.so python tools/bench_attn16.py --prefetch [--f16]
(--prefetch is the only mode left: the one-kernel backward it used to be compared with is retired, tools/README.md.)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldmae_amd import _lib, ops  # noqa: E402


def ms(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    lib = _lib.load()
    if not hasattr(lib, "ldmae_tune"):
        sys.exit("needs the diagnostic build: LDMAE_HIP_LIB=ldmae_amd/libldmae_hip_diag.so")
    dtype = torch.float16 if "--f16" in sys.argv else torch.bfloat16
    B, H, hd = 256, 12, 16
    for N in (1024, 256):
        g = torch.Generator().manual_seed(0)
        qkv = torch.randn(B * N, 3 * H * hd, generator=g).to(dtype).cuda()
        do = torch.randn(B, N, H * hd, generator=g).to(dtype).cuda()
        o, lse = ops.attention_fwd_qkv(qkv, B, N, H, hd, hd ** -0.5)
        bwd = lambda: ops.attention_bwd_qkv(qkv, o, do, lse, B, N, H, hd, hd ** -0.5)      # noqa: E731
        res = {1: [], 3: []}
        for mode in (3, 1, 3, 1, 3, 1):
            _lib.call("ldmae_tune", 25, mode)
            res[mode].append(ms(bwd))
        _lib.call("ldmae_tune", 25, 3)
        a_ = bwd()
        _lib.call("ldmae_tune", 25, 1)
        b_ = bwd()
        _lib.call("ldmae_tune", 25, 0)
        print(f"N {N:5d} {str(dtype)[6:]}: backward pair without prefetch {min(res[3]):.3f} ms ({res[3]}) | PF 1 {min(res[1]):.3f} ms ({res[1]}) | bitwise equal {torch.equal(a_, b_)}", flush=True)


if __name__ == "__main__":
    main()
