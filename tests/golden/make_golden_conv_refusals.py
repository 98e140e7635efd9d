#!/usr/bin/env python3
"""Records what the convolution entry points answer to arguments they refuse: tests/golden/conv_refusals.json.

    LDMAE_HIP_LIB=/path/to/the/OLD/libldmae_hip.so python tests/golden/make_golden_conv_refusals.py

The file is a record of behaviour that must not change, so it is generated from a build of the commit BEFORE the change under test (the
parent of the commit that gave the convolutions their shared skeleton, csrc/conv_igemm_common.h, wrote the one committed here), never from
the code a test then checks against it.  One call per LDMAE_REQUIRE of each entry; every argument list is a valid small problem with one
thing wrong, on dummy pointers (16: aligned, 20: misaligned, null), so a call that is not refused would reach a launch: run this where no
GPU is present, like the test.  A refusal that cannot be provoked is not listed: the grid bound of the 16-bit entries, cdiv(M, 128) *
cdiv(N, 128) < 2^31, always holds once M * N < 2^40 does.
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from ldmae_amd import _lib  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_refusals.json")
P, P20, NUL = 16, 20, None
BIG = dict(B=1 << 11, H=1 << 10, W=1 << 10)                # B H W = 2^31
M30 = dict(B=1, H=1 << 15, W=1 << 15)                      # B H W = 2^30


def conv2d(**k):
    a = dict(x=P, ldx=8, xoff=0, w=P, bias=P, out=P, ldo=8, ooff=0, B=1, H=4, W=4, Cin=8, Cout=8, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, relu=1)
    a.update(k)
    return [a[n] for n in "x ldx xoff w bias out ldo ooff B H W Cin Cout kh kw sh sw ph pw relu".split()] + [None]


def dgrad(**k):
    a = dict(dy=P, y=P, w=P, dx=P, B=1, H=4, W=4, Cy=8, Cx=8)
    a.update(k)
    return [a[n] for n in "dy y w dx B H W Cy Cx".split()] + [None]


def relu16(**k):
    a = dict(x=P, w=P, bias=P, out=P, B=1, H=4, W=4, Cin=8, Cout=8)
    a.update(k)
    return [a[n] for n in "x w bias out B H W Cin Cout".split()] + [None]


def vae(f16, **k):
    a = dict(mode=0, x_dtype=0, x=P, w=P, bias=P, res=P, mean=P, rstd=P, gamma=P, beta=P, G=2, silu=1, out=P, B=1, H=4, W=4, Cin=8, Cout=8)
    a.update(k)
    names = "mode x_dtype x w bias res mean rstd gamma beta G silu out B H W Cin Cout".split()
    return [a[n] for n in names if f16 or n != "x_dtype"] + [None]


def res1x1(**k):
    a = dict(x=P, w=P, bias=P, res=P, out=P, M=16, Cin=8, Cout=8)
    a.update(k)
    return [a[n] for n in "x w bias res out M Cin Cout".split()] + [None]


def cases():
    c = []
    add = lambda entry, what, args: c.append({"id": f"{entry[6:]}-{what}", "entry": entry, "args": args})
    e = "ldmae_conv2d_nhwc_f32"
    add(e, "null", conv2d(x=NUL))
    add(e, "nonpositive", conv2d(B=0))
    add(e, "slice", conv2d(xoff=4))
    add(e, "kernel_larger", conv2d(H=2, kh=5, ph=0))
    add(e, "large_M", conv2d(kh=1, kw=1, ph=0, pw=0, **BIG))
    add(e, "large_input", conv2d(kh=1, kw=1, ph=0, pw=0, ldx=1 << 10, ldo=1 << 10, **M30))
    add(e, "large_K", conv2d(kh=1, kw=1, ph=0, pw=0, Cin=1 << 24, ldx=1 << 24))
    for e, ch in (("ldmae_conv3x3_relu_dgrad_nhwc_f32", 4), ("ldmae_conv3x3_relu_dgrad_nhwc_bf16", 8)):
        add(e, "null", dgrad(dy=NUL))
        add(e, "nonpositive", dgrad(B=0))
        add(e, "multiple", dgrad(Cy=ch + ch // 2))
        add(e, "misaligned", dgrad(dy=P20))
        add(e, "large_M", dgrad(**BIG))
        add(e, "large_dy", dgrad(Cy=1 << 10, **M30))
        add(e, "large_K", dgrad(Cy=1 << 21))
    add("ldmae_conv3x3_relu_dgrad_nhwc_bf16", "large_dx", dgrad(Cx=1 << 10, **M30))
    e = "ldmae_conv3x3_relu_nhwc_f16"
    add(e, "null", relu16(x=NUL))
    add(e, "nonpositive", relu16(B=0))
    add(e, "multiple", relu16(Cin=12))
    add(e, "misaligned", relu16(x=P20))
    add(e, "large_M", relu16(**BIG))
    add(e, "large_out", relu16(Cout=1 << 10, **M30))
    add(e, "large_in", relu16(Cin=1 << 10, **M30))
    add(e, "large_K", relu16(Cin=1 << 21))
    for e, f16, ch in (("ldmae_conv3x3_vae_nhwc_f32", False, 4), ("ldmae_conv3x3_vae_nhwc_f16", True, 8)):
        add(e, "mode", vae(f16, mode=7))
        if f16:
            add(e, "x_dtype", vae(f16, x_dtype=1))
            add(e, "f16_outside_plain", vae(f16, x_dtype=2, mode=1))
        add(e, "null", vae(f16, x=NUL))
        add(e, "nonpositive", vae(f16, B=0))
        add(e, "multiple", vae(f16, Cin=ch + ch // 2))
        add(e, "misaligned", vae(f16, x=P20))
        add(e, "norm_act_without_stats", vae(f16, mode=1, mean=NUL))
        add(e, "groups", vae(f16, mode=1, G=3))
        add(e, "gamma_misaligned", vae(f16, mode=1, gamma=P20))
        add(e, "down_1xN", vae(f16, mode=2, H=1))
        add(e, "large_M", vae(f16, **BIG))
        add(e, "large_M_up", vae(f16, mode=3, B=1 << 9, H=1 << 10, W=1 << 10))
        add(e, "large_out", vae(f16, Cout=1 << 10, **M30))
        add(e, "large_in", vae(f16, Cin=1 << 10, **M30))
        add(e, "large_K", vae(f16, Cin=1 << 21))
    for e, ch in (("ldmae_conv1x1_res_nhwc_f32", 4), ("ldmae_conv1x1_res_nhwc_f16", 8)):
        add(e, "null", res1x1(x=NUL))
        add(e, "nonpositive", res1x1(M=0))
        add(e, "multiple", res1x1(Cin=ch + ch // 2))
        add(e, "misaligned", res1x1(x=P20))
        add(e, "large_out", res1x1(M=1 << 30, Cout=1 << 10))
        add(e, "large_in", res1x1(M=1 << 30, Cin=1 << 10))
        add(e, "large_K", res1x1(Cin=1 << 24))
    add("ldmae_conv1x1_res_nhwc_f16", "large_M", res1x1(M=(1 << 31) - 1))
    return c


def main():
    import torch
    if torch.cuda.is_available():
        sys.exit("run this where no GPU is present: a call that is not refused would launch a kernel on address 16")
    lib = _lib.load()
    out = cases()
    for c in out:
        c["rc"] = getattr(lib, c["entry"])(*c["args"])
        c["message"] = _lib.last_error()
        if c["rc"] != -1:
            sys.exit(f"{c['id']}: not refused (rc {c['rc']}: {c['message']!r})")
    head = ("Recorded by tests/golden/make_golden_conv_refusals.py from the library of the commit BEFORE the convolutions moved onto "
            "csrc/conv_igemm_common.h: the old behaviour, never the code under test.")
    with open(OUT, "w") as f:
        json.dump({"_comment": head, "cases": out}, f, indent=1)
        f.write("\n")
    print(f"{len(out)} refusals from {_lib.LIB_PATH} -> {OUT}")


if __name__ == "__main__":
    main()
