"""The MXFP8 sampling mode without a GPU: the quantiser rule of the contract (include/ldmae_hip.h) on planted blocks,
the new C-ABI symbols, the refusals of LightningDiT.set_gemm_precision, the sampling driver's gemm_precision plumbing and the keying of
ops.cached_weight_mx8."""
import ctypes
import math
import os
import re

import pytest
import torch

import mx8_check as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ldmae_mx8_quantize", "ldmae_rmsnorm_modulate_fwd_mx8", "ldmae_gemm_nt_mx8_ok", "ldmae_gemm_nt_mx8", "ldmae_gemm_nt_qkv_rope_mx8_ok",
               "ldmae_gemm_nt_qkv_rope_mx8", "ldmae_mx8_launch_counts")


def _rule(amax: float) -> int:
    """The exponent rule written out on one number with math.frexp (independent of the helper's tensor code)."""
    if amax == 0:
        return -127
    m, ex = math.frexp(amax)                    # amax = m * 2^ex, m in [0.5, 1)
    e = (ex - 1) - (8 if 2 * m <= 1.75 else 7)
    return max(-127, min(127, e))


def test_quantiser_rule_on_planted_blocks():
    """Planted: all zero; amax exactly 448 * 2^k and one f32 ulp above; mantissa exactly 1.75 and just above; values on e4m3 subnormals; amax
    2^-130 (e clamps to -127); the largest bf16.  For every block: the E8M0 byte is the rule's e + 127 and never 0xFF; amax * 2^-e <= 448 and
    e is the smallest such exponent (unless clamped); every element errs by at most HALF the e4m3 spacing at its own scaled magnitude,
    2^(e-4) * max(2^binade, 2^-6) -- binade of |x * 2^-e|, 2^-6 the smallest normal binade, whose spacing the subnormals share.

    The issue's line "dequantised magnitude never exceeds amax" cannot hold under round-to-nearest-even (the largest bf16, 255 * 2^120, scales
    to 255 and rounds to 256).  What the non-saturating rule does guarantee, and what is asserted instead: no dequantised magnitude exceeds the
    block's dequantised amax element, that element is within half a spacing of amax, and it never exceeds 448 * 2^e (nothing saturates)."""
    P = mc.planted_blocks()
    amax = P.double().abs().amax(1)
    q, s = mc.quantize(P)
    e = s.to(torch.int64).flatten() - 127
    assert [int(v) for v in e] == [_rule(float(a)) for a in amax]
    assert int(s.max()) < 0xFF and int(e[0]) == -127
    k_of = {float(448.0 * 2.0 ** k): k for k in (-20, 0, 9)}
    for a, ee in zip(amax.tolist(), e.tolist()):
        if a in k_of:                                           # 448 * 2^k sits exactly on the top of the e4m3 range: e = k
            assert ee == k_of[a]
        if a > 0 and ee > -127:
            assert a * 2.0 ** -ee <= 448.0 < a * 2.0 ** -(ee - 1)       # the smallest exponent that does not saturate
    assert int(e[-2]) == -127 and float(amax[-2]) == 2.0 ** -130         # clamped
    assert float(amax[-1]) == float(torch.finfo(torch.bfloat16).max) and int(e[-1]) == 120
    d = mc.dequantize(q, s)
    scaled = torch.ldexp(P.double(), (-e).unsqueeze(1).expand_as(P))
    _, ex = torch.frexp(scaled.abs())
    binade = torch.where(scaled == 0, torch.full_like(ex, -6), ex - 1).clamp(min=-6)
    half_spacing = torch.ldexp(torch.ones_like(scaled), binade - 4 + e.unsqueeze(1))
    assert bool(((P.double() - d).abs() <= half_spacing).all())
    dmax = d.abs().amax(1)
    i = P.double().abs().argmax(1)
    assert bool((d.abs()[torch.arange(len(P)), i] == dmax).all())                     # rounding is monotone: the amax element stays the largest
    assert bool((dmax <= 448.0 * torch.ldexp(torch.ones_like(dmax), e)).all())      # nothing saturates
    # the subnormal row: multiples of 2^-9 survive exactly, 2^-10 ties to even (0), 3 * 2^-10 rounds to 2 * 2^-9, -2^-11 flushes to (minus) zero
    row = [float(a) for a in amax].index(256.0)
    got = dict(zip(P[row].tolist(), d[row].tolist()))
    assert got[2.0 ** -9] == 2.0 ** -9 and got[-5 * 2.0 ** -9] == -5 * 2.0 ** -9 and got[2.0 ** -10] == 0.0 and got[3 * 2.0 ** -10] == 2 * 2.0 ** -9
    assert got[-2.0 ** -11] == 0.0 and int(mc.canon(q)[row][P[row] == -2.0 ** -11][0]) == 0
    # bf16 sources go through the same rule
    qb, sb = mc.quantize(P.bfloat16())
    assert torch.equal(sb.flatten().to(torch.int64) - 127, mc.scale_exponents(P.bfloat16().float()).flatten())


def test_one_gemm_error_of_the_contract():
    """The figure quoted in the header / DESIGN for one GEMM with Gaussian operands at K = 768: MXFP8 about 3.7e-2, bf16 about 2.4e-3."""
    g = torch.Generator().manual_seed(0)
    A, W = torch.randn(512, 768, generator=g), torch.randn(384, 768, generator=g)
    ref = A.double() @ W.double().T
    e8 = mc.rel_l2(mc.fake_quant(A) @ mc.fake_quant(W).T, ref)
    e16 = mc.rel_l2(A.bfloat16().double() @ W.bfloat16().double().T, ref)
    assert 3.3e-2 < e8 < 4.1e-2 and 2.0e-3 < e16 < 2.8e-3, (e8, e16)


def test_new_symbols_in_header_signatures_and_library():
    from ldmae_amd import _lib
    header = open(os.path.join(ROOT, "include", "ldmae_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, name + " is not declared in include/ldmae_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
        assert hasattr(handle, name), name
    assert "The mode's effect on FID has not been measured.  It needs a trained checkpoint." in header
    lib = _lib.load()
    assert lib.ldmae_gemm_nt_mx8_ok(256, 256, 128, 128, 128) == 1 and lib.ldmae_gemm_nt_mx8_ok(264, 320, 256, 256, 256) == 1
    assert lib.ldmae_gemm_nt_mx8_ok(256, 256, 64, 64, 64) == 0 and lib.ldmae_gemm_nt_mx8_ok(260, 256, 128, 128, 128) == 0
    assert lib.ldmae_gemm_nt_qkv_rope_mx8_ok(4, 128, 2, 64, 128, 128, 128) == 1 and lib.ldmae_gemm_nt_qkv_rope_mx8_ok(8, 256, 16, 72, 1152, 1152, 1152) == 0
    assert set(_lib.mx8_launch_counts()) == {"quantize", "norm_quantize", "gemm"}
    assert len(_lib.COUNT_NAMES) == 9                               # the nine family slots stay


def _dit(**over):
    from ldmae_amd.models.lightningdit import LightningDiT
    kw = dict(input_size=8, patch_size=1, in_channels=16, hidden_size=128, depth=2, num_heads=2, mlp_ratio=3.0, num_classes=10,
              use_qknorm=True, use_swiglu=True, use_rope=True, use_rmsnorm=True)
    kw.update(over)
    return LightningDiT(**kw)


def test_set_gemm_precision_default_and_refusals():
    m = _dit()
    assert m.gemm_precision is None and all(b.gemm_precision is None for b in m.blocks)
    assert m.set_gemm_precision("mxfp8") is m and m.gemm_precision == "mxfp8" and all(b.gemm_precision == "mxfp8" for b in m.blocks)
    m.set_gemm_precision(None)
    assert m.gemm_precision is None and all(b.gemm_precision is None for b in m.blocks)
    with pytest.raises(ValueError, match="fp4"):
        m.set_gemm_precision("fp4")
    for over, msg in ((dict(use_rmsnorm=False, use_qknorm=False), "use_rmsnorm=False"),
                      (dict(use_swiglu=False), "use_swiglu=False"),
                      (dict(use_rmsnorm=False, use_qknorm=True), "nn.LayerNorm QK-norm"),
                      (dict(hidden_size=192, num_heads=3), "hidden size 192 is not a multiple of 128"),
                      (dict(mlp_ratio=4.0), "SwiGLU width 341 is not a multiple of 128")):
        t = _dit(**over)
        with pytest.raises(NotImplementedError, match=re.escape(msg)):
            t.set_gemm_precision("mxfp8")
        assert t.gemm_precision is None
    # the padded widths of L and 1p6B are refused by name (their block geometry, shallow)
    from ldmae_amd.models.lightningdit import LightningDiT
    for hidden, heads, width in ((1024, 16, 2730), (1792, 28, 4778)):
        t = LightningDiT(input_size=4, patch_size=2, in_channels=16, hidden_size=hidden, depth=1, num_heads=heads, num_classes=10, use_qknorm=True,
                         use_swiglu=True, use_rope=True, use_rmsnorm=True)
        with pytest.raises(NotImplementedError, match=f"SwiGLU width {width}.*2730 / 4778"):
            t.set_gemm_precision("mxfp8")
    # forward-only bf16: a grad-enabled forward, an f32 activation type and input_grad_only refuse before any kernel is reached
    m.set_gemm_precision("mxfp8")
    x, t_, y = torch.zeros(2, 16, 8, 8), torch.zeros(2), torch.zeros(2, dtype=torch.long)
    with pytest.raises(RuntimeError, match="forward-only bf16"):
        m(x, t_, y)
    with torch.no_grad(), pytest.raises(RuntimeError, match="forward-only bf16"):
        m(x, t_, y)                                               # no autocast: f32 activations
    with pytest.raises(RuntimeError, match="forward-only bf16"):
        with m.input_grad_only():
            pass


def test_driver_flag_and_yaml_parsing():
    import ldmae_amd.inference as inf
    ap = inf.build_parser()
    assert ap.parse_args([]).gemm_precision is None
    assert ap.parse_args(["--gemm_precision", "mxfp8"]).gemm_precision == "mxfp8"
    with pytest.raises(SystemExit):
        ap.parse_args(["--gemm_precision", "fp4"])
    assert inf.resolve_gemm_precision({"sample": {}}) is None                                   # key absent: behaviour as before
    assert inf.resolve_gemm_precision({"sample": {"gemm_precision": "mxfp8"}}) == "mxfp8"
    assert inf.resolve_gemm_precision({"sample": {}}, "mxfp8") == "mxfp8"
    assert inf.resolve_gemm_precision({"sample": {"gemm_precision": "mxfp8"}}, "none") is None   # the flag overrides the YAML
    assert inf.resolve_gemm_precision({"sample": {"gemm_precision": None}}, "mxfp8") == "mxfp8"
    with pytest.raises(SystemExit, match="gemm_precision"):
        inf.resolve_gemm_precision({"sample": {"gemm_precision": "int8"}})
    import inspect
    assert inspect.signature(inf.do_sample).parameters["gemm_precision"].default is None
    assert "MXFP8" in inf.MX8_NOTICE and "FID has not been measured" in inf.MX8_NOTICE
    # the shipped YAMLs do not set the key
    import yaml
    for ds in ("imagenet", "celeba_hq"):
        cfg = yaml.safe_load(open(os.path.join(ROOT, f"ldmae_amd/configs/{ds}/lightningdit_b_vmae_f8d16_cfg.yaml")))
        assert inf.resolve_gemm_precision(cfg) is None


def test_cached_weight_mx8_keying(monkeypatch):
    """One quantiser call per (weight object, storage pointer, version counter, WEIGHT_EPOCH), as cached_weight_copy; the kernel call stubbed."""
    from ldmae_amd import ops
    calls = []

    def stub(w):
        calls.append(w)
        return mc.quantize(w.detach())
    monkeypatch.setattr(ops, "mx8_quantize", stub)
    monkeypatch.setattr(ops, "_WCACHE", {})
    w = torch.nn.Parameter(torch.randn(8, 128))
    a = ops.cached_weight_mx8(w)
    assert ops.cached_weight_mx8(w) is a and len(calls) == 1
    assert torch.equal(a[0], mc.quantize(w.detach())[0]) and a[1].shape == (8, 4)
    with torch.no_grad():
        w.mul_(2.0)                                              # version counter
    b = ops.cached_weight_mx8(w)
    assert b is not a and len(calls) == 2 and ops.cached_weight_mx8(w) is b
    ops.invalidate_weight_cache()                                # WEIGHT_EPOCH
    assert ops.cached_weight_mx8(w) is not b and len(calls) == 3
    w.data = torch.randn(8, 128)                                 # storage pointer
    ops.cached_weight_mx8(w)
    assert len(calls) == 4
    # the bf16 copy cache of the same weight is a different entry
    assert (id(w), "mx8") in ops._WCACHE and (id(w), torch.bfloat16) not in ops._WCACHE
    w2 = torch.nn.Parameter(torch.randn(8, 128))
    ops.cached_weight_mx8(w2)
    assert len(calls) == 5 and len(ops._WCACHE) == 2
