"""The TF32-class (fp16-MFMA) path of the convolutional KL-VAE tokenizers on the GPU: ldmae_conv3x3_vae_nhwc_f16, ldmae_conv1x1_res_nhwc_f16
and ldmae_groupnorm_apply_nhwc_f16out per element against f64 with derived bounds, the modules under set_precision("tf32") against the f64
goldens within the reference's own error under this arithmetic (tests/golden/make_golden_convvae_tf32.py), and the command line.

Contract under test: both operands of every product are rounded ONCE to fp16 (nearest even, saturating at +-65504), products (exact in f32)
are accumulated in f32, bias and residual are added in f32, the output is f32.  U = 2^-24, u = 2^-11 (fp16's unit roundoff), eta = 2^-25
(half the spacing of fp16's subnormals).

Bound 1, against f64 on HOST-ROUNDED operands (rf = round_f16): |got - conv(rf(a), rf(w)) - bias - res| <= gemm_check.sum_bound(ref, S,
9 Cin, f32) with S = conv(|rf(a)|, |rf(w)|) + |bias| + |res|: f32 accumulation only (gemm_check's derivation; the products are exact).
Under norm-act the kernel rounds ITS f32 activation a_dev, the host rounds the f64 one, a.  With t = gamma (x - mean) rstd and y = t + beta,
|a_dev - a| <= d = 1.1 (3 U |t| + U |y|) + |a| (sig_err(y) + 2 U): two roundings of t and the fma's (SiLU's slope is below 1.1), then
gemm_check._sig_err, the documented error of fast_sigmoid, and the product y * sigmoid.  Rounding is monotonic, so rf(a_dev) lies between
rf(a - d) and rf(a + d): the operand may differ from rf(a) by da = max |rf(a +- d) - rf(a)|, which is 0 except next to a rounding boundary,
where it is one fp16 spacing.  The bound grows by conv(da, |rf(w)|) -- for almost every output element by nothing.

Bound 2, against the UNROUNDED f64 convolution: an operand v becomes rf(v) with |rf(v) - v| <= e(v) = u |v| + eta (eta: the subnormal range,
which the small weights reach), so the host-rounded reference of bound 1 is within conv(|a|, e(w)) + conv(e(a), |w|) + conv(e(a), e(w)) of
the unrounded one -- the (2 u + u^2) sum |a| |w| of normal-range operands plus the subnormal terms -- and the kernel within bound 1 of that
reference (triangle inequality; bound 1 carries the accumulation and, under norm-act, the activation's error).
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_check as gc
from gemm_check import U
from make_golden_convvae_tf32 import round_f16

pytestmark = pytest.mark.gpu
F32 = torch.float32
G, EPS = 32, 1e-6
U16, ETA = 2.0 ** -11, 2.0 ** -25


def _ops():
    from ldmae_amd import ops
    return ops


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F32)


def _act64(x, mean, rstd, gamma, beta, silu=True):
    """(a, y, t) in f64, NHWC, from the statistics as returned (f32 values): t = gamma (x - mean) rstd, y = t + beta, a = silu(y) (or y)."""
    cpg = x.shape[3] // mean.shape[1]
    mu = mean.double().repeat_interleave(cpg, 1)[:, None, None, :]
    rs = rstd.double().repeat_interleave(cpg, 1)[:, None, None, :]
    t = gamma.double() * (x.double() - mu) * rs
    y = t + beta.double()
    return (y * torch.sigmoid(y) if silu else y), y, t


def _conv64(a, w, stride=1, pad=(1, 1, 1, 1)):
    """f64 convolution of NHWC a with w [Cout, 3, 3, Cin] (the kernels' layout); pad = (left, right, top, bottom).  Returns NHWC."""
    an = F.pad(a.permute(0, 3, 1, 2), pad)
    return F.conv2d(an, w.double().permute(0, 3, 1, 2), stride=stride).permute(0, 2, 3, 1)


def _conv_inputs(B, H, W, Cin, Cout, seed):
    x = _randn(B, H, W, Cin, seed=seed)
    w = _randn(Cout, 3, 3, Cin, seed=seed + 1) / math.sqrt(9 * Cin)
    return x, w, 0.3 * _randn(Cout, seed=seed + 2), 1 + 0.1 * _randn(Cin, seed=seed + 3), 0.1 * _randn(Cin, seed=seed + 4)


def _e(v):
    return U16 * v.abs() + ETA


def _check_both(name, got, a, w, K, adds=(), d=None, stride=1, pad=(1, 1, 1, 1)):
    """Bounds 1 and 2 of the module docstring for got = conv(a, w) + sum(adds); a, w f64 (unrounded), d the norm-act operand error or None."""
    conv = lambda p, q: _conv64(p, q, stride=stride, pad=pad)
    A, Wd = a.double(), w.double()
    ar, wr = round_f16(A), round_f16(Wd)
    ref, S, ref_u = conv(ar, wr), conv(ar.abs(), wr.abs()), conv(A, Wd)
    for t in adds:
        if t is not None:
            ref, S, ref_u = ref + t.double(), S + t.double().abs(), ref_u + t.double()
    b1 = gc.sum_bound(ref, S, K, F32)
    if d is not None:
        b1 = b1 + conv(torch.maximum((round_f16(A + d) - ar).abs(), (round_f16(A - d) - ar).abs()), wr.abs())
    assert got.shape == ref.shape
    r1 = gc.check(name + " [host-rounded operands]", got, ref, b1)
    b2 = conv(A.abs(), _e(Wd)) + conv(_e(A), Wd.abs()) + conv(_e(A), _e(Wd)) + b1
    r2 = gc.check(name + " [unrounded f64]", got, ref_u, b2)
    print(f"{name}: x{r1:.3g} of the accumulation bound, x{r2:.3g} of the fp16 rounding bound")
    return ref


def _pack16(w):
    return _ops().cast(w.cuda().contiguous(), torch.float16)


def _norm_act(name, x, w, bias, res, gamma, beta, form, silu=True):
    ops = _ops()
    xc, w16 = x.cuda(), _pack16(w)
    stats = ops.groupnorm_stats_nhwc(xc, G, EPS)
    a, y, t = _act64(x, stats[0].cpu(), stats[1].cpu(), gamma, beta, silu)
    d = 1.1 * (3 * U * t.abs() + U * y.abs()) + a.abs() * (gc._sig_err(y) + 2 * U)
    cu = lambda v: None if v is None else v.cuda()
    if form == "fused":
        got = ops.conv3x3_vae_nhwc(xc, w16, cu(bias), mode=ops.VAE_NORM_ACT, res=cu(res), stats=stats, gamma=gamma.cuda(), beta=beta.cuda(),
                                   silu=silu, precision="tf32")
    else:
        act = ops.groupnorm_apply_nhwc(xc, stats, gamma.cuda(), beta.cuda(), silu=silu, out_dtype=torch.float16)
        assert act.dtype == torch.float16
        got = ops.conv3x3_vae_nhwc(act, w16, cu(bias), mode=ops.VAE_PLAIN, res=cu(res), precision="tf32")
    ref = _check_both(f"{name} {form}", got.cpu(), a, w, 9 * x.shape[3], (bias, res), d=d)
    return got.cpu(), ref


# channels per group 1, 2, 16 and 4; one ragged M tile spanning both images; several M tiles with N below one 128-wide tile; Cout = 3
NORM_SHAPES = [(2, 9, 7, 32, 32), (2, 18, 18, 64, 96), (1, 5, 3, 512, 128), (1, 6, 5, 128, 3)]


# every case with SiLU, as the tokenizers run it, plus one fused case without per instantiation conv_vae_f16_kernel<NORM, false, false> that
# only such a call reaches (1, 4 and 16 channels per group: NORM 3, 2 and 1), against the same references and bounds (their sigmoid term then
# only widens them)
NORM_ACT_CASES = [(*s, rb, f, True) for f in ("fused", "two-pass") for rb in (False, True) for s in NORM_SHAPES] + \
                 [(*NORM_SHAPES[i], False, "fused", False) for i in (0, 3, 2)]


@pytest.mark.parametrize("B,H,W,Cin,Cout,with_res_bias,form,silu", NORM_ACT_CASES,
                         ids=["-".join(map(str, c[:7])) + ("" if c[7] else "-nosilu") for c in NORM_ACT_CASES])
def test_conv_norm_act(B, H, W, Cin, Cout, with_res_bias, form, silu):
    x, w, bias, gamma, beta = _conv_inputs(B, H, W, Cin, Cout, seed=Cin + Cout)
    res = _randn(B, H, W, Cout, seed=5) if with_res_bias else None
    _norm_act(f"norm-act {B}x{H}x{W} {Cin}->{Cout} res/bias={with_res_bias} silu={silu}", x, w, bias if with_res_bias else None, res, gamma, beta, form,
              silu)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 7, 5, 8, 40), (1, 4, 4, 16, 512), (2, 5, 6, 40, 72)])
def test_conv_plain(B, H, W, Cin, Cout):
    ops = _ops()
    x, w, bias, _, _ = _conv_inputs(B, H, W, Cin, Cout, seed=Cin)
    res = _randn(B, H, W, Cout, seed=9)
    got = ops.conv3x3_vae_nhwc(x.cuda(), _pack16(w), bias.cuda(), res=res.cuda(), precision="tf32")
    _check_both(f"plain {B}x{H}x{W} {Cin}->{Cout}", got.cpu(), x, w, 9 * Cin, (bias, res))


@pytest.mark.parametrize("B,H,W", [(1, 8, 8), (2, 7, 9)])
def test_conv_down(B, H, W):
    ops = _ops()
    x, w, bias, _, _ = _conv_inputs(B, H, W, 32, 32, seed=H)
    got = ops.conv3x3_vae_nhwc(x.cuda(), _pack16(w), bias.cuda(), mode=ops.VAE_DOWN, precision="tf32")
    assert tuple(got.shape[1:3]) == {8: (4, 4), 7: (3, 4)}[H]
    _check_both(f"down {H}x{W}", got.cpu(), x, w, 9 * 32, (bias,), stride=2, pad=(0, 1, 0, 1))


def test_conv_up():
    ops = _ops()
    B, H, W, Cin, Cout = 2, 5, 3, 32, 40
    x, w, bias, _, _ = _conv_inputs(B, H, W, Cin, Cout, seed=11)
    up = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest").permute(0, 2, 3, 1)
    got = ops.conv3x3_vae_nhwc(x.cuda(), _pack16(w), bias.cuda(), mode=ops.VAE_UP, precision="tf32")
    assert tuple(got.shape) == (B, 10, 6, Cout)
    _check_both("up", got.cpu(), up, w, 9 * Cin, (bias,))


def test_conv1x1_residual():
    ops = _ops()
    M = 130
    x, w, bias, res = _randn(2, 5, 13, 64, seed=1), _randn(96, 64, seed=2) / 8, _randn(96, seed=3), _randn(2, 5, 13, 96, seed=4)
    got = ops.conv1x1_res_nhwc(x.cuda(), _ops().cast(w.cuda(), torch.float16), bias.cuda(), res.cuda(), precision="tf32").cpu().view(M, 96)
    xr, wr = round_f16(x.double()).view(M, 64), round_f16(w.double())
    ref, S = gc.nt_ref(xr, wr, bias, res.view(M, 96))
    r1 = gc.check_sum("conv1x1_res [host-rounded operands]", got, ref, S, 64)
    X, Wd = x.double().view(M, 64), w.double()
    ref_u, _ = gc.nt_ref(X, Wd, bias, res.view(M, 96))
    b2 = X.abs() @ _e(Wd).T + _e(X) @ Wd.abs().T + _e(X) @ _e(Wd).T + gc.sum_bound(ref, S, 64, F32)
    r2 = gc.check("conv1x1_res [unrounded f64]", got, ref_u, b2)
    print(f"conv1x1_res M={M}: x{r1:.3g} of the accumulation bound, x{r2:.3g} of the fp16 rounding bound")


@pytest.mark.parametrize("form", ["fused", "two-pass"])
def test_conv_norm_act_border_taps_are_zero(form):
    """Constant input: norm(x) = beta everywhere, silu(beta) != 0, so padding BEFORE the activation (or normalising a padded 0) shows in every
    border pixel.  With unit weights an interior pixel sums 9 taps and a corner pixel 4."""
    B, H, W, C = 1, 5, 6, 32
    x = torch.full((B, H, W, C), 0.75)
    w = torch.ones(C, 3, 3, C) / 256                         # exact in fp16
    gamma, beta = torch.ones(C), torch.ones(C)
    got, ref = _norm_act("border", x, w, None, None, gamma, beta, form)
    assert float(ref[0, 0, 0, 0] / ref[0, 2, 2, 0]) == pytest.approx(4 / 9, rel=1e-12) and float(ref[0, 2, 2, 0]) > 0.5
    assert float(got[0, 0, 0, 0] / got[0, 2, 2, 0]) == pytest.approx(4 / 9, rel=1e-5)
    assert float(got[0, 0, 3, 0] / got[0, 2, 2, 0]) == pytest.approx(6 / 9, rel=1e-5)


def test_saturation():
    """One input element of 1e5 is read as 65504 (fp16's largest), not as infinity; the host reference saturates the same way."""
    ops = _ops()
    x, w, bias, _, _ = _conv_inputs(1, 6, 5, 16, 24, seed=3)
    x[0, 2, 3, 5] = 1e5
    assert float(round_f16(x.double())[0, 2, 3, 5]) == 65504.0
    got = ops.conv3x3_vae_nhwc(x.cuda(), _pack16(w), bias.cuda(), precision="tf32").cpu()
    assert bool(torch.isfinite(got).all())
    xr, wr = round_f16(x.double()), round_f16(w.double())
    ref, S = _conv64(xr, wr) + bias.double(), _conv64(xr.abs(), wr.abs()) + bias.double().abs()
    r = gc.check_sum("saturation", got, ref, S, 9 * 16)
    assert float(ref.abs().max()) > 100                      # the saturated element dominates its neighbourhood
    print(f"saturation: x{r:.3g} of bound, max |ref| {float(ref.abs().max()):.4g}")


def test_groupnorm_apply_f16_is_the_rounded_f32_kernel():
    """fp16 output against the host rounding of ldmae_groupnorm_apply_nhwc_f32's output: equal, or the other neighbour where the f32 value
    sits within one f32 ulp of the rounding tie (the two kernels may contract their arithmetic differently)."""
    ops = _ops()
    for C in (64, 128, 40):                                  # cpg 2 and 4 on the 8-wide path; 40 channels in 8 groups of 5
        g = 32 if C != 40 else 8
        x = _randn(2, 18, 18, C, seed=C)
        gamma, beta = (1 + 0.1 * _randn(C, seed=1)).cuda(), (0.1 * _randn(C, seed=2)).cuda()
        stats = ops.groupnorm_stats_nhwc(x.cuda(), g, EPS)
        a32 = ops.groupnorm_apply_nhwc(x.cuda(), stats, gamma, beta, silu=True).cpu()
        a16 = ops.groupnorm_apply_nhwc(x.cuda(), stats, gamma, beta, silu=True, out_dtype=torch.float16).cpu()
        want = a32.half()
        diff = a16 != want
        share = float(diff.double().mean())
        print(f"groupnorm_apply fp16 C={C}: {int(diff.sum())} of {diff.numel()} elements differ from the host rounding (share {share:.2e})")
        if diff.any():
            v, lo, hi = a32[diff].double(), a16[diff].double(), want[diff].double()
            tie = 0.5 * (lo + hi)
            assert bool(((lo - hi).abs() <= gc.ulp(v, torch.float16)).all()), "differs by more than one fp16 spacing"
            assert bool(((v - tie).abs() <= gc.ulp(v, F32)).all()), "differs away from a rounding tie"
        assert share < 1e-3


def test_determinism():
    ops = _ops()
    x, w, bias, gamma, beta = _conv_inputs(2, 18, 18, 64, 96, seed=7)
    res = _randn(2, 18, 18, 96, seed=8).cuda()
    xc, w16 = x.cuda(), _pack16(w)
    stats = ops.groupnorm_stats_nhwc(xc, G, EPS)
    run = lambda: ops.conv3x3_vae_nhwc(xc, w16, bias.cuda(), mode=ops.VAE_NORM_ACT, res=res, stats=stats, gamma=gamma.cuda(), beta=beta.cuda(),
                                       precision="tf32")
    assert torch.equal(run(), run())
    plain = lambda: ops.conv3x3_vae_nhwc(xc, w16, bias.cuda(), precision="tf32")
    assert torch.equal(plain(), plain())


def test_entry_points_refuse():
    from ldmae_amd import _lib
    lib = _lib.load()
    dev = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device="cuda")
    x, x16, w, out = dev(1, 4, 4, 16), dev(1, 4, 4, 16, dt=torch.float16), dev(8, 3, 3, 16, dt=torch.float16), dev(1, 4, 4, 8)
    st, vec = dev(1, 4), dev(16)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    N = None

    def refused(rc, word):
        assert rc == -1, rc                                   # LDMAE_ERR_INVALID
        assert word in _lib.last_error(), _lib.last_error()

    f = lib.ldmae_conv3x3_vae_nhwc_f16
    x12, w12 = dev(1, 4, 4, 12), dev(8, 3, 3, 12, dt=torch.float16)
    refused(f(0, _lib.F32, P(x12), P(w12), N, N, N, N, N, N, 0, 0, P(out), 1, 4, 4, 12, 8, N), "multiple of 8")
    refused(f(1, _lib.F16, P(x16), P(w), N, N, P(st), P(st), P(vec), P(vec), 4, 1, P(out), 1, 4, 4, 16, 8, N), "plain mode only")
    refused(f(0, _lib.F32, P(x), N, N, N, N, N, N, N, 0, 0, P(out), 1, 4, 4, 16, 8, N), "null pointer")
    refused(f(0, _lib.F32, ctypes.c_void_p(x.data_ptr() + 4), P(w), N, N, N, N, N, N, 0, 0, P(out), 1, 4, 3, 16, 8, N), "16-B aligned")
    refused(f(0, _lib.BF16, P(x), P(w), N, N, N, N, N, N, 0, 0, P(out), 1, 4, 4, 16, 8, N), "x_dtype")
    refused(lib.ldmae_conv1x1_res_nhwc_f16(P(x12), P(w12), N, N, P(out), 16, 12, 8, N), "multiple of 8")
    refused(lib.ldmae_conv1x1_res_nhwc_f16(P(x), N, N, N, P(out), 16, 16, 8, N), "null pointer")
    refused(lib.ldmae_groupnorm_apply_nhwc_f16out(P(x), P(st), P(st), P(vec), P(vec), N, 1, 16, 16, 4, 1, N), "null pointer")
    refused(lib.ldmae_groupnorm_apply_nhwc_f16out(P(x), P(st), P(st), P(vec), P(vec), P(x16), 1, 16, 16, 3, 1, N), "not divisible")
    ops = _ops()
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.conv3x3_vae_nhwc(x12, w12, precision="tf32")
    with pytest.raises(ValueError, match="precision"):
        ops.conv3x3_vae_nhwc(x, w, precision="bf16")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- goldens
@pytest.fixture(scope="module")
def fx(golden):
    return golden("convvae"), golden("convvae_tf32")


def _golden(fx, key, got):
    ref = torch.from_numpy(fx[0][key])
    e_tf32 = float(fx[1]["e_tf32_" + key])
    tol = 4 * e_tf32
    assert got.shape == ref.shape
    err = float((got.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"{key}: normalised max-abs error {err:.3e} = x{err / tol:.3g} of 4 e_tf32 = {tol:.3e} (e_tf32 {e_tf32:.3e})")
    assert math.isfinite(err) and err <= tol, f"{key}: {err:.3e} > 4 e_tf32 = {tol:.3e}"
    assert err > 8 * float(fx[0]["e_ref_" + key]), f"{key}: as accurate as the f32 path -- the fp16 kernels did not run"


def _case_a_halves():
    from convvae_weights import CASE_A, weights_for
    from ldmae_amd.tokenizer.autoencoder import Decoder, Encoder
    enc, dec = Encoder(double_z=True, **CASE_A), Decoder(**CASE_A)
    enc.load_state_dict(weights_for(enc, 1))
    dec.load_state_dict(weights_for(dec, 2))
    return enc.cuda().eval(), dec.cuda().eval()


def _case_b():
    from convvae_weights import CASE_B, weights_for
    from ldmae_amd.tokenizer.autoencoder import AutoencoderKL
    m = AutoencoderKL(use_variational=True, model_type="vavae", **CASE_B)
    m.load_state_dict(weights_for(m, 3))
    return m.cuda().eval()


def _diffusers_case_a():
    from convvae_weights import CASE_A_DIFFUSERS
    from ldmae_amd.tokenizer import sdvae
    enc, dec = _case_a_halves()
    vae = sdvae.Diffusers_AutoencoderKL(**CASE_A_DIFFUSERS)
    sd = {}
    for half, mod in (("encoder", enc), ("decoder", dec)):
        for k, v in mod.state_dict().items():
            if k in sdvae.LINEAR_AS_CONV:
                v = v.reshape(v.shape[0], v.shape[1])
            sd[sdvae.ldm_to_diffusers_key(f"{half}.{k}", 4)] = v
    vae.load_state_dict(sd)
    return vae.cuda().eval()


@pytest.mark.parametrize("fused", [False, True])
def test_golden_case_a(fx, fused, monkeypatch):
    from ldmae_amd.tokenizer import autoencoder
    monkeypatch.setattr(autoencoder, "TF32_FUSED_NORM_ACT", fused)
    x, z = torch.from_numpy(fx[0]["A_x"]).cuda(), torch.from_numpy(fx[0]["A_z"]).cuda()
    enc, dec = _case_a_halves()
    assert enc.set_precision("tf32") is enc and dec.set_precision("tf32").precision == "tf32"
    _golden(fx, "A_moments", enc(x))
    _golden(fx, "A_dec", dec(z))
    # back to f32: bitwise what a module that never left f32 computes (the mode switch and both weight-pack caches)
    fe, fd = _case_a_halves()
    assert torch.equal(enc.set_precision("f32")(x), fe(x)) and torch.equal(dec.set_precision("f32")(z), fd(z))


@pytest.mark.parametrize("fused", [False, True])
def test_golden_case_b(fx, fused, monkeypatch):
    from ldmae_amd.tokenizer import autoencoder
    monkeypatch.setattr(autoencoder, "TF32_FUSED_NORM_ACT", fused)
    x, z = torch.from_numpy(fx[0]["B_x"]), torch.from_numpy(fx[0]["B_z"])
    m = _case_b().set_precision("tf32")
    _golden(fx, "B_moments", m.encode(x).parameters)
    _golden(fx, "B_dec", m.decode(z))
    m.set_precision("f32")
    f = _case_b()
    assert torch.equal(m.encode(x).parameters, f.encode(x).parameters) and torch.equal(m.decode(z), f.decode(z))


@pytest.mark.parametrize("fused", [False, True])
def test_golden_through_diffusers_names(fx, fused, monkeypatch):
    from ldmae_amd.tokenizer import autoencoder
    monkeypatch.setattr(autoencoder, "TF32_FUSED_NORM_ACT", fused)
    x, z = torch.from_numpy(fx[0]["A_x"]), torch.from_numpy(fx[0]["A_z"])
    vae = _diffusers_case_a().set_precision("tf32")
    _golden(fx, "A_moments", vae.encode(x, return_dict=False)[0].parameters)
    _golden(fx, "A_dec", vae.decode(z).sample)
    vae.set_precision("f32")
    f = _diffusers_case_a()
    assert torch.equal(vae.decode(z).sample, f.decode(z).sample)
    assert torch.equal(vae.encode(x, return_dict=False)[0].parameters, f.encode(x, return_dict=False)[0].parameters)


# ---------------------------------------------------------------------------------------------------- the command line
def test_cli_end_to_end_tf32(tmp_path, capsys, monkeypatch):
    """--synthetic 8 at 64 x 64 --precision tf32 with case-A-sized weights; the LPIPS and Inception weight files are random ones written to
    tmp_path, as in the f32 command-line test."""
    from ldmae_amd import evaluate_conv_tokenizer as ect
    from ldmae_amd import fid
    from ldmae_amd.models.lpips import CONVS, random_state_dict
    from ldmae_amd.tokenizer.sdvae import Diffusers_AutoencoderKL
    from convvae_weights import CASE_A_DIFFUSERS, convvae_weights
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.setenv("LDMAE_FID_WEIGHTS", str(tmp_path / "inception.pth"))
    sd = random_state_dict(7)
    vgg = {}
    for i, s, _, _ in CONVS:
        vgg[f"features.{i}.weight"] = sd[f"net.slice{s}.{i}.weight"]
        vgg[f"features.{i}.bias"] = sd[f"net.slice{s}.{i}.bias"]
    torch.save(vgg, tmp_path / "vgg16-397923af.pth")
    torch.save({k: v for k, v in sd.items() if k.startswith("lin")}, tmp_path / "vgg.pth")
    torch.save(fid.random_state_dict(0), tmp_path / "inception.pth")
    vae = Diffusers_AutoencoderKL(**{**CASE_A_DIFFUSERS, "img_size": 64})
    torch.save({"model": convvae_weights({k: tuple(v.shape) for k, v in vae.state_dict().items()}, 4)}, tmp_path / "sdvae.pt")
    res = ect.main(["--family", "sdvae", "--weights", str(tmp_path / "sdvae.pt"), "--synthetic", "8", "--image_size", "64",
                    "--block_out_channels", "32,64,128,128", "--output_path", str(tmp_path / "o"), "--batch_size", "4", "--num_workers", "0",
                    "--lpips_vgg", str(tmp_path / "vgg16-397923af.pth"), "--lpips_lin", str(tmp_path / "vgg.pth"),
                    "--fid_weights", str(tmp_path / "inception.pth"), "--precision", "tf32"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    js = json.loads(lines[0])
    assert js["metric"] == "tokenizer_eval" and js["model_type"] == "sdvae" and js["images"] == 8 and js["precision"] == "tf32"
    for k in ("rfid", "psnr", "lpips", "ssim"):
        assert np.isfinite(js[k]) and js[k] == res[k]
    assert len(os.listdir(tmp_path / "o" / "sdvae_0" / "decoded_images")) == 8
