"""The convolutional KL-VAE tokenizers on the GPU: csrc/conv_vae.hip per element against f64 with derived bounds, the modules against the
goldens the reference's own tokenizer/autoencoder.py produced (tests/golden/make_golden_convvae.py), the wrappers and the new command line.

Bounds (gemm_check.py has the derivation of acc_bound / sum_bound; U = 2^-24):

statistics.  The kernel makes two passes: mean = sum(x) / K, then var = sum((x - mean)^2) / K.  acc_bound(S, K) with S = sum |x| covers the
first sum for ANY summation order, so |mean - mean_ref| <= dm = acc_bound(S, K) / K + 2 U |mean| (the product with the rounded 1 / K).  For
the mean the kernel used, sum (x - mean)^2 = K (var_ref + (mean - mean_ref)^2) exactly; each term is rounded twice more (subtract, square:
3 U relative) and the sum of these non-negative terms is again within acc_bound of its own value, so
|var - var_ref| <= dv = dm^2 + (acc_bound(S2, K) + 5 U S2) / K with S2 = K (var_ref + dm^2).  rstd = 1 / sqrt(var + eps) then moves by at
most 1/2 rstd^3 dv (evaluated at the smallest admissible variance) plus 4 U rstd for the addition, the square root and the division.

fused convolution.  Two steps, as gemm_check does for nonlinear epilogues: the operand a = silu(gamma (x - mean) rstd + beta) is formed in
f64 from the mean / rstd the statistics kernel RETURNED, the convolution of a is taken in f64, and the kernel may differ by
sum_bound(ref, S, 9 Cin, f32) + sum |a| sig_err(y) |w| with S = sum |a| |w| + |bias| + |res| and sig_err gemm_check._sig_err, the documented
error of common.h's fast_sigmoid.  The four roundings of the normalisation sit inside the factor C_ACC = 2 of acc_bound (K + 4 <= 2 K).

attention.  attn_check.py covers the flash kernels' operand roundings and shifts, not this route (two f32 GEMMs around a row softmax), so
the gemm_check bound is used on both products with the softmax error propagated.  s = q k^T has |ds| <= es = acc_bound(|q| |k|^T, C).  With
t = scale s and m the row maximum, the kernel's exp(t - m) has relative error at most expm1(D), D = scale es + U (2 |t| + |m| + 3): the error
of s, the roundings of scale s and of the subtraction, and expf (1 ulp of the result, 1 ulp of argument reduction).  A common error of m
cancels in the quotient.  The row sum of these positive terms adds (2 N + 1) U, the division U, so p = softmax has relative error
rel_ij <= expm1(D_ij) + max_j expm1(D_ij) + (2 N + 2) U.  The second product then differs by at most
sum_j p_ij rel_ij |v_jc| + sum_bound(ref, sum_j p_ij (1 + rel_ij) |v_jc| + |bias_c|, Np, f32), Np the zero-padded key count.
"""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_check as gc
from gemm_check import U

pytestmark = pytest.mark.gpu
F32 = torch.float32
G, EPS = 32, 1e-6


def _ops():
    from ldmae_amd import ops
    return ops


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F32)


# ---------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("C", [32, 64, 512])
def test_groupnorm_stats(C):
    ops = _ops()
    B, H, W, cpg = 2, 9, 7, C // G
    K = H * W * cpg
    x = _randn(B, H, W, C, seed=C)
    x[:, 0, 0, 0::cpg] = 1e3                    # first pixel, first channel of every group
    x[:, -1, -1, cpg - 1::cpg] = 1e3            # last pixel, last channel of every group
    xg = x.double().view(B, H * W, G, cpg).permute(0, 2, 1, 3).reshape(B, G, K)
    mean_ref, var_ref = xg.mean(-1), xg.var(-1, unbiased=False)
    S = xg.abs().sum(-1)
    dm = gc.acc_bound(S, K) / K + 2 * U * mean_ref.abs()
    # the corner elements are what an off-by-one in the group's extent loses or counts twice: either moves the mean by 1e3 / K >> dm
    # (an interior N(0,1) element can be arbitrarily close to 0, so no bound separates every one of those)
    assert xg[..., 0].eq(1e3).all() and xg[..., -1].eq(1e3).all()
    assert bool((1e3 / K > 100 * dm).all()) and bool((1e3 / (K + 1) > 100 * dm).all())
    mean, rstd = ops.groupnorm_stats_nhwc(x.cuda(), G, EPS)
    r = gc.check(f"mean C={C}", mean.cpu(), mean_ref, dm)
    S2 = K * (var_ref + dm * dm)
    dv = dm * dm + (gc.acc_bound(S2, K) + 5 * U * S2) / K
    rstd_ref = (var_ref + EPS).rsqrt()
    drs = 0.5 * (var_ref - dv + EPS).clamp(min=EPS / 2) ** -1.5 * dv + 4 * U * rstd_ref
    r2 = gc.check(f"rstd C={C}", rstd.cpu(), rstd_ref, drs)
    print(f"stats C={C}: mean x{r:.3g} of bound, rstd x{r2:.3g} of bound")


# ---------------------------------------------------------------------------------------------------- fused convolution
def _act64(x, mean, rstd, gamma, beta, silu=True):
    """(a, y) in f64, NHWC, from the statistics as returned (f32 values)."""
    B, H, W, C = x.shape
    cpg = C // mean.shape[1]
    mu = mean.double().repeat_interleave(cpg, 1)[:, None, None, :]
    rs = rstd.double().repeat_interleave(cpg, 1)[:, None, None, :]
    y = gamma.double() * (x.double() - mu) * rs + beta.double()
    return (y * torch.sigmoid(y) if silu else y), y


def _conv64(a, w, stride=1, pad=(1, 1, 1, 1)):
    """f64 convolution of NHWC a with w [Cout, 3, 3, Cin] (the kernels' layout); pad = (left, right, top, bottom).  Returns NHWC."""
    an = F.pad(a.permute(0, 3, 1, 2), pad)
    return F.conv2d(an, w.double().permute(0, 3, 1, 2), stride=stride).permute(0, 2, 3, 1)


def _conv_inputs(B, H, W, Cin, Cout, seed):
    x = _randn(B, H, W, Cin, seed=seed)
    w = _randn(Cout, 3, 3, Cin, seed=seed + 1) / math.sqrt(9 * Cin)
    return x, w, 0.3 * _randn(Cout, seed=seed + 2), 1 + 0.1 * _randn(Cin, seed=seed + 3), 0.1 * _randn(Cin, seed=seed + 4)


def _check_norm_act(name, x, w, bias, res, gamma, beta, silu=True):
    ops = _ops()
    xc, wc = x.cuda(), w.cuda()
    stats = ops.groupnorm_stats_nhwc(xc, G, EPS)
    a, y = _act64(x, stats[0].cpu(), stats[1].cpu(), gamma, beta, silu)
    ref, S = _conv64(a, w), _conv64(a.abs(), w.abs())
    sig = _conv64(a.abs() * gc._sig_err(y), w.abs())
    for t in (bias, res):
        if t is not None:
            ref, S = ref + t.double(), S + t.double().abs()
    bound = gc.sum_bound(ref, S, 9 * x.shape[3], F32) + sig
    cu = lambda t: None if t is None else t.cuda()
    fused = ops.conv3x3_vae_nhwc(xc, wc, cu(bias), mode=ops.VAE_NORM_ACT, res=cu(res), stats=stats, gamma=gamma.cuda(), beta=beta.cuda(),
                                 silu=silu)
    r1 = gc.check(name + " fused", fused.cpu(), ref, bound)
    act = ops.groupnorm_apply_nhwc(xc, stats, gamma.cuda(), beta.cuda(), silu=silu)
    two = ops.conv3x3_vae_nhwc(act, wc, cu(bias), mode=ops.VAE_PLAIN, res=cu(res))
    r2 = gc.check(name + " two-pass", two.cpu(), ref, bound)
    print(f"{name}: fused x{r1:.3g}, two-pass x{r2:.3g} of bound")
    return fused.cpu(), ref


# the smallest shapes that reach every edge of the 128 x 64 x 16 tile: one ragged M tile spanning both images with ragged N (K = 288);
# several M tiles and N over one tile; 1, 2 and 16 channels per group
CONV_SHAPES = [(2, 9, 7, 32, 32), (2, 18, 18, 64, 96), (1, 5, 3, 512, 128)]


# every case with SiLU, as the tokenizers run it, plus one without per instantiation conv_vae_kernel<NORM, false> that only such a call
# reaches (1 and 16 channels per group: NORM 2 and 1), against the same reference and bound (its sigmoid term then only widens it)
NORM_ACT_CASES = [(*s, rb, True) for rb in (False, True) for s in CONV_SHAPES] + [(*CONV_SHAPES[0], False, False), (*CONV_SHAPES[2], False, False)]


@pytest.mark.parametrize("B,H,W,Cin,Cout,with_res_bias,silu", NORM_ACT_CASES,
                         ids=["-".join(map(str, c[:6])) + ("" if c[6] else "-nosilu") for c in NORM_ACT_CASES])
def test_conv_norm_act(B, H, W, Cin, Cout, with_res_bias, silu):
    x, w, bias, gamma, beta = _conv_inputs(B, H, W, Cin, Cout, seed=Cin + Cout)
    res = _randn(B, H, W, Cout, seed=5) if with_res_bias else None
    _check_norm_act(f"norm-act {B}x{H}x{W} {Cin}->{Cout} res/bias={with_res_bias} silu={silu}", x, w, bias if with_res_bias else None, res, gamma, beta,
                    silu)


def test_conv_norm_act_border_taps_are_zero():
    """Constant input: norm(x) = beta everywhere, silu(beta) != 0, so padding BEFORE the activation (or normalising a padded 0) shows in every
    border pixel.  With unit weights an interior pixel sums 9 taps and a corner pixel 4."""
    B, H, W, C = 1, 5, 6, 32
    x = torch.full((B, H, W, C), 0.75)
    w = torch.ones(C, 3, 3, C) / (9 * C)
    gamma, beta = torch.ones(C), torch.ones(C)
    got, ref = _check_norm_act("border", x, w, None, None, gamma, beta)
    silu1 = 1 / (1 + math.exp(-1.0))
    assert float(ref[0, 2, 2, 0]) == pytest.approx(silu1, rel=1e-3) and float(ref[0, 0, 0, 0] / ref[0, 2, 2, 0]) == pytest.approx(4 / 9, rel=1e-12)
    assert float(got[0, 0, 0, 0] / got[0, 2, 2, 0]) == pytest.approx(4 / 9, rel=1e-5)
    assert float(got[0, 0, 3, 0] / got[0, 2, 2, 0]) == pytest.approx(6 / 9, rel=1e-5)


@pytest.mark.parametrize("B,H,W", [(1, 8, 8), (2, 7, 9)])
def test_conv_down(B, H, W):
    ops = _ops()
    x, w, bias, _, _ = _conv_inputs(B, H, W, 32, 32, seed=H)
    ref = _conv64(x.double(), w, stride=2, pad=(0, 1, 0, 1)) + bias.double()
    S = _conv64(x.double().abs(), w.abs(), stride=2, pad=(0, 1, 0, 1)) + bias.double().abs()
    assert tuple(ref.shape[1:3]) == ((H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1) == {8: (4, 4), 7: (3, 4)}[H]
    got = ops.conv3x3_vae_nhwc(x.cuda(), w.cuda(), bias.cuda(), mode=ops.VAE_DOWN)
    assert got.shape == ref.shape
    gc.check_sum(f"down {H}x{W}", got.cpu(), ref, S, 9 * 32)


def test_conv_up():
    ops = _ops()
    B, H, W, Cin, Cout = 2, 5, 3, 32, 64
    x, w, bias, _, _ = _conv_inputs(B, H, W, Cin, Cout, seed=11)
    up = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest").permute(0, 2, 3, 1)
    assert tuple(up.shape) == (B, 10, 6, Cin)
    ref = _conv64(up, w) + bias.double()                                                                   # interpolate + conv(padding=1)
    ref_pad = F.conv2d(F.pad(up.permute(0, 3, 1, 2), (1, 1, 1, 1)), w.double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1) + bias.double()   # pad + conv
    S = _conv64(up.abs(), w.abs()) + bias.double().abs()
    got = ops.conv3x3_vae_nhwc(x.cuda(), w.cuda(), bias.cuda(), mode=ops.VAE_UP)
    assert got.shape == ref.shape
    gc.check_sum("up interpolate+conv", got.cpu(), ref, S, 9 * Cin)
    gc.check_sum("up pad+conv", got.cpu(), ref_pad, S, 9 * Cin)


def test_conv1x1_residual():
    ops = _ops()
    x, w, bias, res = _randn(3, 7, 5, 64, seed=1), _randn(96, 64, seed=2) / 8, _randn(96, seed=3), _randn(3, 7, 5, 96, seed=4)
    ref, S = gc.nt_ref(x.view(-1, 64), w, bias, res.view(-1, 96))
    got = ops.conv1x1_res_nhwc(x.cuda(), w.cuda(), bias.cuda(), res.cuda())
    gc.check_sum("conv1x1_res", got.cpu().view(-1, 96), ref, S, 64)


def test_entry_points_validate():
    ops = _ops()
    x = torch.zeros(1, 4, 4, 48, device="cuda")
    with pytest.raises(RuntimeError, match="not divisible"):
        ops.groupnorm_stats_nhwc(x, 32)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.conv3x3_vae_nhwc(torch.zeros(1, 4, 4, 6, device="cuda"), torch.zeros(8, 3, 3, 6, device="cuda"))
    with pytest.raises(RuntimeError, match="at least 2 x 2"):
        ops.conv3x3_vae_nhwc(torch.zeros(1, 1, 4, 8, device="cuda"), torch.zeros(8, 3, 3, 8, device="cuda"), mode=ops.VAE_DOWN)


# ---------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("B,N,C", [(2, 16, 32), (2, 81, 64), (1, 1024, 512)])
def test_attention_wide(B, N, C):
    ops = _ops()
    q, k, v = _randn(B, N, C, seed=1), _randn(B, N, C, seed=2), _randn(B, N, C, seed=3)
    bias = _randn(C, seed=4)
    scale = float(C) ** -0.5
    Np = -(-N // ops.ATTN_WIDE_KPAD) * ops.ATTN_WIDE_KPAD
    qk = torch.cat([q, k], -1).cuda()                       # the module's layout: q and k are halves of one buffer
    vt = torch.zeros(B, C, Np)
    vt[:, :, :N] = v.transpose(1, 2)
    got = ops.attention_wide(qk[:, :, :C], qk[:, :, C:], vt.cuda(), scale, bias=bias.cuda()).cpu()
    Q, K_, V = q.double(), k.double(), v.double()
    s = Q @ K_.transpose(1, 2)
    es = gc.acc_bound(Q.abs() @ K_.abs().transpose(1, 2), C)
    t = s * scale
    m = t.max(-1, keepdim=True).values
    D = torch.expm1(scale * es + U * (2 * t.abs() + m.abs() + 3))
    rel = D + D.max(-1, keepdim=True).values + (2 * N + 2) * U
    P = torch.softmax(t, -1)
    ref = P @ V + bias.double()
    S2 = (P * (1 + rel)) @ V.abs() + bias.double().abs()
    bound = (P * rel) @ V.abs() + gc.sum_bound(ref, S2, Np, F32)
    r = gc.check(f"attention N={N} C={C}", got, ref, bound)
    print(f"attention N={N} C={C}: x{r:.3g} of bound")


# ---------------------------------------------------------------------------------------------------- goldens
@pytest.fixture(scope="module")
def fx(golden):
    return golden("convvae")


def _golden(fx, key, got):
    ref = torch.from_numpy(fx[key])
    e_ref = float(fx["e_ref_" + key])
    tol = 8 * e_ref
    assert tol <= 1e-4, f"{key}: 8 e_ref = {tol:.3e} is above the standing 1e-4"
    assert got.shape == ref.shape
    err = float((got.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"{key}: normalised max-abs error {err:.3e} (8 e_ref = {tol:.3e})")
    assert math.isfinite(err) and err <= tol, f"{key}: {err:.3e} > 8 e_ref = {tol:.3e}"


def _case_a_halves():
    from convvae_weights import CASE_A, weights_for
    from ldmae_amd.tokenizer.autoencoder import Decoder, Encoder
    enc, dec = Encoder(double_z=True, **CASE_A), Decoder(**CASE_A)
    enc.load_state_dict(weights_for(enc, 1))
    dec.load_state_dict(weights_for(dec, 2))
    return enc, dec


def _case_b(use_variational=True, model_type="vavae"):
    from convvae_weights import CASE_B, weights_for
    from ldmae_amd.tokenizer.autoencoder import AutoencoderKL
    m = AutoencoderKL(use_variational=use_variational, model_type=model_type, **CASE_B)
    m.load_state_dict(weights_for(m, 3))
    return m.cuda().eval()


@pytest.mark.parametrize("fused", [False, True])
def test_golden_case_a(fx, fused, monkeypatch):
    from ldmae_amd.tokenizer import autoencoder
    monkeypatch.setattr(autoencoder, "FUSED_NORM_ACT", fused)
    enc, dec = _case_a_halves()
    _golden(fx, "A_moments", enc.cuda().eval()(torch.from_numpy(fx["A_x"]).cuda()))
    _golden(fx, "A_dec", dec.cuda().eval()(torch.from_numpy(fx["A_z"]).cuda()))


def test_golden_case_b(fx):
    m = _case_b()
    _golden(fx, "B_moments", m.encode(torch.from_numpy(fx["B_x"])).parameters)
    _golden(fx, "B_dec", m.decode(torch.from_numpy(fx["B_z"])))
    with pytest.raises(NotImplementedError, match="training"):
        m(torch.from_numpy(fx["B_x"]))


def test_golden_case_b_not_variational(fx):
    _golden(fx, "B_moments_nv", _case_b(False).encode(torch.from_numpy(fx["B_x"])).parameters)


def test_golden_case_b_marvae_decoder(fx):
    """model_type='marvae': no attention in the decoder's levels (only in its middle block), through the MAR_VAE wrapper's methods."""
    from ldmae_amd.tokenizer.marvae import MAR_VAE
    m = _case_b(model_type="marvae")
    assert not any(len(up.attn) for up in m.decoder.up) and any(len(d.attn) for d in m.encoder.down)
    z = torch.from_numpy(fx["B_z"])
    dec = m.decode(z)
    _golden(fx, "B_dec_mar", dec)
    vae = object.__new__(MAR_VAE)                # the wrapper's methods around the scaled-down model (its constructor builds the 256-pixel one)
    vae.model, vae.img_size = m, 64
    assert np.array_equal(vae.decode_to_images(z), torch.clamp(127.5 * dec + 128.0, 0, 255).permute(0, 2, 3, 1).to("cpu", dtype=torch.uint8).numpy())
    with pytest.raises(FileNotFoundError, match="not found"):
        MAR_VAE()                                # the reference's empty checkpoint literal: an error, not a download


def _diffusers_case_a(old_attention=False):
    from convvae_weights import CASE_A_DIFFUSERS
    from ldmae_amd.tokenizer import sdvae
    enc, dec = _case_a_halves()
    vae = sdvae.Diffusers_AutoencoderKL(**CASE_A_DIFFUSERS)
    sd = {}
    for half, mod in (("encoder", enc), ("decoder", dec)):
        for k, v in mod.state_dict().items():
            if k in sdvae.LINEAR_AS_CONV:
                v = v.reshape(v.shape[0], v.shape[1])              # diffusers keeps the attention projections as Linear [C, C]
            sd[sdvae.ldm_to_diffusers_key(f"{half}.{k}", 4, old_attention)] = v
    msg = vae.load_state_dict(sd)
    assert not msg.missing_keys and not msg.unexpected_keys
    return vae.cuda().eval()


@pytest.mark.parametrize("old_attention", [False, True])
def test_golden_through_diffusers_names(fx, old_attention):
    vae = _diffusers_case_a(old_attention)
    _golden(fx, "A_moments", vae.encode(torch.from_numpy(fx["A_x"]), return_dict=False)[0].parameters)
    _golden(fx, "A_dec", vae.decode(torch.from_numpy(fx["A_z"])).sample)


# ---------------------------------------------------------------------------------------------------- wrappers
def test_sdvae_image_methods(fx):
    vae = _diffusers_case_a()
    x, z = torch.from_numpy(fx["A_x"]), torch.from_numpy(fx["A_z"])
    lat = vae.encode_images(x)
    assert lat.shape == (2, 16, 4, 4) and torch.equal(lat, vae.encode(x).latent_dist.mode())
    imgs = vae.decode_to_images(z)
    want = torch.clamp(127.5 * vae.decode(z).sample + 128.0, 0, 255).permute(0, 2, 3, 1).to("cpu", dtype=torch.uint8).numpy()
    assert imgs.dtype == np.uint8 and imgs.shape == (2, 32, 32, 3) and np.array_equal(imgs, want)


def test_vavae_image_methods(fx):
    from ldmae_amd.tokenizer.vavae import VA_VAE
    vae = object.__new__(VA_VAE)                 # the wrapper's methods around the scaled-down model (its constructor builds the 256-pixel one)
    vae.model, vae.img_size = _case_b(), 64
    x, z = torch.from_numpy(fx["B_x"]), torch.from_numpy(fx["B_z"])
    torch.manual_seed(5)
    lat = vae.encode_images(x)
    post = vae.model.encode(x)
    torch.manual_seed(5)
    assert torch.equal(lat, post.mean + post.std * torch.randn(post.mean.shape, device="cuda"))
    imgs = vae.decode_to_images(z)
    want = torch.clamp(127.5 * vae.model.decode(z) + 128.0, 0, 255).permute(0, 2, 3, 1).to("cpu", dtype=torch.uint8).numpy()
    assert imgs.shape == (1, 64, 64, 3) and np.array_equal(imgs, want)
    with pytest.raises(FileNotFoundError, match="not found"):
        VA_VAE({"model": {"params": {"embed_dim": 32}}}, ckpt_path="/nonexistent/vavae.pt")


# ---------------------------------------------------------------------------------------------------- the drivers' refusals that need a device
@pytest.mark.parametrize("name", ["ae_f8d16", "dae_f8d16", "vae_f8d16", "sdv3_f8d16"])
def test_extract_features_still_refuses_sdvae_model_types(name, tmp_path, monkeypatch):
    """extract_features.main refuses after it has chosen its device, so this one cannot run in test_conv_vae_cpu.py.  inference.do_sample's
    refusal is pinned by tests/test_gpu_drivers.py::test_do_sample_end_to_end_writes_pngs."""
    import argparse
    from ldmae_amd import extract_features
    monkeypatch.delenv("RANK", raising=False)
    args = argparse.Namespace(data_split="train", output_dir=str(tmp_path / "out"), output_path="", image_size=256, batch_size=2, seed=42,
                              num_workers=0, config="", precision="fp32", synthetic=2)
    cfg = {"vae": {"model_name": name, "weight_path": "x.pt"}, "data": {"image_size": 256, "data_path": str(tmp_path), "origin_path": str(tmp_path)}}
    with pytest.raises(NotImplementedError, match="only the vmae tokenizer"):
        extract_features.main(args, cfg)
    assert not (tmp_path / "out").exists()


# ---------------------------------------------------------------------------------------------------- the command line
def test_cli_end_to_end(tmp_path, capsys, monkeypatch):
    """--synthetic 8 at 64 x 64 with case-A-sized weights; the LPIPS and Inception weight files are random ones written to tmp_path, the rule
    of the tokenizer-evaluation test."""
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
                    "--fid_weights", str(tmp_path / "inception.pth")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    js = json.loads(lines[0])
    assert js["metric"] == "tokenizer_eval" and js["model_type"] == "sdvae" and js["images"] == 8
    for k in ("rfid", "psnr", "lpips", "ssim"):
        assert np.isfinite(js[k]) and js[k] == res[k]
    assert len(os.listdir(tmp_path / "o" / "sdvae_0" / "decoded_images")) == 8
