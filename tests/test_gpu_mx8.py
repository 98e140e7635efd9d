"""The MXFP8 sampling mode on the GPU (include/ldmae_hip.h: the contract): the operand and scale lane maps of the
block-scaled MFMA on exact integers, the quantiser kernels bit for bit against the f64 helper, every epilogue element by element with the
GEMM suite's derived bound, and the tiny DiT against its f64 fake-quant model."""
import copy
import os

import numpy as np
import pytest
import torch

import gemm_check as gc
import mx8_check as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F32 = torch.bfloat16, torch.float32


def dev(t):
    return t.cuda().contiguous()


# ----------------------------------------------------------------------------- 1. exact integers
def _int_operand(rows, K, g, lo, hi):
    """(q bytes, scale bytes, f64 value): integers in [lo, hi] (|v| <= 8: exact in e4m3) times per-(row, 32-block) powers of two 2^0 .. 2^2 that
    differ from block to block and from row to row.  Built directly as (q, scales), not through the quantiser."""
    v = torch.randint(lo, hi + 1, (rows, K), generator=g)
    ex = (torch.arange(rows).unsqueeze(1) * 2 + torch.arange(K // 32).unsqueeze(0) + torch.randint(0, 3, (rows, K // 32), generator=g)) % 3
    q = v.float().to(torch.float8_e4m3fn).view(torch.uint8)
    s = (ex + 127).to(torch.uint8)
    return q, s, mc.dequantize(q, s)


@pytest.mark.parametrize("M,N,K", [(256, 256, 128),       # one K-step
                                   (256, 256, 768),       # six K-steps: the five-slot ring wraps
                                   (264, 320, 256),       # clamped edge pieces in M and N
                                   (10240, 2048, 128)])   # 320 tiles on 256 persistent workgroups: tile boundaries of the seamless ring
def test_exact_integer_products_pin_the_lane_maps(M, N, K):
    """Every partial sum is an integer below 2^24 (|a|, |w| <= 8 * 4, K <= 768: at most 768 * 1024), so the f32 result through EPI_BIAS must
    EQUAL the integer product: a wrong A / B lane map, a scale byte from the wrong (row, block) or lane, or a stale ring slot cannot."""
    from ldmae_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    aq, asc, a = _int_operand(M, K, g, -8, 7)              # asymmetric ranges: a sign or operand swap shows
    wq, wsc, w = _int_operand(N, K, g, -5, 8)
    bias = torch.randint(-9, 10, (N,), generator=g).float()
    ref = a @ w.T + bias.double()
    assert float(ref.abs().max()) < 2 ** 24
    out = ops.gemm_nt_mx8(dev(aq), dev(asc), dev(wq), dev(wsc), dev(bias), out_dtype=F32)
    torch.cuda.synchronize()
    got = out.cpu().double()
    bad = (got != ref).nonzero()
    assert len(bad) == 0, f"{len(bad)} of {ref.numel()} wrong; first at {bad[0].tolist()}: got {float(got[tuple(bad[0])])}, want {float(ref[tuple(bad[0])])}"


# ----------------------------------------------------------------------------- 2. quantiser kernel
def _quant_source():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(40, 256, generator=g) * torch.logspace(-3, 3, 40).unsqueeze(1)
    P = mc.planted_blocks()
    x[:len(P), 64:96] = P
    x[20:20 + len(P), 224:256] = -P
    return x


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("strided", [False, True])
def test_mx8_quantize_bitwise(dtype, strided):
    from ldmae_amd import ops
    x = _quant_source().to(dtype)
    if strided:
        buf = torch.full((40, 384), 7e4, dtype=dtype).cuda()      # ld > K; what lies between the rows must not leak into amax
        buf[:, :256] = x.cuda()
        src = buf[:, :256]
        assert src.stride(0) == 384
    else:
        src = dev(x)
    q, s = ops.mx8_quantize(src)
    torch.cuda.synchronize()
    qr, sr = mc.quantize(x)
    assert torch.equal(s.cpu(), sr)
    assert torch.equal(mc.canon(q.cpu()), mc.canon(qr))


# ----------------------------------------------------------------------------- 3. norm + quantise
@pytest.mark.parametrize("D,M,rpb", [(256, 24, 8), (768, 24, 8),       # the guarded form of the norm kernel
                                     (768, 32, 16), (1152, 32, 16)])    # its whole-workgroup form (B/1's width), and XL's width
@pytest.mark.parametrize("with_shift", [True, False])
def test_rmsnorm_modulate_fwd_mx8_bitwise_against_the_pair(D, M, rpb, with_shift):
    from ldmae_amd import ops
    g = torch.Generator().manual_seed(D)
    x = dev(torch.randn(M, D, generator=g) * 3)
    w = dev(1 + 0.2 * torch.randn(D, generator=g))
    mod = dev(torch.randn(M // rpb, 6 * D, generator=g) * 0.5)
    shift, scale = (mod[:, :D] if with_shift else None), mod[:, D:2 * D]
    out, rstd = ops.rmsnorm_modulate_fwd(x, w, shift, scale, rpb, BF16)
    q0, s0 = ops.mx8_quantize(out)
    q, s, r = ops.rmsnorm_modulate_fwd_mx8(x, w, shift, scale, rpb)
    torch.cuda.synchronize()
    assert torch.equal(r, rstd), f"rstd: {int((r != rstd).sum())} of {M} rows differ"
    assert torch.equal(s, s0), f"scales: {int((s != s0).sum())} differ"
    assert torch.equal(q, q0), f"elements: {int((q != q0).sum())} differ"
    qr, sr = mc.quantize(out.cpu())                              # and the pair itself is the contract's quantiser of the bf16 values
    assert torch.equal(s.cpu(), sr) and torch.equal(mc.canon(q.cpu()), mc.canon(qr))


# ----------------------------------------------------------------------------- 4. epilogues, element by element
def _operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(M, K, generator=g) * torch.logspace(-1, 1, K // 32).repeat_interleave(32)).bfloat16()
    w = torch.randn(N, K, generator=g) * 0.2
    (aq, asc), (wq, wsc) = mc.quantize(a), mc.quantize(w)
    bias = torch.randn(N, generator=g)
    return g, (dev(aq), dev(asc), dev(wq), dev(wsc)), mc.dequantize(aq, asc), mc.dequantize(wq, wsc), bias


@pytest.mark.parametrize("K", [128, 768])
@pytest.mark.parametrize("out_dtype", [F32, BF16])
def test_epilogue_bias(K, out_dtype):
    from ldmae_amd import ops
    M, N = 512, 384
    _, ops_, a, w, bias = _operands(M, N, K, K)
    out = ops.gemm_nt_mx8(*ops_, dev(bias), out_dtype=out_dtype)
    torch.cuda.synchronize()
    ref, S = gc.nt_ref(a, w, bias)
    r = mc.check_sum(f"mx8 bias K={K} {out_dtype}", out.cpu(), ref, S, K, out_dtype)
    print(f"mx8 bias K={K} {out_dtype}: worst |err| / bound = {r:.3f}")


def test_epilogue_gate_res():
    from ldmae_amd import ops
    M, N, K, rpb = 512, 256, 256, 128
    g, ops_, a, w, bias = _operands(M, N, K, 5)
    xin = torch.randn(M, N, generator=g)
    mod = dev(torch.randn(M // rpb, 3 * N, generator=g))
    gate = mod[:, N:2 * N]                                        # a strided view
    xout, y = ops.gemm_nt_gate_res_mx8(*ops_, dev(bias), dev(xin), gate, rpb, save_y=True)
    torch.cuda.synchronize()
    ref, S = gc.nt_ref(a, w, bias)
    r1 = mc.check_sum("mx8 gate_res y", y.cpu(), ref, S, K, BF16)
    r2 = mc.check_gate_res("mx8 gate_res xout", xout.cpu(), xin, gate.cpu().repeat_interleave(rpb, 0), ref, S, K, BF16)
    print(f"mx8 gate_res: worst ratios y {r1:.3f} xout {r2:.3f}")
    xout2, none = ops.gemm_nt_gate_res_mx8(*ops_, dev(bias), dev(xin), gate, rpb)        # forward-only form: y is not stored
    assert none is None and torch.equal(xout2, xout)


def test_epilogue_swiglu():
    from ldmae_amd import ops
    M, N, K = 512, 512, 256                                      # Hs = 256
    _, ops_, a, w, bias = _operands(M, N, K, 6)
    h12, hid = ops.gemm_nt_swiglu_mx8(*ops_, dev(bias), save_h12=True)
    torch.cuda.synchronize()
    ref, S = gc.nt_ref(a, w, bias)
    r1 = mc.check_sum("mx8 swiglu h12", h12.cpu(), ref, S, K, BF16)      # the w12 row interleave lands every column where the plain layout has it
    r2 = gc.check_swiglu("mx8 swiglu hid", hid.cpu(), h12.cpu())         # the existing two-step form: the activation of the STORED halves
    print(f"mx8 swiglu: worst ratios h12 {r1:.3f} hid {r2:.3f}")
    none, hid2 = ops.gemm_nt_swiglu_mx8(*ops_, dev(bias))
    assert none is None and torch.equal(hid2, hid)


@pytest.mark.parametrize("qknorm", [True, False])
def test_epilogue_qkv_rope(qknorm):
    from ldmae_amd import ops
    B, N, H, hd, K = 4, 128, 2, 64, 128
    g, ops_, a, w, bias = _operands(B * N, 3 * H * hd, K, 7)
    wq = dev(1 + 0.3 * torch.randn(hd, generator=g)) if qknorm else None
    wk = dev(1 + 0.3 * torch.randn(hd, generator=g)) if qknorm else None
    ang = torch.rand(N, hd, generator=g) * 6.28
    cos, sin = dev(torch.cos(ang)), dev(torch.sin(ang))
    assert ops.gemm_nt_qkv_rope_mx8_ok(ops_[0], ops_[2], B, N, H, hd)
    qkv, q2, k2 = ops.gemm_nt_qkv_rope_mx8(*ops_, dev(bias), wq, wk, cos, sin, B, N, H, hd, 1e-6, store_raw_qk=True)
    torch.cuda.synchronize()
    ref, S = gc.nt_ref(a, w, bias)
    r = mc.check_sum("mx8 qkv", qkv.cpu(), ref, S, K, BF16)
    print(f"mx8 qkv_rope: worst ratio of the packed qkv {r:.3f}")
    # the existing reference of the epilogue: ldmae_qknorm_rope_fwd on the stored qkv, bit for bit
    q_ref, k_ref, _ = ops.qknorm_rope_fwd(qkv, wq, wk, cos, sin, B, N, H, hd, 1e-6, copy_v=False)
    assert torch.equal(q2, q_ref) and torch.equal(k2, k_ref)
    qkv_f, q2_f, k2_f = ops.gemm_nt_qkv_rope_mx8(*ops_, dev(bias), wq, wk, cos, sin, B, N, H, hd, 1e-6, store_raw_qk=False)
    assert torch.equal(q2_f, q2) and torch.equal(k2_f, k2) and torch.equal(qkv_f[:, 2 * H * hd:], qkv[:, 2 * H * hd:])
    assert not ops.gemm_nt_qkv_rope_mx8_ok(ops_[0], ops_[2], B * 2, N // 2, H, hd)      # 64 tokens per sample: off the fused epilogue's grid


# ----------------------------------------------------------------------------- 5 - 7. the tiny model
def _tiny():
    from ldmae_amd.models.lightningdit import LightningDiT
    torch.manual_seed(4)
    # hidden 128, 2 heads of 64, depth 2; mlp_ratio 3 makes the SwiGLU width 256 (ratio 4 gives 341, which the mode refuses by name)
    m = LightningDiT(input_size=16, patch_size=1, in_channels=16, hidden_size=128, depth=2, num_heads=2, mlp_ratio=3.0, num_classes=10,
                     use_qknorm=True, use_swiglu=True, use_rope=True, use_rmsnorm=True)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "adaLN_modulation" in n or n.startswith("final_layer.linear"):
                p.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 else 0.02))
            elif n.endswith("norm1.weight") or n.endswith("norm2.weight") or "q_norm" in n or "k_norm" in n:
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith(".bias") and "blocks" in n:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    x = torch.randn(2, 16, 16, 16, generator=g)
    t = torch.tensor([0.37, 0.37])
    y = torch.tensor([3, 10])
    return m.eval(), x, t, y


@pytest.fixture(scope="module")
def tiny_runs():
    """forward_with_cfg of the tiny model under no_grad, three times on the GPU (f32 kernels, bf16, bf16 + mxfp8) with the launch counts of the
    last two, and the f64 exact / fake-quant pair of the helper.  Computed once, shared, left unchanged."""
    from ldmae_amd import ops
    from oracle import dit as odit
    m, x, t, y = _tiny()
    sd = {k: v.double() for k, v in m.state_dict().items()}
    sd.setdefault("feat_rope.freqs_cos", m.feat_rope.freqs_cos.double())
    sd.setdefault("feat_rope.freqs_sin", m.feat_rope.freqs_sin.double())
    cfg = odit.DiTConfig(input_size=16, patch_size=1, in_channels=16, hidden_size=128, depth=2, num_heads=2, mlp_ratio=3.0, num_classes=10)
    exact = mc.dit_forward_with_cfg_f64(sd, x, t, y, cfg, 4.0, quant=False)
    emul = mc.dit_forward_with_cfg_f64(sd, x, t, y, cfg, 4.0, quant=True)
    mg = copy.deepcopy(m).cuda()
    xg, tg, yg = x.cuda(), t.cuda(), y.cuda()
    r = {"exact": exact, "emul": emul, "model": mg, "args": (xg, tg, yg)}
    with torch.no_grad():
        r["f32"] = mg.forward_with_cfg(xg, tg, yg, 4.0).float().cpu()
        with torch.autocast("cuda", dtype=BF16):
            ops.launch_counts(reset=True)
            r["bf16"] = mg.forward_with_cfg(xg, tg, yg, 4.0).float().cpu()
            r["counts_bf16"] = ops.launch_counts(reset=True)
            mg.set_gemm_precision("mxfp8")
            r["mx8"] = mg.forward_with_cfg(xg, tg, yg, 4.0).float().cpu()          # quantises the eight block weights once (ops.cached_weight_mx8)
            ops.launch_counts(reset=True)
            ops.mx8_launch_counts(reset=True)
            r["mx8_again"] = mg.forward_with_cfg(xg, tg, yg, 4.0).float().cpu()    # counted with the weight cache warm: what a sampler's steps launch
            r["counts_mx8"] = ops.launch_counts(reset=True)
            r["mx8_counts"] = ops.mx8_launch_counts(reset=True)
            mg.set_gemm_precision(None)
            r["bf16_again"] = mg.forward_with_cfg(xg, tg, yg, 4.0).float().cpu()
    torch.cuda.synchronize()
    return r


def test_tiny_model_is_no_noisier_than_its_contract(tiny_runs):
    """E_gpu <= 1.25 * E_emul + E_bf16 (relative L2): E_gpu = mxfp8 against the f32 kernels on the GPU, E_emul = the helper's f64 fake-quant model
    against its exact model, E_bf16 = bf16 against f32 on the GPU.  The only term beyond the contract is quantiser decisions flipped by the bf16
    rounding of the quantiser's input; 1.25 is margin over the 1.002 that term measures on the CPU."""
    r = tiny_runs
    depth = 2
    assert torch.isfinite(r["mx8"]).all() and not torch.equal(r["mx8"], r["bf16"])
    assert r["mx8_counts"] == {"gemm": 4 * depth, "norm_quantize": 2 * depth, "quantize": 2 * depth}
    # no bf16 NT GEMM inside the blocks: the four per block that the bf16 run launches are gone, everything outside the blocks is unchanged
    assert r["counts_bf16"]["nt_bf16"] - r["counts_mx8"]["nt_bf16"] == 4 * depth
    assert {k: v for k, v in r["counts_mx8"].items() if k != "nt_bf16"} == {k: v for k, v in r["counts_bf16"].items() if k != "nt_bf16"}
    assert mc.rel_l2(r["f32"], r["exact"]) < 1e-4                # the f64 model is the model the GPU runs
    e_gpu, e_emul, e_bf16 = mc.rel_l2(r["mx8"], r["f32"]), mc.rel_l2(r["emul"], r["exact"]), mc.rel_l2(r["bf16"], r["f32"])
    print(f"tiny DiT: E_gpu {e_gpu:.4e}  E_emul {e_emul:.4e}  E_bf16 {e_bf16:.4e}  E_gpu / E_emul {e_gpu / e_emul:.4f}  "
          f"bound {1.25 * e_emul + e_bf16:.4e}")
    assert e_emul > 1e-4                                         # the quantiser is at work in the emulation
    assert e_gpu <= 1.25 * e_emul + e_bf16, (e_gpu, e_emul, e_bf16)


def test_tiny_model_reproducible_and_default_restored(tiny_runs):
    r = tiny_runs
    assert torch.equal(r["mx8"], r["mx8_again"])                 # fixed K order, no split-K, no atomics
    assert torch.equal(r["bf16_again"], r["bf16"])               # set_gemm_precision(None): the plain bf16 path, bit for bit


def test_grad_enabled_forward_raises(tiny_runs):
    m = tiny_runs["model"]
    x, t, y = tiny_runs["args"]
    m.set_gemm_precision("mxfp8")
    try:
        with torch.autocast("cuda", dtype=BF16):
            with pytest.raises(RuntimeError, match="forward-only bf16"):
                m(x, t, y)
            with pytest.raises(RuntimeError, match="forward-only bf16"):
                with m.input_grad_only():
                    m(x, t, y)
        with torch.no_grad(), pytest.raises(RuntimeError, match="forward-only bf16"):
            m(x, t, y)                                           # f32 activations
    finally:
        m.set_gemm_precision(None)


# ----------------------------------------------------------------------------- 8. the sampling driver
def test_do_sample_mxfp8_writes_pngs(tmp_path, monkeypatch, capsys):
    """do_sample(..., gemm_precision="mxfp8") at the driver test's tiny configuration (64-pixel images, 8 x 8 latents, depth 2, two Euler steps,
    CFG 4) -- with hidden 256 / 4 heads / mlp_ratio 3 in place of 192 / 3 / 4, which the mode refuses by name: PNGs are written, differ from
    the bf16 folder's, and the notice is printed.  No pixel threshold here: accuracy is gated by the epilogue and tiny-model tests."""
    import yaml
    from PIL import Image
    import ldmae_amd.inference as inf
    import ldmae_amd.train_accum as t
    from ldmae_amd.models import lightningdit as L
    from ldmae_amd.tokenizer import models_mae
    monkeypatch.setitem(L.LightningDiT_models, "LightningDiT-B/1",
                        lambda **kw: L.LightningDiT(depth=2, hidden_size=256, patch_size=1, num_heads=4, mlp_ratio=3.0, **kw))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "ldmae_amd/configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml")))
    cfg["data"].update(image_size=64, num_workers=0, data_path=str(tmp_path / "feat"), latent_multiplier=1.0)
    cfg["train"].update(global_batch_size=8, output_dir=str(tmp_path), exp_name="t")
    cfg["vae"]["weight_path"] = str(tmp_path / "vmae.pth")
    cfg["sample"].update(num_sampling_steps=2, per_proc_batch_size=4, fid_num=8, cfg_scale=4.0)
    torch.manual_seed(0)
    dit = t.build_model(cfg)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, p in dit.named_parameters():
            if "adaLN_modulation" in n or n.startswith("final_layer.linear"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    torch.save({"ema": dit.state_dict(), "model": dit.state_dict()}, tmp_path / "ckpt.pt")
    vae = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, kl_loss_weight=True, smooth_output=True, img_size=64)
    torch.save({"model": vae.state_dict()}, cfg["vae"]["weight_path"])
    os.makedirs(str(tmp_path / "feat_sample"))
    torch.save({"mean": torch.randn(1, 16, 1, 1, generator=g) * 0.1, "std": torch.rand(1, 16, 1, 1, generator=g) + 0.5},
               tmp_path / "feat_sample" / "latents_stats.pt")
    out16 = inf.do_sample(cfg, str(tmp_path / "ckpt.pt"), str(tmp_path / "bf16"))
    assert inf.MX8_NOTICE not in capsys.readouterr().out
    out8 = inf.do_sample(cfg, str(tmp_path / "ckpt.pt"), str(tmp_path / "mx8"), gemm_precision="mxfp8")
    assert inf.MX8_NOTICE in capsys.readouterr().out
    files = [f"{i:06d}.png" for i in range(8)]
    assert sorted(os.listdir(out8)) == files and sorted(os.listdir(out16)) == files
    a = [np.asarray(Image.open(os.path.join(out16, f))) for f in files]
    b = [np.asarray(Image.open(os.path.join(out8, f))) for f in files]
    assert all(im.shape == (64, 64, 3) and im.std() > 0 for im in b)
    assert any((x != y).any() for x, y in zip(a, b))
    # the YAML key alone switches the mode on as well
    cfg["sample"]["gemm_precision"] = "mxfp8"
    inf.do_sample(cfg, str(tmp_path / "ckpt.pt"), str(tmp_path / "mx8_yaml"))
    assert inf.MX8_NOTICE in capsys.readouterr().out
    c = [np.asarray(Image.open(os.path.join(tmp_path / "mx8_yaml", f))) for f in files]
    assert all((x == y).all() for x, y in zip(b, c))
