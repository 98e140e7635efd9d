"""The MXFP8 sampling mode's arithmetic contract (include/ldmae_hip.h) restated in torch f64 on the CPU: the MX block
quantiser, its dequantiser, and an f64 model of the tiny DiT with the quantiser in front of the four block GEMMs and on their weights
(no bf16 roundings: what the contract alone costs).  Helper of tests/test_mx8_cpu.py and tests/test_gpu_mx8.py."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import dit as odit

BLOCK = 32


def scale_exponents(x: torch.Tensor) -> torch.Tensor:
    """e [M, K/32] (int64) of the rows of x [M, K]: amax = m * 2^x, m in [1, 2); e = x - 8 if m <= 1.75 else x - 7, clamped to [-127, 127];
    -127 for an all-zero block."""
    M, K = x.shape
    assert K % BLOCK == 0
    amax = x.double().abs().reshape(M, K // BLOCK, BLOCK).amax(-1)
    m, ex = torch.frexp(amax)                              # amax = m * 2^ex, m in [0.5, 1)
    e = torch.where(2 * m <= 1.75, ex - 9, ex - 8).to(torch.int64).clamp(-127, 127)
    return torch.where(amax == 0, torch.full_like(e, -127), e)


def quantize(x: torch.Tensor):
    """(q [M,K] uint8: OCP e4m3fn bytes of x * 2^-e, round to nearest even; scales [M,K/32] uint8: E8M0 bytes e + 127)."""
    M, K = x.shape
    e = scale_exponents(x)
    scaled = torch.ldexp(x.double().reshape(M, K // BLOCK, BLOCK), (-e).unsqueeze(-1).expand(M, K // BLOCK, BLOCK))     # a power of two: exact
    q = scaled.reshape(M, K).to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, (e + 127).to(torch.uint8)


def dequantize(q: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """f64 [M,K] of (q, scales)."""
    M, K = q.shape
    v = q.view(torch.float8_e4m3fn).to(torch.float32).double().reshape(M, K // BLOCK, BLOCK)
    e = (scales.to(torch.int64) - 127).unsqueeze(-1).expand(M, K // BLOCK, BLOCK)
    return torch.ldexp(v, e).reshape(M, K)


def canon(q: torch.Tensor) -> torch.Tensor:
    """Element bytes with -0 (0x80) mapped to +0: one value under the contract."""
    return torch.where(q == 0x80, torch.zeros_like(q), q)


def fake_quant(x: torch.Tensor) -> torch.Tensor:
    """dequantize(quantize(x)) along the last dimension, any leading shape, f64 out."""
    shp = x.shape
    q, s = quantize(x.reshape(-1, shp[-1]))
    return dequantize(q, s).reshape(shp)


# ----------------------------------------------------------------------------- f64 model of the DiT with the quantiser at the four GEMMs
def _rmsnorm(x, w, eps=1e-6):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def _lin(x, w, b, quant):
    """x @ w^T + b in f64; quant: both operands through the quantiser (the weight from its f32 master value)."""
    if quant:
        x, w = fake_quant(x), fake_quant(w.float())
    return F.linear(x, w.double(), b)


def _block(sd, i, x, c, cfg, cos, sin, quant):
    p = f"blocks.{i}."
    B, N, C = x.shape
    H, hd = cfg.num_heads, cfg.head_dim
    mod = F.linear(F.silu(c), sd[p + "adaLN_modulation.1.weight"], sd[p + "adaLN_modulation.1.bias"])
    sh1, s1, g1, sh2, s2, g2 = mod.chunk(6, dim=1)
    xm = odit.modulate(_rmsnorm(x, sd[p + "norm1.weight"]), sh1, s1)
    qkv = _lin(xm, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"], quant).reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    if cfg.use_qknorm:
        q, k = _rmsnorm(q, sd[p + "attn.q_norm.weight"]), _rmsnorm(k, sd[p + "attn.k_norm.weight"])
    if cfg.use_rope:
        q, k = odit.apply_rope(q, cos, sin), odit.apply_rope(k, cos, sin)
    o = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1) @ v
    o = o.transpose(1, 2).reshape(B, N, C)
    x = x + g1.unsqueeze(1) * _lin(o, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"], quant)
    xm2 = odit.modulate(_rmsnorm(x, sd[p + "norm2.weight"]), sh2, s2)
    x1, x2 = _lin(xm2, sd[p + "mlp.w12.weight"], sd[p + "mlp.w12.bias"], quant).chunk(2, dim=-1)
    return x + g2.unsqueeze(1) * _lin(F.silu(x1) * x2, sd[p + "mlp.w3.weight"], sd[p + "mlp.w3.bias"], quant)


def dit_forward_with_cfg_f64(sd, x, t, y, cfg: "odit.DiTConfig", cfg_scale, quant: bool) -> torch.Tensor:
    """LightningDiT.forward_with_cfg (RMSNorm + SwiGLU + shift form) in f64 from an f64 state dict; quant: the MX quantiser in front of
    the qkv, projection, w12 and w3 GEMMs of every block and on their weights -- everything else exact."""
    half = x[: len(x) // 2]
    xx = torch.cat([half, half], 0).double()
    cos, sin = (sd["feat_rope.freqs_cos"], sd["feat_rope.freqs_sin"]) if cfg.use_rope else (None, None)
    h = odit.patch_embed(sd, xx, cfg)
    temb = F.linear(odit.timestep_embedding(t).double(), sd["t_embedder.mlp.0.weight"], sd["t_embedder.mlp.0.bias"])
    c = F.linear(F.silu(temb), sd["t_embedder.mlp.2.weight"], sd["t_embedder.mlp.2.bias"]) + sd["y_embedder.embedding_table.weight"][y]
    for i in range(cfg.depth):
        h = _block(sd, i, h, c, cfg, cos, sin, quant)
    mod = F.linear(F.silu(c), sd["final_layer.adaLN_modulation.1.weight"], sd["final_layer.adaLN_modulation.1.bias"])
    shift, scale = mod.chunk(2, dim=1)
    out = F.linear(odit.modulate(_rmsnorm(h, sd["final_layer.norm_final.weight"]), shift, scale), sd["final_layer.linear.weight"], sd["final_layer.linear.bias"])
    out = odit.unpatchify(out, cfg)
    eps, rest = out[:, :3], out[:, 3:]
    cond, uncond = torch.split(eps, len(eps) // 2, dim=0)
    half_eps = uncond + cfg_scale * (cond - uncond)
    return torch.cat([torch.cat([half_eps, half_eps], 0), rest], dim=1)


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


# ----------------------------------------------------------------------------- per-element bound of the block-scaled GEMM
# gemm_check's C_ACC = 2 is derived for round-to-nearest f32 additions.  The summation INSIDE one 128-deep scaled MFMA is not documented and
# is not that: a one-instruction probe (gemm_nt_mx8 at K = 128 without bias, f32 output: the accumulator operand is zero, so the result is one
# instruction's sum) on random e4m3 codes with random E8M0 scales measures its worst error against f64 relative to S = sum |a| |w|
# (tools/bench_mx8.py --probe).  MFMA_E1 is that worst figure; the bound allows twice it per instruction, plus
# round-to-nearest f32 additions between the K / 128 instructions and in the epilogue.
MFMA_E1 = 3.535e-4          # measured worst over 16 draws of 256 x 256 outputs, scale spreads 2^0 .. 2^+-20; the mean is 2.5e-5


def acc_bound(S: torch.Tensor, K: int) -> torch.Tensor:
    import gemm_check as gc
    return 2.0 * MFMA_E1 * S + gc.C_ACC * (K // 128 + 3) * gc.U * S


def sum_bound(ref: torch.Tensor, S: torch.Tensor, K: int, out_dtype) -> torch.Tensor:
    """acc + 1/2 ulp_out(|ref| + acc), as gemm_check.sum_bound with the accumulation term of the scaled MFMA."""
    import gemm_check as gc
    a = acc_bound(S, K)
    return a + 0.5 * gc.ulp(ref.abs() + a, out_dtype)


def check_sum(name, got, ref, S, K, out_dtype):
    import gemm_check as gc
    return gc.check(name, got, ref, sum_bound(ref, S, K, out_dtype))


def check_gate_res(name, xout, xin, gate_rows, ref_y, S_y, K, y_dtype):
    """gemm_check.check_gate_res with the bound above for y."""
    import gemm_check as gc
    by = sum_bound(ref_y, S_y, K, y_dtype)
    X, G = xin.double(), gate_rows.double()
    ref = X + G * ref_y
    return gc.check(name, xout, ref, G.abs() * by + 0.5 * gc.ulp(X.abs() + G.abs() * (ref_y.abs() + by), torch.float32))


# ----------------------------------------------------------------------------- planted blocks of the quantiser tests
def planted_blocks() -> torch.Tensor:
    """[n, 32] f32 rows, one block each, at the corners of the exponent rule (see tests/test_mx8_cpu.py)."""
    rows = []

    def blk(amax, fill):
        r = torch.tensor(fill, dtype=torch.float32).repeat(32)[:32].clone()
        r[5] = amax
        return r

    rows.append(torch.zeros(32))                                             # all zero -> e = -127
    for k in (-20, 0, 9):
        rows.append(blk(448.0 * 2.0 ** k, [0.3 * 2.0 ** k, -1.7 * 2.0 ** k]))                # amax exactly 448 * 2^k
        rows.append(blk(448.0 * 2.0 ** k * (1 + 2.0 ** -23), [0.3 * 2.0 ** k, -100.0 * 2.0 ** k]))      # just above
        rows.append(blk(-1.75 * 2.0 ** k, [1.0 * 2.0 ** k, 0.013 * 2.0 ** k]))                 # mantissa exactly 1.75 (negative amax element)
        rows.append(blk(1.75 * 2.0 ** k * (1 + 2.0 ** -22), [1.0 * 2.0 ** k, -0.6 * 2.0 ** k]))  # just above 1.75
    # values landing on e4m3 subnormals: amax 256 -> e = 0; e4m3 subnormals are multiples of 2^-9 below 2^-6
    rows.append(blk(256.0, [2.0 ** -9, 3 * 2.0 ** -9, -5 * 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -7 + 2.0 ** -10, 7.4 * 2.0 ** -9, -2.0 ** -11]))
    rows.append(blk(2.0 ** -130, [2.0 ** -132, 0.0]))                          # x = -130 -> e = -138 -> clamped to -127
    rows.append(blk(float(torch.finfo(torch.bfloat16).max), [1e30, -3e38, 1.0]))              # largest bf16
    return torch.stack(rows)
