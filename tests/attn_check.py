"""Per-element error bounds for the attention family (csrc/attention.hip), in the manner of gemm_check.py.

Every check is |got - ref| <= bound for EVERY element.  `ref` is f64 softmax attention of the operands as stored; each bound is built from
the rounding steps one can read in the kernels.  u = 2^-24 (f32 unit roundoff); r = unit roundoff of the operand type: 2^-8 for bf16
(8 significant bits), 2^-11 for fp16 (11), 0 for f32.  (Half an ulp is at most r relative; the average is half of that, which is the
2^-9 / 2^-12 one sometimes sees quoted.  A bound has to take the maximum.)

Kinds of kernel
  "mfma16"   attn_fwd_bf16_kernel / attn_bwd_dq_bf16_kernel / attn_bwd_dkdv_bf16_kernel, bf16 or fp16 operands
  "f32"      attn_fwd_f32_kernel / attn_bwd_*_f32_kernel (scores scaled AFTER the product)
  "f32_hd16" attn_fwd_f32_hd16_kernel (q scaled in f32 before the product)

Forward
 1. c32 = (float)scale * 1.4426950408889634f, an f32 product (attention_fwd_core).  "mfma16" and "f32_hd16" multiply q by c32 in f32
    and round to the operand type, to nearest even (frag_scale / from_f; `Q[...] * c`).  torch does the same bit for bit
    ((q.float() * c32).to(dtype)), so the reference takes that q' as its operand and the step costs nothing.  "f32": s * c after the
    product; the reference uses c32 * (q . k), the product rounding is one of the `+5` below.
 2. s2_ij, the score in log2 units, is an f32 sum of hd products that starts from -ms (the MFMA C operand) or has ms subtracted after
    it.  bf16 / fp16 products are exact in f32.  However the MFMA groups the sum, a term passes through at most hd additions, then
    at most one product rounding (f32 operands), the scale multiply ("f32"), the subtraction of ms and, in the rescale branch, `s -= d`:
    hd + 5 roundings, each relative to a partial sum of magnitude at most A_ij + M_i, A = |q'| |k|^T, M_i >= |ms|.
    ms is always (a rounding of) one of the row's scores or the static shift, so M_i = max(max_j |s2_ij|, static shift).
    The tracked form updates `ms += d` in f32, at most once per 64-key tile (nt = ceil(N / 64) times; data dependent, so the worst
    case is taken): each update can move the shift of later tiles against earlier ones by u |ms|.  Together
        es_ij = u ((hd + 5) (A_ij + M_i) + nt M_i)                                  [log2 units]
 3. p = v_exp_f32(s) (1 ulp = 2 u relative; exp2f of the f32 kernels likewise), so p carries a relative error
        ep_ij = expm1(ln 2 * es_ij) + 2 u.
    For the P.V product p is rounded to the operand type: + r (acc_frag / acc_frag_h; p <= 2^6 < fp16 max).  fp16 values below 2^-14
    are subnormal with spacing 2^-24: an absolute 2^-25, in units in which the row's largest p is at least 1 (ms is within
    RESCALE_THR of the row maximum from above), so at most 2^-25 in units of P as well.
 4. The row sum l adds the UNROUNDED p for head dims 32 / 64 / 128 and in the f32 kernels, and the ROUNDED p (ones column of the V image,
    LSUM) for the padded head dims 16 and 72: el_ij = ep_ij (+ r and the fp16 term when LSUM).
 5. Accumulation: a term of l or of the P.V product passes through at most N additions; each rescale multiplies l and the accumulators
    by the SAME alpha = exp2(-d), so alpha's own error cancels in O = acc / l except that the f32 kernels compute
    alpha = exp2f(ms - ms_new), whose argument rounds (sum over the tiles of |ms - ms_new| <= 2 M_i): relative u (nt * 4 + 2 M_i) for
    alpha (2 u), the two product roundings and that argument; 1 / l and acc * inv: 3 u.  g_i = u (N + 4 nt + 2 M_i + 3).
 6. O = acc / l rounded once to the output type.  With P = softmax, E_i = sum_j P_ij (el_ij + g_i) (relative error of l),
        |dO_id| <= (sum_j P_ij (ep_ij + r + g_i) |v_jd| [+ 2^-25 sum_j |v_jd|] + |O_id| E_i) / (1 - E_i) + 1/2 ulp_out(.)
    which needs P |V|, the analogue of S = |A| |B|^T of the GEMM bounds.
 7. lse = (ms + log2f(l)) * ln 2 in f32: d ln l <= E_i / (1 - E_i); log2f (2 u of |log2 l|, |log2 l| <= |lse2| + M), the sum and the product:
        |d lse_i| <= E_i / (1 - E_i) + 4 u ln 2 (|lse2_i| + M_i) + 1/2 ulp_f32(.)

Backward, a function of (q, k, v, o, dO, lse) as GIVEN (the tests feed o and lse made by the f64 reference and rounded to their storage
types, so a forward fault can neither mask nor cause a backward failure):
 8. lse2 = lse * 1.4426950408889634f in f32: reproduced bit for bit, no error.  The dQ kernel scales q (q' = round(q c32)), the dK/dV kernel
    scales k (k' likewise, frag_scale_t at both places); the reference therefore computes TWO probability matrices,
    Pq = exp2(q' k^T - lse2) for dQ and Pk = exp2(q k'^T - lse2) for dK / dV, and neither scaling costs anything.  The chains start from -lse2:
    es as in step 2 with M_i = |lse2_i| and no running maximum (nt term dropped); ep as in step 3.
 9. delta_i = sum_d dO_id o_id: f32 sum of hd products, ed_i = (hd + 1) u sum_d |dO o|.  dP_ij = dO_i . v_j - delta_i, a chain that starts at
    -delta: edp_ij = (hd + 3) u (|dO| |v|^T + |delta_i|) + ed_i.
10. dS = p * dP in f32 (u), rounded to the operand type (r; fp16 subnormals 2^-25) before the dQ / dK product:
        DSb_ij = (1 + r) (p |dP| (ep + u) + p (1 + ep) edp) + r p |dP| [+ 2^-25]
11. dQ = scale * dS K, dK = scale * dS^T Q, dV = round(p)^T dO: f32 sums of N terms (N + 3 roundings with the scale product), one rounding
    to the output type:  |d dQ| <= scale (DSb |K| + (N + 3) u (|dS| + DSb) |K|) + 1/2 ulp_out(.), the same for dK with Q, and
    |d dV| <= (Pk (ep + r) [+ 2^-25])^T |dO| + (N + 3) u (Pk (1 + ep + r))^T |dO| + 1/2 ulp_out(.).

Fused backward (ldmae_attention_bwd_pv_qknorm): the q | k slots of dqkv are the RoPE adjoint and the RMSNorm backward (qknorm_rows_math)
applied to dq / dk AFTER their rounding to bf16.  For fixed pre-norm row x, weights and tables that map is linear in the gradient g:
t = R^T g, dn = t w, n = x rs, out = (dn - n mean(dn n)) rs.  The bound is the dQ / dK bound (its 1/2 ulp included) pushed through the
same operator with absolute values of every coefficient, plus the operator's own f32 roundings: rs = rsqrtf(sum x^2 / hd + eps) carries
(hd + 6) u / 2 + 2 u (the sum, halved by the square root, and rsqrtf), it enters `out` three times, the rest is at most hd + 8 roundings on any path:
c_op = (hd + 8 + 3 (hd / 2 + 5)) u times the absolute-value operator applied to |g| + bound, then one rounding to bf16.
"""
from __future__ import annotations

import math

import torch

from gemm_check import BoundError, check, ulp  # noqa: F401  (re-exported for the tests)

U = 2.0 ** -24
LN2 = math.log(2.0)
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
R_OP = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 0.0}
SUB16 = 2.0 ** -25                    # half the spacing of fp16 subnormals
RESCALE_THR = 6.0                     # csrc/attention.hip
STATIC_MAX = 50.0                     # bounds up to 50 take the static shift


def c32(scale: float) -> float:
    """(float)scale * 1.4426950408889634f as the kernels form it."""
    return float(torch.tensor(scale, dtype=F32) * torch.tensor(1.4426950408889634, dtype=F32))


def s32(scale: float) -> float:
    return float(torch.tensor(scale, dtype=F32))


def kind_of(dtype, hd: int) -> str:
    return "mfma16" if dtype != F32 else ("f32_hd16" if hd == 16 else "f32")


def scaled(x: torch.Tensor, scale: float, kind: str) -> torch.Tensor:
    """The stationary operand as the kernel holds it, in f64: round(x * c32) in the operand type, or c32 * x for the f32 kernel."""
    c = c32(scale)
    if kind == "f32":
        return x.double() * c
    return (x.float() * torch.tensor(c, dtype=F32, device=x.device)).to(x.dtype).double()


def _lsum(kind, hd):
    return kind == "mfma16" and hd % 32 != 0


def fwd_ref(q, k, v, scale, kind=None, shift=None):
    """q, k, v [B,H,N,hd] as stored -> dict(o, lse [f64, head-major], bo, bl [bounds], smax [B,H,N] = max_j |s2_ij|, finite).
    shift: the static shift the kernel may use (scalar or broadcastable to [B,H,N]); values above 50 are ignored as the kernel ignores them."""
    dtype, hd, N = q.dtype, q.shape[-1], q.shape[-2]
    kind = kind or kind_of(dtype, hd)
    nt = (N + 63) // 64
    r = R_OP[dtype]
    Q, K, V = scaled(q, scale, kind), k.double(), v.double()
    s2 = Q @ K.transpose(-1, -2)
    A = Q.abs() @ K.abs().transpose(-1, -2)
    smax = s2.abs().amax(-1, keepdim=True)
    M = smax
    if shift is not None:
        sh = torch.as_tensor(shift, dtype=torch.float64, device=q.device)
        sh = sh.reshape(sh.shape + (1,)) if sh.dim() == 3 else sh
        M = torch.maximum(M, torch.where(sh <= STATIC_MAX, sh, torch.zeros_like(sh)).expand_as(M))
    mx = s2.amax(-1, keepdim=True)
    p = torch.exp2(s2 - mx)
    l = p.sum(-1, keepdim=True)
    P = p / l
    O = P @ V
    lse2 = mx + torch.log2(l)
    lse = lse2 * LN2
    es = U * ((hd + 5) * (A + M) + nt * M)
    ep = torch.expm1(LN2 * es) + 2 * U
    sub = SUB16 if dtype == F16 else 0.0
    g = U * (N + 4 * nt + 2 * M + 3)
    el = ep + (r if _lsum(kind, hd) else 0.0)
    E = (P * (el + g)).sum(-1, keepdim=True) + (N * sub if _lsum(kind, hd) else 0.0)
    num = (P * (ep + r + g)) @ V.abs() + sub * V.abs().sum(-2, keepdim=True)
    fn = (num + O.abs() * E) / (1 - E)
    bo = fn + 0.5 * ulp(O.abs() + fn, dtype)
    fl = E / (1 - E) + 4 * U * LN2 * (lse2.abs() + M)
    bl = fl + 0.5 * ulp(lse.abs() + fl, F32)
    finite = bool(torch.isfinite(O).all() and torch.isfinite(lse).all() and torch.isfinite(bo).all() and torch.isfinite(bl).all())
    return dict(o=O, lse=lse[..., 0], bo=bo, bl=bl[..., 0], smax=smax[..., 0], finite=finite, s2=s2)


def bwd_ref(q, k, v, o, do, lse, scale, kind=None):
    """All of q, k, v, o, do [B,H,N,hd] as stored, lse [B,H,N] f32 -> dict(dq, dk, dv, bdq, bdk, bdv) in f64, head-major."""
    dtype, hd, N = q.dtype, q.shape[-1], q.shape[-2]
    kind = kind or kind_of(dtype, hd)
    r = R_OP[dtype]
    sub = SUB16 if dtype == F16 else 0.0
    sc = s32(scale)
    Q, K, V, O, dO = (t.double() for t in (q, k, v, o, do))
    lse2 = (lse.float() * torch.tensor(1.4426950408889634, dtype=F32, device=lse.device)).double()[..., None]
    M = lse2.abs()
    delta = (dO * O).sum(-1, keepdim=True)
    ed = (hd + 1) * U * (dO.abs() * O.abs()).sum(-1, keepdim=True)
    dP = dO @ V.transpose(-1, -2) - delta
    edp = (hd + 3) * U * (dO.abs() @ V.abs().transpose(-1, -2) + delta.abs()) + ed

    def side(Qx, Kx):
        s2 = Qx @ Kx.transpose(-1, -2)
        A = Qx.abs() @ Kx.abs().transpose(-1, -2)
        es = U * (hd + 5) * (A + M)
        ep = torch.expm1(LN2 * es) + 2 * U
        p = torch.exp2(s2 - lse2)
        a = p * dP.abs()
        dsb = (1 + r) * (a * (ep + U) + p * (1 + ep) * edp) + r * a + sub
        return p, ep, p * dP, dsb

    _, _, dSq, bq_ = side(scaled(q, scale, kind), K)
    pk, epk, dSk, bk_ = side(Q, scaled(k, scale, kind))
    acc = (N + 3) * U

    def fin(ref, fn):
        return ref, fn + 0.5 * ulp(ref.abs() + fn, dtype)

    dq, bdq = fin(sc * (dSq @ K), sc * (bq_ @ K.abs() + acc * ((dSq.abs() + bq_) @ K.abs())))
    dk, bdk = fin(sc * (dSk.transpose(-1, -2) @ Q), sc * (bk_.transpose(-1, -2) @ Q.abs() + acc * ((dSk.abs() + bk_).transpose(-1, -2) @ Q.abs())))
    dv, bdv = fin(pk.transpose(-1, -2) @ dO, (pk * (epk + r) + sub).transpose(-1, -2) @ dO.abs() + acc * ((pk * (1 + epk + r)).transpose(-1, -2) @ dO.abs()))
    return dict(dq=dq, dk=dk, dv=dv, bdq=bdq, bdk=bdk, bdv=bdv, delta=delta[..., 0])


# ----------------------------------------------------------------------------- fused QK-norm / RoPE epilogue
def qknorm_bwd_op(g, x, w, cos, sin, eps, absolute=False):
    """qknorm_rows_math in f64: g, x [B,H,N,hd] (gradient, pre-norm row), w [hd] or None (RoPE only), cos / sin [N,hd].
    absolute=True: the same operator with absolute values of all coefficients (an upper bound of its action on |g|).
    -> (out [B,H,N,hd], per-row weight-gradient terms t * n [B,H,N,hd])."""
    hd = g.shape[-1]
    c, s = cos.double(), sin.double()
    ge, go = g[..., 0::2], g[..., 1::2]
    if absolute:
        t0 = ge * c[:, 0::2].abs() + go * s[:, 1::2].abs()
        t1 = go * c[:, 1::2].abs() + ge * s[:, 0::2].abs()
    else:
        t0 = ge * c[:, 0::2] + go * s[:, 1::2]
        t1 = go * c[:, 1::2] - ge * s[:, 0::2]
    t = torch.stack([t0, t1], -1).reshape(g.shape)
    if w is None:
        return t, None
    X = x.double()
    rs = torch.rsqrt((X * X).sum(-1, keepdim=True) / hd + eps)
    n = X * rs
    W = w.double()
    if absolute:
        n, W = n.abs(), W.abs()
    dn = t * W
    m = (dn * n).sum(-1, keepdim=True) / hd
    out = (dn + n * m) * rs if absolute else (dn - n * m) * rs
    return out, t * n


def qknorm_bwd_bound(g_ref, g_bound, x, w, cos, sin, eps, out_dtype=BF16):
    """(ref, bound) of the fused epilogue's stored row given the f64 dq (dk) and its bound (which includes its rounding to bf16)."""
    hd = g_ref.shape[-1]
    ref, _ = qknorm_bwd_op(g_ref, x, w, cos, sin, eps)
    push, _ = qknorm_bwd_op(g_bound, x, w, cos, sin, eps, absolute=True)
    mag, _ = qknorm_bwd_op(g_ref.abs() + g_bound, x, w, cos, sin, eps, absolute=True)
    fn = push + (hd + 8 + 3 * (hd / 2 + 5)) * U * mag
    return ref, fn + 0.5 * ulp(ref.abs() + fn, out_dtype)


# ----------------------------------------------------------------------------- inputs
def make_inputs(B, H, N, hd, dtype, family, seed, device="cpu", gain=None):
    """q, k, v, do [B,H,N,hd] in `dtype`.  family "unit": N(0, 1).  "peaked": q and k scaled so that the row maxima of the scores in log2
    units reach 15 .. 40, and every 37th query row gets one key late in the sequence aligned with it (score about 35): the running maximum
    jumps there, the static-shift margin and a large |ms| are exercised.  gain: per-head factor on q and k ([H] list)."""
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(B, H, N, hd, generator=g) for _ in range(4))
    c = c32(hd ** -0.5)
    if family == "peaked":
        f = (22.0 / (c * hd ** 0.5 * max(1.0, (2 * math.log(max(N, 2))) ** 0.5))) ** 0.5
        q, k = q * f, k * f
        for i in range(5 % N, N, 37):
            j = N - 1 - (i * 7) % max(1, N // 3)
            qi = q[:, :, i]
            k[:, :, j] = qi * (35.0 / (c * (qi * qi).sum(-1, keepdim=True)))
    if gain is not None:
        gn = torch.tensor(gain, dtype=torch.float32).view(1, H, 1, 1)
        q, k = q * gn, k * gn
    return tuple(t.to(dtype).to(device) for t in (q, k, v, do))
