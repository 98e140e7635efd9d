"""Per-element error bounds for the GEMM family (gemm_nt and its epilogues, gemm_tn, colsum, thin_nt / thin_tn).

Every check compares a kernel's output element by element with an f64 reference computed from the SAME rounded operands the kernel
reads, and allows

    |got - ref| <= acc + 1/2 ulp_out(|ref| + acc),      acc = C_ACC * K * 2^-24 * S_ij

where K is the contraction length (M for TN products, the summed row count for column sums) and S_ij the same sum taken over absolute
values (|A| |B|^T plus the absolute values of every term the epilogue adds before the one rounding to the output type).

Derivation of C_ACC = 2.  bf16 and f16 products are exact in f32 (8 + 8 and 11 + 11 significant bits fit in 24), so only the f32
additions round; f32 x f32 products round once more.  With round-to-nearest every f32 addition has a relative error |d| <= u = 2^-24.
However the kernel groups its sums (MFMA dot steps, K-blocks, split-K slabs reduced in fixed order, row groups of a column sum), a term
passes through at most K - 1 additions on its way to the accumulator; then come at most three epilogue additions (bias, pos or
beta * C) and, for f32 operands, one product rounding.  So each term of S carries a relative error of at most (1 + u)^(K + 3) - 1,
which is below (K + 4) u for K u << 1, and K + 4 <= 2 K for every K >= 4 (the smallest contraction this suite runs is 8).  The final
rounding to a 16-bit output adds at most half an ulp of the stored value, whose magnitude is at most |ref| + acc.

Nonlinear epilogues are checked in two steps: the stored pre-activation (pre, h12) with the bound above, then the activation output
against the f64 activation of what the kernel fed it, allowing 1 ulp of the output, the documented approximation error of the device
functions in csrc/common.h (16-bit GELU: 1.5e-7, the figure stated for the Abramowitz-Stegun erf these types used before erf_act
became erff for every type -- erff meets it; erff: 2 ulp; fast_sigmoid: __expf and a
reciprocal, 1 ulp each plus the rounding of the exponent argument), and -- where the kernel applies the activation to the UNROUNDED f32
value but stores the pre-activation rounded -- the slope of the activation times half an ulp of the pre-activation.
"""
from __future__ import annotations

import math

import torch

U = 2.0 ** -24          # unit roundoff of f32
C_ACC = 2.0             # see the module docstring
ERF_AS = 1.5e-7         # erf of the 16-bit GELU epilogues (stated for the former A-S 7.1.26 evaluation; erff, which they call now, meets it)
ERF_LIBM = 2 * 2.0 ** -24   # erff: 2 ulp of a value in [-1, 1]

# (explicit mantissa bits, smallest normal exponent; subnormals share its spacing)
_FMT = {torch.bfloat16: (7, -126), torch.float16: (10, -14), torch.float32: (23, -126)}


def ulp(x: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of `dtype` numbers at |x| (f64 tensor in, f64 tensor out)."""
    p, emin = _FMT[dtype]
    _, e = torch.frexp(x.abs())
    e = torch.where(x == 0, torch.full_like(e, emin), e - 1).clamp(min=emin)
    return torch.ldexp(torch.ones_like(x), e - p)


def acc_bound(S: torch.Tensor, K: int) -> torch.Tensor:
    """Error of the f32 accumulation of K terms whose absolute values sum to S (before any rounding to the output type)."""
    return C_ACC * K * U * S


def sum_bound(ref: torch.Tensor, S: torch.Tensor, K: int, out_dtype) -> torch.Tensor:
    """acc + 1/2 ulp_out(|ref| + acc): an f32-accumulated sum of K terms stored in out_dtype."""
    a = acc_bound(S, K)
    return a + 0.5 * ulp(ref.abs() + a, out_dtype)


class BoundError(AssertionError):
    pass


def check(name: str, got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """Assert |got - ref| <= bound everywhere (NaN or inf in `got` fails).  Returns max |got - ref| / bound (0/0 counts as 0).
    On failure the message names the worst element: index, value got, reference and bound."""
    g = got.double()
    err = (g - ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, math.inf))
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    flat = int(torch.argmax(torch.nan_to_num(ratio, nan=math.inf)))
    worst = float(ratio.flatten()[flat])
    if not worst <= 1.0:
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
        nbad = int((~(ratio <= 1.0)).sum())
        raise BoundError(f"{name}: {nbad} of {ratio.numel()} elements out of bound; worst at {idx}: got {float(g[idx])!r}, "
                         f"ref {float(ref[idx])!r}, |diff| {float(err[idx]):.3e} > bound {float(bound[idx]):.3e} (x{worst:.3g})")
    return worst


# ----------------------------------------------------------------------------- references
def nt_ref(a: torch.Tensor, b: torch.Tensor, *adds):
    """(ref, S) of a[M,K] @ b[N,K]^T + sum(adds) in f64 from the operands as stored; adds broadcast to [M,N] (bias, pos, beta*C)."""
    A, B = a.double(), b.double()
    ref, S = A @ B.T, A.abs() @ B.abs().T
    for t in adds:
        if t is not None:
            ref = ref + t.double()
            S = S + t.double().abs()
    return ref, S


def tn_ref(a: torch.Tensor, b: torch.Tensor, old=None):
    """(ref, S) of old + a[M,N]^T @ b[M,K] in f64."""
    A, B = a.double(), b.double()
    ref, S = A.T @ B, A.abs().T @ B.abs()
    if old is not None:
        ref, S = ref + old.double(), S + old.double().abs()
    return ref, S


def colsum_ref(x: torch.Tensor, old=None):
    X = x.double()
    ref, S = X.sum(0), X.abs().sum(0)
    if old is not None:
        ref, S = ref + old.double(), S + old.double().abs()
    return ref, S


def check_sum(name, got, ref, S, K, out_dtype=None) -> float:
    return check(name, got, ref, sum_bound(ref, S, K, out_dtype or got.dtype))


def check_gate_res(name, xout, xin, gate_rows, ref_y, S_y, K, y_dtype) -> float:
    """xout = fma(gate, round_y(y), xin): y rounded to y_dtype (its own sum bound), then one f32 rounding of the fused multiply-add."""
    by = sum_bound(ref_y, S_y, K, y_dtype)
    X, G = xin.double(), gate_rows.double()
    ref = X + G * ref_y
    bound = G.abs() * by + 0.5 * ulp(X.abs() + G.abs() * (ref_y.abs() + by), torch.float32)
    return check(name, xout, ref, bound)


def _gelu(x):
    return 0.5 * x * (1.0 + torch.special.erf(x * 0.7071067811865476))


def _gelu_slope(x):
    return 0.5 * (1.0 + torch.special.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


def check_gelu(name, out, pre_in, pre_is_exact, out_dtype, erf_err) -> float:
    """out = round(gelu(p)) where pre_in is the stored pre-activation; pre_is_exact: the kernel applied gelu to exactly that value
    (f32 outputs), otherwise to the unrounded f32 value within half an ulp of it."""
    x = pre_in.double()
    h = torch.zeros_like(x) if pre_is_exact else 0.5 * ulp(x, out_dtype)
    ref = _gelu(x)
    slope = torch.maximum(torch.maximum(_gelu_slope(x - h).abs(), _gelu_slope(x).abs()), _gelu_slope(x + h).abs())
    # 0.5 * y * (1 + erf): the approximation error of erf, the f32 roundings of y * c, 1 + erf and the two products
    fn = 0.5 * x.abs() * (erf_err + 2 * U) + 4 * U * ref.abs()
    dev = slope * h + 0.5 * h * h
    bound = fn + dev + ulp(ref.abs() + fn + dev, out_dtype)
    return check(name, out, ref, bound)


def check_gelu_bwd(name, out, ref_acc, S_acc, K, v, act_dtype, out_dtype, erf_err) -> float:
    """out = round_out(round_act(acc) * gelu'(v)), v the stored pre-activation, acc the f32 product dy @ w2t^T."""
    V = v.double()
    sl = _gelu_slope(V)
    ba = sum_bound(ref_acc, S_acc, K, act_dtype)
    pdf = torch.exp(-0.5 * V * V) * 0.3989422804014327
    # cdf: erf error / 2 and 2 roundings; pdf: __expf (1 ulp) of an argument rounded twice (relative 2u of 0.5 v^2), then v * pdf and the sum
    e_sl = 0.5 * erf_err + 4 * U + V.abs() * pdf * (4 * U + V * V * U) + 2 * U * sl.abs()
    ref = ref_acc * sl
    fn = sl.abs() * ba + (ref_acc.abs() + ba) * e_sl
    bound = fn + ulp(ref.abs() + fn, out_dtype)
    return check(name, out, ref, bound)


def _sig_err(a):
    """Relative error of fast_sigmoid(a) = rcp(1 + __expf(-a)): v_exp of the argument scaled by log2(e) (relative error |a| u from that
    rounding, 1 ulp from v_exp), the addition and v_rcp (1 ulp each)."""
    return (a.abs() * 2 + 6) * U


def check_swiglu(name, hid, h12) -> float:
    """hid = round(x1 * fast_sigmoid(x1) * x2) of the STORED bf16 h12 halves."""
    Hs = h12.shape[1] // 2
    x1, x2 = h12[:, :Hs].double(), h12[:, Hs:].double()
    s = torch.sigmoid(x1)
    ref = x1 * s * x2
    fn = ref.abs() * (_sig_err(x1) + 3 * U)
    return check(name, hid, ref, fn + ulp(ref.abs() + fn, hid.dtype))


def check_swiglu_bwd(name, dh12, ref_acc, S_acc, K, h12) -> float:
    """dh12 = round(g*b*s*(1 + a*(1 - s)) | g*a*s), g = acc rounded to bf16 first, a / b the stored h12 halves, s = fast_sigmoid(a)."""
    Hs = h12.shape[1] // 2
    a, b = h12[:, :Hs].double(), h12[:, Hs:].double()
    s = torch.sigmoid(a)
    bg = sum_bound(ref_acc, S_acc, K, torch.bfloat16)
    G = ref_acc.abs() + bg
    es = s * _sig_err(a)                                       # absolute error of s
    fa = s * (1 + a * (1 - s))
    ref_a, ref_b = ref_acc * b * fa, ref_acc * a * s
    # d fa / d s = 1 + a - 2 a s; five f32 roundings in each product chain
    fn_a = (b * fa).abs() * bg + G * b.abs() * ((1 + a - 2 * a * s).abs() * es + 5 * U * (s * (1 + a.abs() * (1 + s))))
    fn_b = (a * s).abs() * bg + G * a.abs() * (es + 3 * U * s)
    ra = check(name + "[da]", dh12[:, :Hs], ref_a, fn_a + ulp(ref_a.abs() + fn_a, dh12.dtype))
    rb = check(name + "[db]", dh12[:, Hs:], ref_b, fn_b + ulp(ref_b.abs() + fn_b, dh12.dtype))
    return max(ra, rb)
