"""Per-element references and error bounds for the row kernels of csrc/elementwise.hip and csrc/qk_rope.hip, in the manner of gemm_check.py / attn_check.py.

Every check is |got - ref| <= bound for EVERY element (gemm_check.check).  `ref` is f64, computed from the operands AS STORED (bf16 widened
exactly) and from the mathematical definition of the operation (oracle/dit.py: rmsnorm, modulate, apply_rope; LayerNorm without affine
parameters; their adjoints), never from the kernel's order of operations.  Each bound is built from the rounding steps one can read in
the kernel.  u = 2^-24; gam(n) = n u / (1 - n u) bounds the relative error (1 + u)^n - 1 of n chained f32 roundings (Higham); a 16-bit
output adds half an ulp of its type at the stored value (gemm_check.ulp).  An f32 output adds nothing: its last f32 operation IS the store.
Every count below is a number of roundings on the longest path; a product contracted into the following add only removes one.

Row statistics (rmsnorm_mod_fwd_kernel, the qknorm_rope kernels; row_stats)
  R1. `ss += hsum(xv * xv)`, wave_sum / group_sum / the LDS loop of the dense kernels: an f32 sum of D nonnegative products in SOME
      association.  A term passes through its product and at most D - 1 additions; `ss / (float)D` is one more: relative gam(D + 1).
  R2. `+ eps`: one rounding; with the division's, rho = E_ss / D / arg + gam(2) relative on arg = ss / D + eps (both parts >= 0).
  R3. `rsqrtf`: 2 u relative (the 2 u of attn_check.py, "Fused backward"), on top of (1 - rho)^(-1/2) - 1 <= rho / (2 (1 - rho)):
          e_rs = (1 + rho / (2 (1 - rho))) (1 + 2 u) - 1                 [relative error of rs; rstd is stored as computed]
  R4. center: `mean = wave_sum(s1) / (float)D` with s1 = sum_i hsum(xv[i]).  Here the terms do not share a sign, so the error is
      relative to sum |x| and the ASSOCIATION matters: hsum is 2 additions deep, `s1 +=` NCH = ceil(D / 256) deep, the butterfly 6, the
      division 1: L = NCH + 9 roundings on any path, |d mean| <= em = gam(L) mean|x|.  `xv - f4(mean)` then rounds once more:
          exc_i = em (1 + u) + u |xc_i|                                  [ABSOLUTE error of the centred element; u |mean|-sized]
      and ss of the centred row moves by at most sum_i (2 |xc_i| exc_i + exc_i^2) before R1 applies.
Norm + modulate forward, both forms: `y = (xv * rs) * wv; y = y * (f4(1) + scale); y = y + shift`
  F1. the inherited errors: |w (1 + scale)| rs (exc (1 + e_rs) + |xc| e_rs).
  F2. x rs, . w (skipped without w: exact), 1 + scale and its product (skipped when scale == NULL), + shift (skipped when NULL): k <= 5
      roundings, each relative to a partial result of magnitude at most mag + |shift|, mag = (|xc| + exc) rs (1 + e_rs) |w (1 + scale)|.
      fn = F1 + gam(k) (mag + |shift|), then the store.
Norm + modulate backward (rmsnorm_mod_bwd_kernel, every instantiation), a function of (dout, x, w, scale, rstd) AS GIVEN: rs is exact.
  B1. n = (x - mean) rs: `(x - f4(mean)) * rs`, en = rs exc + u rs (|xc| + exc); N = |n| + en.  (RMS form: exc = 0, en = u |n|.)
  B2. dn = dout (1 + scale) w: `dy = g * sc; dn = dy * wc` with sc = fl(1 + scale): k_dn = 2 [scale] + 1 [w] roundings, edn = gam(k_dn) |dn|.
  B3. `dot = wave_sum(dot) / (float)D` of `dn * nv`: (sum (edn N + |dn| en) + gam(D + 2) sum (|dn| + edn) N) / D; `msum` (center) likewise
      with gam(D + 1) and no n.  (Sums of D terms in any association; the FULL form's wave_sum_dpp is another one.)
  B4. `d0 = ((dn - nv * dot) - f4(msum)) * rs`: for fixed x, w, scale, rstd a linear map of dout.  Its absolute-value operator applied to
      |dout| gives Z = rs (|dn| + edn + N (|dot| + edot) + |msum| + emsum); the four roundings of the line cost gam(4) Z, the inherited errors
      rs (edn + en (|dot| + edot) + |n| edot + emsum).  beta_x = 1: `*p + d0`, one more rounding u (|old| + |d0| + ed0).
  B5. column sums (a_sh, a_sc, a_w, a_g; the 4-wave combine, mod_partials_reduce_kernel, group_reduce_kernel): the sum_bound form with
      K = rows summed (rows_per_batch for dshift / dscale / dgate, M for dw) and each term's own error E added:
      fn = E + 2 K u (S + E) (+ |old| in S for beta_w = 1).  Terms: dshift: g, exact.  dscale: `g * (nv * wc)`: |g w| (en + gam(2) N).
      dw: `dy * nv`: |g (1 + scale)| (en + gam(2 [scale] + 1) N).  dgate: `gn * y`: |y| (edx + u (|dx| + edx)).
  B6. `dy = mul_rn(gn, gate)`, rounded to T: |gate| edx + u |gate| (|dx| + edx), then the store.
  B7. dbias = column sums of dy AS STORED (the kernel's comment): reference = f64 column sum of the dy the kernel wrote, exact terms, K = M.
gate_bwd_kernel alone: B6 / B5 / B7 with an exact dx (edx = 0); gate == NULL: dy = round_T(dx).
QK-norm + RoPE forward (qknorm_rope_fwd_kernel, fwd8, fwd_dense, fwd_dense8)
  Q1. rq as R1 - R3 with D = hd.  `(qv * rq) * wqv`: e_t = (1 + e_rs) (1 + gam(2)) - 1 relative (0 in the RoPE-only mode: x * 1 * 1 is exact).
  Q2. rope_apply: two products and one add per element, out_e = t_e c_e - t_o s_e, out_o = t_o c_o + t_e s_o with independent tables:
      fn = ((1 + e_t) (1 + gam(2)) - 1) (|t_e c_e| + |t_o s_e|), then the store.  Plain relayout and v in every mode: bit exact.
QK-norm + RoPE backward (qknorm_rope_bwd_kernel): the q | k slots are attn_check.qknorm_bwd_bound (the same per-row map as the fused
  attention backward) with an exact incoming gradient; the v slot is a bit-exact copy.  dwq / dwk: sums over the B N H items of
  `tq * nq`: tq three roundings, nq e_rs and one, the product one: E = ((1 + gam(3)) (1 + e_rs) (1 + gam(2)) - 1) |t|_abs |n|, K = B N H (B5).
  dbias: column sums of dqkv as stored, K = B N (B7).
rope_kernel: Q2 with e_t = 0; transposed: the adjoint, out_e = g_e c_e + g_o s_o, out_o = g_o c_o - g_e s_e.
"""
from __future__ import annotations

import torch

import attn_check as ac
from gemm_check import BoundError, U, acc_bound, check, sum_bound, ulp  # noqa: F401  (re-exported for the tests)

F32, BF16 = torch.float32, torch.bfloat16


def gam(n):
    return n * U / (1 - n * U)


def nch(D: int) -> int:
    """DISPATCH_NCH: float4 chunks per lane."""
    return (D // 4 + 63) // 64


def stored(ref, fn, dtype):
    """Bound of a value with f32 error fn stored in `dtype`."""
    return fn if dtype == F32 else fn + 0.5 * ulp(ref.abs() + fn, dtype)


def finite(*ts) -> bool:
    return all(bool(torch.isfinite(t).all()) for t in ts if t is not None)


def centred(x, center):
    """-> (xc, exc): the (centred) row in f64 and the absolute error of the kernel's copy of it (R4)."""
    X = x.double()
    if not center:
        return X, torch.zeros_like(X)
    D = X.shape[-1]
    em = gam(nch(D) + 9) * X.abs().mean(-1, keepdim=True)
    xc = X - X.mean(-1, keepdim=True)
    return xc, em * (1 + U) + U * xc.abs()


def row_stats(x, eps, center=False):
    """-> (xc, exc, rs [.., 1], e_rs [.., 1]) of R1 - R4."""
    xc, exc = centred(x, center)
    D = xc.shape[-1]
    ss = (xc * xc).sum(-1, keepdim=True)
    dss = (2 * xc.abs() * exc + exc * exc).sum(-1, keepdim=True)
    arg = ss / D + eps
    rho = (dss + gam(D + 1) * (ss + dss)) / D / arg + gam(2)
    return xc, exc, torch.rsqrt(arg), (1 + 0.5 * rho / (1 - rho)) * (1 + 2 * U) - 1


def _rows(v, rpb, M, D, fill):
    """A per-sample [B, D] vector (or None) as [M, D] f64."""
    if v is None:
        return torch.full((1, D), fill, dtype=torch.float64)
    return v.double().repeat_interleave(rpb, 0)


def norm_fwd_ref(x, w, shift, scale, rpb, eps, center, out_dtype):
    """x [M,D] f32, w [D] or None, shift / scale [B,D] or None -> dict(y, by, rstd, brstd)."""
    M, D = x.shape
    xc, exc, rs, e_rs = row_stats(x, eps, center)
    W = torch.ones(D, dtype=torch.float64, device=x.device) if w is None else w.double()
    sc1 = _rows(scale, rpb, M, D, 0.0).to(x.device) + 1
    sh = _rows(shift, rpb, M, D, 0.0).to(x.device)
    core = (W * sc1).abs()
    k = 1 + (w is not None) + 2 * (scale is not None) + (shift is not None)
    mag = (xc.abs() + exc) * rs * (1 + e_rs) * core
    fn = core * rs * (exc * (1 + e_rs) + xc.abs() * e_rs) + gam(k) * (mag + sh.abs())
    y = xc * rs * W * sc1 + sh
    return dict(y=y, by=stored(y, fn, out_dtype), rstd=rs[:, 0], brstd=(e_rs * rs)[:, 0])


def colsum_bound(term, eterm, K, groups, old=None):
    """B5: term / eterm [M, D] summed in `groups` equal row groups -> (ref [groups, D], bound)."""
    assert K >= 4, "the sum_bound form needs K >= 4 (gemm_check.py)"
    D = term.shape[-1]
    t, e = term.reshape(groups, -1, D), eterm.reshape(groups, -1, D)
    ref, S, E = t.sum(1), t.abs().sum(1), e.sum(1)
    if old is not None:
        ref, S = ref + old.double(), S + old.double().abs()
    fn = E + acc_bound(S + E, K)
    return ref, fn + 0.5 * ulp(ref.abs() + fn, F32)


def norm_bwd_ref(dout, x, w, scale, rstd, rpb, center, dx_old=None, dw_old=None, y=None, gate=None):
    """dout [M,D] (T), x [M,D], w [D] or None, scale [B,D] or None, rstd [M] f32 as given, dx_old [M,D] (beta_x = 1) or None,
    dw_old [D] (beta_w = 1) or None; y [M,D] (T) and gate [B,D] for the gate-fused form.
    -> dict of f64 (ref, bound) pairs: dx, dshift, dscale [B,D], dw [D], and dy [M,D], dgate [B,D] with a gate."""
    M, D = x.shape
    B = M // rpb
    T = dout.dtype
    G = dout.double()
    rs = rstd.double()[:, None]
    xc, exc = centred(x, center)
    n = xc * rs
    en = rs * exc + U * rs * (xc.abs() + exc)
    N = n.abs() + en
    W = torch.ones(D, dtype=torch.float64, device=x.device) if w is None else w.double()
    sc1 = _rows(scale, rpb, M, D, 0.0).to(x.device) + 1
    ksc, kw = 2 * (scale is not None), int(w is not None)
    dn = G * sc1 * W
    edn = gam(ksc + kw) * dn.abs()
    DN = dn.abs() + edn
    dot = (dn * n).mean(-1, keepdim=True)
    edot = ((edn * N + dn.abs() * en).sum(-1, keepdim=True) + gam(D + 2) * (DN * N).sum(-1, keepdim=True)) / D
    DOT = dot.abs() + edot
    if center:
        msum = dn.mean(-1, keepdim=True)
        ems = (edn.sum(-1, keepdim=True) + gam(D + 1) * DN.sum(-1, keepdim=True)) / D
    else:
        msum, ems = torch.zeros_like(dot), torch.zeros_like(dot)
    d0 = (dn - n * dot - msum) * rs
    ed0 = rs * (edn + en * DOT + n.abs() * edot + ems) + gam(4) * rs * (DN + N * DOT + msum.abs() + ems)
    if dx_old is not None:
        old = dx_old.double()
        dx, edx = old + d0, ed0 + U * (old.abs() + d0.abs() + ed0)
    else:
        dx, edx = d0, ed0
    out = dict(dx=(dx, edx))
    out["dshift"] = colsum_bound(G, torch.zeros_like(G), rpb, B)
    out["dscale"] = colsum_bound(G * n * W, (G * W).abs() * (en + gam(2) * N), rpb, B)
    r, b = colsum_bound(G * sc1 * n, (G * sc1).abs() * (en + gam(ksc + 1) * N), M, 1, dw_old)
    out["dw"] = (r[0], b[0])
    if gate is not None:
        out.update(gate_bwd_ref(dx, edx, y, gate, rpb, T))
    return out


def gate_bwd_ref(dx, edx, y, gate, rpb, T):
    """B6 / B5: dx [M,D] f64 with error edx (0: an exact input), y [M,D] (T) or None, gate [B,D] or None -> dict(dy, dgate)."""
    M, D = dx.shape
    gr = _rows(gate, rpb, M, D, 1.0).to(dx.device)
    dy = dx * gr
    fn = gr.abs() * edx + (U * gr.abs() * (dx.abs() + edx) if gate is not None else 0.0)
    out = dict(dy=(dy, stored(dy, fn, T)))
    if y is not None:
        Y = y.double()
        out["dgate"] = colsum_bound(dx * Y, Y.abs() * (edx + U * (dx.abs() + edx)), rpb, M // rpb)
    return out


def stored_colsum(name, got, stored_rows, K=None):
    """B7: `got` against the f64 column sums of the rows as stored."""
    X = stored_rows.double()
    ref, S = X.sum(0), X.abs().sum(0)
    bound = sum_bound(ref, S, K or X.shape[0], F32)
    assert finite(ref, bound), f"{name}: reference or bound not finite"
    return check(name, got, ref, bound)


# ----------------------------------------------------------------------------- RoPE
def rope_ref(t, cos, sin, transposed=False, e_t=0.0):
    """t [..., N, hd] f64, cos / sin [N, hd] independent per element -> (ref, fn): Q2 with the relative error e_t of t."""
    c, s = cos.double(), sin.double()
    te, to = t[..., 0::2], t[..., 1::2]
    ce, co, se, so = c[:, 0::2], c[:, 1::2], s[:, 0::2], s[:, 1::2]
    if transposed:
        oe, oo = te * ce + to * so, to * co - te * se
        ae, ao = (te * ce).abs() + (to * so).abs(), (to * co).abs() + (te * se).abs()
    else:
        oe, oo = te * ce - to * se, to * co + te * so
        ae, ao = (te * ce).abs() + (to * se).abs(), (to * co).abs() + (te * so).abs()
    ref = torch.stack([oe, oo], -1).reshape(t.shape)
    A = torch.stack([ae, ao], -1).reshape(t.shape)
    return ref, ((1 + e_t) * (1 + gam(2)) - 1) * A


def qk_fwd_ref(x, w, cos, sin, eps, out_dtype):
    """x [B,H,N,hd] (one of the q | k slots, head-major view), w [hd] or None (RoPE only), cos / sin [N,hd] -> (ref, bound)."""
    X = x.double()
    if w is None:
        ref, fn = rope_ref(X, cos, sin)
    else:
        _, _, rs, e_rs = row_stats(x, eps)
        ref, fn = rope_ref(X * rs * w.double(), cos, sin, e_t=(1 + e_rs) * (1 + gam(2)) - 1)
    return ref, stored(ref, fn, out_dtype)


def qk_bwd_ref(g, x, w, cos, sin, eps, out_dtype):
    """g [B,H,N,hd] (dq or dk as stored), x the pre-norm row or None, w [hd] or None -> (ref, bound) of the dqkv slot."""
    return ac.qknorm_bwd_bound(g.double(), torch.zeros_like(g, dtype=torch.float64), x, w, cos, sin, eps, out_dtype=out_dtype)


def qk_dw_ref(g, x, w, cos, sin, eps, old=None):
    """-> (ref [hd], bound) of dwq (dwk): the sum over all B H N items of t n."""
    hd = g.shape[-1]
    _, tn = ac.qknorm_bwd_op(g.double(), x, w, cos, sin, eps)
    _, ta = ac.qknorm_bwd_op(g.double().abs(), x, w, cos, sin, eps, absolute=True)
    _, _, _, e_rs = row_stats(x, eps)
    e = ((1 + gam(3)) * (1 + e_rs) * (1 + gam(2)) - 1) * ta
    ref, b = colsum_bound(tn.reshape(-1, hd), e.reshape(-1, hd), tn.numel() // hd, 1, old)
    return ref[0], b[0]


# ----------------------------------------------------------------------------- inputs
def tables(N, hd, gen):
    """Independent per-element cos / sin tables: no two neighbouring values equal, so a swapped pair, a swapped c.x / c.y, the adjoint in
    place of the forward or row n +- 1 each changes the result."""
    a = torch.rand(2, N, hd, generator=gen) * 6.28
    return a[0].cos().contiguous(), (0.3 + 0.7 * a[1].sin()).contiguous()


def hot(t, gen, k=3, f=50.0):
    """A few columns at 50 x magnitude, as real residual streams have: the per-element bound then varies across the row."""
    D = t.shape[-1]
    idx = torch.randperm(D, generator=gen)[:min(k, D)]
    t[..., idx] *= f
    return t
