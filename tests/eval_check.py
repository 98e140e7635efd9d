"""Per-element references and error bounds for the evaluation kernels: csrc/inception.hip (FID), csrc/adm_eval.hip (ADM evaluator) and the
tokenizer evaluation of csrc/tokenizer_eval.hip (LPIPS pre-processing and head, SSIM, quantiser, SSE), in the manner of row_check.py and
layer_check.py.

Every check is |got - ref| <= bound for EVERY element (gemm_check.check), `ref` in f64 (80-bit long double for the kernels that themselves
accumulate in f64) from the operands AS STORED and from the definition of the operation, never from the kernel's order of operations.
u = 2^-24 (gemm_check.U), u64 = 2^-53, gam(n) = n u / (1 - n u) (row_check.gam); `Fl` (layer_check) carries (value, error bound) and
adds one rounding per operation; `/` and sqrtf round once (layer_check E1), expf is C_EXPF u relative on [-87, 88] (layer_check, measured
there with csrc/probe/intrinsic_probe) with the absolute floor TINY where it underflows.  No constant of this module is measured anew.

Rules per entry point (each restates the kernel line it covers).
conv2d_nhwc_f32 (conv_igemm_f32_kernel): `acc[i][j][r] + bn` after K = kh kw Cin MFMA products of which the padded ones are exact zeros:
  sum_bound(ref, S, K, f32), S = |x| * |w| + |bias| (gemm_check: every term passes through at most K - 1 additions, the bias add and
  one product rounding; K + 1 <= 2 K).  fmaxf(v, 0) is 1-Lipschitz and exact: the bound is unchanged.
pool2d_nhwc_f32: mode 0 `acc = fmaxf(acc, v)` over the in-image taps from -inf: exact, compared by bits.  mode 1 `acc += v` over the n <= k^2
  in-image taps in order from 0.f (the first add is exact: depth n - 1), then `acc / (float)n`: one rounding.
global_avgpool_nhwc_f32: `s += p[j ldx]`, HW terms in order (depth HW - 1), `s / (float)HW`: one rounding.
fid_preprocess: shf = (float)H / (float)Ho is the correctly rounded f32 quotient (taken as such).  sy = max(shf (oy + 0.5) - 0.5, 0): oy + 0.5 is
  exact, the product and the subtraction round (a contraction only removes one): |dsy| <= 2 u (|sy| + 1/2).  The interpolant is continuous and
  piecewise linear in (sy, sx), so moving the coordinate -- even across a tap boundary, where y0 changes -- moves it by at most
  dsy Ly + dsx Lx, Ly (Lx) the largest difference of vertically (horizontally) adjacent pixel values / 255 in the 5 x 5 neighbourhood of the
  reference's own first tap.  On top of that the roundings of the kernel line AT THE KERNEL'S OWN coordinate, whose taps may be the
  neighbours of the reference's: every quantity lies in [0, 1], so each rounding is at most u whatever the taps: v / 255 (1), ly0 = 1 - ly1
  (1; ly1 = sy - y0 is exact), lx0 v00 + lx1 v01 (3 on top of the 2 inherited per term: 5), the second lerp (3 + 5 + 1 = 9), `v * 2.f`
  exact (18), `- 1.f` (1): 20 u in all, the same for every element.
fid_stats_accumulate: (double)x - (double)s rounds once in f64; sum[d] += the serial sum of n such terms: (n + 2) u64 (|old| + sum |x - s|).
  cross[i, j] += n fma steps: (n + 2) u64 (|old| + sum |y_i| |y_j| (1 + 2 u64)).  cross must come out bitwise symmetric when it went in so.
adm_preprocess: the kernel states its arithmetic with contraction off; `adm_preprocess_f32` restates it operation by operation in numpy
  float32: equal bits.  adm_spatial_tap: a copy: equal bits.
row_sqnorms_f32: f64 fma chain of ceil(D / 64) terms per lane and 6 butterfly steps: gam64(ceil(D / 64) + 6) ref, then `(float)s`: half an f32 ulp.
pairwise_logits: sum_bound(ref, |u| |w|^T, D, f32).
knn_radii / pr_flags: d = fmaxf(__fadd_rn(__fsub_rn(nu, 2.f * acc), nv), 0.f) with nu, nv THE F32 NORMS PASSED IN: acc carries
  acc_bound(|u| |v|^T, D); `2.f * acc` is exact; the subtraction and the addition round once each; the clamp is 1-Lipschitz: `pair_dist`
  returns (d, e) that way with Fl.  The k-th smallest of values each within e of d lies in
  [k-th smallest of max(d - e, 0), k-th smallest of d + e]: `knn_interval`.  A flag must be 1 if some j has d + e <= r, must be 0 if every j
  has max(d - e, 0) > r, and is undecided otherwise: `pr_decide`.
adm_softmax_is (is_softmax_kernel and the two column-sum kernels): t = x - mx rounds once (|t| u absolute, mx itself is exact); E = expf(t):
  relative expm1((|t| + C_EXPF) u), absolute floor TINY; s = the sum of the positive E: ceil(C / 256) terms per thread, 6 butterfly steps and
  2 adds of the four waves; p = E / s: one rounding.  So (test_gpu_conv_vae.py's derivation) p has relative error
  rel_c = (1 + dE_c) (1 + u) / ((1 - max_c dE_c) (1 - gam(depth))) - 1 and absolute floor 2 TINY (s >= 1): dp.  h = sum_c p log p in f64 of
  the kernel's f32 p: |d (p log p)| <= max |1 + log xi| dp over [p - dp, p + dp]; where p itself may have underflowed (p < 2^-100) the term
  is at most |b log b|, b = p + dp, an absolute term; plus 8 (ceil(C / 256) + 8) u64 sum |p log p| for log, product and the f64 sum.
  S[s, c]: sum of dp over the split's rows plus (rows + 2) u64 S.
lpips_prep / lpips_prep_f16: (src - shift) / scale with f32 literals: two roundings (Fl); the 16-bit form then clamps to +-65504 (1-Lipschitz)
  and rounds once: half an f16 ulp (row_check.stored).  The padding channels are exact zeros: compared by bits.
lpips_layer / lpips_layer_f16 and ssim: restated line by line with Fl in the docstrings of `lpips_layer_ref` and `ssim_ref` / `_blur` /
  `ssim_gauss` below.  Equal halves add exactly 0 to `out` and a constant image gives exactly 1: compared by bits.
recon_quantize_psnr / sse_u8: `quantize_f32` restates png_quantize in numpy float32 (product and sum rounded separately, clamp, truncation);
  the SSE is an integer: equality.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as Fn

from gemm_check import BoundError, U, acc_bound, check, sum_bound, ulp  # noqa: F401  (re-exported for the tests)
from layer_check import C_EXPF, C_LOGF, Fl, TINY, finite, fsum, gam, stored  # noqa: F401

F32, F16, F64 = torch.float32, torch.float16, torch.float64
U64 = 2.0 ** -53
LD = np.longdouble


# ----------------------------------------------------------------------------- convolution
def conv_out(H, W, kh, kw, sh, sw, ph, pw):
    return (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1


def conv_ref(x, w, bias, sh, sw, ph, pw, relu):
    """x [B,H,W,Cin], w [Cout,kh,kw,Cin] (k = (ky kw + kx) Cin + c), bias [Cout] or None -> (ref, bound, pre-activation) [B,Ho,Wo,Cout]."""
    X, Wt = x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2)
    b = None if bias is None else bias.double()
    pre = Fn.conv2d(X, Wt, b, (sh, sw), (ph, pw))
    S = Fn.conv2d(X.abs(), Wt.abs(), None if b is None else b.abs(), (sh, sw), (ph, pw))
    K = w.shape[1] * w.shape[2] * w.shape[3]
    bound = sum_bound(pre, S, K, F32)
    ref = pre.clamp_min(0.0) if relu else pre
    return ref.permute(0, 2, 3, 1).contiguous(), bound.permute(0, 2, 3, 1).contiguous(), pre.permute(0, 2, 3, 1).contiguous()


# ----------------------------------------------------------------------------- pools
def _windows(x, k, s, p, fill):
    """x [B,H,W,C] f64 -> (taps [B,Ho,Wo,C,k*k] with `fill` outside the image, inside [1,Ho,Wo,1,k*k] bool), taps in the kernel's (dy, dx) order."""
    B, H, W, C = x.shape
    xp = Fn.pad(x.permute(0, 3, 1, 2), (p, p, p, p), value=fill)
    mp = Fn.pad(torch.ones(1, 1, H, W, dtype=F64), (p, p, p, p), value=0.0)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    t = xp.unfold(2, k, s).unfold(3, k, s)[:, :, :Ho, :Wo].reshape(B, C, Ho, Wo, k * k).permute(0, 2, 3, 1, 4)
    m = mp.unfold(2, k, s).unfold(3, k, s)[:, :, :Ho, :Wo].reshape(1, 1, Ho, Wo, k * k).permute(0, 2, 3, 1, 4)
    return t, m > 0


def maxpool_exact(x, k, s, p):
    """f32 in, f32 out: the maximum of the in-image taps (exact in any order)."""
    t, m = _windows(x.double(), k, s, p, -math.inf)
    assert bool(m.any(-1).all())
    return t.max(-1).values.float()


def avgpool_ref(x, k, s, p):
    t, m = _windows(x.double(), k, s, p, 0.0)
    n = m.sum(-1).double()
    assert bool((n > 0).all())
    depth = (n - 1).clamp_min(0)                            # per pixel: the taps inside the image
    g = depth * U / (1 - depth * U)
    q = Fl(t.sum(-1), g * t.abs().sum(-1)) / Fl(n.expand_as(t[..., 0]))
    return q.v, q.e


def global_avgpool_ref(x):
    """x [B,HW,C] -> (ref, bound) [B,C]."""
    X = x.double()
    HW = X.shape[1]
    q = Fl(X.sum(1), gam(HW - 1) * X.abs().sum(1)) / Fl(float(HW))
    return q.v, q.e


# ----------------------------------------------------------------------------- FID pre-processing
def _fid_axis(n_in, n_out):
    """-> (s f64 [n_out] from the f32 scale, ds, lo index, hi index, l1) of the ATen rule."""
    scale = float(np.float32(n_in) / np.float32(n_out))
    o = torch.arange(n_out, dtype=F64)
    raw = scale * (o + 0.5) - 0.5
    s = raw.clamp_min(0.0)
    ds = 2 * U * (raw.abs() + 0.5)
    i0 = s.floor().long().clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    l1 = (s - i0).clamp(0.0, 1.0)
    return s, ds, i0, i1, l1


def fid_preprocess_ref(img, Ho, Wo):
    """img [B,H,W,3] uint8 -> (ref, bound) [B,Ho,Wo,3]."""
    B, H, W, _ = img.shape
    _, dsy, y0, y1, ly1 = _fid_axis(H, Ho)
    _, dsx, x0, x1, lx1 = _fid_axis(W, Wo)
    V = img.double() / 255.0
    def tap(yi, xi):
        return V[:, yi][:, :, xi]
    LY1, LX1 = ly1[None, :, None, None], lx1[None, None, :, None]
    top = (1.0 - LX1) * tap(y0, x0) + LX1 * tap(y0, x1)
    bot = (1.0 - LX1) * tap(y1, x0) + LX1 * tap(y1, x1)
    ref = 2.0 * ((1.0 - LY1) * top + LY1 * bot) - 1.0
    # continuity across tap boundaries: the Lipschitz constants of the interpolant near the reference's taps
    P = (img.double() / 255.0).permute(0, 3, 1, 2)
    dy = torch.zeros_like(P)
    dx = torch.zeros_like(P)
    if H > 1:
        dy[:, :, :-1] = (P[:, :, 1:] - P[:, :, :-1]).abs()
    if W > 1:
        dx[:, :, :, :-1] = (P[:, :, :, 1:] - P[:, :, :, :-1]).abs()
    Ly = Fn.max_pool2d(dy, 5, 1, 2)[:, :, y0][:, :, :, x0].permute(0, 2, 3, 1)
    Lx = Fn.max_pool2d(dx, 5, 1, 2)[:, :, y0][:, :, :, x0].permute(0, 2, 3, 1)
    lip = 2.0 * (dsy[None, :, None, None] * Ly + dsx[None, None, :, None] * Lx) * (1 + 8 * U)
    return ref, torch.full_like(ref, 20 * U) + lip


# ----------------------------------------------------------------------------- ADM pre-processing (exact)
def adm_preprocess_f32(img, Ho, Wo, half_pixel=False):
    """The kernel's f32 arithmetic in numpy float32, operation by operation (numpy never contracts).  img [B,H,W,3] uint8 numpy."""
    f = np.float32
    B, H, W, _ = img.shape
    shf, swf = f(H) / f(Ho), f(W) / f(Wo)
    oy, ox = np.arange(Ho, dtype=np.float32), np.arange(Wo, dtype=np.float32)
    if half_pixel:                                          # the planted fault: half-pixel centres
        sy, sx = np.maximum((oy + f(0.5)) * shf - f(0.5), f(0)), np.maximum((ox + f(0.5)) * swf - f(0.5), f(0))
    else:
        sy, sx = oy * shf, ox * swf
    fy, fx = np.floor(sy), np.floor(sx)
    y0, x0 = np.minimum(fy.astype(np.int64), H - 1), np.minimum(fx.astype(np.int64), W - 1)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    yl, xl = (sy - fy)[None, :, None, None], (sx - fx)[None, None, :, None]
    I = img.astype(np.float32)
    tl, tr = I[:, y0][:, :, x0], I[:, y0][:, :, x1]
    bl, br = I[:, y1][:, :, x0], I[:, y1][:, :, x1]
    top = tl + (tr - tl) * xl
    bot = bl + (br - bl) * xl
    v = top + (bot - top) * yl
    out = (v - f(128.0)) * f(0.0078125)
    assert out.dtype == np.float32
    return out


# ----------------------------------------------------------------------------- f64 reductions (reference in long double)
def check64(name, got, ref, bound):
    """got f64 numpy, ref long double, bound f64: every element; returns the worst ratio."""
    g = np.asarray(got, dtype=np.float64)
    err = np.abs(g.astype(LD) - ref).astype(np.float64)
    err = np.where(np.isfinite(g), err, np.inf)
    b = np.asarray(bound, dtype=np.float64)
    assert np.isfinite(b).all() and np.isfinite(np.asarray(ref, dtype=np.float64)).all(), f"{name}: reference or bound not finite"
    ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    if not worst <= 1.0:
        idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise BoundError(f"{name}: {int((~(ratio <= 1.0)).sum())} of {ratio.size} elements out of bound; worst at {idx}: got {g[idx]!r}, "
                         f"ref {float(ref[idx])!r}, |diff| {err[idx]:.3e} > bound {b[idx]:.3e} (x{worst:.3g})")
    return worst


def fid_stats_ref(x, shift, sum_old, cross_old):
    """x [n,D] f32, shift [D] f32, old contents f64 (numpy) -> dict sum / cross -> (ref long double, bound)."""
    Y = x.astype(LD) - shift.astype(LD)[None, :]
    n = x.shape[0]
    A = np.abs(Y).astype(np.float64)
    s_ref = sum_old.astype(LD) + Y.sum(0)
    s_b = (n + 2) * U64 * (np.abs(sum_old) + A.sum(0))
    c_ref = cross_old.astype(LD) + Y.T @ Y
    c_b = (n + 2) * U64 * (np.abs(cross_old) + (A.T @ A) * (1 + 2 * U64))
    return dict(sum=(s_ref, s_b), cross=(c_ref, c_b))


def row_sqnorms_ref(x):
    X = x.double()
    ref = (X * X).sum(-1)
    e = (math.ceil(X.shape[-1] / 64) + 6) * U64 * ref * 2
    return ref, e + 0.5 * ulp(ref + e, F32)


# ----------------------------------------------------------------------------- pairwise
def logits_ref(u, w):
    A, B = u.double(), w.double()
    ref, S = A @ B.T, A.abs() @ B.abs().T
    return ref, sum_bound(ref, S, u.shape[1], F32)


def pair_dist(u, nu, v, nv):
    """-> (d, e) [M,N]: the clamped squared distance from the f32 norms as passed, and the bound of the kernel's error."""
    A, B = u.double(), v.double()
    dot = Fl(A @ B.T, acc_bound(A.abs() @ B.abs().T, u.shape[1]))
    t = (Fl(nu.double()[:, None]) - dot.exact_scale(2.0)) + Fl(nv.double()[None, :])
    return t.v.clamp_min(0.0), t.e


def knn_interval(d, e, nhood):
    """-> (lo, hi) [N, nk]: the interval of the nhood[t]-th smallest (0-based) of each row."""
    lo = (d - e).clamp_min(0.0).sort(-1).values
    hi = (d + e).sort(-1).values
    idx = torch.tensor(list(nhood), dtype=torch.long)
    return lo[:, idx], hi[:, idx]


def check_interval(name, got, lo, hi):
    """lo <= got <= hi for every element; returns the worst |got - mid| / half width (0 / 0 counts as 0)."""
    g = got.double()
    ok = torch.isfinite(g) & (g >= lo) & (g <= hi)
    if not bool(ok.all()):
        idx = tuple(int(i) for i in (~ok).nonzero()[0])
        raise BoundError(f"{name}: {int((~ok).sum())} of {ok.numel()} outside their interval; first at {idx}: got {float(g[idx])!r}, "
                         f"interval [{float(lo[idx])!r}, {float(hi[idx])!r}]")
    half = (hi - lo) / 2
    dev = (g - (lo + hi) / 2).abs()
    r = torch.where(half > 0, dev / half.clamp_min(1e-300), torch.zeros_like(dev))
    return float(r.max()) if r.numel() else 0.0


def pr_decide(d, e, r_cols, r_rows):
    """d, e [M,N]; r_cols [N,nk] (radii of the columns), r_rows [M,nk] -> (u_must1, u_must0, v_must1, v_must0) bool [M,nk] / [N,nk]."""
    dl, dh = (d - e).clamp_min(0.0), (d + e).clamp_min(0.0)
    u1 = (dh[:, :, None] <= r_cols.double()[None, :, :]).any(1)
    u0 = (dl[:, :, None] > r_cols.double()[None, :, :]).all(1)
    v1 = (dh[:, :, None] <= r_rows.double()[:, None, :]).any(0)
    v0 = (dl[:, :, None] > r_rows.double()[:, None, :]).all(0)
    return u1, u0, v1, v0


def check_flags(name, got, must1, must0, cap=0.01):
    """got int [*, nk]: exactly 0 / 1, 1 where must1, 0 where must0; at most `cap` undecided.  Returns the undecided fraction."""
    assert bool(((got == 0) | (got == 1)).all()), f"{name}: a flag is neither 0 nor 1"
    assert not bool((must1 & must0).any()), f"{name}: reference contradicts itself"
    bad = (must1 & (got != 1)) | (must0 & (got != 0))
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise BoundError(f"{name}: {int(bad.sum())} of {bad.numel()} decided flags wrong; first at {idx}: got {int(got[idx])}")
    und = float((~(must1 | must0)).double().mean())
    if und > cap:
        raise BoundError(f"{name}: {und:.3%} of the flags undecided (cap {cap:.0%})")
    return und


# ----------------------------------------------------------------------------- softmax + Inception Score sums
def softmax_is_ref(logits, split):
    """logits [M,C] f32 -> dict p (ref, bound) torch f64; h / S -> (ref long double numpy, bound numpy)."""
    X = logits.double()
    M, C = X.shape
    t = X - X.max(-1, keepdim=True).values
    E = torch.exp(t)
    dE = torch.expm1((t.abs() + C_EXPF) * U)
    depth = math.ceil(C / 256) + 8
    s = E.sum(-1, keepdim=True)
    p = E / s
    rel = (1 + dE) * (1 + U) / ((1 - dE.max(-1, keepdim=True).values) * (1 - gam(depth))) - 1
    dp = p * rel + 2 * TINY
    # h
    pl = p.numpy().astype(LD)
    plogp = np.where(pl > 0, pl * np.log(np.where(pl > 0, pl, 1.0)), 0.0)
    h_ref = plogp.sum(-1)
    lo, hi = (p - dp).clamp_min(1e-300), p + dp
    slope = torch.maximum((1 + lo.log()).abs(), (1 + hi.log()).abs())
    term = torch.where(p < 2.0 ** -100, (hi * hi.log()).abs() + (p * p.clamp_min(1e-300).log()).abs(), slope * dp)
    h_b = term.sum(-1) + 8 * depth * U64 * torch.from_numpy(np.abs(plogp).sum(-1).astype(np.float64))
    # S
    ns = (M + split - 1) // split
    S_ref = np.zeros((ns, C), dtype=LD)
    S_b = torch.zeros(ns, C, dtype=F64)
    for q in range(ns):
        r0, r1 = q * split, min((q + 1) * split, M)
        S_ref[q] = pl[r0:r1].sum(0)
        S_b[q] = dp[r0:r1].sum(0) + (r1 - r0 + 2) * U64 * (p[r0:r1].sum(0) + dp[r0:r1].sum(0))
    return dict(p=(p, dp), h=(h_ref, h_b.numpy()), S=(S_ref, S_b.numpy()))


# ----------------------------------------------------------------------------- LPIPS pre-processing
LP_SHIFT = (-0.030, -0.088, -0.188)
LP_SCALE = (0.458, 0.448, 0.450)


def lpips_prep_ref(in0, in1, dtype):
    """in0 / in1 [B,3,H,W] f32 -> (ref, bound) [2B,H,W,3] for the three real channels."""
    x = torch.cat([in0, in1], 0).double().permute(0, 2, 3, 1)
    sh = torch.tensor([float(np.float32(v)) for v in LP_SHIFT], dtype=F64)
    sc = torch.tensor([float(np.float32(v)) for v in LP_SCALE], dtype=F64)
    q = (Fl(x) - Fl(sh)) / Fl(sc)
    if dtype == F32:
        return q.v, q.e
    ref = q.v.clamp(-65504.0, 65504.0)
    return ref, stored(ref, q.e, F16)


# ----------------------------------------------------------------------------- quantiser (exact)
def quantize_f32(x, nearest=False):
    """png_quantize in numpy float32: x float32 array -> uint8."""
    f = np.float32
    v = (f(127.5) * x.astype(np.float32)).astype(np.float32) + f(128.0)
    v = np.minimum(np.maximum(v, f(0)), f(255))
    if nearest:                                             # the planted fault
        v = np.rint(v)
    return v.astype(np.int32).astype(np.uint8)


def sse_exact(a8, b8):
    """a8 / b8 [B, n] uint8 numpy -> int64 [B]."""
    d = a8.astype(np.int64) - b8.astype(np.int64)
    return (d * d).reshape(d.shape[0], -1).sum(-1)


# ----------------------------------------------------------------------------- LPIPS head of one tap
def lpips_chunks(HW):
    return min(128, max(1, (HW + 511) // 512))


def lpips_layer_ref(f, lw, old, B):
    """f [2B,HW,C] as stored (f32 or f16, widened exactly), lw [C], old [B] f32 (the seeded contents of `out`) -> (ref, bound) [B].
    lpips_layer_kernel line by line (contraction off: every product and sum rounds): L = min(64, C / 4) lanes per pixel, V = C / (4 L)
    float4 per lane.  s0 / s1: one rounded square per channel, 4 V terms per lane in a chain, log2 L butterfly steps.  r = 1 / (sqrtf(s) +
    1e-10f): three roundings.  dx = a r0 - c r1: two rounded products and the subtraction; w dx dx: two products; d: 4 V terms per lane and the
    butterfly.  acc: the thread's ceil(HW / (chunks PPB)) pixels in a chain (the other lanes add exact zeros), 6 wave butterfly steps and the
    four wave sums from 0.f.  lpips_finish_kernel: the chunks in f64 (chunks u64), / HW in f64, one rounding to f32, and `out[b] +=`: one more."""
    F = f.double()
    C, HW = F.shape[-1], F.shape[1]
    L = min(64, C // 4)
    V = C // (4 * L)
    lg = int(math.log2(L))
    a, c = Fl(F[:B]), Fl(F[B:])
    s0, s1 = (a * a).sum(-1, 4 * V + lg, keepdim=True), (c * c).sum(-1, 4 * V + lg, keepdim=True)
    eps = float(np.float32(1e-10))
    r0, r1 = 1.0 / (s0.sqrt() + eps), 1.0 / (s1.sqrt() + eps)
    dx = a * r0 - c * r1
    d = ((Fl(lw) * dx) * dx).sum(-1, 4 * V + lg)                 # [B, HW]
    chunks, PPB = lpips_chunks(HW), 256 // L
    depth = -(-HW // (chunks * PPB)) + 6 + 4
    # the exact value: the definition in f64 (not Fl's own value, which is the same expression)
    n0, n1 = F[:B] / ((F[:B] ** 2).sum(-1, keepdim=True).sqrt() + 1e-10), F[B:] / ((F[B:] ** 2).sum(-1, keepdim=True).sqrt() + 1e-10)
    dref = (lw.double() * (n0 - n1) ** 2).sum(-1)
    assert float((dref - d.v).abs().max()) <= 1e-9 * (1 + float(dref.abs().max()))
    tot = d.sum(-1, depth)                                       # every partial and their f64 sum; non-negative terms
    mean = Fl(tot.v / HW, tot.e / HW + (chunks + 2) * U64 * tot.v / HW)
    mean = Fl(mean.v, mean.e + U * mean.mag())                   # (float)(s / HW)
    out = Fl(old.double()) + mean
    return out.v, out.e


# ----------------------------------------------------------------------------- SSIM
SS_T, SS_R = 32, 5


def ssim_gauss():
    """-> (g f64 [11], eg): the normalised Gaussian of the definition and the bound of the host's f32 copy (expf 1 ulp, the rounded
    argument (3 roundings of a value <= 5.6: 6 u relative on the result), 10 additions, one division: 20 u relative in all)."""
    d = (torch.arange(11, dtype=F64) - 5) / 1.5
    g = torch.exp(-(d * d) / 2)
    g = g / g.sum()
    return g, 20 * U * g


def ssim_consts(data_range):
    f = np.float32
    return float((f(0.01) * f(data_range)) * (f(0.01) * f(data_range))), float((f(0.03) * f(data_range)) * (f(0.03) * f(data_range)))


def _blur(q: Fl, G: Fl, dim):
    """11 taps along `dim`: `s += g * q` eleven times from 0.f: two roundings per term at most (one if contracted), a chain of 11."""
    w = q.v.unfold(dim, 11, 1), q.e.unfold(dim, 11, 1)
    terms = Fl(w[0], w[1]) * G
    return terms.sum(-1, 11)


def ssim_ref(X, Y, lo, hi, data_range):
    """X, Y [B,C,H,W] f32 -> (ref, bound) [B]: torchmetrics' SSIM (11-tap Gaussian, sigma 1.5, valid region) of the clamped images in f64,
    with the bound of ssim_tile_kernel's shifted evaluation propagated per output pixel, tile by tile (the shift differs per tile)."""
    B, C, H, W = X.shape
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    c1, c2 = ssim_consts(data_range)
    g, eg = ssim_gauss()
    G = Fl(g, eg)
    Xc, Yc = X.double().clamp(lo, hi).reshape(B * C, H, W), Y.double().clamp(lo, hi).reshape(B * C, H, W)
    tot_v, tot_e = torch.zeros(B * C, dtype=F64), torch.zeros(B * C, dtype=F64)
    ntiles = 0
    for oy0 in range(SS_R, H - SS_R, SS_T):
        for ox0 in range(SS_R, W - SS_R, SS_T):
            ntiles += 1
            y1, x1 = min(oy0 + SS_T + SS_R, H), min(ox0 + SS_T + SS_R, W)
            shx, shy = Xc[:, oy0, ox0][:, None, None], Yc[:, oy0, ox0][:, None, None]
            xs, ys = Fl(Xc[:, oy0 - SS_R:y1, ox0 - SS_R:x1]) - Fl(shx), Fl(Yc[:, oy0 - SS_R:y1, ox0 - SS_R:x1]) - Fl(shy)
            m = [_blur(_blur(q, G, 2), G, 1) for q in (xs, ys, xs * xs, ys * ys, xs * ys)]
            vx = m[2] - m[0] * m[0]
            vy = m[3] - m[1] * m[1]
            vx, vy = Fl(vx.v.clamp_min(0.0), vx.e), Fl(vy.v.clamp_min(0.0), vy.e)          # fmaxf(., 0): 1-Lipschitz
            cxy = m[4] - m[0] * m[1]
            mx, my = m[0] + Fl(shx), m[1] + Fl(shy)
            num = ((mx * my).exact_scale(2.0) + c1) * (cxy.exact_scale(2.0) + c2)
            den = (mx * mx + my * my + c1) * (vx + vy + c2)
            s = num / den
            blk = s.sum((1, 2), (SS_T * SS_T) // 256 + 6 + 4)
            tot_v, tot_e = tot_v + blk.v, tot_e + blk.e
    count = C * (H - 2 * SS_R) * (W - 2 * SS_R)
    v = tot_v.reshape(B, C).sum(-1) / count
    e = tot_e.reshape(B, C).sum(-1) / count + (C * ntiles + 2) * U64 * tot_v.abs().reshape(B, C).sum(-1) / count
    return v, e + U * (v.abs() + e)


def ssim_plain(X, Y, lo, hi, data_range):
    """The unshifted definition in f64 (the cross-check of ssim_ref's value)."""
    B, C, H, W = X.shape
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    g, _ = ssim_gauss()
    k = (g[:, None] * g[None, :])[None, None]
    x, y = X.double().clamp(lo, hi).reshape(B * C, 1, H, W), Y.double().clamp(lo, hi).reshape(B * C, 1, H, W)
    mx, my = Fn.conv2d(x, k), Fn.conv2d(y, k)
    vx, vy, cxy = Fn.conv2d(x * x, k) - mx * mx, Fn.conv2d(y * y, k) - my * my, Fn.conv2d(x * y, k) - mx * my
    s = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx.clamp_min(0) + vy.clamp_min(0) + c2))
    return s.reshape(B, -1).mean(-1)
