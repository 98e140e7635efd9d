"""References and error bounds for the guidance rules (csrc/guidance.hip: ldmae_guidance_combine; ldmae_amd/guidance.py), in the manner of
kid_check.py: every reference is an f64 numpy restatement of the DEFINITION (include/ldmae_hip.h), computed from the operands as stored and
from the scalars as the kernel receives them (float32(scale), float32(phi), ...), never from the kernel's order of operations.

Arrays are [B, C, H, W]; the first k channels of each sample are guided (n = k H W elements), the rest of the result is p.  Sums run over the
n guided elements of ONE sample.  Time convention x_t = t x1 + (1 - t) x0, v = x1 - x0, data prediction u = x + (1 - t) p.

    cfg      g = q + s (p - q)
    rescale  g0 = cfg; g = g0 (phi std(p) / std(g0) + 1 - phi), std unbiased (ddof 1); std(g0) == 0: g = g0
    apg      d = (p - q) + beta m_prev; u = x + (1 - t) p; gamma = min(1, r / ((1 - t) |d|)) when r > 0 and the denominator > 0, else 1;
             par = (<d, u> / <u, u>) u, zero when <u, u> == 0; g = p + (s - 1) gamma (d - (1 - eta) par); the new momentum is d

THE BOUND (guidance_bound).  u = 2^-24 (unit round-off of f32), u64 = 2^-53.  |v| is the exact (f64) magnitude; e_v bounds the error of the
kernel's f32 value of v.  A rounding of a result of exact value v costs at most u |v| (first order; the factor SLACK = 1 + 2^-10 on the final
bound covers every product of two error terms not written out below, all of which are below u times a term that is written out).

cfg.  dq = fl(p - q): e <= u |p - q|.  g = fl(s dq + q), one fma: e_cfg = |s| u |p - q| + u |g|.

rescale.  g0 as cfg: e_g0 = e_cfg.  The kernel's std(g0) is the std of its OWN f32 values g0~; std is a seminorm, std(a) = |a - mean(a)|_2 /
sqrt(n - 1), so |std(g0~) - std(g0)| <= |g0~ - g0|_2 / sqrt(n - 1) <= sqrt(sum e_g0^2 / (n - 1)) =: E.  std(p) has no such term (p is an
input).  Each variance comes from f64 sums of the shifted values (v - v_0) and their squares, (S2 - S1^2 / n) / (n - 1): S2 is a sum of n
non-negative terms, relative error <= n u64; S1^2 / n <= S2 (Cauchy-Schwarz) with relative error <= 2 n u64; the subtraction, division and
the square root add a few u64: |d var| <= (3 n + 8) u64 S2 / (n - 1), so a std has relative error v64 = (3 n + 8) u64 S2 / ((n - 1) var) / 2
+ 2 u64 from the sums (S2 bounded here by the sum of squares about the first element, in f64).  ratio = std(p) / std(g0):
e_ratio = ratio (E / (std(g0) - E) + v64_p + v64_g + 4 u64).  f = fl32(1 + phi (ratio - 1)): e_f = phi e_ratio + u |f|.  g = fl(g0~ f~):
e = |f| e_g0 + |g0| e_f + u |g|.  (std(g0) <= E: the bound is infinite -- that is the degenerate case, checked exactly elsewhere.)

apg.  omt = fl(1 - t): e <= u |1 - t|.  dq = fl(p - q): u |p - q|; d = fl(beta m_prev + dq) (only when beta != 0): e_d = u |p - q| + u |d|,
and e_d = u |p - q| when beta == 0 (m_prev is an operand as stored).  u~ = fl(omt~ p + x): e_u = u |1 - t| |p| + u |u|.
Sums in f64 of exact products of f32 values: only the (n + 8) u64 accumulation term on top of the propagated operand errors:
    e_dd = sum (2 |d| e_d + e_d^2) + (n + 8) u64 sum d^2          e_uu likewise        e_du = sum (|d| e_u + |u| e_d + e_d e_u) + (n + 8) u64 sum |d u|
c = du / uu: e_c = (e_du + |c| e_uu) / (uu - e_uu).  |d| = sqrt(dd): e_norm = sqrt(dd) - sqrt(max(dd - e_dd, 0)) (sqrt is concave).
den = (1 - t) |d|: e_den = |1 - t| e_norm + u |den| + 4 u64 |den|.  gamma = min(1, r / den), min is 1-Lipschitz:
e_gamma = r e_den / (den (den - e_den)) (0 when r == 0 or den == 0, where gamma is exactly 1 on both sides; when r / (den + e_den) >= 1 both
sides are exactly 1 as well).  a = fl32((s - 1) gamma): e_a = |s - 1| e_gamma + u |a|.  b = fl32((1 - eta) c): e_b = |1 - eta| e_c + u |b|.
w = fl(d~ - b~ u~), one fma: e_w = e_d + |b| e_u + |u| e_b + e_b e_u + u |w|.  g = fl(p + a~ w~), one fma: e = |a| e_w + |w| e_a + e_a e_w + u |g|.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -10


def f32(v):
    return float(np.float32(v))


def _guided(a, k):
    """[B, C, H, W] -> f64 [B, n] of the first k channels."""
    a = np.asarray(a, np.float64)
    return a[:, :k].reshape(a.shape[0], -1)


def _finish(p, g, k):
    out = np.asarray(p, np.float64).copy()
    out[:, :k] = g.reshape(out[:, :k].shape)
    return out


def _std(v):
    return np.sqrt(((v - v.mean(1, keepdims=True)) ** 2).sum(1) / (v.shape[1] - 1))


def cfg_ref(p, q, s, k):
    P, Q = _guided(p, k), _guided(q, k)
    return _finish(p, Q + f32(s) * (P - Q), k)


def rescale_ref(p, q, s, k, phi):
    P, Q = _guided(p, k), _guided(q, k)
    g0 = Q + f32(s) * (P - Q)
    sp, sg = _std(P), _std(g0)
    ratio = np.where(sg > 0, sp / np.where(sg > 0, sg, 1.0), 1.0)
    fac = np.where(sg > 0, f32(phi) * ratio + 1.0 - f32(phi), 1.0)
    return _finish(p, g0 * fac[:, None], k)


def apg_parts(p, q, x, t, s, k, eta, r, beta, m_prev=None):
    """-> dict of the f64 quantities of the definition, all [B, n] or [B]."""
    P, Q, X = _guided(p, k), _guided(q, k), _guided(x, k)
    omt = (1.0 - np.asarray(t, np.float32).astype(np.float64))[:, None]
    d = P - Q
    if f32(beta) != 0.0:
        d = d + f32(beta) * np.asarray(m_prev, np.float64).reshape(d.shape)
    u = X + omt * P
    dd, du, uu = (d * d).sum(1), (d * u).sum(1), (u * u).sum(1)
    den = omt[:, 0] * np.sqrt(dd)
    on = (f32(r) > 0) & (den > 0)
    gamma = np.where(on, np.minimum(1.0, f32(r) / np.where(on, den, 1.0)), 1.0)
    c = np.where(uu > 0, du / np.where(uu > 0, uu, 1.0), 0.0)
    par = c[:, None] * u
    w = d - (1.0 - f32(eta)) * par
    g = P + (f32(s) - 1.0) * gamma[:, None] * w
    return dict(P=P, Q=Q, omt=omt, d=d, u=u, dd=dd, du=du, uu=uu, den=den, gamma=gamma, c=c, par=par, w=w, g=g)


def apg_ref(p, q, x, t, s, k, eta=0.0, r=0.0, beta=0.0, m_prev=None):
    """-> (g [B, C, H, W] f64, the new momentum d [B, n] f64)."""
    a = apg_parts(p, q, x, t, s, k, eta, r, beta, m_prev)
    return _finish(p, a["g"], k), a["d"]


def guidance_ref(rule, p, q, s, k, x=None, t=None, phi=0.7, eta=0.0, r=0.0, beta=0.0, m_prev=None):
    if rule == "cfg":
        return cfg_ref(p, q, s, k)
    if rule == "rescale":
        return rescale_ref(p, q, s, k, phi)
    return apg_ref(p, q, x, t, s, k, eta, r, beta, m_prev)[0]


def _cfg_bound(P, Q, s):
    g0 = Q + s * (P - Q)
    return g0, abs(s) * U * np.abs(P - Q) + U * np.abs(g0)


def guidance_bound(rule, p, q, s, k, x=None, t=None, phi=0.7, eta=0.0, r=0.0, beta=0.0, m_prev=None):
    """Per-element bound [B, C, H, W] (f64) of |kernel - reference| by the module docstring's derivation; 0 on the pass-through channels
    (they are p bit for bit).  apg: also the bound of the stored momentum, -> (bound, bound_m [B, n])."""
    s = f32(s)
    P, Q = _guided(p, k), _guided(q, k)
    n = P.shape[1]
    full = np.zeros(np.asarray(p).shape, np.float64)

    def place(e):
        full[:, :k] = (SLACK * e).reshape(full[:, :k].shape)
        return full

    if rule == "cfg":
        return place(_cfg_bound(P, Q, s)[1])
    if rule == "rescale":
        phi = f32(phi)
        g0, e0 = _cfg_bound(P, Q, s)
        sp, sg = _std(P), _std(g0)
        E = np.sqrt((e0 ** 2).sum(1) / (n - 1))

        def v64(v, sd):
            s2 = ((v - v[:, :1]) ** 2).sum(1)
            with np.errstate(divide="ignore", invalid="ignore"):
                return (3 * n + 8) * U64 * s2 / ((n - 1) * sd ** 2) / 2 + 2 * U64
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = sp / sg
            e_ratio = np.where(sg > E, ratio * (E / (sg - E) + v64(P, sp) + v64(g0, sg) + 4 * U64), np.inf)
        fac = phi * ratio + 1.0 - phi
        e_f = phi * e_ratio + U * np.abs(fac)
        g = g0 * fac[:, None]
        return place(np.abs(fac)[:, None] * e0 + np.abs(g0) * e_f[:, None] + U * np.abs(g))
    a = apg_parts(p, q, x, t, s, k, eta, r, beta, m_prev)
    eta, r, beta = f32(eta), f32(r), f32(beta)
    omt, d, u = np.abs(a["omt"]), a["d"], a["u"]
    e_d = U * np.abs(P - Q) + (U * np.abs(d) if beta != 0.0 else 0.0)
    e_u = U * omt * np.abs(P) + U * np.abs(u)
    acc = (n + 8) * U64
    e_dd = (2 * np.abs(d) * e_d + e_d ** 2).sum(1) + acc * a["dd"]
    e_uu = (2 * np.abs(u) * e_u + e_u ** 2).sum(1) + acc * a["uu"]
    e_du = (np.abs(d) * e_u + np.abs(u) * e_d + e_d * e_u).sum(1) + acc * np.abs(d * u).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_c = np.where(a["uu"] > e_uu, (e_du + np.abs(a["c"]) * e_uu) / (a["uu"] - e_uu), np.where(a["uu"] == 0, 0.0, np.inf))
        e_norm = np.sqrt(a["dd"]) - np.sqrt(np.maximum(a["dd"] - e_dd, 0.0))
        den = np.abs(a["den"])
        e_den = omt[:, 0] * e_norm + (U + 4 * U64) * den
        settled = (r == 0.0) | (den == 0.0) | (r >= den + e_den)           # gamma is exactly 1 on both sides
        e_gamma = np.where(settled, 0.0, np.where(den > e_den, r * e_den / (den * (den - e_den)), np.inf))
    ca, cb = (s - 1.0) * a["gamma"], (1.0 - eta) * a["c"]
    e_a = abs(s - 1.0) * e_gamma + U * np.abs(ca)
    e_b = abs(1.0 - eta) * e_c + U * np.abs(cb)
    w = a["w"]
    e_w = e_d + np.abs(cb)[:, None] * e_u + np.abs(u) * e_b[:, None] + e_b[:, None] * e_u + U * np.abs(w)
    e_g = np.abs(ca)[:, None] * e_w + np.abs(w) * e_a[:, None] + e_a[:, None] * e_w + U * np.abs(a["g"])
    return place(e_g), SLACK * e_d


def worst_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound, an element with bound 0 must match exactly (ratio 0 then, else inf); inf where got is not
    finite."""
    g, r_, b = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    err = np.abs(g - r_)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(g), ratio, np.inf)
    return float(ratio.max())
