"""Per-element references and error bounds for csrc/vmae.hip and csrc/pointwise.hip (colsum, casts, thin GEMMs,
multi_add, embedders, AdamW / EMA), in the manner of row_check.py.

Every check is |got - ref| <= bound for EVERY element (gemm_check.check).  `ref` is f64, computed from the operands AS STORED (16-bit inputs
widened exactly; host scalars as the f32 values the entry point rounds them to) and from the mathematical definition of the operation
(oracle/mae.py, oracle/dit.py, oracle/train.py, torch.nn.functional in f64), never from the kernel's order of operations.

How a bound is built.  u = 2^-24 (gemm_check.U); gam(n) = n u / (1 - n u) bounds (1 + u)^n - 1 (row_check.gam).  `Fl` carries a pair (v, e):
the f64 value of a quantity and a bound e of the absolute error of the kernel's f32 copy of it.  Every arithmetic operation on Fl values
propagates the operand errors exactly (products: |a| eb + |b| ea + ea eb; quotients and roots: the worst slope over the operand's
interval) and then adds ONE rounding, u (|v| + e): so a bound written with Fl is literally the count of roundings readable in the kernel
line it restates.  A product contracted into the following add (fmaf, or the compiler's contraction) only removes a rounding.
  E1. `+ - *`: one rounding each (IEEE).  `/` and sqrtf: one rounding each -- derived, not measured: device code is compiled with the
      compiler's default -fhip-fp32-correctly-rounded-divide-sqrt (the option text of `hipcc --help`; csrc/Makefile does not turn it off).
  E2. rsqrtf: 2 u relative (the 2 u of attn_check.py, "Fused backward", as row_check R3): taken from that document, not measured.
  E3. sums (`Fl.sum`, `fsum`): n terms added in SOME association whose longest chain of additions is `depth` deep:
      e = sum e_i + gam(depth) sum (|t_i| + e_i).  depth = n - 1 holds for every association; the device tests pass the depth readable in
      the kernel (below), the CPU emulations that of the association they emulate.
  E4. a 16-bit output adds half an ulp of its type at the stored value (row_check.stored); an f32 output adds nothing.
Which constants are derived, taken from a document, or measured: E1 (derived from IEEE arithmetic and the compiler default), E2 and
the 1.5e-7 of the 16-bit GELU's erf (taken from attn_check.py / gemm_check.ERF_AS), S1 and the 2 |x| u of __expf (derived), and the seven C_* constants of
v_exp, expf, logf, cosf, sinf, erff and v_rcp (MEASURED: no document shipped with the toolchain states them; value, range and margin stand
next to each constant below, "device math functions").

Rules per family (depths are those of the kernels; NV = ceil(D / 64)).
LayerNorm forward (layernorm_fwd_kernel)
  L1. mu = group_sum<16>(s) * invD: hsum of a float4 (2 deep), `s +=` over NV chunks, 4 butterfly steps: depth NV + 6; invD = fl(1 / D)
      carries u / D and the product rounds once.
  L2. v = sum (x - mu)^2: one subtraction and one product per term, 4 NV terms per lane and 4 butterfly steps: depth 4 NV + 4;
      `* invD + eps`: two roundings; rsqrtf: E2.  mean and rstd are stored as computed.
  L3. y = ((x - mu) * rs) * w + b: four roundings on top of the inherited errors, then E4.
LayerNorm backward (layernorm_bwd_kernel, ln_reduce_kernel), a function of (dout, x, w, mean, rstd, dx_accum, dw, db) AS GIVEN
  L4. xh = (x - mu) * rs, gy = g * w; s1 = sum gy * invD, s2 = sum (gy * xh) * invD: per lane 4 NV terms, 4 butterfly steps: depth 4 NV + 4.
  L5. dx = old + rs * ((gy - s1) - xh * s2); dx_cast = the same value rounded to T (E4).
  L6. dw = beta old + sum_m g xh, db = beta old + sum_m g: per lane ceil(128 / 16) = 8 rows, 16 row groups through LDS, then the G = ceil(M / 128)
      partial rows by lanes (ceil(G / 64) deep) and a 6-step butterfly, `beta * q` and its add: depth 8 + 16 + ceil(G / 64) + 6 + 1.
colsum (colsum_kernel + group_reduce): exact terms; rows of a group by `nsub` streams (ceil(rows / nsub) deep) folded in order (nsub - 1),
  the G groups by RL = 8 (32 from G = 256 on) row lanes (ceil(G / RL)) folded in order (RL - 1), beta (1): colsum_depth.
restore_tokens: one f32 add -> bit exact.  restore_tokens_bwd: kept rows are copies -> bit exact; the mask-token gradient is a sum of the
  masked rows (exact terms): a lane's rows, 16 row groups, then colsum over the workgroups (restore_depth); no masked row -> exactly 0.
thin_nt: acc = bias; K fmaf steps; + pos: depth K + 1 with one product rounding per term allowed for (an unfused build), then E4.
thin_tn: sum over M rows of g t (+ beta old): thin_tn_depth (512 rows in order per chunk, the chunks by lanes and a butterfly), one product
  rounding per term.
conv3x3 forward / dx: bias + 9 C products in some order: depth 9 C; dw / db: sums over the B H W pixels: conv_bwd_depth.
mae_loss_fwd: the sum over pixels of m (a - c)^2 and of (1 - m) (a - c)^2: per term a subtraction, a square, the 4-pixel hsum (2), the two
  products with m; then per thread ceil(n4 / (256 G)) float4 terms, 6 butterfly steps, the 4 waves (2): `depth` is passed in.  Non-negative
  terms: the error is relative to the sum itself.
mae_loss_bwd: 2 (cm m + cv (1 - m)) (a - c): restated with Fl.
latent_prologue with sample = 0: ((m - mu) / sd) * mult, or (m - mu) * mult, restated with Fl.
adamw_ema: every line of adamw_ema_kernel restated with Fl on the host scalars as rounded to f32 (the struct AdamArgs); m and v carry their
  errors into p and ema.  ema_only: ema d + a p.
label_embed_bwd: old + the sum of at most B rows, added per 256-sample pass: depth <= (hits) + (passes).
GELU / tanh-GELU / SwiGLU / SiLU, forward and backward, the timestep embedding and latent_prologue with sample = 1: each kernel line restated
  with Fl, the device functions through `mono` with their constants (fexp, rcp1p, tanh_exp, _erf), constants of the definition as f32
  literals (K), saturation by S1.  cos / sin: the absolute error of the argument t f_j passes with slope <= 1, so it grows with |t f_j|.
Bit exact (asserted as equality of bits in the device tests, no bound): random_masking, gather_rows / scatter_rows, patch_gather, the
casts (one rounding of the source = torch's .to()), multi_add, label_embed_fwd, restore_tokens, the zero column of an odd timestep embedding.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as Fn

from gemm_check import BoundError, U, acc_bound, check, sum_bound, ulp  # noqa: F401  (re-exported for the tests)
from row_check import finite, gam, stored  # noqa: F401

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
F64 = torch.float64


def f32(v: float) -> float:
    """A host double as the f32 value the entry point rounds it to."""
    return float(np.float32(v))


def _t(x):
    return x.double() if isinstance(x, torch.Tensor) else torch.tensor(float(x), dtype=F64)


class Fl:
    """(v, e): the f64 value of a quantity and a bound of the absolute error of the kernel's f32 copy.  Each operation rounds once (E1)."""

    def __init__(self, v, e=None):
        self.v = _t(v)
        self.e = torch.zeros_like(self.v) if e is None else _t(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, Fl) else Fl(x)

    @staticmethod
    def _r(v, e):
        return Fl(v, e + U * (v.abs() + e))

    def mag(self):
        return self.v.abs() + self.e

    def __add__(self, o):
        o = Fl.of(o)
        return Fl._r(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = Fl.of(o)
        return Fl._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Fl.of(o) - self

    def __mul__(self, o):
        o = Fl.of(o)
        return Fl._r(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Fl.of(o)
        lo = (o.v.abs() - o.e).clamp_min(1e-300)          # smallest |denominator| of the interval
        q = self.v / o.v
        return Fl._r(q, (self.e + q.abs() * o.e) / lo)

    def __rtruediv__(self, o):
        return Fl.of(o) / self

    def sqrt(self):
        lo = (self.v - self.e).clamp_min(0.0)
        e = torch.minimum(self.e / (self.v.sqrt() + lo.sqrt()).clamp_min(1e-300), self.e.sqrt())
        return Fl._r(self.v.sqrt(), e)

    def rsqrt(self):
        """E2: 2 u relative on top of the slope 1/2 t^(-3/2) at the low end of the interval."""
        lo = (self.v - self.e).clamp_min(1e-300)
        v = self.v.rsqrt()
        e = 0.5 * self.e * lo.pow(-1.5)
        return Fl(v, e + 2 * U * (v + e))

    def exact_scale(self, c):
        """Multiplication by a power of two (or 0 / 1): no rounding."""
        return Fl(self.v * c, self.e * abs(c))

    def sum(self, dim, depth, keepdim=False):
        """E3."""
        return Fl(self.v.sum(dim, keepdim=keepdim), self.e.sum(dim, keepdim=keepdim) + gam(depth) * self.mag().sum(dim, keepdim=keepdim))


def nv(D: int) -> int:
    return (D + 63) // 64


# ----------------------------------------------------------------------------- LayerNorm
def ln_fwd_ref(x, w, b, eps, out_dtype, d_mean=None, d_var=None):
    """x [M,D] f32, w / b [D] -> dict of (ref, bound): y (out_dtype), mean, rstd.  d_mean / d_var: the depths of L1 / L2 (default: the kernel's)."""
    M, D = x.shape
    d_mean = nv(D) + 6 if d_mean is None else d_mean
    d_var = 4 * nv(D) + 4 if d_var is None else d_var
    invD = Fl(1.0 / D, U / D)
    X = Fl(x)
    mu = X.sum(-1, d_mean, keepdim=True) * invD
    # the reference is the definition: mean and variance of the row in f64; Fl's own values ARE those (Fl never reorders)
    c = X - mu
    var = (c * c).sum(-1, d_var, keepdim=True) * invD + f32(eps)
    rs = var.rsqrt()
    y = (c * rs) * Fl(w) + Fl(b)
    return dict(y=(y.v, stored(y.v, y.e, out_dtype)), mean=(mu.v[:, 0], mu.e[:, 0]), rstd=(rs.v[:, 0], rs.e[:, 0]))


def ln_bwd_depth(M: int) -> int:
    G = (M + 127) // 128
    return 8 + 16 + (G + 63) // 64 + 6 + 1


def ln_bwd_ref(dout, x, w, mean, rstd, dx_old, dw_old, db_old, beta_w, d_row=None, d_col=None):
    """dout [M,D] (T), x [M,D], w [D], mean / rstd [M] f32 AS GIVEN, dx_old [M,D], dw_old / db_old [D] (used when beta_w = 1)
    -> dict of (ref, bound): dx, dx_cast (T = dout.dtype; meaningful for 16-bit T), dw, db."""
    M, D = x.shape
    d_row = 4 * nv(D) + 4 if d_row is None else d_row
    d_col = ln_bwd_depth(M) if d_col is None else d_col
    invD = Fl(1.0 / D, U / D)
    g, mu, rs = Fl(dout), Fl(mean[:, None]), Fl(rstd[:, None])
    xh = (Fl(x) - mu) * rs
    gy = g * Fl(w)
    s1 = gy.sum(-1, d_row, keepdim=True) * invD
    s2 = (gy * xh).sum(-1, d_row, keepdim=True) * invD
    dx = Fl(dx_old) + rs * ((gy - s1) - xh * s2)
    dw = (g * xh).sum(0, d_col)
    db = g.sum(0, d_col)
    if beta_w != 0.0:
        assert beta_w == 1.0
        dw = Fl(dw.v + dw_old.double(), dw.e + gam(1) * (dw.mag() + dw_old.double().abs()))
        db = Fl(db.v + db_old.double(), db.e + gam(1) * (db.mag() + db_old.double().abs()))
    T = dout.dtype
    return dict(dx=(dx.v, dx.e), dx_cast=(dx.v, stored(dx.v, dx.e, T)), dw=(dw.v, dw.e), db=(db.v, db.e))


# ----------------------------------------------------------------------------- column sums
def colsum_rows(M: int, N: int) -> int:
    """colsum_rows of csrc/pointwise.hip: rows summed by one workgroup."""
    groups = max(512 // ((N + 1023) // 1024), 1)
    rows, r = (M + groups - 1) // groups, 8
    while r < rows and r < 256:
        r <<= 1
    return r


def colsum_depth(M: int, N: int) -> int:
    """The longest chain of additions of ldmae_colsum: a row stream (ceil(rows / nsub)), the nsub streams folded in order, then group_reduce
    (RL = 32 row lanes from 256 groups on, else 8: ceil(G / RL) deep, RL folded in order) and the `beta * old +` add."""
    rows = colsum_rows(M, N)
    G = -(-M // rows)
    last = N // 4 - ((N + 1023) // 1024 - 1) * 256
    d = 0
    for ncol4 in {min(N // 4, 256), last}:
        nsub = 256 // ncol4
        d = max(d, -(-min(rows, M) // nsub) + nsub - 1)
    RL = 32 if G >= 256 else 8
    return d + -(-G // RL) + RL


def colsum_ref(x, old=None, depth=None):
    """x [M,N] as stored (any float type), old [N] (beta = 1) or None -> (ref, bound); depth: default the kernel's (colsum_depth)."""
    X = x.double()
    M, N = X.shape
    ref, S = X.sum(0), X.abs().sum(0)
    if old is not None:
        ref, S = ref + old.double(), S + old.double().abs()
    return ref, gam(colsum_depth(M, N) if depth is None else depth) * S


def fsum(terms: Fl, dim, depth, old=None):
    """E3 on an Fl, plus `+ old` (one more level) -> (ref, bound)."""
    s = terms.sum(dim, depth)
    if old is not None:
        s = Fl(s.v + old.double(), s.e + gam(1) * (s.mag() + old.double().abs()))
    return s.v, s.e


# ----------------------------------------------------------------------------- restore_tokens
def restore_ref(x, mtok, pos, ids, keep):
    """out[b, l] = (ids < keep ? x[b, ids] : mtok) + pos[l], in f32 (one correctly rounded add: compare bits)."""
    B, L = ids.shape
    D = x.shape[-1]
    cat = torch.cat([x.view(B, keep, D), mtok.view(1, 1, D).expand(B, L - keep, D)], 1)        # models_mae.py:536-541
    return torch.gather(cat, 1, ids[:, :, None].expand(B, L, D)) + pos.view(1, L, D)


def restore_depth(rows: int, D: int) -> int:
    """restore_tokens_bwd_kernel: a lane's rows, the 16 row groups through LDS, then ldmae_colsum over the workgroups' partial rows."""
    grid = min(max((rows + 15) // 16, 1), 2048)
    return -(-rows // (16 * grid)) + 16 + colsum_depth(grid, D)


def restore_bwd_ref(dout, ids, keep, depth=None):
    """-> (dx [B,keep,D] f32 exact copy, (dmask ref, bound)); depth: default the kernel's (restore_depth)."""
    B, L = ids.shape
    D = dout.shape[-1]
    g = dout.view(B, L, D)
    kept = ids < keep
    dx = torch.zeros(B, keep, D, dtype=dout.dtype, device=dout.device)
    bi = torch.arange(B, device=dout.device)[:, None].expand(B, L)
    dx[bi[kept], ids[kept]] = g[kept]
    masked = g[~kept].double()
    depth = restore_depth(B * L, D) if depth is None else depth
    return dx, (masked.sum(0), gam(depth) * masked.abs().sum(0))


# ----------------------------------------------------------------------------- thin GEMMs
def thin_nt_ref(T, W, bias, pos, rpb, out_dtype):
    """out[m, n] = sum_k T[m, k] W[n, k] + bias[n] + pos[m % rpb, n] -> (ref, bound)."""
    A, B = T.double(), W.double()
    M, K = A.shape
    ref, S = A @ B.T, A.abs() @ B.abs().T
    if bias is not None:
        ref, S = ref + bias.double(), S + bias.double().abs()
    if pos is not None:
        p = pos.double()[torch.arange(M, device=T.device) % rpb]
        ref, S = ref + p, S + p.abs()
    return ref, stored(ref, gam(K + 2) * S, out_dtype)


def thin_tn_depth(M: int) -> int:
    """thin_tn_kernel + thin_reduce_kernel: a workgroup's <= 512 rows in order, the chunks by lanes (ceil(chunks / 64)), a 6-step butterfly, beta."""
    return min(M, 512) + -(-((M + 511) // 512) // 64) + 6 + 1


def thin_tn_ref(G, T, dW_old=None, db_old=None, depth=None):
    """dW[n, k] = sum_m G[m, n] T[m, k] (+ old), dbias[n] = sum_m G[m, n] (+ old) -> ((ref, bound), (ref, bound)); one product rounding
    per term of dW on top of `depth` (default thin_tn_depth)."""
    g, t = G.double(), T.double()
    M = thin_tn_depth(g.shape[0]) if depth is None else depth
    rw, Sw = g.T @ t, g.abs().T @ t.abs()
    rb, Sb = g.sum(0), g.abs().sum(0)
    if dW_old is not None:
        rw, Sw = rw + dW_old.double(), Sw + dW_old.double().abs()
    if db_old is not None:
        rb, Sb = rb + db_old.double(), Sb + db_old.double().abs()
    return (rw, gam(M + 1) * Sw), (rb, gam(M) * Sb)


# ----------------------------------------------------------------------------- conv3x3
def conv_ref(x, w, b):
    X, Wt = x.double().cpu(), w.double().cpu()
    C = Wt.shape[0]
    bb = None if b is None else b.double().cpu()
    ref = Fn.conv2d(X, Wt, bb, padding=1)
    S = Fn.conv2d(X.abs(), Wt.abs(), None if bb is None else bb.abs(), padding=1)
    return ref, gam(9 * C + 2) * S


def conv_bwd_depth(npix: int) -> int:
    """conv3x3_bwd_dw_kernel + conv3x3_bwd_reduce_kernel: a thread's pixels, 6 butterfly steps, the 4 waves (2), then the G partial rows by
    256 threads, 6 butterfly steps and the 4 waves (2)."""
    G = min((npix + 255) // 256, 1024)
    return -(-npix // (256 * G)) + 8 + -(-G // 256) + 8


def conv_bwd_ref(dout, x, w, want_dx=True, depth=None):
    """-> dict of (ref, bound) on the CPU: dx (or absent), dw [C,C,3,3], db [C]; depth of the pixel sums: default conv_bwd_depth."""
    g, X, Wt = dout.double().cpu(), x.double().cpu(), w.double().cpu()
    B, C, H, Wd = g.shape
    K = conv_bwd_depth(B * H * Wd) if depth is None else depth
    out = {}
    if want_dx:
        out["dx"] = (Fn.conv_transpose2d(g, Wt, padding=1), gam(9 * C + 1) * Fn.conv_transpose2d(g.abs(), Wt.abs(), padding=1))
    xp = Fn.pad(X, (1, 1, 1, 1))
    dw, Sw = torch.zeros(C, C, 3, 3, dtype=F64), torch.zeros(C, C, 3, 3, dtype=F64)
    for ky in range(3):
        for kx in range(3):
            win = xp[:, :, ky:ky + H, kx:kx + Wd]
            dw[:, :, ky, kx] = torch.einsum("nohw,nihw->oi", g, win)
            Sw[:, :, ky, kx] = torch.einsum("nohw,nihw->oi", g.abs(), win.abs())
    out["dw"] = (dw, gam(K + 1) * Sw)
    out["db"] = (g.sum((0, 2, 3)), gam(K) * g.abs().sum((0, 2, 3)))
    return out


# ----------------------------------------------------------------------------- MAE loss
def _pixel_mask(mask, B, C, H, W, p):
    """mask [B, (H/p) (W/p)] -> [B, C, H, W]: the mask value of the patch a pixel lies in (row-major patches, W / p per row)."""
    return mask.double().view(B, 1, H // p, 1, W // p, 1).expand(B, C, H // p, p, W // p, p).reshape(B, C, H, W)


def mae_loss_fwd_ref(pred, img, mask, p, depth):
    """-> (ref [2], bound [2]): sum m d^2 and sum (1 - m) d^2 over all pixels; `depth`: the longest chain of additions."""
    B, C, H, W = pred.shape
    m = _pixel_mask(mask, B, C, H, W, p)
    d2 = (pred.double() - img.double()) ** 2
    ref = torch.stack([(m * d2).sum(), ((1 - m) * d2).sum()])
    S = torch.stack([(m.abs() * d2).sum(), ((1 - m).abs() * d2).sum()])
    # per term: a - c, the square, 1 - m, the product with the mask factor: 4 roundings (two of them doubled by the square: 3 u for d^2)
    return ref, gam(depth + 5) * S


def mae_loss_depth(n4: int, groups: int) -> int:
    return 2 + -(-n4 // (256 * groups)) + 6 + 2


def mae_loss_bwd_ref(pred, img, mask, coef, p):
    B, C, H, W = pred.shape
    m = Fl(_pixel_mask(mask, B, C, H, W, p))
    cm, cv = Fl(coef[0]), Fl(coef[1])
    k = (cm * m + cv * (1.0 - m)).exact_scale(2.0)
    out = k * (Fl(pred) - Fl(img))
    return out.v, out.e


# ----------------------------------------------------------------------------- latent prologue (sample = 0)
def latent_ref(lat, lmean, lstd, mult):
    """lat [B,C,HW], lmean / lstd [C] or None -> (ref, bound) of ((lat - mean) / std) * mult."""
    v = Fl(lat)
    if lstd is not None:
        v = (v - Fl(lmean[None, :, None])) / Fl(lstd[None, :, None])
    v = v * f32(mult)
    return v.v, v.e


# ----------------------------------------------------------------------------- optimizer
def adam_scalars(step, lr, beta1, beta2, eps, wd, ema_decay, grad_scale):
    """The struct AdamArgs of ldmae_adamw_ema: python doubles rounded to f32 at the point of use (torch/optim/adamw.py _single_tensor_adamw)."""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return dict(decay_mul=f32(1.0 - lr * wd), w1=f32(1.0 - beta1), beta2=f32(beta2), w2=f32(1.0 - beta2), bc2_sqrt=f32(math.sqrt(bc2)),
                eps=f32(eps), neg_step=f32(-(lr / bc1)), ema_d=f32(ema_decay), ema_a=f32(1.0 - ema_decay), gscale=f32(grad_scale))


def adamw_ref(p, g, m, v, ema, a, state=None):
    """One step as a function of (p, g, m, v, ema) as given; `state`: the Fl values (p, m, v, ema) of the previous step of a chain, whose
    errors then propagate.  -> dict name -> Fl (ema absent when ema is None)."""
    P, M_, V, E = state if state is not None else (Fl(p), Fl(m), Fl(v), None if ema is None else Fl(ema))
    gj = Fl(g) if a["gscale"] == 1.0 else Fl(g) * a["gscale"]
    P = P * a["decay_mul"]
    M_ = M_ + a["w1"] * (gj - M_)
    V = V * a["beta2"] + a["w2"] * (gj * gj)
    denom = V.sqrt() / a["bc2_sqrt"] + a["eps"]
    P = P + a["neg_step"] * (M_ / denom)
    out = dict(p=P, m=M_, v=V)
    if E is not None:
        out["ema"] = E * a["ema_d"] + a["ema_a"] * P
    return out


def ema_ref(ema, p, decay):
    e = Fl(ema) * f32(decay) + f32(1.0 - decay) * Fl(p)
    return e.v, e.e


# ----------------------------------------------------------------------------- label embedding
def label_rows(y, drop, num_classes):
    return y if drop is None else torch.where(drop.bool(), torch.full_like(y, num_classes), y)


def label_bwd_ref(dout, y, drop, old, num_classes):
    """dtable[r] = old[r] + sum_{b: row(b) == r} dout[b] -> (ref, bound); rows nobody hits have bound 0 (bit-equal to old)."""
    rows = label_rows(y, drop, num_classes)
    R, D = old.shape
    B = dout.shape[0]
    hit = torch.zeros(R, B, dtype=F64, device=dout.device)
    hit[rows, torch.arange(B, device=dout.device)] = 1.0
    g = dout.double()
    ref = old.double() + hit @ g
    S = old.double().abs() + hit @ g.abs()
    cnt = hit.sum(1, keepdim=True)
    depth = cnt + (B + 255) // 256                        # the hits in order, one `+=` per pass
    return ref, torch.where(cnt > 0, (depth * U / (1 - depth * U)) * S, torch.zeros_like(S))


# ----------------------------------------------------------------------------- random masking
def masking_ref(noise: torch.Tensor, keep: int):
    """models_mae.py random_masking with a STABLE argsort (numpy): -> ids_restore, mask, ids_keep."""
    nz = noise.cpu().numpy()
    shuffle = np.argsort(nz, axis=1, kind="stable")
    restore = np.argsort(shuffle, axis=1, kind="stable")
    mask = (restore >= keep).astype(np.float32)
    return torch.from_numpy(restore.astype(np.int64)), torch.from_numpy(mask), torch.from_numpy(shuffle[:, :keep].astype(np.int64))


def patch_gather_ref(img, ids, pos, p):
    """-> (tok [N*keep, C p p] f32, posg [N*keep, D]) : PatchEmbed's (c, i, j) order of the kept patches."""
    N, C, S, _ = img.shape
    grid = S // p
    pt = img.view(N, C, grid, p, grid, p).permute(0, 2, 4, 1, 3, 5).reshape(N, grid * grid, C * p * p)
    keep = ids.shape[1]
    tok = torch.gather(pt, 1, ids[:, :, None].expand(N, keep, C * p * p)).reshape(N * keep, -1)
    return tok, pos[ids.reshape(-1)]


# ----------------------------------------------------------------------------- device math functions (measured constants)
# MEASURED with csrc/probe/intrinsic_probe (each function alone on an MI355X against the f64 host function of the same f32 argument, 2^22
# arguments per range: half uniform, half log-spaced down to 1e-30, both signs, the ends and +-0).  Each constant is the measured worst
# error TIMES 2 (the factor 2: the measurement samples a finite grid), in units of u = 2^-24.
#   function        range            measured worst     constant
C_EXP2 = 2 * 1.384   # v_exp_f32     [-126, 128)        1.384 u relative   (at -29.938)
C_EXPF = 2 * 1.396   # expf          [-87, 88]          1.390 u relative; [-15, 10]: 1.396 u (at 0.0431): the larger
C_LOGF = 2 * 3.043   # logf          [1, 1e5]           3.043 u relative   (at 67248.76)
C_COS = 2 * 1.134    # cosf          [0, 1000]          1.134 u absolute   (at 567.86)
C_SIN = 2 * 1.168    # sinf          [0, 1000]          1.168 u absolute   (at 544.29)
C_ERFF = 2 * 1.387   # erff          [-8.5, 8.5]        1.387 u absolute   (at 0.966)
C_RCP = 2 * 1.535    # v_rcp_f32     [1, 1e30]          1.535 u relative   (at 7.08e22; [1, 4]: 1.534 u)
# The same run, for information (not used as constants): __expf on [-87, 88]: max (rel - 2 |x| u) = 1.281 u, below the 1.384 u of v_exp alone,
# which confirms the derived 2 |x| u; fast_sigmoid on [-87, 87]: 1.756 u absolute; tanh_exp on [-72, 72]: 3.162 u absolute; erf_as (the
# Abramowitz-Stegun 7.1.26 evaluation that served the 16-bit types until this suite) on [-8.5, 8.5]: 9.035 u = 5.4e-7 absolute (at -0.0497),
# MORE than the 1.5e-7 its comment stated (the error of the formula in exact arithmetic; the f32 evaluation adds the roundings of
# 1 - poly * exp).  erf_act now calls erff for every type (csrc/common.h).
# TAKEN FROM THE ISSUE / THE PROJECT'S COMMENT (gemm_check.ERF_AS): 1.5e-7 absolute for the erf of the 16-bit GELU kernels; not measured.  It
# is kept for them although they now call erff: it is the tighter of the two (2.52 u against C_ERFF = 2.77 u), and erff meets it (1.387 u).
C_ERF_AS = 1.5e-7 / U
# DERIVED: __expf(x) = v_exp(x * log2 e): the product and the f32 constant log2 e each move the argument y = x log2 e by |y| u, and
# exp2(y (1 + d)) = exp2(y) (1 + |y| ln 2 d): 2 |x| u relative on top of C_EXP2.  (The probe prints max (rel - 2 |x|) of __expf itself as a
# cross-check of this model; it is not used as a constant.)
# S1. saturation: v_exp and v_rcp flush denormal results, __expf / expf overflow to inf where the true value is still a finite f64.  Every
#     such value only ever enters 1 / (1 + E), 2 / (E + 1) or v / (1 + E), whose true value is then below 2^-126 (times |v|): `TINY` is
#     added as an ABSOLUTE error wherever a flushed or saturated value can arrive (derived from the formats, not measured).
TINY = 2.0 ** -125
FLT_MAX = 3.4028234663852886e38


def K(c: float) -> Fl:
    """A constant of the definition, as the f32 literal the kernel holds: relative error u."""
    return Fl(c, abs(c) * U)


def mono(x: Fl, f, rel=0.0, abs_=0.0, floor=0.0) -> Fl:
    """A monotone function of an Fl: the inherited error is the larger one-sided change of f over [v - e, v + e]; then rel u |f| + abs u + floor."""
    v = f(x.v)
    e = torch.maximum((f(x.v + x.e) - v).abs(), (f(x.v - x.e) - v).abs())
    return Fl(v, e + rel * U * (v.abs() + e) + abs_ * U + floor)


def fexp(x: Fl) -> Fl:
    """__expf: C_EXP2 + 2 |x| relative (derived above), TINY absolute (S1)."""
    return mono(x, torch.exp, rel=C_EXP2 + 2 * x.mag(), floor=TINY)


def rcp1p(E: Fl) -> Fl:
    """v_rcp(1 + E), E >= 0 (fast_sigmoid): the add, then C_RCP relative and S1."""
    D = 1.0 + E
    lo = (D.v - D.e).clamp_min(1.0)
    v = 1.0 / D.v
    e = D.e / (lo * D.v)
    return Fl(v, e + C_RCP * U * (v + e) + TINY)


def sigmoid_fast(a: Fl) -> Fl:
    return rcp1p(fexp(Fl(-a.v, a.e)))


def tanh_exp(u: Fl) -> Fl:
    """1 - 2 / (__expf(2 u) + 1) (csrc/vmae.hip): a correctly rounded division (E1) and S1."""
    D = fexp(u.exact_scale(2.0)) + 1.0
    q = 2.0 / D
    return 1.0 - Fl(q.v, q.e + TINY)


def _erf(x: Fl, dtype) -> Fl:
    """erf_act<T> = erff: C_ERFF for f32; the 16-bit kernels keep the stated 1.5e-7 (C_ERF_AS, the tighter figure); both absolute."""
    return mono(x, torch.special.erf, abs_=C_ERFF if dtype == F32 else C_ERF_AS)


R2 = 0.7071067811865476
RPI = 0.3989422804014327
KT = 0.7978845608028654


def gelu_fwd_ref(x):
    v = Fl(x)
    y = v.exact_scale(0.5) * (1.0 + _erf(v * K(R2), x.dtype))
    return y.v, stored(y.v, y.e, x.dtype)


def gelu_bwd_ref(dout, x):
    v, T = Fl(x), x.dtype
    cdf = (1.0 + _erf(v * K(R2), T)).exact_scale(0.5)
    pdf = K(RPI) * fexp(v.exact_scale(-0.5) * v)
    d = Fl(dout) * (cdf + v * pdf)
    return d.v, stored(d.v, d.e, T)


def _tanh_arg(v: Fl) -> Fl:
    return K(KT) * (v + ((K(0.044715) * v) * v) * v)


def gelu_tanh_fwd_ref(x):
    v = Fl(x)
    y = v.exact_scale(0.5) * (1.0 + tanh_exp(_tanh_arg(v)))
    return y.v, stored(y.v, y.e, x.dtype)


def gelu_tanh_bwd_ref(dout, x):
    v = Fl(x)
    t = tanh_exp(_tanh_arg(v))
    d = (1.0 + t).exact_scale(0.5) + ((v.exact_scale(0.5) * (1.0 - t * t)) * K(KT)) * (1.0 + (K(0.134145) * v) * v)
    # the definition's 3 * 0.044715 = 0.134145 exactly
    d = Fl(dout) * d
    return d.v, stored(d.v, d.e, x.dtype)


def swiglu_fwd_ref(h12):
    Hs = h12.shape[1] // 2
    a, b = Fl(h12[:, :Hs]), Fl(h12[:, Hs:])
    o = (a * sigmoid_fast(a)) * b
    return o.v, stored(o.v, o.e, h12.dtype)


def swiglu_bwd_ref(dhid, h12):
    Hs = h12.shape[1] // 2
    a, b, g = Fl(h12[:, :Hs]), Fl(h12[:, Hs:]), Fl(dhid)
    s = sigmoid_fast(a)
    da = ((g * b) * s) * (1.0 + a * (1.0 - s))
    db = (g * a) * s
    ref, fn = torch.cat([da.v, db.v], 1), torch.cat([da.e, db.e], 1)
    return ref, stored(ref, fn, h12.dtype)


def _sig_libm(v: Fl):
    """1 + expf(-v) (silu kernels): -> (E, D) with expf's C_EXPF and S1."""
    E = mono(Fl(-v.v, v.e), torch.exp, rel=C_EXPF, floor=TINY)
    return E, 1.0 + E


def silu_fwd_ref(x, out_dtype):
    v = Fl(x)
    _, D = _sig_libm(v)
    y = v / D
    fn = y.e + TINY * (1 + v.v.abs())                       # S1: expf -> inf gives -0 where the true value is |v| / E <= |v| / FLT_MAX
    return y.v, stored(y.v, fn, out_dtype)


def silu_bwd_ref(dy, x):
    v = Fl(x)
    _, D = _sig_libm(v)
    s = 1.0 / D
    s = Fl(s.v, s.e + TINY)
    d = (Fl(dy) * s) * (1.0 + v * (1.0 - s))
    return d.v, d.e


def timestep_ref(t, dim, max_period, wrong_div=None):
    """lightningdit.py:124-129: [cos(t f_j) | sin(t f_j) | 0], f_j = exp(-ln(max_period) j / half) -> (ref, bound)."""
    half = dim // 2
    j = torch.arange(half, dtype=F64, device=t.device)[None]
    L = mono(Fl(f32(max_period)), torch.log, rel=C_LOGF)
    arg = (Fl(-L.v, L.e) * j) / float(half if wrong_div is None else wrong_div)
    a = Fl(t[:, None]) * mono(arg, torch.exp, rel=C_EXPF)
    c, s = Fl(a.v.cos(), a.e + C_COS * U), Fl(a.v.sin(), a.e + C_SIN * U)          # |cos'|, |sin'| <= 1: the argument's error passes as it is
    pad = [torch.zeros(t.shape[0], dim - 2 * half, dtype=F64, device=t.device)]
    return torch.cat([c.v, s.v] + pad, 1), torch.cat([c.e, s.e] + pad, 1)


def latent_sample_ref(mom, noise, lmean, lstd, mult, clamp=True):
    """mom [B,2C,HW] (mean | logvar), noise [B,C,HW]: ((mean + exp(0.5 clamp(logvar, -30, 20)) noise - lat_mean) / lat_std) * mult."""
    C = mom.shape[1] // 2
    lv = mom[:, C:].double()
    if clamp:
        lv = lv.clamp(-30.0, 20.0)
    std = mono(Fl(lv).exact_scale(0.5), torch.exp, rel=C_EXPF)
    v = Fl(mom[:, :C]) + std * Fl(noise)
    if lstd is not None:
        v = (v - Fl(lmean[None, :, None])) / Fl(lstd[None, :, None])
    v = v * f32(mult)
    return v.v, v.e
