"""References and error bounds for KID and density / coverage (csrc/adm_eval.hip: pairwise_kernel<PW_KID>, pairwise_kernel<PW_COUNT>,
kid_fold_kernel, count_merge_kernel; ldmae_amd/evaluator.py), in the manner of eval_check.py: every reference is computed from the operands
AS STORED and from the definition, never from the kernel's order of operations.  u = 2^-24 (gemm_check.U), u64 = 2^-53.

KID.  Per subset s of m positions, with x_i = a[idx_a[s, i]], y_j = b[idx_b[s, j]] and k(x, y) = (gamma x.y + coef0)^3:
    aa = sum_{i != j} k(x_i, x_j),  bb = sum_{i != j} k(y_i, y_j),  ab = sum_{i, j} k(x_i, y_j)             (kid_sums_ref)
    mmd^2 = aa / (m (m - 1)) + bb / (m (m - 1)) - 2 ab / m^2;  KID = (mean, numpy.std) over the subsets   (evaluator.kid_from_sums)
gamma is the f32 the kernel receives (float(np.float32(gamma))), coef0 likewise.

Exact case (kid_sums_exact): integer features, gamma = 1 / den with den a power of two, coef0 = 1: p = (den + g) / den and
p^3 = (den + g)^3 / den^3 with g an integer.  For |x| <= 2, D = 16, den = 16: |g| <= 64, p is a multiple of 1/16 below 8 (7 bits),
p^2 a multiple of 1/256 below 64 (14 bits), p^3 a multiple of 1/4096 below 512 (21 bits): every f32 step of the kernel is exact, and the f64
sum of at most 2^16 such terms is an integer multiple of 2^-12 below 2^25, exact in any order.  The reference is computed in int64 and
divided by den^3 once (a power of two: exact), so equality of BITS is the check.

Bound of the general case (kid_sums_bound), per element and then summed, from the actual operands:
  1. g: the exact-f32 MFMA chain of D products: |dg| <= (D + 1) u sum_k |x_k y_k|                                        =: eg
  2. p = fmaf(gamma, g, coef0), one rounding: |dp| <= |gamma| eg + u (|p| + |gamma| eg)                                   =: ep
  3. q = p * p, one rounding: |dq| <= 2 |p| ep + ep^2 + u (|p| + ep)^2                                                    =: eq
  4. p3 = q * p, one rounding: |dp3| <= eq (|p| + ep) + p^2 ep + u (p^2 + eq) (|p| + ep)                                  =: e3
  5. the f64 sum: (double)p3 is exact; a term passes through at most 32 additions in its thread, 6 butterfly steps, 2 additions of the
     four wave sums and the fold over the T = row tiles x column tiles partials: depth = 40 + T, so the accumulation adds at most
     depth u64 sum (|p^3| + e3) (first order in u64; depth u64 < 2^-40 here).
  bound = sum e3 + depth u64 sum (|p^3| + e3), over the elements the sum runs over.
The reference itself is computed in 80-bit long double (products and sums): its own error, at most (D + m^2) 2^-64 relative to
sum |p^3|, is more than 2^10 times below the f64 term of the bound and is covered by doubling that term (the factor 2 below).

Ball counts.  counts[i] = #{ j : d(i, j) < r_i }, d = max((|u|^2 - 2 u.v) + |v|^2, 0) (ball_counts_ref: f64 from the f32 norms and radii
as passed; `strict=False` gives the <= variant).  Exact case: integer features with |x| small and D = 8: every product, norm, distance and
radius is an integer far below 2^24: the f32 kernel computes the same integers, ties d == r occur, equality is the check.  General case:
(d, E) = eval_check.pair_dist (the bound of the kernel's distance error of that pair); the device count of row i must lie in
[#{ j : d < r_i - E }, #{ j : d < r_i + E }] (ball_counts_interval); the pairs with |d - r_i| <= E are the undecided ones.
Density = sum_i counts[i] / (k N_fake), coverage = mean_i (counts[i] > 0): monotone in the counts, so the same interval carries over
(density_coverage_interval, which also lets the radii vary inside eval_check.knn_interval when they come from the device).
"""
from __future__ import annotations

import numpy as np
import torch

from eval_check import knn_interval, pair_dist
from gemm_check import U

U64 = 2.0 ** -53
LD = np.longdouble
TILE_M, TILE_N = 128, 64


def f32(x):
    return float(np.float32(x))


# ----------------------------------------------------------------------------- KID
def kid_from_sums_ref(sums, m):
    """-> (mean, std, mmd2 [S]) in f64 from sums [S, 3]."""
    s = np.asarray(sums, np.float64)
    mmd2 = s[:, 0] / (m * (m - 1)) + s[:, 1] / (m * (m - 1)) - 2.0 * s[:, 2] / (m * m)
    return float(mmd2.mean()), float(np.sqrt(((mmd2 - mmd2.mean()) ** 2).mean())), mmd2


def _positions(m, drop_row_mask):
    """Row positions the sum runs over: 0..m-1, or (the planted fault `i < m dropped`) the whole 128-row tiles, whose rows past m the
    kernel fills with the row of position m - 1."""
    if not drop_row_mask:
        return np.arange(m), np.arange(m)
    full = -(-m // TILE_M) * TILE_M
    return np.arange(full), np.minimum(np.arange(full), m - 1)


def kid_sums_exact(a, b, idx_a, idx_b, den, num=1, diagonal=False, drop_row_mask=False):
    """Integer features, gamma = num / den (den a power of two), coef0 = 1 -> f64 [S, 3], exact (int64 arithmetic, one exact division).
    diagonal / drop_row_mask / num = den (gamma = 1) are the three wrong variants the exact test must tell apart."""
    A, B = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    assert np.array_equal(A, np.asarray(a)) and np.array_equal(B, np.asarray(b)), "integer features only"
    S, m = idx_a.shape
    out = np.zeros((S, 3), np.float64)
    pos_i, src_i = _positions(m, drop_row_mask)
    for s in range(S):
        X, Y = A[idx_a[s]], B[idx_b[s]]
        for w, (P, Q) in enumerate(((X, X), (Y, Y), (X, Y))):
            g = P[src_i] @ Q.T
            c = (den + num * g) ** 3
            if w < 2 and not diagonal:
                c = np.where(pos_i[:, None] != np.arange(m)[None, :], c, 0)
            tot = int(c.sum())
            assert abs(tot) < 2 ** 53
            out[s, w] = tot / float(den ** 3)
    return out


def kid_sums_ref(a, b, idx_a, idx_b, gamma, coef0):
    """f32 features (numpy) -> (ref long double [S, 3], bound f64 [S, 3]) by the module docstring's derivation."""
    A, B = np.asarray(a, np.float32).astype(LD), np.asarray(b, np.float32).astype(LD)
    D = A.shape[1]
    gam, c0 = LD(f32(gamma)), LD(f32(coef0))
    S, m = idx_a.shape
    tiles = (-(-m // TILE_M)) * (-(-m // TILE_N))
    depth = 40 + tiles
    ref, bound = np.zeros((S, 3), LD), np.zeros((S, 3), np.float64)
    off = ~np.eye(m, dtype=bool)
    for s in range(S):
        X, Y = A[idx_a[s]], B[idx_b[s]]
        for w, (P, Q) in enumerate(((X, X), (Y, Y), (X, Y))):
            g = P @ Q.T
            Sabs = (np.abs(P) @ np.abs(Q).T).astype(np.float64)
            p = gam * g + c0
            pa = np.abs(p).astype(np.float64)
            eg = (D + 1) * U * Sabs
            ga = abs(float(gam))
            ep = ga * eg + U * (pa + ga * eg)
            eq = 2 * pa * ep + ep * ep + U * (pa + ep) ** 2
            e3 = eq * (pa + ep) + pa * pa * ep + U * (pa * pa + eq) * (pa + ep)
            p3 = p * p * p
            mask = off if w < 2 else np.ones((m, m), dtype=bool)
            ref[s, w] = np.where(mask, p3, LD(0)).sum()
            mag = np.where(mask, pa ** 3 + e3, 0.0).sum()
            bound[s, w] = np.where(mask, e3, 0.0).sum() + 2 * depth * U64 * mag
    return ref, bound


def kid_bound(bound, m):
    """bound [S, 3] of the sums -> (bound of the mean, bound of the std) of mmd^2: mmd^2 is linear in the sums; the mean of S values each
    within e_s moves by at most mean e_s; numpy.std is 1-Lipschitz in the Euclidean norm scaled by 1 / sqrt(S): at most
    sqrt(mean e_s^2) <= max e_s.  The host's own f64 arithmetic (three divisions, two additions, the mean and the std of S values) adds at most
    (S + 16) u64 of the magnitudes involved, taken here as (S + 16) u64 (1 + sum of the three terms' magnitudes): see kid_host_term."""
    b = np.asarray(bound, np.float64)
    e = b[:, 0] / (m * (m - 1)) + b[:, 1] / (m * (m - 1)) + 2.0 * b[:, 2] / (m * m)
    return float(e.mean()), float(e.max())


def kid_host_term(sums, m):
    s = np.abs(np.asarray(sums, np.float64))
    mag = s[:, 0] / (m * (m - 1)) + s[:, 1] / (m * (m - 1)) + 2.0 * s[:, 2] / (m * m)
    return (s.shape[0] + 16) * U64 * (1.0 + float(mag.max()))


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over all elements (got f64, ref long double); inf where got is not finite."""
    g = np.asarray(got, np.float64)
    err = np.abs(g.astype(LD) - ref).astype(np.float64)
    err = np.where(np.isfinite(g), err, np.inf)
    assert (np.asarray(bound) > 0).all()
    return float((err / bound).max())


# ----------------------------------------------------------------------------- ball counts, density and coverage
def sqdist64(u, nu, v, nv):
    """max((|u|^2 - 2 u.v) + |v|^2, 0) in f64 from the norms as passed (numpy)."""
    U_, V_ = np.asarray(u, np.float64), np.asarray(v, np.float64)
    return np.maximum((np.asarray(nu, np.float64)[:, None] - 2.0 * (U_ @ V_.T)) + np.asarray(nv, np.float64)[None, :], 0.0)


def ball_counts_ref(u, nu, ru, v, nv, strict=True):
    d = sqdist64(u, nu, v, nv)
    r = np.asarray(ru, np.float64)[:, None]
    return ((d < r) if strict else (d <= r)).sum(1).astype(np.int64)


def ball_counts_interval(u, nu, ru, v, nv):
    """torch f32 tensors (CPU) -> (lo [M], hi [M] int64, undecided fraction): lo = #{d < r - E}, hi = #{d < r + E}, undecided = |d - r| <= E."""
    d, e = pair_dist(u, nu, v, nv)
    r = ru.double()[:, None]
    lo, hi = (d < r - e).sum(1), (d < r + e).sum(1)
    und = float(((d - r).abs() <= e).double().mean())
    return lo.numpy(), hi.numpy(), und


def check_counts(name, got, lo, hi):
    g = np.asarray(got, np.int64)
    bad = (g < lo) | (g > hi)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {g.size} counts outside their interval; first row {int(np.nonzero(bad)[0][0])}: " \
                          f"got {int(g[bad][0])}, interval [{int(lo[bad][0])}, {int(hi[bad][0])}]"


def density_coverage_interval(real, fake, k):
    """torch f32 [M, D], [N, D] (CPU) -> ((density lo, hi), (coverage lo, hi), undecided fraction): the radii are the k-th sorted squared
    distance among the real rows, known only inside eval_check.knn_interval (the f64 row norms rounded to f32 are what ops.row_sqnorms
    gives to within half an ulp -- that half ulp is inside pair_dist's bound only for the norms AS PASSED, so the norms here are the
    correctly rounded ones and one ulp of each norm is added to E)."""
    nr = (real.double() ** 2).sum(1).float()
    nf = (fake.double() ** 2).sum(1).float()
    ulp_r, ulp_f = nr.double() * 2 * U, nf.double() * 2 * U
    d_rr, e_rr = pair_dist(real, nr, real, nr)
    e_rr = e_rr + ulp_r[:, None] + ulp_r[None, :]
    rlo, rhi = knn_interval(d_rr, e_rr, (k,))
    d, e = pair_dist(real, nr, fake, nf)
    e = e + ulp_r[:, None] + ulp_f[None, :]
    lo, hi = (d + e < rlo).sum(1), (d - e < rhi).sum(1)
    und = float((((d + e) >= rlo) & ((d - e) < rhi)).double().mean())
    n = fake.shape[0]
    return ((float(lo.sum()) / (k * n), float(hi.sum()) / (k * n)),
            (float((lo > 0).double().mean()), float((hi > 0).double().mean())), und)


def density_coverage_ref(real, fake, k):
    """The definition in f64 (numpy): (density, coverage, counts)."""
    R, Fk = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    nr, nf = (R * R).sum(1), (Fk * Fk).sum(1)
    r = np.sort(sqdist64(R, nr, R, nr), 1)[:, k]
    counts = (sqdist64(R, nr, Fk, nf) < r[:, None]).sum(1)
    return float(counts.sum() / (k * Fk.shape[0])), float((counts > 0).mean()), counts
