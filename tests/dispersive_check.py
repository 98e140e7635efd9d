"""The f64 restatement of the Dispersive Loss (include/ldmae_hip.h: the contract) and the error bounds of the two kernels.

Distances come from direct differences, never through the Gram matrix: the restatement does not share the kernels' cancellation.

    d_ij = ||z_i - z_j||^2,  e_ij = exp(-d_ij / (K tau)),  r_i = sum_j e_ij,  S = sum_i r_i
    L = log(S / B^2),  C_ij = 4 / (S K tau) (e_ij - delta_ij r_i),  dL/dz = C z

THE BOUNDS (u = 2^-24, gamma_n = n u / (1 - n u); hatted values are the kernel's).
  Gram.  hat G_ij is an f32 fma chain over the at most `slab` elements of each K-slab, then a chain of slabs - 1 f32 adds: every product
    passes through at most n = slab + slabs - 1 roundings, so |hat G_ij - G_ij| <= gamma_n sum_k |z_ik z_jk| <= gamma_n (n_i + n_j) / 2
    (n_i = ||z_i||^2; Cauchy-Schwarz and the AM-GM inequality), and |hat n_i - n_i| <= gamma_n n_i.
  Distance.  hat d_ij = max(hat n_i + hat n_j - 2 hat G_ij, 0) is formed in f64 from the f32 values (its own error, a few 2^-53 (n_i + n_j), is
    counted as u^2 (n_i + n_j)); the clamp moves hat d towards the true d >= 0.  So |hat d_ij - d_ij| <= dd_ij = (2 gamma_n + u^2)(n_i + n_j) for
    i != j, and hat d_ii = d_ii = 0 exactly (set, not computed).
  exp.  hat e_ij = e_ij exp(+-dd_ij / (K tau')) with tau' the f32 tau the kernel is given (the caller passes it on to the restatement), times
    the f64 exp's own rounding (counted as 4 * 2^-53): |hat e_ij - e_ij| <= de_ij = e_ij (exp(dd_ij / (K tau)) - 1 + 2^-51), de_ii = 0.
  Sums (f64, at most B + 8 terms each: 2^-53 (B + 8) relative): dr_i = sum_j de_ij + 2^-53 (B + 8) r_i; dS = sum_i dr_i + 2^-53 (B + 8) S.
  L.  |hat L - L| <= dS / (S - dS) + 2^-50 + u |L| (log of a perturbed argument, the f64 log and division, the f32 rounding of the result).
  C.  with c = 4 / (S K tau) and c+ = 4 / ((S - dS) K tau): |hat C_ij - C_ij| <= c+ (de_ij + delta_ij dr_i) + |C_ij| dS / (S - dS)
    + u (|C_ij| + that) + 2^-50 |C_ij|   (the terms' errors, the factor's error, the f32 rounding of the result).
  Backward.  hat dz_ik = g (x) chain_j fma(hat C_ij, z_jk): a chain of B fmas and one multiply on the f32 hat C, so against g C z:
    |hat dz_ik - g (C z)_ik| <= |g| (sum_j dC_ij |z_jk| + gamma_(B+1) sum_j (|C_ij| + dC_ij) |z_jk|).
"""
import torch

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def reference(z, tau, K=None):
    """z [B, K] (any float dtype, taken to f64), tau -> dict of f64 tensors: d, e [B, B], r [B], S, L (0-dim), C [B, B], dz [B, K] = C z.
    K: the row length when z holds only the columns of a longer row that are not zero (the rest contributes nothing to any distance)."""
    z = z.detach().to("cpu", torch.float64)
    B, K = z.shape[0], (z.shape[1] if K is None else K)
    d = torch.zeros(B, B, dtype=torch.float64)
    for i in range(B):                                   # direct differences, row by row (B^2 K / B memory)
        d[i] = ((z - z[i]) ** 2).sum(1)
    d.fill_diagonal_(0.0)
    e = torch.exp(-d / (K * float(tau)))
    r = e.sum(1)
    S = r.sum()
    L = torch.log(S / (B * B))
    C = 4.0 / (S * K * float(tau)) * (e - torch.diag(r))
    return {"d": d, "e": e, "r": r, "S": S, "L": L, "C": C, "dz": C @ z}


def loss_autograd(z, tau):
    """L as torch ops on z (f64, requires_grad) for autograd: log mean_ij exp(-||z_i - z_j||^2 / (K tau)), distances by differences."""
    B, K = z.shape
    d = ((z[:, None, :] - z[None, :, :]) ** 2).sum(-1)
    d = d * (1.0 - torch.eye(B, dtype=z.dtype))
    return torch.log(torch.exp(-d / (K * float(tau))).sum() / (B * B))


def bounds(z, tau, slab, slabs, g=1.0, K=None):
    """The bounds above for z [B, K] (the f32 values the kernel reads), the kernel's split plan (slab length, number of slabs) and the
    upstream factor g -> (ref, {'L': float, 'C': [B, B], 'dz': [B, K]}), all f64 on the CPU; ref = reference(z, tau, K).  K as in reference."""
    ref = reference(z, tau, K)
    z64 = z.detach().to("cpu", torch.float64)
    B, K = z64.shape[0], (z64.shape[1] if K is None else K)
    n = (z64 ** 2).sum(1)
    gn = gamma(min(slab, K) + slabs - 1)
    nn = n[:, None] + n[None, :]
    dd = (2.0 * gn + U * U) * nn
    dd.fill_diagonal_(0.0)
    e, r, S, C = ref["e"], ref["r"], ref["S"], ref["C"]
    de = e * (torch.expm1(dd / (K * float(tau))) + 2.0 ** -51)
    de.fill_diagonal_(0.0)
    fs = 2.0 ** -53 * (B + 8)
    dr = de.sum(1) + fs * r
    dS = dr.sum() + fs * S
    relS = dS / (S - dS)
    bL = float(relS) + 2.0 ** -50 + U * abs(float(ref["L"]))
    cplus = 4.0 / ((S - dS) * K * float(tau))
    bC = cplus * (de + torch.diag(dr)) + C.abs() * relS
    bC = bC + U * (C.abs() + bC) + 2.0 ** -50 * C.abs() + 2.0 ** -149         # (the last term: a result in f32's subnormal range)
    az = z64.abs()
    bdz = abs(float(g)) * (bC @ az + gamma(B + 1) * ((C.abs() + bC) @ az)) + 2.0 ** -149
    return ref, {"L": bL, "C": bC, "dz": bdz}


def rms_rows(B, K, rms, seed):
    """B rows of K N(0, rms^2) f32 values (a CPU generator: the same rows wherever the test runs)."""
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(B, K, generator=gen, dtype=torch.float64) * rms).to(torch.float32)
