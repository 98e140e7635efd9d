"""f64 restatements and derived error bounds of the linear-probe / k-NN kernels (csrc/linprobe.hip), in the manner of kid_check.py and
row_check.py.  Nothing here is tuned to a kernel's output: every bound is a count of roundings.

Model.  U = 2^-24 is half an ulp of a f32 result relative to it.  A f32 sum of n terms in ANY order errs by at most (n - 1) U sum|terms| to
first order; every other f32 operation (+, -, *, /, sqrtf, fma, a conversion from f64) rounds once: U |result|.  The device's expf and logf
are MEASURED (csrc/probe/intrinsic_probe on an MI355X; layer_check.py lists the run): expf 1.396 U relative on [-87, 88], logf 3.043 U
relative on [1, 1e5]; twice that is allowed (C_EXPF, C_LOGF), and TINY (2^-125) is the absolute floor where expf underflows or flushes.
Sums the kernels accumulate in f64 (BatchNorm statistics, LARS norms) contribute F64 = 2^-50 relative, stated where used.  SECOND multiplies
the first-order bounds by 1.001 for the products of error terms that the first order drops (every relative error here is below 1e-3).
"""
import math

import numpy as np

from layer_check import C_EXPF, C_LOGF, TINY

U = 2.0 ** -24
F64 = 2.0 ** -50
SECOND = 1.001


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ token_mean
TM_GROUPS = 16


def token_mean_ref(x, col0=0, d=None):
    """x [B, N, W] (the stored values, any float type) -> (mean over N of channels [col0, col0 + d) in f64, bound).  The kernel adds
    ceil(N / 16) terms per row group and then the 16 group sums: at most ceil(N / 16) + 14 additions on any path to the total, each U of a
    partial sum <= sum|x|; then one division (U |mean|)."""
    x = _f64(x)
    N = x.shape[1]
    d = x.shape[2] - col0 if d is None else d
    xs = x[:, :, col0:col0 + d]
    ref = xs.mean(axis=1)
    nadd = -(-N // TM_GROUPS) + TM_GROUPS - 2
    bound = SECOND * (nadd * U * np.abs(xs).sum(axis=1) / N + U * np.abs(ref))
    return ref, bound


# ------------------------------------------------------------------------------------------------ bn1d
def bn1d_ref(x, eps, run_mean, run_var, momentum=0.1):
    """Training-mode BatchNorm1d(affine=False) of x [B, D] (f32 values) in f64 -> dict of references and bounds.
    mean_k = the f32 rounding of the f64 column mean: |mean_k - mean| <= dm = U |mean| (+ F64).
    e_i = fl(x_i - mean_k), var_k = fl(sum e_i^2 / B), the sum exact to F64.  sum (x_i - mean_k)^2 = sum (x_i - mean)^2 + B (mean_k - mean)^2
    exactly (the cross term vanishes), each e_i^2 carries (1 + U)^2, the rounding of var one more U:
        |var_k - var| <= dv = dm^2 + 3 U (var + dm^2).
    rstd_k = fl(1 / fl(sqrt(fl(var_k + eps)))): half the relative error of the argument, + U / 2 (the sum under the root), + U (root), + U
    (division): rr = dv / (2 (var + eps)) + 2.5 U.
    xhat_k = fl(e_i rstd_k): |xhat_k - xhat| <= dm rstd + |x_i - mean| rstd (U + rr + U).
    Running statistics: new_k = fma(momentum, stat_k, fl(fl(1 - momentum) old)): |old| (1 - momentum) 2 U + momentum d(stat) + U |new|; the
    unbiased variance is sum e_i^2 / (B - 1) rounded: the bound of var times B / (B - 1)."""
    x, rm, rv = _f64(x), _f64(run_mean), _f64(run_var)
    B = x.shape[0]
    eps, momentum = float(np.float32(eps)), float(np.float32(momentum))
    mean = x.mean(axis=0)
    dm = U * np.abs(mean) * (1 + F64) + F64 * np.abs(x).max(axis=0)
    dev = x - mean
    var = (dev * dev).mean(axis=0)
    dv = (dm * dm + 3 * U * (var + dm * dm)) * SECOND
    rstd = 1.0 / np.sqrt(var + eps)
    rr = dv / (2 * (var + eps)) + 2.5 * U
    xhat = dev * rstd
    bound = SECOND * (dm * rstd + np.abs(dev) * rstd * (2 * U + rr))
    keep = 1.0 - momentum
    new_mean = keep * rm + momentum * mean
    d_mean = SECOND * (np.abs(rm) * keep * 2 * U + momentum * dm + U * np.abs(new_mean))
    unb = var * B / (B - 1)
    new_var = keep * rv + momentum * unb
    d_var = SECOND * (np.abs(rv) * keep * 2 * U + momentum * dv * B / (B - 1) + U * np.abs(new_var))
    return {"xhat": xhat, "bound": bound, "mean": mean, "dmean": dm, "var": var, "dvar": dv, "rstd": rstd, "drstd": SECOND * rstd * rr,
            "run_mean": new_mean, "drun_mean": d_mean, "run_var": new_var, "drun_var": d_var}


def bn1d_eval_ref(x, eps, run_mean, run_var):
    """Eval mode: xhat = (x - run_mean) / sqrt(run_var + eps) on the given f32 statistics: fl(x - m) U, rstd 2.5 U (sum, root, division), the
    product U."""
    x, rm, rv = _f64(x), _f64(run_mean), _f64(run_var)
    rstd = 1.0 / np.sqrt(rv + float(np.float32(eps)))
    xhat = (x - rm) * rstd
    return xhat, SECOND * np.abs(xhat) * 4.5 * U


def bn1d_naive_f32(x, eps):
    """What a one-pass E[x^2] - mean^2 formulation in f32 computes (the formulation the kernel must NOT use): for the tests' negative control."""
    x = np.asarray(x, dtype=np.float32)
    B = np.float32(x.shape[0])
    s1 = np.zeros(x.shape[1], np.float32)
    s2 = np.zeros(x.shape[1], np.float32)
    for row in x:
        s1 = s1 + row
        s2 = s2 + row * row
    mean = s1 / B
    var = np.maximum(s2 / B - mean * mean, np.float32(0))
    return ((x - mean) / np.sqrt(var + np.float32(eps))).astype(np.float64)


# ------------------------------------------------------------------------------------------------ softmax cross-entropy
def xent_iters(C):
    """Terms a thread adds before the block reduction: the kernel's register paths (C <= 256, 1024, 4096) and its strided loop beyond."""
    return 1 if C <= 256 else 4 if C <= 1024 else 16 if C <= 4096 else -(-C // 256)


def rank_ref(l, y):
    """Exact: #{c : l[c] > l[y]} + #{c < y : l[c] == l[y]} on the given values, row by row."""
    l = np.asarray(l)
    ly = l[np.arange(l.shape[0]), y][:, None]
    cols = np.arange(l.shape[1])[None, :]
    return ((l > ly) | ((l == ly) & (cols < np.asarray(y)[:, None]))).sum(axis=1).astype(np.int32)


def softmax_xent_ref(logits, y, grad_scale):
    """logits [B, C] (f32 values), y [B] -> dict(loss, dloss, dlogits, ddlogits, rank).
    t_k = fl(l - m): U |t|.  e_k = expf(t_k): relative expm1((|t| + C_EXPF) U) (the argument error U |t| moves exp by that factor), absolute
    floor TINY.  s_k: iters + 8 additions (the thread's terms, six butterfly steps, two joins): (iters + 8) U s + sum of the e errors.
    loss_k = fl(fl(m + logf(s_k)) - l_y): C_LOGF U |log s| + ds / s, then U |m + log s| and U |loss|.
    p_k = fl(e_k / s_k): p (re + ds / s + U); at the label fl(p - 1): U |p - 1|; times grad_scale: U |g|; TINY for a flushed result."""
    l = _f64(logits)
    B, C = l.shape
    rows = np.arange(B)
    m = l.max(axis=1, keepdims=True)
    t = l - m
    E = np.exp(t)
    s = E.sum(axis=1, keepdims=True)
    re = np.expm1((np.abs(t) + C_EXPF) * U)
    de = E * re + TINY
    ds = SECOND * (de.sum(axis=1, keepdims=True) + (xent_iters(C) + 8) * U * s)
    logs = np.log(s)
    ly = l[rows, y][:, None]
    loss = (m + logs) - ly
    dlog = C_LOGF * U * np.abs(logs) + ds / s
    dloss = SECOND * (dlog + U * np.abs(m + logs) + U * np.abs(loss))
    P = E / s
    dP = SECOND * (P * (re + ds / s + U) + TINY / s + TINY)
    G = P.copy()
    G[rows, y] -= 1.0
    dG = dP.copy()
    dG[rows, y] += U * np.abs(G[rows, y])
    gs = float(np.float32(grad_scale))
    ref = G * gs
    bound = SECOND * (dG * abs(gs) + U * np.abs(ref)) + TINY
    return {"loss": loss[:, 0], "dloss": dloss[:, 0], "dlogits": ref, "ddlogits": bound, "rank": rank_ref(np.asarray(logits), np.asarray(y))}


# ------------------------------------------------------------------------------------------------ LARS
def lars_step_ref(p, g, mu, lr, wd, momentum, trust, scaled):
    """The reference's util/lars.py, restated in f64 on flat arrays.  scaled: the tensor has more than one dimension."""
    p, g, mu = _f64(p), _f64(g), _f64(mu)
    dp = g
    if scaled:
        dp = g + wd * p
        pn, un = math.sqrt(float((p * p).sum())), math.sqrt(float((dp * dp).sum()))
        q = trust * pn / un if (pn > 0.0 and un > 0.0) else 1.0
        dp = dp * q
    mu = momentum * mu + dp
    return p - lr * mu, mu


def lars_trajectory_ref(p0, grads, lrs, wd, momentum, trust, scaled):
    """Steps of lars_step_ref from mu = 0 -> (list of p, list of mu, list of elementwise bounds on p, on mu) for a kernel that starts from the
    same f32-representable p0 and is fed the same f32-representable gradients.  The bounds are propagated step by step (ep, emu = elementwise
    bounds on the state so far; hyper-parameters reach the kernel as f32: U relative each):
        dp_k = fma(wd, p_k, g):            edp = wd ep + U wd |p| + U |dp|
        norms (f64 sums, f32 results):     epn = |ep|_2 + U pn (+ F64), eun = |edp|_2 + U un
        q_k = fl(fl(trust pn_k) / un_k):   rq = epn / pn + eun / un + 3 U
        dp'_k = fl(dp_k q_k):              edp' = q edp + |dp q| (rq + U)
        mu_k = fma(momentum, mu_k, dp'_k): emu' = momentum emu + U momentum |mu| + edp' + U |mu'|
        p_k = fma(-lr, mu_k, p_k):         ep' = ep + lr emu' + U lr |mu'| + U |p'|
    A step whose trust ratio switches off (a zero norm) must do so in both arithmetics: asserted (a zero norm with a zero bound, or a norm
    ten times its bound)."""
    p, mu = _f64(p0).copy(), np.zeros_like(_f64(p0))
    ep, emu = np.zeros_like(p), np.zeros_like(p)
    ps, mus, eps_, emus = [], [], [], []
    for g, lr in zip(grads, lrs):
        g = _f64(g)
        if scaled:
            dp = g + wd * p
            edp = SECOND * (wd * ep + U * wd * np.abs(p) + U * np.abs(dp))
            pn, un = math.sqrt(float((p * p).sum())), math.sqrt(float((dp * dp).sum()))
            epn = math.sqrt(float((ep * ep).sum())) + (U + F64) * pn
            eun = math.sqrt(float((edp * edp).sum())) + (U + F64) * un
            for nrm, e in ((pn, epn), (un, eun)):
                assert (nrm == 0.0 and e == 0.0) or nrm > 10 * e, "the fixture sits on the trust-ratio branch"
            if pn > 0.0 and un > 0.0:
                q = trust * pn / un
                rq = epn / pn + eun / un + 3 * U
            else:
                q, rq = 1.0, 0.0
            edp = SECOND * (q * edp + np.abs(dp * q) * (rq + U))
            dp = dp * q
        else:
            dp, edp = g, np.zeros_like(p)
        mu_new = momentum * mu + dp
        emu = SECOND * (momentum * emu + U * momentum * np.abs(mu) + edp + U * np.abs(mu_new))
        p_new = p - lr * mu_new
        ep = SECOND * (ep + lr * emu + U * lr * np.abs(mu_new) + U * np.abs(p_new))
        p, mu = p_new, mu_new
        ps.append(p.copy()), mus.append(mu.copy()), eps_.append(ep.copy()), emus.append(emu.copy())
    return ps, mus, eps_, emus


# ------------------------------------------------------------------------------------------------ top-k and the vote
def topk_ref(S, k):
    """Per row of the f32 matrix S: the k largest by a STABLE descending sort (equal values by ascending column), padded with (-inf, -1)."""
    S = np.asarray(S, dtype=np.float32)
    M, N = S.shape
    order = np.argsort(-S.astype(np.float64), axis=1, kind="stable")[:, :k]
    vals = np.full((M, k), -np.inf, dtype=np.float32)
    idx = np.full((M, k), -1, dtype=np.int32)
    n = min(k, N)
    vals[:, :n] = np.take_along_axis(S, order, axis=1)[:, :n]
    idx[:, :n] = order[:, :n]
    return vals, idx


def knn_vote_ref(vals, idx, bank_labels, qlabels, C, T):
    """f64 class scores sum exp(sim / T) over each query's neighbours, the rank of the true class, and which queries the bound cannot decide.
    w_k = expf(fl(v fl(1 / T))): the argument a = v / T carries 2 U |a| (the reciprocal and the product), so w is off by relative
    expm1((2 |a| + C_EXPF) U); a class score adds at most k terms in sequence: (k - 1) U score.  A query is AMBIGUOUS when some other class's
    f64 score lies within the two bounds of the true class's: only those may be left out of an exact comparison of ranks."""
    vals, idx = _f64(vals), np.asarray(idx)
    bank_labels, qlabels = np.asarray(bank_labels), np.asarray(qlabels)
    M, k = vals.shape
    T = float(np.float32(T))
    scores, dscores = np.zeros((M, C)), np.zeros((M, C))
    for m in range(M):
        for j in range(k):
            if idx[m, j] < 0:
                continue
            a = vals[m, j] / T
            w = math.exp(a)
            c = int(bank_labels[idx[m, j]])
            scores[m, c] += w
            dscores[m, c] += w * math.expm1((2 * abs(a) + C_EXPF) * U)
    dscores = SECOND * (dscores + (k - 1) * U * scores)
    rank = rank_ref(scores, qlabels)
    sy, dy = scores[np.arange(M), qlabels][:, None], dscores[np.arange(M), qlabels][:, None]
    close = np.abs(scores - sy) <= dscores + dy
    close[np.arange(M), qlabels] = False
    return scores, dscores, rank, close.any(axis=1)
