"""f64 restatements and derived error bounds for the post-hoc EMA kernels (ldmae_adamw_ema_tracks, ldmae_ema_tracks_only,
ldmae_snapshot_accumulate, ldmae_snapshot_finish).  Nothing here runs the code under test; nothing in a bound comes from its results.

THE CONTRACT (Karras et al. 2024, section 3).  Step t counts optimizer steps from 1; with exponent gamma
    beta(t) = (1 - 1/t)^(gamma+1),   e(t) = beta e(t-1) + (1 - beta) theta(t),   theta(t) = the parameter after the AdamW update of step t;
    beta(1) = 0: e(1) = theta(1) whatever the slab held;  w_tau = (1 - beta(tau)) (tau/t)^(gamma+1), summing to 1 over tau = 1..t.
The kernel takes c = 1 - beta(t) from the host (f64, -expm1((gamma+1) log1p(-1/t)), rounded to f32) and computes e + c (theta - e) in f32.

TRACK BOUND (U = 2^-24, f32 round to nearest).  One step is one subtraction d = theta - e, one product q = c d and one addition e' = e + q:
    |error of e'| <= (1 - c) err + U |d| + U |q| + min(U |e'|, |q|)
with err the error of the stored e, carried through (1 - c) because d inherits -err and e' inherits err - c err.  The last term is the
rounding of the addition: at most U |e'|, and never more than |q| itself (e is a representable number, so the nearest representable number
to e + q is no further away than e is).  This is the issue's U (|theta - e| + |c (theta - e)| + |e'|) with that one refinement, which only
tightens it; with the product and the addition contracted into one fma the product's rounding is absent and the bound holds all the more.
The magnitudes are taken at the f64 reference; the stored e differs from it by at most err, so err is added to each magnitude
(|d| + err, |e'| + err): first order made rigorous.  The refinement matters at the fixed point: for a constant parameter d = 0, the bound is 0,
and e + c (theta - e) indeed never moves, whereas beta e + (1-beta) theta with two rounded coefficients drifts by (beta_f32 + (1-beta)_f32 -
1) per step towards a fixed point ~0.17 % away at t = 1e6, gamma = 16.97 (test_posthoc_ema_cpu.py).
c == 1 stores theta: exact, err = 0, and the old slab is never read.

COMBINATION BOUND (u = 2^-53).  acc <- acc + coef x in f64, term by term: per term u |coef x| (the product) + u |acc'| (the addition), summed
over the terms; then one rounding to f32, U |acc| (+ 2^-150 where the result is subnormal).  The reference is accumulated in long double.
"""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
TINY = 2.0 ** -149          # an f32 result below the normal range rounds with an absolute, not a relative, error


def f32(x) -> float:
    """A python float rounded to f32 and back: the value the kernel's argument struct carries."""
    return float(np.float32(x))


def track_step_ref(e, err, theta, c):
    """One step of one track on f64 arrays: (e', err').  e None (or c == 1): the store of step 1.  c is the f32-rounded coefficient."""
    theta = np.asarray(theta, dtype=np.float64)
    if c == 1.0 or e is None:
        if c != 1.0:
            raise ValueError("a track without a value can only take the step c == 1")
        return theta.copy(), np.zeros_like(theta)
    d = theta - e
    q = c * d
    en = e + q
    dm = np.abs(d) + err
    new = (1.0 - c) * err + U * dm + U * c * dm + np.minimum(U * (np.abs(en) + err), c * dm) + 3 * TINY
    return en, new


def track_trajectory_ref(e0, thetas, cs):
    """All steps of one track from the f32 inputs: e0 the slab before the first step (None, or anything at all when cs[0] == 1), thetas the
    parameters after each step's update (f32 arrays, as the kernel wrote them), cs the f32-rounded coefficients.  Returns the lists of
    references and bounds after each step."""
    e = None if e0 is None or cs[0] == 1.0 else np.asarray(e0, dtype=np.float64)
    err = None if e is None else np.zeros_like(e)
    refs, errs = [], []
    for theta, c in zip(thetas, cs):
        e, err = track_step_ref(e, err, theta, c)
        refs.append(e)
        errs.append(err)
    return refs, errs


def combine_ref(xs, coefs):
    """sum_k coefs[k] xs[k] (f32 arrays, f64 coefficients) in long double, the bound of the f64 accumulation in the given order and of the
    final rounding to f32."""
    acc = np.zeros(xs[0].shape, dtype=np.longdouble)
    bound = np.zeros(xs[0].shape, dtype=np.float64)
    for x, c in zip(xs, coefs):
        term = np.longdouble(c) * x.astype(np.longdouble)
        acc = acc + term
        bound += U64 * (np.abs(term).astype(np.float64) + np.abs(acc).astype(np.float64) + bound)
    ref = acc.astype(np.float64)
    return ref, bound, bound + U * (np.abs(ref) + bound) + TINY


def actual_weights(cs):
    """The weights the recursion REALLY gives theta(1..t) when it runs with the coefficients cs[0..t-1] (f32-rounded, so they differ from the
    ideal w_tau in the 8th digit): w_tau = c_tau prod_{s > tau} (1 - c_s), f64."""
    cs = np.asarray(cs, dtype=np.float64)
    tail = np.concatenate([np.cumprod((1.0 - cs)[::-1])[::-1][1:], [1.0]])
    return cs * tail


def integrate_inner(ta, ga, tb, gb, n=200001):
    """<a, b> = integral over [0, min(t_a, t_b)] of p_a(tau) p_b(tau) by composite Simpson's rule on tau, f64 (the integrand is a power
    tau^(gamma_a + gamma_b): smooth enough for the rule's h^4 once gamma_a + gamma_b >= 4)."""
    top = float(min(ta, tb))
    tau = np.linspace(0.0, top, n)
    with np.errstate(divide="ignore"):
        lp = np.log(ga + 1.0) + np.log(gb + 1.0) + (ga + gb) * np.log(tau) - (ga + 1.0) * np.log(ta) - (gb + 1.0) * np.log(tb)
    f = np.exp(lp)
    h = top / (n - 1)
    return float(h / 3.0 * (f[0] + f[-1] + 4.0 * f[1:-1:2].sum() + 2.0 * f[2:-1:2].sum()))
