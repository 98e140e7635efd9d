"""The adaptive dopri5 ODE sampler, host side: a restatement of the solver written from the published method (Dormand & Prince 1980 for the
pair, Shampine 1986 for the dense-output midpoint, Hairer / Norsett / Wanner II.4 for the starting step, and the controller torchdiffeq documents:
RMS error ratio over the whole state, accept at <= 1, next step h min(10, max(0.9 / ratio^(1/5), 1 if accepted else 0.2))), the tableau
identities on it and on the constants ldmae_amd/transport/integrators.py exports, the closed forms of the two test problems, and the C ABI.

tests/test_gpu_ode_dopri5.py imports the restatement and the problems from here: the GPU solver must take the same steps.

Measured with this file (restatement in f32 against itself in f64, max over the 11 grid points of max|x32 - x64| / max|x64|; the GPU test allows
4x these): sin 2.2e-6 (rtol 1e-3) and 7.3e-6 (rtol 1e-5), lin 3.2e-6 and 4.8e-6 -- F32_DRIFT below."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ----------------------------------------------------------------------------- the method, from the literature
C = [0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1, 1]
A = [[],
     [1 / 5],
     [3 / 40, 9 / 40],
     [44 / 45, -56 / 15, 32 / 9],
     [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
     [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
     [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]]
B5 = [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0]                       # 5th order (propagated)
B4 = [1951 / 21600, 0, 22642 / 50085, 451 / 720, -12231 / 42400, 649 / 6300, 1 / 60]      # embedded 4th order
E = [b5 - b4 for b5, b4 in zip(B5, B4)]
MID = [6025192743 / 30085553152 / 2, 0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2, 187940372067 / 1594534317056 / 2,
       -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2]


def shifted_grid(num, shift, dt=np.float32):
    """The sampler's grid as the package builds it: f32 linspace, then t -> s t / (1 + (s - 1) t) in f32."""
    t = torch.linspace(0, 1, num)
    return [float(v) for v in torch.tensor([(shift * tn) / (1 + (shift - 1) * tn) for tn in t])]


def dopri5_restated(f, y0, grid, rtol, atol, dt=np.float64, max_steps=10000):
    """Returns (trajectory [len(grid), ...], stats).  Every quantity (state, t, h, ratio) is kept in `dt`."""
    rtol, atol = dt(rtol), dt(atol)
    cast = lambda row: [dt(v) for v in row]
    a, b5, e, mid, c = [cast(r) for r in A], cast(B5), cast(E), cast(MID), cast(C)

    def norm(v):
        return np.sqrt(np.mean(v * v, dtype=dt), dtype=dt)

    def comb(y, ks, w, h):
        acc = w[0] * ks[0]
        for j in range(1, len(w)):
            acc = acc + w[j] * ks[j]
        return y + h * acc

    st = dict(nfe=0, accepted=0, rejected=0, ratios=[], h=[])

    def fe(t, y):
        st["nfe"] += 1
        return f(dt(t), y).astype(dt)

    y = y0.astype(dt)
    t = dt(grid[0])
    f0 = fe(t, y)
    scale = atol + rtol * np.abs(y)
    d0, d1 = norm(y / scale), norm(f0 / scale)
    h0 = dt(1e-6) if (d0 < 1e-5 or d1 < 1e-5) else dt(0.01) * d0 / d1
    f1 = fe(t + h0, y + h0 * f0)
    d2 = norm((f1 - f0) / scale) / h0
    h1 = max(dt(1e-6), h0 * dt(1e-3)) if (d1 <= 1e-15 and d2 <= 1e-15) else (dt(0.01) / max(d1, d2)) ** dt(0.2)
    h = min(dt(100) * h0, h1)
    out = [y.copy()]
    t_start = t_end = t
    interp = None
    for tg in grid[1:]:
        tg = dt(tg)
        while tg > t_end:
            assert st["accepted"] + st["rejected"] < max_steps and t + h > t
            ks = [f0]
            for s in range(1, 7):
                ks.append(fe(t + c[s] * h, comb(y, ks, a[s], h)))
            y1 = comb(y, ks, b5[:6], h)
            err = h * (comb(np.zeros_like(y), ks, e, dt(1)))
            ratio = norm(err / (atol + rtol * np.maximum(np.abs(y), np.abs(y1))))
            st["ratios"].append(float(ratio))
            st["h"].append(float(h))
            accept = ratio <= 1
            dfac = dt(1) if ratio < 1 else dt(0.2)
            factor = dt(10) if ratio == 0 else min(dt(10), max(dt(0.9) / ratio ** dt(0.2), dfac))
            if accept:
                st["accepted"] += 1
                ym = comb(y, ks, mid, h)
                interp = (y, y1, ym, ks[0], ks[6], h)
                t_start, t_end = t, t + h
                t, y, f0 = t + h, y1, ks[6]
            else:
                st["rejected"] += 1
            h = h * factor
        ya, yb, ym, fa, fb, hh = interp
        x = (tg - t_start) / hh
        qa = dt(2) * hh * (fb - fa) - dt(8) * (yb + ya) + dt(16) * ym
        qb = hh * (dt(5) * fa - dt(3) * fb) + dt(18) * ya + dt(14) * yb - dt(32) * ym
        qc = hh * (fb - dt(4) * fa) - dt(11) * ya - dt(5) * yb + dt(16) * ym
        out.append(ya + x * (hh * fa) + x ** 2 * qc + x ** 3 * qb + x ** 4 * qa)
    return np.stack(out), st


# ----------------------------------------------------------------------------- the two problems (state [4, 16, 8, 8], t in [0, 1])
SHAPE = (4, 16, 8, 8)
GRID = shifted_grid(11, 0.3)
CASES = [(1e-3, 1e-6), (1e-5, 1e-8)]                     # (rtol, atol)
A_DAMP, A_SCALE = 0.5, 1.0


def initial_state(problem):
    """States that stay away from zero over [0, 1] (sin: x >= 2 at t = 0, decaying to >= 0.5; lin: 3 +- 0.3 under a rotation of less than a
    radian): with the mixed tolerance atol + rtol |x| an element near zero has a tolerance near atol, its error quotient is then dominated by
    f32 rounding of the stage values, and the accept decisions of an f32 solver would not be reproducible by an f64 restatement."""
    r = np.random.RandomState(11).standard_normal(SHAPE)
    return (2 + np.abs(r) if problem == "sin" else 3 + 0.3 * r).astype(np.float32)


def matrix_a():
    """A fixed 16 x 16 matrix: skew-symmetric rotation part plus uniform damping."""
    m = np.random.RandomState(12).standard_normal((16, 16))
    return (A_SCALE * (m - m.T) / 2 / np.sqrt(16) - A_DAMP * np.eye(16)).astype(np.float32)


def f_sin(t, x):
    return -x + np.sin(x.dtype.type(5) * t)


def exact_sin(t, x0):
    """x' = -x + sin 5t: x = (x0 + 5/26) e^-t + (sin 5t - 5 cos 5t) / 26."""
    x0 = x0.astype(np.float64)
    return (x0 + 5 / 26) * np.exp(-t) + (np.sin(5 * t) - 5 * np.cos(5 * t)) / 26


def f_lin(t, x):
    return np.einsum("ij,bjhw->bihw", matrix_a().astype(x.dtype), x)


def exact_lin(t, x0):
    from scipy.linalg import expm
    return np.einsum("ij,bjhw->bihw", expm(matrix_a().astype(np.float64) * t), x0.astype(np.float64))


PROBLEMS = {"sin": (f_sin, exact_sin), "lin": (f_lin, exact_lin)}

# max over the grid of max|x_f32 - x_f64| / max|x_f64| of the restatement run in f32 against itself in f64 (measured here, printed by
# test_restatement_in_f32_takes_the_same_steps); the GPU test allows 4x these.  Most of it is not rounding of the state but the step sizes: the
# first step's error is at the f32 noise level, its growth factor 0.9 / ratio^(1/5) differs by some per cent, and the later steps then differ
# within what the tolerance allows
F32_DRIFT = {("sin", 1e-3): 2.2e-6, ("sin", 1e-5): 7.3e-6, ("lin", 1e-3): 3.2e-6, ("lin", 1e-5): 4.8e-6}


_cache = {}


def restated(problem, rtol, atol, dt=np.float64):
    key = (problem, rtol, atol, dt)
    if key not in _cache:
        _cache[key] = dopri5_restated(PROBLEMS[problem][0], initial_state(problem), GRID, rtol, atol, dt)
    return _cache[key]


def exact(problem):
    x0 = initial_state(problem)
    return np.stack([PROBLEMS[problem][1](t, x0) for t in GRID])


def f32_drift(problem, rtol, atol):
    a, b = restated(problem, rtol, atol)[0], restated(problem, rtol, atol, np.float32)[0]
    return float(np.abs(a - b).max() / np.abs(a).max())


# ----------------------------------------------------------------------------- tests
def _tableau_identities(c, a, b, e):
    for i in range(7):
        assert abs(sum(a[i]) - c[i]) < 1e-15, i
    assert abs(sum(b) - 1) < 1e-15 and abs(sum(e)) < 1e-15
    assert list(a[6]) == list(b[:6]) and b[6] == 0              # FSAL: the last stage is evaluated at the new point


def test_tableau_identities():
    _tableau_identities(C, A, B5, E)
    # order conditions up to 2 for both weight sets, and the midpoint weights sum to 1/2
    assert abs(sum(b * c for b, c in zip(B5, C)) - 0.5) < 1e-15 and abs(sum(b * c for b, c in zip(B4, C)) - 0.5) < 1e-15
    assert abs(sum(MID) - 0.5) < 1e-15
    from ldmae_amd.transport import integrators as I
    _tableau_identities(I.DP_C, I.DP_A, I.DP_B, I.DP_E)
    assert list(I.DP_MID) == MID and list(I.DP_B) == B5 and [list(r) for r in I.DP_A] == A and np.allclose(I.DP_E, E, atol=1e-17, rtol=0)
    assert (I.DP_SAFETY, I.DP_IFACTOR, I.DP_DFACTOR, I.DP_ORDER) == (0.9, 10.0, 0.2, 5)


def test_restatement_matches_torchdiffeq():
    torchdiffeq = pytest.importorskip("torchdiffeq", reason="torchdiffeq is not installed: the restatement is checked against the closed forms only")
    for problem in PROBLEMS:
        for rtol, atol in CASES:
            want, st = restated(problem, rtol, atol)
            f = PROBLEMS[problem][0]
            calls = [0]

            def func(t, x):
                calls[0] += 1
                return torch.from_numpy(f(np.float64(t), x.numpy()))
            got = torchdiffeq.odeint(func, torch.from_numpy(initial_state(problem)).double(), torch.tensor(GRID, dtype=torch.float64), rtol=rtol,
                                     atol=atol, method="dopri5").numpy()
            assert calls[0] == st["nfe"], (problem, rtol)
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (problem, rtol)


@pytest.mark.parametrize("problem", list(PROBLEMS))
@pytest.mark.parametrize("rtol,atol", CASES)
def test_restatement_against_the_closed_form(problem, rtol, atol):
    traj, st = restated(problem, rtol, atol)
    ex = exact(problem)
    err = np.abs(traj - ex).reshape(len(GRID), -1).max(1)
    print(f"{problem} rtol {rtol:g}: nfe {st['nfe']} accepted {st['accepted']} rejected {st['rejected']}; max err / (rtol max|x|) = "
          f"{err.max() / (rtol * np.abs(ex).max()):.3f}; ratios {[round(r, 4) for r in st['ratios']]}")
    assert np.array_equal(traj[0], initial_state(problem).astype(np.float64))
    assert (err <= 10 * rtol * np.abs(ex).max()).all()
    assert st["nfe"] == 2 + 6 * (st["accepted"] + st["rejected"])
    # the condition the GPU test's step-count equality rests on: no accept decision that f32 rounding could flip
    assert not any(0.98 <= r <= 1.02 for r in st["ratios"]), st["ratios"]


def test_a_step_is_rejected_in_some_case():
    rej = {(p, rtol): restated(p, rtol, atol)[1]["rejected"] for p in PROBLEMS for rtol, atol in CASES}
    assert rej[("sin", 1e-3)] >= 1 and rej[("sin", 1e-5)] >= 1, rej          # the GPU test's rejection path: both "sin" cases


@pytest.mark.parametrize("problem", list(PROBLEMS))
@pytest.mark.parametrize("rtol,atol", CASES)
def test_restatement_in_f32_takes_the_same_steps(problem, rtol, atol):
    a, b = restated(problem, rtol, atol)[1], restated(problem, rtol, atol, np.float32)[1]
    assert (a["nfe"], a["accepted"], a["rejected"]) == (b["nfe"], b["accepted"], b["rejected"])
    d = f32_drift(problem, rtol, atol)
    print(f"{problem} rtol {rtol:g}: f32 restatement against f64, max|dx| / max|x| = {d:.3e}")
    assert d <= 1.5 * F32_DRIFT[(problem, rtol)]                 # the recorded figures are what this computes (room for another libm)


def test_abi_declares_and_binds_the_ode_entry_points():
    from ldmae_amd import _lib
    header = open(os.path.join(ROOT, "include", "ldmae_hip.h")).read()
    for name in ("ldmae_rk_stage_f32", "ldmae_dopri5_finish_f32", "ldmae_rms_norm_scaled_f32", "ldmae_dopri5_interp_f32", "ldmae_dopri5_advance",
                 "ldmae_dopri5_initial_step", "ldmae_ode_partials"):
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\);", header)
        assert m, name + " is not declared in include/ldmae_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
    assert _lib.load().ldmae_ode_partials(1) == 1 and _lib.load().ldmae_ode_partials(4096) == 1 and _lib.load().ldmae_ode_partials(4097) == 2


def _fixed_step_as_before(method, t, x, f):
    """The fixed-step loop of integrators.py as it stood before dopri5 was added."""
    xs = [x]
    for k in range(len(t) - 1):
        dt = t[k + 1] - t[k]
        if method == "euler":
            x = x + dt * f(t[k], x)
        elif method == "midpoint":
            x = x + dt * f(t[k] + dt / 2, x + dt / 2 * f(t[k], x))
        else:
            k1 = f(t[k], x)
            x = x + dt / 2 * (k1 + f(t[k + 1], x + dt * k1))
        xs.append(x)
    return torch.stack(xs)


def test_constructor_and_fixed_step_solvers_unchanged():
    from ldmae_amd.transport.integrators import METHODS, ode, shifted_grid as grid_of
    drift = lambda x, t, model, **kw: model(x, t, **kw)
    model = lambda x, t: -x * t.view(-1, 1) + torch.sin(3 * t).view(-1, 1)
    o = ode(drift, t0=0, t1=1, sampler_type="dopri5", num_steps=9, atol=1e-6, rtol=1e-3, timestep_shift=0.3)
    assert o.sampler_type == "dopri5" and (o.atol, o.rtol) == (1e-6, 1e-3) and o.max_num_steps == 2 ** 31 - 1 and METHODS[-1] == "dopri5"
    assert torch.equal(o.t, grid_of(0, 1, 9, 0.3))
    with pytest.raises(RuntimeError, match="HIP device"):                 # the solver's arithmetic is HIP: no CPU fallback
        o.sample(torch.zeros(2, 3), model)
    with pytest.raises(NotImplementedError, match="euler / heun / midpoint / dopri5"):
        ode(drift, t0=0, t1=1, sampler_type="rk4", num_steps=9, atol=1e-6, rtol=1e-3)
    with pytest.raises(AssertionError):                                   # reverse time stays refused
        ode(drift, t0=1, t1=0, sampler_type="dopri5", num_steps=9, atol=1e-6, rtol=1e-3)
    x = torch.randn(3, 5, generator=torch.Generator().manual_seed(0))
    for method in ("euler", "heun", "midpoint"):
        s = ode(drift, t0=0, t1=1, sampler_type=method, num_steps=9, atol=1e-6, rtol=1e-3, timestep_shift=0.3)
        want = _fixed_step_as_before(method, s.t, x, lambda tk, xk: model(xk, torch.ones(xk.size(0)) * tk))
        assert torch.equal(s.sample(x, model), want), method
