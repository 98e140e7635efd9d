"""The identities of the f64 restatement of the guidance rules (tests/guidance_check.py), each to f64 round-off: the GPU tests measure the
kernel against this restatement, so it is checked against the properties the rules are defined by."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guidance_check as gc     # noqa: E402

B, C, H, W = 3, 5, 3, 4
EPS = 2.0 ** -40               # f64 round-off of sums of a few hundred O(1) terms, with room


def draw(seed=0):
    rng = np.random.default_rng(seed)
    p, q, x = (rng.standard_normal((B, C, H, W)).astype(np.float32) for _ in range(3))
    t = rng.uniform(0.05, 0.9, B).astype(np.float32)
    return p, q, x, t


def close(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= EPS * (1 + np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("k", [C, 2])
def test_apg_with_eta_1_no_threshold_no_momentum_is_cfg(k):
    p, q, x, t = draw()
    g, _ = gc.apg_ref(p, q, x, t, 4.0, k, eta=1.0, r=0.0, beta=0.0)
    assert close(g, gc.cfg_ref(p, q, 4.0, k))


def test_rescale_with_phi_0_is_cfg():
    p, q, _, _ = draw(1)
    assert close(gc.rescale_ref(p, q, 7.5, C, 0.0), gc.cfg_ref(p, q, 7.5, C))


@pytest.mark.parametrize("k", [C, 3])
def test_rescale_with_phi_1_has_the_std_of_p(k):
    p, q, _, _ = draw(2)
    g = gc.rescale_ref(p, q, 10.0, k, 1.0)
    sg = g[:, :k].reshape(B, -1).std(1, ddof=1)
    sp = p[:, :k].astype(np.float64).reshape(B, -1).std(1, ddof=1)
    assert close(sg, sp)
    assert not close(gc.cfg_ref(p, q, 10.0, k)[:, :k].reshape(B, -1).std(1, ddof=1), sp)


def test_apg_with_eta_0_is_orthogonal_to_the_data_prediction():
    p, q, x, t = draw(3)
    a = gc.apg_parts(p, q, x, t, 6.0, C, eta=0.0, r=0.0, beta=0.0)
    dot = ((a["g"] - a["P"]) * a["u"]).sum(1)
    scale = np.sqrt(((a["g"] - a["P"]) ** 2).sum(1) * a["uu"])
    assert (np.abs(dot) <= EPS * scale).all() and (scale > 1).all()


def test_norm_threshold_limits_the_data_space_step():
    p, q, x, t = draw(4)
    r = 2.5
    a = gc.apg_parts(p, q, x, t, 6.0, C, eta=0.3, r=r, beta=0.0)
    step = a["omt"][:, 0] * np.sqrt(((a["gamma"][:, None] * a["d"]) ** 2).sum(1))
    assert (step <= gc.f32(r) * (1 + EPS)).all()
    assert (a["gamma"] < 1).all(), "the threshold must bind for this draw, or the test shows nothing"
    big = gc.apg_parts(p, q, x, t, 6.0, C, eta=0.3, r=1e6, beta=0.0)
    assert (big["gamma"] == 1).all()


def test_momentum_recursion_over_three_calls():
    beta = -0.5
    m = np.zeros((B, C * H * W))
    ds = []
    for call in range(3):
        p, q, x, t = draw(10 + call)
        _, m = gc.apg_ref(p, q, x, t, 5.0, C, eta=0.0, r=0.0, beta=beta, m_prev=m)
        ds.append((p.astype(np.float64) - q).reshape(B, -1))
    assert close(m, ds[2] + beta * (ds[1] + beta * ds[0]))
    # the first call of a trajectory: m_prev = 0, the momentum is p - q
    p, q, x, t = draw(10)
    assert close(gc.apg_ref(p, q, x, t, 5.0, C, beta=beta, m_prev=np.zeros((B, C * H * W)))[1], ds[0])


def test_degenerate_cases_are_finite_and_as_specified():
    p, q, x, t = draw(5)
    # d = 0: every rule returns p
    for rule in ("cfg", "rescale", "apg"):
        g = gc.guidance_ref(rule, p, p, 9.0, C, x=x, t=t, r=1.0)
        assert np.isfinite(g).all() and np.array_equal(g, p.astype(np.float64)), rule
    # u = 0 (x = -(1 - t) p exactly, with t = 0.5 and p exactly halved): par = 0, g = p + (s - 1) d
    t5 = np.full(B, 0.5, np.float32)
    g, _ = gc.apg_ref(p, q, -0.5 * p, t5, 3.0, C, eta=0.0)
    assert np.isfinite(g).all() and close(g, p + 2.0 * (p.astype(np.float64) - q))
    # std(g0) = 0 (p and q constant per sample): g = g0
    pc, qc = np.ones_like(p) * 2.0, np.ones_like(p) * 0.5
    g = gc.rescale_ref(pc, qc, 3.0, C, 0.7)
    assert np.isfinite(g).all() and np.array_equal(g, np.full(p.shape, 0.5 + 3.0 * 1.5))


def test_bounds_are_positive_finite_and_of_the_order_of_the_round_off():
    p, q, x, t = draw(6)
    for rule in ("cfg", "rescale", "apg"):
        b = gc.guidance_bound(rule, p, q, 4.0, 2, x=x, t=t, phi=0.7, eta=0.25, r=3.0)
        b = b[0] if rule == "apg" else b
        ref = gc.guidance_ref(rule, p, q, 4.0, 2, x=x, t=t, phi=0.7, eta=0.25, r=3.0)
        assert np.isfinite(b).all() and (b[:, :2] > 0).all() and (b[:, 2:] == 0).all(), rule
        assert (b[:, :2] < 64 * gc.U * (np.abs(ref[:, :2]) + 4.0 * (np.abs(p[:, :2]) + np.abs(q[:, :2])) + 1)).all(), rule
        assert gc.worst_ratio(ref, ref, b) == 0.0
        off = ref.copy()
        off[0, 3, 0, 0] += 1e-3
        assert gc.worst_ratio(off, ref, b) == np.inf, "a pass-through element must match exactly"
