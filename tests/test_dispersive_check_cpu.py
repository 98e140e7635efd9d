"""The f64 restatement of the Dispersive Loss (tests/dispersive_check.py) against torch's f64 autograd, and the properties of the definition
that the GPU tests lean on.  No GPU."""
import math

import pytest
import torch

from dispersive_check import bounds, loss_autograd, reference, rms_rows

SHAPES = [(5, 1000), (37, 260), (2, 64), (8, 4096), (1, 64)]


def rows(B, K, seed=0, scale=1.0):
    gen = torch.Generator().manual_seed(1000 * B + K + seed)
    return torch.randn(B, K, generator=gen, dtype=torch.float64) * scale


@pytest.mark.parametrize("B,K", SHAPES)
@pytest.mark.parametrize("tau", [0.5, 2.0])
def test_gradient_form_equals_f64_autograd(B, K, tau):
    z = rows(B, K).requires_grad_(True)
    L = loss_autograd(z, tau)
    (g,) = torch.autograd.grad(L, z)
    ref = reference(z, tau)
    assert abs(float(ref["L"]) - float(L.detach())) <= 1e-14 * max(1.0, abs(float(L.detach())))
    # both are f64 evaluations of the same expression: a few 2^-53 of the terms' magnitude sum_j |C_ij z_jk|
    tol = 64 * 2.0 ** -53 * (ref["C"].abs() @ z.detach().abs()) + 1e-300
    assert bool(((ref["dz"] - g).abs() <= tol).all()), float((ref["dz"] - g).abs().max())


@pytest.mark.parametrize("B,K", SHAPES)
def test_gradient_sums_to_zero_and_the_loss_ignores_a_translation(B, K):
    z = rows(B, K, seed=1)
    ref = reference(z, 0.5)
    C = ref["C"]
    assert torch.equal(C, C.t())
    assert float(C.sum(1).abs().max()) <= 16 * 2.0 ** -53 * float(C.abs().sum(1).max()) + 1e-300
    tol = 64 * 2.0 ** -53 * (C.abs() @ z.abs()).sum(0) + 1e-300
    assert bool((ref["dz"].sum(0).abs() <= tol).all())
    shifted = reference(z + rows(1, K, seed=2), 0.5)
    assert abs(float(shifted["L"]) - float(ref["L"])) <= 1e-12
    assert float((shifted["dz"] - ref["dz"]).abs().max()) <= 1e-12 * max(1.0, float(ref["dz"].abs().max()) * K)


def test_one_sample_has_no_loss_and_no_gradient():
    ref = reference(rows(1, 64), 0.5)
    assert float(ref["L"]) == 0.0 and float(ref["S"]) == 1.0
    assert not ref["C"].any() and not ref["dz"].any()


def test_identical_rows_give_zero_loss():
    z = rows(1, 260).expand(6, 260).clone()
    ref = reference(z, 0.5)
    assert float(ref["L"]) == 0.0 and float(ref["S"]) == 36.0


def test_far_rows_underflow_to_minus_log_b_with_a_zero_gradient():
    """rows of rms 30 at K = 4096, tau = 0.5: d_ij / (K tau) is about 3600, every off-diagonal e is exactly 0 in f64."""
    B = 8
    z = rms_rows(B, 4096, 30.0, seed=3)
    ref = reference(z, 0.5)
    off = ref["e"] - torch.eye(B, dtype=torch.float64)
    assert not off.any()
    assert float(ref["S"]) == float(B) and abs(float(ref["L"]) + math.log(B)) <= 2.0 ** -51 * math.log(B)
    assert not ref["C"].any() and not ref["dz"].any()


def test_bounds_are_positive_finite_and_zero_where_the_result_is_exact():
    z = rms_rows(5, 1000, 1.0, seed=4)
    ref, b = bounds(z, 0.5, slab=1024, slabs=1, g=0.25)
    assert 0.0 < b["L"] < 1e-2 and bool(torch.isfinite(b["C"]).all()) and bool(torch.isfinite(b["dz"]).all())
    assert bool((b["C"] > 0).all()) and bool((b["dz"] > 0).all())
    # the bound is far below the values it guards: a transposed or shifted tile would not fit under it
    assert float(b["C"].max()) < 1e-2 * float(ref["C"].abs().max())
