"""KID and density / coverage without a GPU: the subset draws, the estimator from the kernel's sums, the refusals that run before any kernel,
the four new C-ABI symbols and the command line's flags."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import kid_check as kc
from ldmae_amd import evaluator as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ldmae_kid_workspace_bytes", "ldmae_kid_sums", "ldmae_ball_counts_partials_bytes", "ldmae_ball_counts")


# ------------------------------------------------------------------------------------------------ subset indices
def test_subset_indices_reproducible_without_repeats():
    a1, b1 = ev.kid_subset_indices(50, 37, 6, 30, seed=7)
    a2, b2 = ev.kid_subset_indices(50, 37, 6, 30, seed=7)
    a3, _ = ev.kid_subset_indices(50, 37, 6, 30, seed=8)
    assert a1.shape == b1.shape == (6, 30) and a1.dtype == b1.dtype == np.int32
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(b1, b2)
    assert not np.array_equal(a1, a3)
    for s in range(6):
        assert len(set(a1[s].tolist())) == 30 and len(set(b1[s].tolist())) == 30, "no repeats inside a subset"
        assert 0 <= a1[s].min() and a1[s].max() < 50 and 0 <= b1[s].min() and b1[s].max() < 37
    assert not np.array_equal(a1[0], a1[1]), "subsets differ"


def test_subset_indices_alternate_the_two_choice_calls():
    """RandomState(seed): choice(n1), choice(n2), choice(n1), ... -- one stream, the two sets taking turns."""
    rng = np.random.RandomState(2020)
    a, b = ev.kid_subset_indices(41, 29, 4, 11, seed=2020)
    for s in range(4):
        np.testing.assert_array_equal(a[s], rng.choice(41, 11, replace=False))
        np.testing.assert_array_equal(b[s], rng.choice(29, 11, replace=False))
    # the wrong order (all of set 1 first) gives other tables
    rng = np.random.RandomState(2020)
    first = np.stack([rng.choice(41, 11, replace=False) for _ in range(4)])
    assert not np.array_equal(first, a)


# ------------------------------------------------------------------------------------------------ the estimator
def _gram_kid(x, y, gamma, coef0):
    """One subset, straight from the definition: Gram matrices in f64."""
    m = x.shape[0]
    kxx, kyy, kxy = (gamma * x @ x.T + coef0) ** 3, (gamma * y @ y.T + coef0) ** 3, (gamma * x @ y.T + coef0) ** 3
    return ((kxx.sum() - np.trace(kxx)) / (m * (m - 1)) + (kyy.sum() - np.trace(kyy)) / (m * (m - 1)) - 2 * kxy.mean(),
            (kxx.sum() - np.trace(kxx), kyy.sum() - np.trace(kyy), kxy.sum()))


def test_kid_from_sums_against_gram_matrices():
    rng = np.random.default_rng(3)
    a, b = rng.normal(0, 1, (12, 5)), rng.normal(0.3, 1.2, (12, 5))
    idx_a = np.stack([rng.permutation(12)[:8] for _ in range(3)])
    idx_b = np.stack([rng.permutation(12)[:8] for _ in range(3)])
    want, sums = zip(*[_gram_kid(a[idx_a[s]], b[idx_b[s]], 0.2, 1.0) for s in range(3)])
    mean, std = ev.kid_from_sums(np.array(sums), 8)
    assert abs(mean - np.mean(want)) <= 1e-13 * (1 + abs(np.mean(want)))
    assert abs(std - np.std(want)) <= 1e-13 * (1 + np.std(want)), "numpy.std: the population form"
    # the restatement of kid_check agrees with the same definition
    ref, _ = kc.kid_sums_ref(a.astype(np.float32), b.astype(np.float32), idx_a, idx_b, 0.2, 1.0)
    g32 = kc.f32(0.2)
    _, sums32 = zip(*[_gram_kid(a.astype(np.float32).astype(np.float64)[idx_a[s]], b.astype(np.float32).astype(np.float64)[idx_b[s]], g32, 1.0)
                      for s in range(3)])
    np.testing.assert_allclose(ref.astype(np.float64), np.array(sums32), rtol=1e-12)


def test_kid_of_a_set_against_itself_is_negative_and_known():
    """a is b with equal index tables: aa = bb = T - tr and ab = T (T the sum of the whole Gram matrix, tr its trace), so
    mmd^2 = 2 (T - tr) / (m (m - 1)) - 2 T / m^2 = 2 (T - m tr) / (m^2 (m - 1)): negative by Cauchy-Schwarz (k is a kernel: T <= m tr)."""
    rng = np.random.default_rng(4)
    a = rng.normal(0, 1, (12, 6))
    idx = np.stack([np.arange(12), rng.permutation(12)])
    m = 12
    sums, closed = [], []
    for s in range(2):
        x = a[idx[s]]
        k = (x @ x.T / 6 + 1.0) ** 3
        T, tr = k.sum(), np.trace(k)
        sums.append((T - tr, T - tr, T))
        closed.append(2 * (T - m * tr) / (m * m * (m - 1)))
    mean, std = ev.kid_from_sums(np.array(sums), m)
    assert closed[0] < 0 and abs(closed[0] - closed[1]) <= 1e-12 * abs(closed[0]), "a permutation of the same rows: the same value"
    assert abs(mean - closed[0]) <= 1e-12 * abs(closed[0]) and std <= 1e-12 * abs(closed[0])


def test_exact_restatement_variants_differ():
    """The three wrong variants of kid_check.kid_sums_exact differ from the right one on a small integer case (the GPU test relies on it)."""
    rng = np.random.default_rng(5)
    a, b = rng.integers(-2, 3, (20, 16)), rng.integers(-2, 3, (17, 16))
    idx_a, idx_b = ev.kid_subset_indices(20, 17, 2, 9, 0)
    right = kc.kid_sums_exact(a, b, idx_a, idx_b, 16)
    for kw in (dict(diagonal=True), dict(drop_row_mask=True), dict(num=16)):
        assert not np.array_equal(right, kc.kid_sums_exact(a, b, idx_a, idx_b, 16, **kw)), kw
    ref, _ = kc.kid_sums_ref(a.astype(np.float32), b.astype(np.float32), idx_a, idx_b, 1 / 16, 1.0)
    np.testing.assert_array_equal(ref.astype(np.float64), right)


# ------------------------------------------------------------------------------------------------ refusals before any kernel
def test_subset_size_above_the_smaller_set_is_refused_by_name():
    e = ev.Evaluator(state_dict={})
    ref, sample = np.zeros((30, 8), np.float32), np.zeros((20, 8), np.float32)
    with pytest.raises(ValueError, match=r"subset_size 21 .*20 rows.*subset_size=20"):
        e.compute_kid(ref, sample, num_subsets=2, subset_size=21)
    with pytest.raises(ValueError, match="subset_size 21"):
        ev.kid_subset_indices(30, 20, 2, 21, 0)


@pytest.mark.parametrize("k", [0, 8])
def test_nearest_k_outside_1_to_7_is_refused(k):
    m = ev.ManifoldEstimator()
    x = np.zeros((20, 4), np.float32)
    with pytest.raises(ValueError, match=rf"nearest_k {k} outside 1\.\.7"):
        m.density_coverage(x, x, nearest_k=k)
    with pytest.raises(ValueError, match="nearest_k"):
        ev.Evaluator(state_dict={}).compute_density_coverage(x, x, nearest_k=k)


@pytest.mark.parametrize("bad,where", [(-1, (1, 2)), (10, (0, 3))])
def test_index_outside_the_feature_rows_is_refused_on_the_host(bad, where):
    from ldmae_amd import ops
    idx = np.tile(np.arange(4, dtype=np.int32), (2, 1))
    ok = ops.check_kid_index_table(idx, 10, "idx_a")
    assert ok.dtype == torch.int32 and ok.shape == (2, 4) and not ok.is_cuda
    idx[where] = bad
    with pytest.raises(ValueError, match=rf"idx_a\[{where[0]}, {where[1]}\] = {bad} \(subset {where[0]}, position {where[1]}\) is outside \[0, 10\)"):
        ops.check_kid_index_table(idx, 10, "idx_a")
    with pytest.raises(ValueError, match="S, m"):
        ops.check_kid_index_table(np.arange(4), 10, "idx_b")


def _refused(fn, *args, **kw):
    with pytest.raises((RuntimeError, ValueError)) as e:
        fn(*args, **kw)
    return str(e.value)


def test_wrapper_argument_checks_run_before_any_kernel():
    """ops._arg checks attributes only, so host tensors reach every refusal (and, with everything right, the device-pointer refusal)."""
    from ldmae_amd import ops
    F32, F16 = torch.float32, torch.float16
    u, v, ru = torch.zeros(6, 8), torch.zeros(5, 8), torch.zeros(6)
    assert _refused(ops.ball_counts, u.to(F16), ru, v).startswith("ball_counts u: dtype")
    assert _refused(ops.ball_counts, u, ru, torch.zeros(5, 9)).startswith("ball_counts v: shape")
    assert _refused(ops.ball_counts, u, torch.zeros(6, 1), v).startswith("ball_counts ru: shape")
    assert _refused(ops.ball_counts, u, torch.zeros(12)[::2], v).startswith("ball_counts ru: the kernel reads")
    assert _refused(ops.ball_counts, torch.zeros(6, 16)[:, ::2], ru, v).startswith("ball_counts u: the kernel reads")
    assert "no CPU fallback" in _refused(ops.ball_counts, u, ru, v, nu=torch.zeros(6), nv=torch.zeros(5), nsplit=1)
    assert _refused(ops.ball_counts, u, ru, v, nu=torch.zeros(6), nv=torch.zeros(5), nsplit=0).startswith("ball_counts: nsplit 0")
    ia, ib = np.zeros((2, 4), np.int32) + np.arange(4, dtype=np.int32), np.zeros((2, 4), np.int32) + np.arange(4, dtype=np.int32)
    assert _refused(ops.kid_sums, u.to(F16), v, ia, ib, 0.1).startswith("kid_sums a: dtype")
    assert _refused(ops.kid_sums, u, torch.zeros(5, 9), ia, ib, 0.1).startswith("kid_sums b: shape")
    assert "one shape" in _refused(ops.kid_sums, u, v, ia, ib[:1], 0.1)
    six = np.tile(np.arange(6, dtype=np.int32), (2, 1))
    assert "idx_b[0, 5] = 5 (subset 0, position 5) is outside [0, 5)" in _refused(ops.kid_sums, u, v, six, six, 0.1)
    assert _refused(ops.kid_sums, u, v, ia, ib, 0.1, nsplit=0).startswith("kid_sums: nsplit 0")
    assert "no CPU fallback" in _refused(ops.kid_sums, u, v, ia, ib, 0.1, nsplit=1)


# ------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_are_declared_and_exported():
    from ldmae_amd import _lib
    header = open(os.path.join(ROOT, "include", "ldmae_hip.h")).read()
    declared = set(re.findall(r"\b(ldmae_[a-z0-9_]+)\s*\(", header))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
        assert hasattr(handle, name), name
    res, args = _lib.SIGNATURES["ldmae_kid_sums"]
    assert res is ctypes.c_int and args.count(ctypes.c_float) == 2 and len(args) == 15
    lib = _lib.load()
    # sizes: one f64 per (subset, sum, 128-row tile, 64-column tile); one int per (row, split, half tile); nonsense is -1
    assert lib.ldmae_kid_workspace_bytes(3, 70) == 3 * 3 * 1 * 2 * 8
    assert lib.ldmae_kid_workspace_bytes(100, 1000) == 100 * 3 * 8 * 16 * 8
    assert lib.ldmae_ball_counts_partials_bytes(150, 2) == 150 * 2 * 2 * 4
    assert lib.ldmae_kid_workspace_bytes(0, 70) == -1 and lib.ldmae_ball_counts_partials_bytes(150, 0) == -1


# ------------------------------------------------------------------------------------------------ command line
def test_cli_flags_parse_and_default_to_off():
    p = ev.build_parser()
    a = p.parse_args(["ref.npz", "sample.npz"])
    assert a.kid is False and a.density_coverage is False
    assert (a.kid_subsets, a.kid_subset_size, a.kid_seed, a.nearest_k) == (100, 1000, 2020, 5)
    a = p.parse_args(["ref.npz", "sample.npz", "--kid", "--kid-subsets", "7", "--kid-subset-size", "33", "--kid-seed", "1", "--density-coverage",
                      "--nearest-k", "3"])
    assert a.kid and a.density_coverage and (a.kid_subsets, a.kid_subset_size, a.kid_seed, a.nearest_k) == (7, 33, 1, 3)
