"""KID and density / coverage on the MI355X (csrc/adm_eval.hip: PW_KID, PW_COUNT; ldmae_amd/evaluator.py) against the f64 restatements
and derived bounds of kid_check.py: exact integer cases compared by bits, Gaussian features inside their bounds, every result the same
for every column split, the two Evaluator methods and the command line.

The worst |error| / bound of the KID sums on Gaussian features is printed by test_kid_gaussian_within_bound (run with -s), not fixed in
advance; the run that accompanied this file gave 7.0e-4 (D = 40, m = 70), 5.9e-4 (37, 70), 4.5e-4 (40, 200), 1.5e-4 (37, 200): DESIGN.md
section 22."""
import re

import numpy as np
import pytest
import torch

import kid_check as kc

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.cpu().numpy().view(np.int64)


# ------------------------------------------------------------------------------------------------ 1. KID, exact
def test_kid_exact_integer_case_bitwise():
    from ldmae_amd import ops
    rng = np.random.default_rng(11)
    Na, Nb, D, S, m = 150, 131, 16, 3, 70          # m = 70: a ragged row tile (70 of 128) and a ragged second column tile (6 of 64)
    a, b = rng.integers(-2, 3, (Na, D)), rng.integers(-2, 3, (Nb, D))
    idx_a = np.stack([rng.permutation(Na)[:m] for _ in range(S)]).astype(np.int32)
    idx_b = np.stack([rng.permutation(Nb)[:m] for _ in range(S)]).astype(np.int32)
    for idx, s, shared, n in ((idx_a, 1, idx_a[0, 10:30], Na), (idx_b, 2, idx_b[0, 40:60], Nb)):      # rows repeated across subsets
        rest = np.setdiff1d(np.arange(n), shared)
        idx[s] = np.concatenate([shared, rng.permutation(rest)[:m - 20]])
    for s in range(S):
        assert len(set(idx_a[s].tolist())) == m and len(set(idx_b[s].tolist())) == m
    assert len(set(idx_a[0].tolist()) & set(idx_a[1].tolist())) >= 20
    want = kc.kid_sums_exact(a, b, idx_a, idx_b, 16)
    at, bt = torch.from_numpy(a.astype(np.float32)).cuda(), torch.from_numpy(b.astype(np.float32)).cuda()
    got = {ns: ops.kid_sums(at, bt, idx_a, idx_b, 1.0 / 16, 1.0, nsplit=ns) for ns in (1, 2)}
    for ns, g in got.items():
        assert g.shape == (S, 3) and g.dtype == torch.float64
        assert np.array_equal(_bits(g), want.view(np.int64)), (ns, g.cpu().numpy(), want)
    for kw in (dict(diagonal=True), dict(drop_row_mask=True), dict(num=16)):
        wrong = kc.kid_sums_exact(a, b, idx_a, idx_b, 16, **kw)
        assert not np.array_equal(wrong, want) and not np.array_equal(_bits(got[1]), wrong.view(np.int64)), kw


# ------------------------------------------------------------------------------------------------ 2. KID, Gaussian
@pytest.mark.parametrize("D", [40, 37])             # 40: float4 fetch with a K tail (40 = 2 * 16 + 8); 37: the element path
@pytest.mark.parametrize("m", [70, 200])            # 200: two row tiles, four column tiles
def test_kid_gaussian_within_bound(D, m):
    from ldmae_amd import ops
    rng = np.random.default_rng(100 * D + m)
    Na, Nb, S = 260, 231, 2
    a = rng.normal(0.2, 1.0, (Na, D)).astype(np.float32)
    b = rng.normal(0.0, 1.3, (Nb, D)).astype(np.float32)
    idx_a = np.stack([rng.permutation(Na)[:m] for _ in range(S)]).astype(np.int32)
    idx_b = np.stack([rng.permutation(Nb)[:m] for _ in range(S)]).astype(np.int32)
    gamma = 1.0 / D
    ref, bound = kc.kid_sums_ref(a, b, idx_a, idx_b, gamma, 1.0)
    at, bt = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    g1 = ops.kid_sums(at, bt, idx_a, idx_b, gamma, 1.0, nsplit=1)
    g3 = ops.kid_sums(at, bt, idx_a, idx_b, gamma, 1.0, nsplit=3)
    assert np.array_equal(_bits(g1), _bits(g3)), "the sums must not depend on the column split"
    assert np.array_equal(_bits(g1), _bits(ops.kid_sums(at, bt, idx_a, idx_b, gamma, 1.0))), "nor on the default split"
    worst = kc.worst_ratio(g1.cpu().numpy(), ref, bound)
    print(f"kid_sums D={D} m={m}: worst |error| / bound = {worst:.3g}")
    assert worst <= 1.0, (worst, g1.cpu().numpy(), ref.astype(np.float64), bound)
    assert float(np.abs(ref[:, 0]).min()) > 0 and not np.array_equal(ref[:, 0], ref[:, 1])


# ------------------------------------------------------------------------------------------------ 3. ball counts, exact
def test_ball_counts_exact_integer_case_with_ties():
    from ldmae_amd import ops
    rng = np.random.default_rng(12)
    M, N, D = 150, 70, 8
    u, v = rng.integers(-2, 3, (M, D)).astype(np.float32), rng.integers(-2, 3, (N, D)).astype(np.float32)
    ut, vt = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
    r = ops.knn_radii(ut, (3,))[:, 0].contiguous()
    nu, nv = (u.astype(np.float64) ** 2).sum(1), (v.astype(np.float64) ** 2).sum(1)
    rn = r.cpu().numpy()
    np.testing.assert_array_equal(rn, np.sort(kc.sqdist64(u, nu, u, nu), 1)[:, 3])          # exact integer radii
    want = kc.ball_counts_ref(u, nu, rn, v, nv)
    loose = kc.ball_counts_ref(u, nu, rn, v, nv, strict=False)
    assert not np.array_equal(want, loose), "the input must hold ties d == r"
    for ns in (1, 2, None):
        got = ops.ball_counts(ut, r, vt, nsplit=ns)
        assert got.shape == (M,) and got.dtype == torch.int32
        np.testing.assert_array_equal(got.cpu().numpy().astype(np.int64), want)
    assert 0 < want.sum() < M * N


# ------------------------------------------------------------------------------------------------ 4. ball counts, Gaussian
@pytest.mark.parametrize("D", [37, 40])
def test_ball_counts_gaussian_inside_interval(D):
    from ldmae_amd import ops
    rng = np.random.default_rng(200 + D)
    M, N, k = 150, 131, 5
    u = rng.normal(0, 1, (M, D)).astype(np.float32)
    v = rng.normal(0.1, 0.9, (N, D)).astype(np.float32)
    ut, vt = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
    nu, nv = ops.row_sqnorms(ut), ops.row_sqnorms(vt)
    r = ops.knn_radii(ut, (k,), norms=nu)[:, 0].contiguous()
    lo, hi, und = kc.ball_counts_interval(torch.from_numpy(u), nu.cpu(), r.cpu(), torch.from_numpy(v), nv.cpu())
    print(f"ball_counts D={D}: undecided pairs {und:.3%}")
    assert und <= 0.01, und
    g1 = ops.ball_counts(ut, r, vt, nu=nu, nv=nv, nsplit=1)
    g2 = ops.ball_counts(ut, r, vt, nu=nu, nv=nv, nsplit=2)
    assert torch.equal(g1, g2), "the counts must not depend on the column split"
    kc.check_counts(f"ball_counts D={D}", g1.cpu().numpy(), lo, hi)
    assert 0 < int(hi.sum()) and int(lo.sum()) < M * N and int((lo > 0).sum()) > 0


# ------------------------------------------------------------------------------------------------ 5. end to end
@pytest.fixture(scope="module")
def feats():
    rng = np.random.default_rng(31)
    return rng.normal(0, 1, (180, 48)).astype(np.float32), rng.normal(0.15, 1.1, (160, 48)).astype(np.float32)


def test_evaluator_compute_kid(feats):
    from ldmae_amd import evaluator as ev
    ref_f, sam_f = feats
    e = ev.Evaluator(state_dict={})
    S, m, seed = 4, 90, 5
    mean, std = e.compute_kid(ref_f, sam_f, num_subsets=S, subset_size=m, seed=seed)
    idx1, idx2 = ev.kid_subset_indices(180, 160, S, m, seed)
    sums, bound = kc.kid_sums_ref(ref_f, sam_f, idx1, idx2, 1.0 / 48, 1.0)
    wmean, wstd, _ = kc.kid_from_sums_ref(sums.astype(np.float64), m)
    bm, bs = kc.kid_bound(bound, m)
    host = kc.kid_host_term(sums.astype(np.float64), m) + np.abs(sums.astype(np.float64) - sums).astype(np.float64).max() / (m * (m - 1))
    print(f"compute_kid: {mean} +- {std} (f64 {wmean} +- {wstd}); |d mean| / bound {abs(mean - wmean) / (bm + host):.3g}")
    assert abs(mean - wmean) <= bm + host and abs(std - wstd) <= bs + host
    assert wmean > 0 and wstd > 0
    assert e.compute_kid(ref_f, sam_f, num_subsets=S, subset_size=m, seed=seed) == (mean, std), "bitwise reproducible"
    assert e.compute_kid(ref_f, sam_f, num_subsets=S, subset_size=m, seed=seed + 1) != (mean, std)
    g = e.compute_kid(ref_f, sam_f, num_subsets=S, subset_size=m, seed=seed, gamma=1.0 / 48)
    assert g == (mean, std), "gamma=None is 1 / D"


def test_evaluator_compute_density_coverage(feats):
    from ldmae_amd import evaluator as ev
    ref_f, sam_f = feats
    e = ev.Evaluator(state_dict={})
    for k in (5, 1, 7):
        density, coverage = e.compute_density_coverage(ref_f, sam_f, nearest_k=k)
        (dlo, dhi), (clo, chi), und = kc.density_coverage_interval(torch.from_numpy(ref_f), torch.from_numpy(sam_f), k)
        wd, wc, _ = kc.density_coverage_ref(ref_f, sam_f, k)
        print(f"density / coverage k={k}: {density} / {coverage} (f64 {wd} / {wc}); undecided {und:.3%}")
        assert und <= 0.01
        tiny = 4 * 2.0 ** -53
        assert dlo * (1 - tiny) <= density <= dhi * (1 + tiny) and clo - tiny <= coverage <= chi + tiny
        assert dlo <= wd <= dhi and clo <= wc <= chi and 0 < wd and 0 < wc <= 1
    assert ev.Evaluator(state_dict={}, nsplit=1).compute_density_coverage(ref_f, sam_f, 5) == e.compute_density_coverage(ref_f, sam_f, 5)


def _images(n, h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w] / max(h, w)
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        f = rng.uniform(1, 6, (3, 2))
        ph = rng.uniform(0, 6.3, 3)
        img = np.stack([np.sin(f[c, 0] * 6.3 * yy + f[c, 1] * 6.3 * xx + ph[c]) for c in range(3)], -1)
        out[i] = np.clip(127.5 + 100 * img + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)
    return out


FIVE = ("Inception Score", "FID", "sFID", "Precision", "Recall")


def test_cli_new_lines_after_the_five_unchanged_ones(tmp_path, capsys):
    from ldmae_amd import evaluator as ev, fid
    sd = fid.random_state_dict(5)
    g = torch.Generator().manual_seed(6)
    sd["fc.weight"] = torch.randn(1008, 2048, generator=g) * 0.05
    wpath = tmp_path / "inception.pth"
    torch.save(sd, wpath)
    np.savez(tmp_path / "ref.npz", arr_0=_images(24, 64, 64, 21))
    np.savez(tmp_path / "sample.npz", arr_0=_images(20, 64, 64, 22))
    base = [str(tmp_path / "ref.npz"), str(tmp_path / "sample.npz"), "--weights", str(wpath), "--batch-size", "12"]
    e = ev.Evaluator(state_dict=sd, batch_size=12)
    for name in ("ref.npz", "sample.npz"):          # fill the .npz caches: both runs below read the same stored activations and statistics
        ev.activations_and_statistics(e, tmp_path / name)
    ev.main(base)
    plain = capsys.readouterr().out
    assert not re.search(r"^(KID|Density|Coverage):", plain, re.M), "without the flags nothing new is printed"
    with np.load(tmp_path / "ref.npz") as z:
        files_before = sorted(z.files)
        act_ref = z["act"]
    with np.load(tmp_path / "sample.npz") as z:
        act_sample = z["act"]
    out = ev.main(base + ["--kid", "--kid-subsets", "3", "--kid-subset-size", "16", "--kid-seed", "9", "--density-coverage", "--nearest-k", "3"])
    full = capsys.readouterr().out
    assert full.startswith(plain), "the existing lines are byte for byte what they are without the flags"
    tail = full[len(plain):].splitlines()
    assert [t.split(":")[0] for t in tail] == ["KID", "Density", "Coverage"], tail
    assert [ln.split(":")[0] for ln in plain.splitlines()[-5:]] == list(FIVE)
    with np.load(tmp_path / "ref.npz") as z:
        assert sorted(z.files) == files_before == sorted(("arr_0",) + ev.CACHE_KEYS), "nothing new in the cache"
    kid = e.compute_kid(act_ref, act_sample, num_subsets=3, subset_size=16, seed=9)
    dc = e.compute_density_coverage(act_ref, act_sample, nearest_k=3)
    assert tail[0] == f"KID: {kid[0]} +- {kid[1]}" and tail[1] == f"Density: {dc[0]}" and tail[2] == f"Coverage: {dc[1]}"
    assert (out["kid_mean"], out["kid_std"], out["density"], out["coverage"]) == (*kid, *dc)
