"""Linear probe and k-NN on the MI355X (csrc/linprobe.hip, ldmae_amd/linear_probe.py) against the f64 restatements and derived bounds of
linprobe_check.py: ranks and top-k lists compared exactly, everything else inside its bound; the driver end to end on a tiny seeded VMAE.

Each kernel test prints its worst |error| / bound (run with -s); none of those figures enters a bound."""
import json

import numpy as np
import pytest
import torch

import linprobe_check as lc

pytestmark = pytest.mark.gpu


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to("cuda", dtype)


def _worst(got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return float((err / np.maximum(bound, 1e-300)).max()), err


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


# ------------------------------------------------------------------------------------------------ softmax cross-entropy
def _xent_logits(B, C, seed):
    """Gaussian logits with everything the issue asks for planted: +-80 entries (overflow without the max shift), labels in the first and
    last columns, exact ties with the label's logit on both sides of it."""
    rng = np.random.default_rng(seed)
    l = rng.normal(0, 3, (B, C)).astype(np.float32)
    y = rng.integers(0, C, B)
    y[0] = 0
    y[-1] = C - 1
    if B > 2:
        y[1] = C // 2
    for b in range(B):
        if b % 3 == 0:
            l[b, rng.integers(0, C, max(1, C // 50))] = np.float32(80 if b % 2 == 0 else -80)
        if b % 2 == 1 and C >= 3:                                   # ties: copies of the label's logit below and above the label
            lo, hi = rng.integers(0, max(y[b], 1), 2), rng.integers(min(y[b] + 1, C - 1), C, 2)
            l[b, lo] = l[b, y[b]]
            l[b, hi] = l[b, y[b]]
    if B > 4 and C > 4:
        l[4] = np.float32(-80)
        l[4, y[4]] = np.float32(80)                                 # the whole row at the extremes
    return l, y.astype(np.int64)


@pytest.mark.parametrize("C", [1, 5, 1000, 1003, 2048, 4099])      # 2048: the 16-register path (1025 .. 4096), not in the issue's list
@pytest.mark.parametrize("B", [1, 3, 257])
def test_softmax_xent(B, C):
    from ldmae_amd import ops
    l, y = _xent_logits(B, C, 1000 * B + C)
    ld = C + 5                                                      # a row stride larger than C, the tail poisoned
    buf = torch.full((B, ld), float("nan"), device="cuda")
    buf[:, :C] = _dev(l)
    gs = 1.0 / 7
    dl = torch.full((B, ld), 777.0, device="cuda")
    loss, rank, _ = ops.softmax_xent(buf[:, :C], torch.from_numpy(y), grad_scale=gs, dlogits=dl[:, :C])
    loss2, rank2, none = ops.softmax_xent(buf[:, :C], torch.from_numpy(y))
    assert none is None and torch.equal(loss, loss2) and torch.equal(rank, rank2)
    r = lc.softmax_xent_ref(l, y, gs)
    assert rank.dtype == torch.int32 and np.array_equal(rank.cpu().numpy(), r["rank"]), "ranks are exact: every row"
    w_loss, _ = _worst(loss.cpu().numpy(), r["loss"], r["dloss"])
    d = dl[:, :C].cpu().numpy()
    w_d, _ = _worst(d, r["dlogits"], r["ddlogits"])
    rowsum = np.abs(d.astype(np.float64).sum(axis=1))
    w_s = float((rowsum / r["ddlogits"].sum(axis=1)).max())
    print(f"softmax_xent B={B} C={C}: worst err / bound: loss {w_loss:.3f}, dlogits {w_d:.3f}, row sums {w_s:.3f}")
    assert np.isfinite(loss.cpu().numpy()).all() and w_loss <= 1 and w_d <= 1 and w_s <= 1
    assert bool((dl[:, C:] == 777.0).all()), "columns beyond C are not written"
    top1, top5 = (rank == 0), (rank < 5)
    assert bool((top1 <= top5).all())


def test_softmax_xent_tie_rule_and_bad_label():
    from ldmae_amd import ops
    l = _dev([[1.0, 3.0, 3.0, 0.5, 3.0]] * 5)
    _, rank, _ = ops.softmax_xent(l, torch.arange(5))
    assert rank.tolist() == [3, 0, 1, 4, 2]
    with pytest.raises(ValueError, match=r"labels\[2\] = 5"):
        ops.softmax_xent(l, torch.tensor([0, 1, 5, 2, 3]))
    loss, rank, dl = ops.softmax_xent(l, torch.tensor([0, 1, -1, 2, 7], device="cuda"), grad_scale=1.0)     # device labels are trusted: the guard
    assert rank.tolist() == [3, 0, -1, 1, -1] and torch.isnan(loss[[2, 4]]).all() and not dl[[2, 4]].any()


# ------------------------------------------------------------------------------------------------ bn1d
@pytest.mark.parametrize("D", [1, 16, 192, 1000])
@pytest.mark.parametrize("B", [2, 3, 1000])
def test_bn1d(B, D):
    from ldmae_amd import ops
    rng = np.random.default_rng(B * 7 + D)
    x = rng.normal(0.3, 2.0, (B, D)).astype(np.float32)
    x[:, 0] = (1e3 + 1e-2 * rng.standard_normal(B)).astype(np.float32)      # fails an E[x^2] - mean^2 formulation
    if D > 2:
        x[:, D - 1] = np.float32(3.7)                                       # a constant column
    rm0, rv0 = rng.normal(0, 1, D).astype(np.float32), rng.uniform(0.5, 2, D).astype(np.float32)
    rm, rv = _dev(rm0), _dev(rv0)
    xd = torch.full((B, D + 3), float("nan"), device="cuda")
    xd[:, :D] = _dev(x)
    out, sm, sr = ops.bn1d_fwd(xd[:, :D], rm, rv, training=True, eps=1e-6, momentum=0.1, save=True)
    r = lc.bn1d_ref(x, 1e-6, rm0, rv0, 0.1)
    res = {"xhat": _worst(out.cpu().numpy(), r["xhat"], r["bound"])[0], "mean": _worst(sm.cpu().numpy(), r["mean"], r["dmean"])[0],
           "rstd": _worst(sr.cpu().numpy(), r["rstd"], r["drstd"])[0], "run_mean": _worst(rm.cpu().numpy(), r["run_mean"], r["drun_mean"])[0],
           "run_var": _worst(rv.cpu().numpy(), r["run_var"], r["drun_var"])[0]}
    print(f"bn1d B={B} D={D}: worst err / bound {res}")
    assert all(v <= 1 for v in res.values()), res
    if D > 2:
        assert not out[:, D - 1].any(), "a constant column normalises to exact zeros"
    if B == 1000:
        naive = lc.bn1d_naive_f32(x[:, :1], 1e-6)
        assert (np.abs(naive - r["xhat"][:, :1]) > 10 * r["bound"][:, :1]).mean() > 0.5, "the fixture must defeat the one-pass formulation"
    # eval mode: the running statistics as they now are, nothing updated
    rm1, rv1 = rm.clone(), rv.clone()
    ev = ops.bn1d_fwd(xd[:, :D], rm, rv, training=False, eps=1e-6)
    ref, bound = lc.bn1d_eval_ref(x, 1e-6, rm1.cpu().numpy(), rv1.cpu().numpy())
    w = _worst(ev.cpu().numpy(), ref, bound)[0]
    assert w <= 1 and torch.equal(rm, rm1) and torch.equal(rv, rv1), w
    one = ops.bn1d_fwd(xd[:1, :D], rm, rv, training=False, eps=1e-6)          # a single row is fine in eval mode
    assert torch.equal(one, ev[:1])
    with pytest.raises(ValueError, match="more than 1 value"):
        ops.bn1d_fwd(xd[:1, :D], rm, rv, training=True)


# ------------------------------------------------------------------------------------------------ token_mean
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [16, 192])
@pytest.mark.parametrize("N", [1, 255, 256, 1024])
def test_token_mean(N, D, dtype):
    from ldmae_amd import ops
    rng = np.random.default_rng(N + D)
    B = 3
    x = _dev(rng.normal(0.5, 1.0, (B, N, D)), dtype)
    ref, bound = lc.token_mean_ref(x.float().cpu().numpy())
    a, b = ops.token_mean(x), ops.token_mean(x)
    assert a.dtype == torch.float32 and a.shape == (B, D) and np.array_equal(_bits(a), _bits(b)), "two runs: the same bits"
    w = _worst(a.cpu().numpy(), ref, bound)[0]
    print(f"token_mean N={N} D={D} {dtype}: worst err / bound {w:.3f}")
    assert w <= 1
    if D == 16:                                                     # a channel slice: col0 = 8 of token rows 32 apart, as a view and by argument
        wide = _dev(rng.normal(0, 1, (B, N, 32)), dtype)
        ref, bound = lc.token_mean_ref(wide.float().cpu().numpy(), 8, 16)
        v, c = ops.token_mean(wide[..., 8:24]), ops.token_mean(wide, col0=8, d=16)
        assert np.array_equal(_bits(v), _bits(c)) and _worst(v.cpu().numpy(), ref, bound)[0] <= 1


def test_token_mean_fp16_and_refusals():
    from ldmae_amd import ops
    x = _dev(np.random.default_rng(0).normal(0, 1, (2, 40, 16)), torch.float16)
    ref, bound = lc.token_mean_ref(x.float().cpu().numpy())
    assert _worst(ops.token_mean(x).cpu().numpy(), ref, bound)[0] <= 1
    with pytest.raises(RuntimeError, match="token_mean"):
        ops.token_mean(x.double())
    with pytest.raises(RuntimeError, match="strides"):
        ops.token_mean(x.transpose(1, 2))


# ------------------------------------------------------------------------------------------------ LARS
@pytest.mark.parametrize("case", ["main", "zero_p", "zero_update"])
def test_lars_golden_trajectory(golden, case):
    from ldmae_amd import ops
    g = golden("linprobe")
    wd, momentum, trust = (float(v) for v in g[case + "_hp"])
    worst = 0.0
    for which, scaled in (("w", True), ("b", False)):
        p0, grads, lrs = g[f"{case}_p0_{which}"], g[f"{case}_g{which}"], g[case + "_lr"]
        steps = len(lrs)
        ps, mus, eps, emus = lc.lars_trajectory_ref(p0.reshape(-1), grads.reshape(steps, -1), lrs, wd, momentum, trust, scaled)
        p, mu = _dev(p0), torch.zeros(p0.shape, device="cuda")
        for s in range(steps):
            assert np.allclose(ps[s], g[f"{case}_{which}"][s].reshape(-1), rtol=1e-13, atol=1e-300)      # the restatement IS the reference's trajectory
            gr = _dev(grads[s])
            norms = ops.lars_norms(p, gr, wd) if scaled else None
            ops.lars_step(p, gr, mu, float(lrs[s]), norms, wd, momentum, trust)
            for got, ref, bound, name in ((p, ps[s], eps[s], "p"), (mu, mus[s], emus[s], "mu")):
                w, err = _worst(got.cpu().numpy().reshape(-1), ref, bound)
                if bound.max() == 0:
                    assert err.max() == 0, (case, which, s, name)
                else:
                    worst = max(worst, w)
                    assert w <= 1, (case, which, s, name, w)
    print(f"lars {case}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("n", [1, 4097, 16000])
def test_lars_sizes_and_determinism(n):
    from ldmae_amd import ops
    rng = np.random.default_rng(n)
    p0, g0 = rng.normal(0, 0.05, n).astype(np.float32), rng.normal(0, 0.3, n).astype(np.float32)
    wd, momentum, trust, lr = 0.0625, 0.9, 0.001, 1.5
    runs = []
    for _ in range(2):
        p, mu, g = _dev(p0), torch.zeros(n, device="cuda"), _dev(g0)
        norms = ops.lars_norms(p, g, wd)
        for _s in range(2):
            ops.lars_step(p, g, mu, lr, ops.lars_norms(p, g, wd), wd, momentum, trust)
        runs.append((norms, p, mu))
    for a, b in zip(*runs):
        assert np.array_equal(_bits(a), _bits(b)), "two runs: the same bits"
    dp = g0.astype(np.float64) + wd * p0.astype(np.float64)
    want = np.array([np.sqrt((p0.astype(np.float64) ** 2).sum()), np.sqrt((dp ** 2).sum())])
    err = np.abs(runs[0][0].cpu().numpy() - want)
    assert (err <= lc.SECOND * (2 * lc.U * want + lc.U * wd * np.sqrt((p0.astype(np.float64) ** 2).sum()))).all(), (err, want)
    ps, mus, eps, emus = lc.lars_trajectory_ref(p0, [g0, g0], [lr, lr], wd, momentum, trust, True)
    assert _worst(runs[0][1].cpu().numpy(), ps[-1], eps[-1])[0] <= 1 and _worst(runs[0][2].cpu().numpy(), mus[-1], emus[-1])[0] <= 1


# ------------------------------------------------------------------------------------------------ top-k merge
@pytest.mark.parametrize("k", [1, 20, 200])
@pytest.mark.parametrize("width", [1, 7, 1000])
@pytest.mark.parametrize("M", [1, 65])
def test_topk_merge(M, width, k):
    from ldmae_amd import ops
    rng = np.random.default_rng(M * 31 + width * 7 + k)
    N = {1: 9, 7: 50, 1000: 2300}[width]                            # 9 and 50 bank rows: fewer than k = 20 / 200
    S = rng.normal(0, 1, (M, N)).astype(np.float32)
    S[:, rng.integers(0, N, max(N // 3, 1))] = np.float32(0.25)      # many equal values ...
    for c in range(width - 1, N - 1, 2 * width):
        S[:, c + 1] = S[:, c]                                       # ... and one pair across every other chunk boundary
    S[0, :] = np.float32(1.5)                                       # a whole row of ties: the order is the index order
    Sd = _dev(S)
    vals, idx = ops.topk_empty(M, k, "cuda")
    for c0 in range(0, N, width):
        ops.topk_merge(Sd[:, c0:c0 + width], c0, vals, idx)         # row-strided column slices of the one matrix
    wv, wi = lc.topk_ref(S, k)
    assert np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(_bits(vals), wv.view(np.int32)), (M, width, k)
    if width > 1:                                                   # the chunking does not matter: one chunk, and the chunks in reverse order
        for order in ([0], list(range(0, N, width))[::-1]):
            v2, i2 = ops.topk_empty(M, k, "cuda")
            for c0 in order:
                w = N if order == [0] else width
                ops.topk_merge(Sd[:, c0:c0 + w], c0, v2, i2)
            assert torch.equal(i2, idx) and np.array_equal(_bits(v2), _bits(vals))


def test_topk_refusals():
    from ldmae_amd import ops
    with pytest.raises(ValueError, match="256"):
        ops.topk_empty(2, 257, "cuda")
    S = torch.zeros(2, 8, device="cuda")
    with pytest.raises(ValueError, match="256"):
        ops.topk_merge(S, 0, torch.zeros(2, 300, device="cuda"), torch.zeros(2, 300, dtype=torch.int32, device="cuda"))
    S[0, 3] = float("nan")
    vals, idx = ops.topk_empty(2, 8, "cuda")
    ops.topk_merge(S, 0, vals, idx)
    assert idx[0].tolist() == [0, 1, 2, 4, 5, 6, 7, -1] and idx[1].tolist() == list(range(8)), "a NaN similarity is never taken"


# ------------------------------------------------------------------------------------------------ k-NN vote
def _clusters(C, per, D, seed, spread=0.15):
    """`per` unit vectors around each of C seeded centres (the centres depend on C alone, the samples on `seed`)."""
    cent = np.random.default_rng(C).normal(0, 1, (C, D))
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    rng = np.random.default_rng(seed)
    lab = np.repeat(np.arange(C), per)
    x = cent[lab] + spread * rng.normal(0, 1, (C * per, D))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), lab.astype(np.int64)


@pytest.mark.parametrize("C,k", [(4, 20), (10, 5), (1000, 20)])
def test_knn_vote(C, k):
    from ldmae_amd import ops
    per = {4: 40, 10: 12, 1000: 2}[C]
    bank, bl = _clusters(C, per, 16, 11)
    q, ql = _clusters(C, {4: 30, 10: 8, 1000: 1}[C], 16, 12)
    q, ql = q[:200], ql[:200]
    S = (q.astype(np.float64) @ bank.astype(np.float64).T).astype(np.float32)
    wv, wi = lc.topk_ref(S, k)
    scores, dscores, rank, ambiguous = lc.knn_vote_ref(wv, wi, bl, ql, C, 0.07)
    assert not ambiguous.any(), "the fixture: the f64 restatement itself decides every query (checked on the CPU when it was written)"
    got, sc = ops.knn_vote(_dev(wv), _dev(wi, torch.int32), torch.from_numpy(bl), torch.from_numpy(ql), C, 0.07, return_scores=True)
    w = _worst(sc.cpu().numpy(), scores, np.maximum(dscores, 1e-300))[0] if dscores.max() > 0 else 0.0
    left_out = int(ambiguous.sum())
    assert left_out <= 0.02 * len(ql)
    assert np.array_equal(got.cpu().numpy()[~ambiguous], rank[~ambiguous])
    assert (np.abs(sc.cpu().numpy() - scores) <= dscores).all(), w
    print(f"knn_vote C={C} k={k}: worst score err / bound {w:.3f}, top-1 {(rank == 0).mean():.3f}, left out {left_out}")
    # the whole chain on the device agrees: similarities -> lists -> vote
    vals, idx = ops.topk_empty(len(q), k, "cuda")
    bd, qd = _dev(bank), _dev(q)
    for c0 in range(0, len(bank), 64):
        ops.topk_merge(ops.pairwise_logits(qd, bd[c0:c0 + 64]), c0, vals, idx)
    chain = ops.knn_vote(vals, idx, torch.from_numpy(bl), torch.from_numpy(ql), C, 0.07)
    assert (chain.cpu().numpy() == rank).mean() >= 0.98


def test_knn_vote_refusals():
    from ldmae_amd import ops
    vals, idx = ops.topk_empty(2, 3, "cuda")
    with pytest.raises(ValueError, match="KNN_VOTE_MAX_C"):
        ops.knn_vote(vals, idx, torch.zeros(4, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), ops.KNN_VOTE_MAX_C + 1)
    with pytest.raises(ValueError, match=r"bank_labels\[1\] = 9"):
        ops.knn_vote(vals, idx, torch.tensor([0, 9, 1, 2]), torch.zeros(2, dtype=torch.int64), 4)
    rank = ops.knn_vote(vals, idx, torch.tensor([0, 1, 2, 3]), torch.tensor([2, 0]), 4)      # empty lists: every score 0, ties to the lower class
    assert rank.tolist() == [2, 0]


def test_l2_normalize():
    from ldmae_amd import ops
    x = np.random.default_rng(3).normal(0, 2, (70, 16)).astype(np.float32)
    x[5] = 0
    got = ops.l2_normalize(_dev(x)).cpu().numpy()
    ref = x.astype(np.float64) / np.maximum(np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True), 1e-12)
    assert np.abs(got - ref).max() <= 3 * lc.U and not got[5].any()        # the norm (rounded once), its root, the division


# ------------------------------------------------------------------------------------------------ features
@pytest.fixture(scope="module")
def tiny_vmae():
    from ldmae_amd.tokenizer import models_mae
    torch.manual_seed(0)
    return models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, kl_loss_weight=True, smooth_output=True, img_size=32).to("cuda").eval()


def _encode_as_before(m, x):
    """MaskedAutoencoderViT._encode as it stood before encode_features was factored out of it."""
    from ldmae_amd.tokenizer import fused_encoder, models_mae as mm
    dtype, tf32 = m._docking_dtype(m.blocks, rows=x.shape[0] * m.patch_embed.num_patches)
    with torch.autocast(device_type="cuda", enabled=False):
        x = m._embed(x, dtype)
        if (m.fused_encoder and dtype in (torch.bfloat16, torch.float16) and not torch.is_grad_enabled() and x.dim() == 3 and
                fused_encoder.supported(m, x.shape[1], x.shape[2], tiled=True) and all(m._chain_ok(blk) for blk in m.blocks)):
            x = fused_encoder.encoder_forward_tiled(m, x.float(), dtype=dtype)
        else:
            x = m._run(m.blocks, x, dtype, tf32)
            x = mm._LayerNormFn.apply(x, m.norm.weight, m.norm.bias, m.norm.eps)
        x = mm._latent_map(m.to_latent, x)
    g = m.latent_resolution
    return x.reshape(x.shape[0], g, g, -1).permute(0, 3, 1, 2)


@pytest.mark.parametrize("precision", [torch.float32, torch.bfloat16])
def test_encode_features_against_encode(tiny_vmae, golden, precision):
    m = tiny_vmae
    m.set_precision(precision)
    try:
        x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(1)).cuda()
        with torch.no_grad():
            mom = m._encode(x)                                                  # [B, 2 latent, g, g]
        lat = m.encode_features(x, "latent")
        enc = m.encode_features(x, "encoder")
        assert lat.shape == (4, 16, m.latent_dim) and enc.shape == (4, 16, m.pos_embed.shape[-1]) and not lat.requires_grad
        want = mom[:, :m.latent_dim].permute(0, 2, 3, 1).reshape(4, 16, m.latent_dim)
        assert torch.equal(lat, want), "the latent features are _encode's posterior means, bit for bit"
        with pytest.raises(ValueError, match="encoder or latent"):
            m.encode_features(x, "pixels")
        from ldmae_amd import ops
        pooled = ops.token_mean(lat)
        ref, bound = lc.token_mean_ref(lat.float().cpu().numpy())
        assert _worst(pooled.cpu().numpy(), ref, bound)[0] <= 1
        with torch.no_grad():                                                   # _encode is what it was: its body before the factoring, restated
            assert torch.equal(_encode_as_before(m, x), mom) and torch.equal(m._encode(x), mom)
            assert torch.equal(m.encode(x).latent_dist.mode(), mom[:, :m.latent_dim])
    finally:
        m.set_precision(torch.float32)


# ------------------------------------------------------------------------------------------------ the loader's two options
def test_center_loader_yields_every_image(tmp_path):
    from ldmae_amd import linear_probe as lp, ops
    from ldmae_amd.datasets.packed_images import PackedBatchLoader, PackedImages, center_table
    ds = PackedImages(lp.write_synthetic_pack(str(tmp_path / "p"), 10, 5))
    whole = list(lp.center_loader(ds, 10, 32, "cuda"))
    assert len(whole) == 1 and whole[0][0].shape == (10, 3, 32, 32) and whole[0][1].tolist() == ds.labels.tolist()
    parts = list(lp.center_loader(ds, 4, 32, "cuda"))               # 4 + 4 + 2: the last, partial batch is kept
    assert [p[0].shape[0] for p in parts] == [4, 4, 2] and torch.cat([p[1] for p in parts]).tolist() == ds.labels.tolist()
    assert torch.equal(torch.cat([p[0] for p in parts]), whole[0][0]), "a sample does not depend on its batch"
    for i in (0, 1, 2):                                             # wide, tall, square: the kernel on the centre table of that image alone
        blob = torch.from_numpy(np.array(ds.raw(i))).cuda()
        one = ops.crop_resize_flip(blob, torch.zeros(1, dtype=torch.int64), center_table(ds.sizes[[i]]), 32)
        assert torch.equal(one[0], whole[0][0][i]), i
    dropping = PackedBatchLoader(ds, lp.EpochSampler(10, False), 4, 32, 0, "cuda", center=True)
    assert len(dropping) == 2 and [b[0].shape[0] for b in dropping] == [4, 4]      # the default still drops it


# ------------------------------------------------------------------------------------------------ end to end
CFG ={"data": {"image_size": 32}, "vae": {"model_name": "vmae_f8d16", "weight_path": None}}


def _run(capsys, out, *extra):
    from ldmae_amd import linear_probe as lp
    args = lp.build_parser().parse_args(["--synthetic", "256", "--output_dir", str(out), "--batch_size", "64", "--blr", "4", "--trust", "0.2",
                                         "--warmup_epochs", "1", *extra])
    res = lp.linear_probe(args, CFG)
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert lines[-1]["metric"] == "linear_probe" and {k: lines[-1][k] for k in lp.JSON_KEYS} == res
    return res, [ln for ln in lines if ln["metric"] == "linear_probe_epoch"]


def test_end_to_end_center_resume_eval(tmp_path, capsys):
    """--aug center on the 4-class synthetic packs (colour and spatial frequency): the loss falls, the probe and the k-NN classifier both
    reach 1.0, and head.pt round-trips through --resume and --eval to the same numbers.  (blr 4, trust 0.2: six epochs of four steps
    instead of MAE's 90 x 78; the recipe's defaults are pinned in test_linprobe_cpu.py.)"""
    out = tmp_path / "probe"
    res, epochs = _run(capsys, out, "--aug", "center", "--epochs", "6")
    assert len(epochs) == 6 and epochs[-1]["train_loss"] < 0.7 * epochs[0]["train_loss"], [e["train_loss"] for e in epochs]
    assert res["top1"] == 1.0 and res["top5"] == 1.0 and res["knn_top1"] == 1.0 and res["knn_top5"] == 1.0, res
    assert (res["features"], res["pool"], res["epochs"], res["images"]) == ("latent", "mean", 6, 128)
    sd = torch.load(out / "head.pt")
    assert sd["weight"].shape == (4, 16) and sd["bias"].shape == (4,) and sd["run_mean"].shape == (16,) and sd["epoch"] == 6
    assert set(sd) >= {"weight", "bias", "run_mean", "run_var", "mu_weight", "mu_bias", "epoch"}
    ev, none = _run(capsys, out, "--eval")
    assert not none and ev == res
    again, none = _run(capsys, out, "--aug", "center", "--epochs", "6", "--resume", str(out / "head.pt"))
    assert not none and again == res, "a finished head resumes to its evaluation"


def test_end_to_end_resume_continues(tmp_path, capsys):
    from ldmae_amd import linear_probe as lp
    out = tmp_path / "probe"
    res, epochs = _run(capsys, out, "--aug", "center", "--epochs", "6", "--no-knn")
    assert res["knn_top1"] is None and res["knn_top5"] is None
    # the same run in a fresh directory, stopped once the head of epoch 3 is on disk, then continued with --resume
    out2 = tmp_path / "probe2"
    args = lp.build_parser().parse_args(["--synthetic", "256", "--output_dir", str(out2), "--batch_size", "64", "--blr", "4", "--trust", "0.2",
                                         "--warmup_epochs", "1", "--aug", "center", "--epochs", "6", "--no-knn"])
    real_save = torch.save

    class Stop(Exception):
        pass

    def stop_after_three(obj, path):
        real_save(obj, path)
        if obj["epoch"] == 3:
            raise Stop
    torch.save = stop_after_three
    try:
        with pytest.raises(Stop):
            lp.linear_probe(args, CFG)
    finally:
        torch.save = real_save
    capsys.readouterr()
    res2, epochs2 = _run(capsys, out2, "--aug", "center", "--epochs", "6", "--no-knn", "--resume", str(out2 / "head.pt"))
    assert [e["epoch"] for e in epochs2] == [4, 5, 6] and epochs2 == epochs[3:] and res2 == res, "resumed epochs are the uninterrupted ones, bit for bit"


def test_end_to_end_rrc_epoch_and_flatten(tmp_path, capsys):
    res, epochs = _run(capsys, tmp_path / "rrc", "--aug", "rrc", "--epochs", "1", "--warmup_epochs", "0")
    assert len(epochs) == 1 and np.isfinite(epochs[0]["train_loss"]) and 0 <= res["top1"] <= res["top5"] <= 1 and res["knn_top1"] == 1.0
    # the whole latent grid through the MFMA GEMMs (width 256), no BatchNorm, two accumulated micro-batches per step
    res, epochs = _run(capsys, tmp_path / "flat", "--aug", "center", "--epochs", "2", "--pool", "flatten", "--head_norm", "none", "--accum_iter", "2",
                       "--features", "encoder", "--no-knn")
    assert len(epochs) == 2 and all(np.isfinite(e["train_loss"]) for e in epochs) and 0 <= res["top1"] <= res["top5"] <= 1 and res["pool"] == "flatten"
