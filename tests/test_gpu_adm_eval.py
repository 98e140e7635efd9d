"""The ADM evaluator on the MI355X (csrc/adm_eval.hip, ldmae_amd/evaluator.py) against numpy f64 / torch CPU restatements of the
reference's tools/evaluator.py written out here: the TF pre-processing, the pool_3 / mixed_6/conv features, the k-NN radii, precision /
recall, the Inception Score and the command line with its .npz cache."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = torch.as_tensor(a).double().flatten().cpu(), torch.as_tensor(b).double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


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


# ------------------------------------------------------------------------------------------------ TF pre-processing
def tf_resize_normalise(imgs, size=299):
    """TF1 ResizeBilinear (align_corners=False, legacy: src = dst * in / out in f32), then (v - 128) / 128 (evaluator.py:601-615 feeds
    raw 0..255 values to ExpandDims:0); interpolation in f64."""
    B, H, W, _ = imgs.shape

    def axis(n_in):
        scale = np.float32(n_in) / np.float32(size)
        src = np.arange(size, dtype=np.float32) * scale
        lo = np.floor(src).astype(np.int64)
        hi = np.minimum(lo + 1, n_in - 1)
        return lo, hi, (src - lo.astype(np.float32)).astype(np.float64)

    y0, y1, yl = axis(H)
    x0, x1, xl = axis(W)
    x = imgs.astype(np.float64)
    tl, tr = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
    bl, br = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    xl, yl = xl[None, None, :, None], yl[None, :, None, None]
    top = tl + (tr - tl) * xl
    bot = bl + (br - bl) * xl
    return (top + (bot - top) * yl - 128) / 128


@pytest.mark.parametrize("hw", [(256, 256), (512, 512), (299, 299), (97, 131)])
def test_adm_preprocess_matches_tf_legacy_resize(hw):
    from ldmae_amd import ops
    imgs = _images(2, hw[0], hw[1], sum(hw))
    got = ops.adm_preprocess(torch.from_numpy(imgs).cuda()).cpu().double().numpy()
    want = tf_resize_normalise(imgs)
    assert got.shape == (2, 299, 299, 3)
    assert np.abs(got - want).max() <= 1e-5
    if hw == (299, 299):                       # identity resize: exactly the normalised pixels
        np.testing.assert_array_equal(got, (imgs.astype(np.float64) - 128) / 128)


# ------------------------------------------------------------------------------------------------ features
def cpu_adm_features(sd, imgs):
    """pool_3 and mixed_6/conv[..., :7] of pytorch-fid's network on the CPU with the TF pre-processing: (pool [B, 2048], spatial [B, 2023]
    with Mixed_6d.branch1x1[:, :7] permuted to NHWC and flattened)."""
    def bc(name, x, stride=1, padding=0):
        y = F.conv2d(x, sd[f"{name}.conv.weight"].float(), stride=stride, padding=padding)
        y = F.batch_norm(y, sd[f"{name}.bn.running_mean"].float(), sd[f"{name}.bn.running_var"].float(), sd[f"{name}.bn.weight"].float(),
                         sd[f"{name}.bn.bias"].float(), False, 0.0, 1e-3)
        return F.relu(y)

    def avg(x):
        return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)

    def block_a(p, x):
        b1 = bc(f"{p}.branch1x1", x)
        b5 = bc(f"{p}.branch5x5_2", bc(f"{p}.branch5x5_1", x), padding=2)
        b3 = bc(f"{p}.branch3x3dbl_3", bc(f"{p}.branch3x3dbl_2", bc(f"{p}.branch3x3dbl_1", x), padding=1), padding=1)
        return torch.cat([b1, b5, b3, bc(f"{p}.branch_pool", avg(x))], 1)

    def block_c(p, x):
        b1 = bc(f"{p}.branch1x1", x)
        b7 = bc(f"{p}.branch7x7_3", bc(f"{p}.branch7x7_2", bc(f"{p}.branch7x7_1", x), padding=(0, 3)), padding=(3, 0))
        d = bc(f"{p}.branch7x7dbl_1", x)
        d = bc(f"{p}.branch7x7dbl_2", d, padding=(3, 0))
        d = bc(f"{p}.branch7x7dbl_3", d, padding=(0, 3))
        d = bc(f"{p}.branch7x7dbl_4", d, padding=(3, 0))
        d = bc(f"{p}.branch7x7dbl_5", d, padding=(0, 3))
        return torch.cat([b1, b7, d, bc(f"{p}.branch_pool", avg(x))], 1), b1

    def block_e(p, x, pool):
        b1 = bc(f"{p}.branch1x1", x)
        t = bc(f"{p}.branch3x3_1", x)
        b3 = torch.cat([bc(f"{p}.branch3x3_2a", t, padding=(0, 1)), bc(f"{p}.branch3x3_2b", t, padding=(1, 0))], 1)
        d = bc(f"{p}.branch3x3dbl_2", bc(f"{p}.branch3x3dbl_1", x), padding=1)
        bd = torch.cat([bc(f"{p}.branch3x3dbl_3a", d, padding=(0, 1)), bc(f"{p}.branch3x3dbl_3b", d, padding=(1, 0))], 1)
        return torch.cat([b1, b3, bd, bc(f"{p}.branch_pool", pool(x))], 1)

    x = torch.from_numpy(tf_resize_normalise(imgs)).float().permute(0, 3, 1, 2).contiguous()
    x = bc("Conv2d_2b_3x3", bc("Conv2d_2a_3x3", bc("Conv2d_1a_3x3", x, stride=2)), padding=1)
    x = F.max_pool2d(bc("Conv2d_4a_3x3", bc("Conv2d_3b_1x1", F.max_pool2d(x, 3, 2))), 3, 2)
    for p in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = block_a(p, x)
    b3 = bc("Mixed_6a.branch3x3", x, stride=2)
    d = bc("Mixed_6a.branch3x3dbl_3", bc("Mixed_6a.branch3x3dbl_2", bc("Mixed_6a.branch3x3dbl_1", x), padding=1), stride=2)
    x = torch.cat([b3, d, F.max_pool2d(x, 3, 2)], 1)
    for p in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        x, b1 = block_c(p, x)
        if p == "Mixed_6d":                     # TF mixed_6/conv (mixed_4..mixed_7 = Mixed_6b..6e): the branch1x1 conv after BN + ReLU
            spatial = b1[:, :7].permute(0, 2, 3, 1).reshape(b1.shape[0], -1)
    b3 = bc("Mixed_7a.branch3x3_2", bc("Mixed_7a.branch3x3_1", x), stride=2)
    d = bc("Mixed_7a.branch7x7x3_1", x)
    d = bc("Mixed_7a.branch7x7x3_2", d, padding=(0, 3))
    d = bc("Mixed_7a.branch7x7x3_3", d, padding=(3, 0))
    d = bc("Mixed_7a.branch7x7x3_4", d, stride=2)
    x = torch.cat([b3, d, F.max_pool2d(x, 3, 2)], 1)
    x = block_e("Mixed_7b", x, avg)
    x = block_e("Mixed_7c", x, lambda t: F.max_pool2d(t, 3, 1, 1))
    return x.mean((2, 3)), spatial


@pytest.fixture(scope="module")
def sd():
    from ldmae_amd import fid
    s = fid.random_state_dict(5)
    g = torch.Generator().manual_seed(6)
    s["fc.weight"] = torch.randn(1008, 2048, generator=g) * 0.05
    s["fc.bias"] = torch.randn(1008, generator=g)
    return s


def test_adm_features_against_cpu(sd, monkeypatch):
    from ldmae_amd import fid
    imgs = _images(6, 96, 80, 3)
    model = fid.InceptionFID(dims=2048, state_dict=sd)

    def boom(*a, **k):
        raise AssertionError("torch conv / pool / interpolate called on the ADM feature path")
    with monkeypatch.context() as m:
        for n in ("conv2d", "max_pool2d", "avg_pool2d", "interpolate", "adaptive_avg_pool2d"):
            m.setattr(F, n, boom)
        pool, spatial = model.adm_features(torch.from_numpy(imgs))
    ref_pool, ref_spatial = cpu_adm_features(sd, imgs)
    assert pool.shape == (6, 2048) and spatial.shape == (6, 2023)
    assert rel(pool, ref_pool) <= 1e-4, rel(pool, ref_pool)
    assert rel(spatial, ref_spatial) <= 1e-4, rel(spatial, ref_spatial)
    assert float(spatial.std()) > 0 and float((spatial == 0).float().mean()) < 0.9
    # the pytorch-fid path is untouched: features() still differs from adm_features() only through the pre-processing
    assert rel(model.features(torch.from_numpy(imgs)), pool) > 1e-4


def test_adm_logits_weight_checks():
    from ldmae_amd import fid
    s = fid.random_state_dict(1)
    del s["fc.weight"]
    with pytest.raises(KeyError, match="fc.weight"):
        fid.InceptionFID(dims=2048, state_dict=s).adm_logits_weight()
    s["fc.weight"] = torch.zeros(1000, 2048)
    with pytest.raises(ValueError, match="fc.weight"):
        fid.InceptionFID(dims=2048, state_dict=s).adm_logits_weight()


# ------------------------------------------------------------------------------------------------ k-NN radii
def _sqdist64(u, v):
    """evaluator.py:429-445 in f64: max(|u|^2 - 2 u.v + |v|^2, 0)."""
    u, v = u.astype(np.float64), v.astype(np.float64)
    return np.maximum((u * u).sum(1)[:, None] - 2 * u @ v.T + (v * v).sum(1)[None, :], 0)


@pytest.mark.parametrize("n,d,nhood", [(5, 7, (3,)), (1000, 2023, (3, 5)), (1537, 2048, (7,)), (4099, 2048, (3,)), (1537, 7, (3, 5))])
def test_knn_radii_against_f64_and_split_invariant(n, d, nhood):
    from ldmae_amd import ops
    rng = np.random.default_rng(n + d)
    centers = rng.normal(0, 1, (max(2, n // 50), d))
    x = (centers[rng.integers(0, len(centers), n)] + rng.normal(0, 0.3, (n, d))).astype(np.float32)
    x[1::7] = x[0::7][:len(x[1::7])]                  # duplicated rows: zero distances besides the self-distance
    xt = torch.from_numpy(x).cuda()
    a = ops.knn_radii(xt, nhood, nsplit=1).cpu().numpy()
    b = ops.knn_radii(xt, nhood).cpu().numpy()
    c = ops.knn_radii(xt, nhood, nsplit=3).cpu().numpy()
    assert a.shape == (n, len(nhood)) and a.dtype == np.float32
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(a.view(np.int32), c.view(np.int32)), \
        "radii must not depend on the column split"
    d64 = _sqdist64(x, x)
    ref = np.sort(d64, 1)[:, list(nhood)]             # np.partition(row, seq)[:, k] over the full row (evaluator.py:263-296)
    nrm = (x.astype(np.float64) ** 2).sum(1)
    tol = 1e-5 * (nrm[:, None] + nrm.max())
    assert (np.abs(a - ref) <= tol).all(), np.abs(a - ref).max()


# ------------------------------------------------------------------------------------------------ precision / recall
def _evaluate_pr64(f1, r1, f2, r2):
    """evaluator.py:340-375 / 400-406 in f64: (precision, recall) per neighbourhood size."""
    d = _sqdist64(f1, f2)
    f1_in = (d[:, :, None] <= r2[None, :, :]).any(1)
    f2_in = (d[:, :, None] <= r1[:, None, :]).any(0)
    return f2_in.mean(0), f1_in.mean(0)


def test_precision_recall_against_f64():
    """Clustered integer features: every squared distance is an integer below 2^24, so the f32 kernels and the f64 restatement compute the
    same values exactly and no comparison sits within rounding of its radius -- equality is the right check (ties on the radius included)."""
    from ldmae_amd import evaluator as ev
    rng = np.random.default_rng(0)
    D = 2048
    centers = rng.integers(0, 3, (40, D))

    def draw(n, shift):
        base = centers[rng.integers(0, 40, n)]
        noise = rng.integers(-1, 2, (n, D)) * (rng.random((n, D)) < 0.15)
        return (base + noise + shift * (rng.random((n, D)) < 0.02)).astype(np.float32)

    f1, f2 = draw(1500, 0), draw(2300, 1)
    assert _sqdist64(f1, f2).max() < 2 ** 24 and (np.abs(f1) * np.abs(f1)).sum(1).max() < 2 ** 24
    m = ev.ManifoldEstimator(nhood_sizes=(3, 5))
    r1, r2 = m.manifold_radii(f1), m.manifold_radii(f2)
    for f, r in ((f1, r1), (f2, r2)):
        np.testing.assert_array_equal(r, np.sort(_sqdist64(f, f), 1)[:, [3, 5]])
    p, rc = m.evaluate_pr(f1, r1, f2, r2)
    wp, wr = _evaluate_pr64(f1, r1.astype(np.float64), f2, r2.astype(np.float64))
    np.testing.assert_array_equal(p, wp)
    np.testing.assert_array_equal(rc, wr)
    assert 0 < wp[0] < 1 and 0 < wr[0] < 1, (wp, wr)
    # the column split changes nothing
    p2, rc2 = ev.ManifoldEstimator(nhood_sizes=(3, 5), nsplit=1).evaluate_pr(f1, r1, f2, r2)
    np.testing.assert_array_equal(p2, p)
    np.testing.assert_array_equal(rc2, rc)


# ------------------------------------------------------------------------------------------------ Inception Score
def _is_reference(acts, w, split_size):
    """evaluator.py:194-207 with _create_softmax_graph (:618-629: logits = acts . W, no bias), all f64."""
    logits = acts.astype(np.float64) @ w.astype(np.float64).T
    p = np.exp(logits - logits.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    scores = []
    for i in range(0, len(p), split_size):
        part = p[i:i + split_size]
        kl = part * (np.log(part) - np.log(np.expand_dims(np.mean(part, 0), 0)))
        scores.append(np.exp(np.mean(np.sum(kl, 1))))
    return float(np.mean(scores))


def test_inception_score_against_f64(sd):
    from ldmae_amd import evaluator as ev
    rng = np.random.default_rng(1)
    acts = np.abs(rng.normal(0, 1, (1200, 2048))).astype(np.float32)
    e = ev.Evaluator(state_dict=sd)
    got = e.compute_inception_score(acts, split_size=500)          # splits of 500, 500 and 200 rows
    want = _is_reference(acts, sd["fc.weight"].numpy(), 500)
    assert 1.5 < want and abs(got - want) <= 1e-5 * want, (got, want)
    assert e.compute_inception_score(acts, split_size=500) == got, "bitwise reproducible"
    s2 = dict(sd)
    s2["fc.bias"] = torch.randn(1008) * 10
    assert ev.Evaluator(state_dict=s2).compute_inception_score(acts, split_size=500) == got, "fc.bias is not part of the logits"


def test_softmax_sums_are_fixed_order():
    from ldmae_amd import ops
    g = torch.Generator().manual_seed(2)
    logits = (torch.randn(777, 1008, generator=g) * 4).cuda()
    h1, s1 = ops.adm_softmax_is(logits, 100)
    h2, s2 = ops.adm_softmax_is(logits, 100)
    assert s1.shape == (8, 1008) and torch.equal(h1, h2) and torch.equal(s1, s2)
    p = torch.softmax(logits.double().cpu(), 1)
    assert rel(h1, (p * p.log()).sum(1)) < 1e-6
    assert rel(s1[7], p[700:].sum(0)) < 1e-6


# ------------------------------------------------------------------------------------------------ command line
def _numbers(out):
    got = {}
    for label in ("Inception Score", "FID", "sFID", "Precision", "Recall"):
        m = re.search(rf"^{label}: (\S+)$", out, re.M)
        assert m, (label, out)
        got[label] = float(m.group(1))
    order = [out.index(f"\n{label}:") for label in ("Inception Score", "FID", "sFID", "Precision", "Recall")]
    assert order == sorted(order)
    return got


def test_cli_npz_against_folder_with_cache(sd, tmp_path, capsys):
    from PIL import Image
    from ldmae_amd import evaluator as ev
    wpath = tmp_path / "inception.pth"
    torch.save(sd, wpath)
    ref = _images(40, 64, 64, 21)
    np.savez(tmp_path / "ref.npz", arr_0=ref)
    folder = tmp_path / "samples"
    folder.mkdir()
    for i, im in enumerate(_images(40, 64, 64, 22)):
        Image.fromarray(im).save(folder / f"{i:06d}.png")
    args = [str(tmp_path / "ref.npz"), str(folder), "--weights", str(wpath), "--batch-size", "16"]
    ev.main(args)
    first = _numbers("\n" + capsys.readouterr().out)
    assert all(np.isfinite(v) for v in first.values()), first
    with np.load(tmp_path / "ref.npz") as z:
        assert sorted(z.files) == sorted(("arr_0",) + ev.CACHE_KEYS)
        np.testing.assert_array_equal(z["arr_0"], ref)
        assert z["act"].shape == (40, 2048) and z["act_s"].shape == (40, 2023)
        assert z["mu_s"].shape == (2023,) and z["sigma"].shape == (2048, 2048)
    assert sorted(os.listdir(folder)) == [f"{i:06d}.png" for i in range(40)]
    ev.main(args)
    second = _numbers("\n" + capsys.readouterr().out)
    for k, v in first.items():
        assert abs(second[k] - v) <= 1e-12 * max(1.0, abs(v)), (k, v, second[k])
