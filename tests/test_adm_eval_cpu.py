"""The ADM evaluator without a GPU: the streaming .npz reader, the Inception Score from the kernels' sums, the argument checks that run
before any kernel, save_npz's folder naming and count check, the .npz cache write-back, and FIDStatistics."""
import os
import zipfile

import numpy as np
import pytest

from ldmae_amd import evaluator as ev
from ldmae_amd import fid


# ------------------------------------------------------------------------------------------------ streaming reader
@pytest.mark.parametrize("compressed", [False, True])
@pytest.mark.parametrize("batch", [1, 7, 10, 64])
def test_streaming_reader_equals_np_load(tmp_path, compressed, batch):
    rng = np.random.default_rng(0)
    arr = rng.integers(0, 256, (10, 5, 6, 3), dtype=np.uint8)
    p = str(tmp_path / "x.npz")
    (np.savez_compressed if compressed else np.savez)(p, arr_0=arr, other=np.arange(3))
    with ev.open_npz_array(p, "arr_0") as r:
        assert r.arr is None, "both stored and deflated members are streamed, not loaded whole"
        assert r.remaining() == 10
        got = list(r.read_batches(batch))
    assert [len(b) for b in got] == [min(batch, 10 - i) for i in range(0, 10, batch)]
    np.testing.assert_array_equal(np.concatenate(got), np.load(p)["arr_0"])


def test_streaming_reader_missing_member(tmp_path):
    p = str(tmp_path / "x.npz")
    np.savez(p, foo=np.zeros(3))
    with pytest.raises(ValueError, match="missing arr_0"):
        with ev.open_npz_array(p, "arr_0"):
            pass


# ------------------------------------------------------------------------------------------------ Inception Score
def _is_reference(preds, split_size):
    """evaluator.py:200-207 in f64."""
    scores = []
    for i in range(0, len(preds), split_size):
        part = preds[i:i + split_size]
        kl = part * (np.log(part) - np.log(np.expand_dims(np.mean(part, 0), 0)))
        kl = np.mean(np.sum(kl, 1))
        scores.append(np.exp(kl))
    return float(np.mean(scores))


@pytest.mark.parametrize("n,split", [(300, 100), (317, 100), (50, 5000)])
def test_inception_score_from_sums(n, split):
    rng = np.random.default_rng(1)
    logits = rng.normal(0, 3, (n, 40))
    p = np.exp(logits - logits.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    h = (p * np.log(p)).sum(1)
    S = np.stack([p[i:i + split].sum(0) for i in range(0, n, split)])
    got = ev.inception_score_from_sums(h, S, n, split)
    ref = _is_reference(p, split)
    assert abs(got - ref) <= 1e-12 * ref


def test_inception_score_zero_probability_is_zero_log_zero():
    p = np.array([[0.5, 0.5, 0.0], [0.25, 0.75, 0.0]])
    h = np.array([0.5 * np.log(0.5) * 2, 0.25 * np.log(0.25) + 0.75 * np.log(0.75)])
    got = ev.inception_score_from_sums(h, p.sum(0, keepdims=True), 2, 10)
    assert np.isfinite(got) and abs(got - _is_reference(p[:, :2], 10)) < 1e-12


# ------------------------------------------------------------------------------------------------ checks before any kernel
def test_manifold_rejects_too_few_rows_and_non_finite(monkeypatch):
    from ldmae_amd import ops

    def boom(*a, **k):
        raise AssertionError("a kernel was reached")

    monkeypatch.setattr(ops, "knn_radii", boom)
    monkeypatch.setattr(ops, "pr_flags", boom)
    m = ev.ManifoldEstimator(nhood_sizes=(3, 5), device="cpu")
    with pytest.raises(ValueError, match="no neighbour"):
        m.manifold_radii(np.zeros((5, 8), np.float32))
    x = np.zeros((20, 8), np.float32)
    x[3, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        m.manifold_radii(x)
    x[3, 2] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        m.evaluate_pr(x, np.zeros((20, 2), np.float32), np.zeros((20, 8), np.float32), np.zeros((20, 2), np.float32))
    with pytest.raises(ValueError):
        ev.ManifoldEstimator(nhood_sizes=(8,))


# ------------------------------------------------------------------------------------------------ save_npz
def _cfg(tmp_path):
    return {"model": {"model_type": "LightningDiT-B/1"}, "ckpt_path": "/x/ckpts/0100000.pt",
            "sample": {"sampling_method": "euler", "num_sampling_steps": 250, "cfg_scale": 1.0},
            "train": {"output_dir": str(tmp_path / "out"), "exp_name": "exp"}}


def test_save_npz_naming_and_count(tmp_path):
    from PIL import Image
    from ldmae_amd import inference, save_npz
    cfg = _cfg(tmp_path)
    d = save_npz.sample_dir_of(cfg)
    assert d == os.path.join(str(tmp_path / "out"), "exp", inference.sample_folder_name(cfg, cfg["ckpt_path"]))
    assert os.path.basename(d) == "lightningdit-b-1-ckpt-0100000-euler-250"
    os.makedirs(d)
    rng = np.random.default_rng(2)
    imgs = rng.integers(0, 256, (4, 6, 5, 3), dtype=np.uint8)
    for i, name in enumerate(["000003.png", "000001.png", "000002.png", "000000.png"]):
        Image.fromarray(imgs[i]).save(os.path.join(d, name))
    with pytest.raises(ValueError, match="holds 4 PNG files"):
        save_npz.create_npz_from_sample_folder(d, 5)
    out = save_npz.create_npz_from_sample_folder(d, 3)
    assert out == d + ".npz"
    arr = np.load(out)["arr_0"]
    assert arr.dtype == np.uint8 and arr.shape == (3, 6, 5, 3)
    np.testing.assert_array_equal(arr, imgs[[3, 1, 2]])          # sorted names: 000000, 000001, 000002


# ------------------------------------------------------------------------------------------------ cache write-back
def _fake_evaluator(monkeypatch, calls):
    e = ev.Evaluator(device="cpu")

    def acts(batches):
        n = sum(len(b) for b in batches)
        calls.append(n)
        rng = np.random.default_rng(n)
        return rng.normal(size=(n, 6)).astype(np.float32), rng.normal(size=(n, 4)).astype(np.float32)

    def stats(a):
        return ev.FIDStatistics(np.mean(a, 0), np.cov(a, rowvar=False))

    monkeypatch.setattr(e, "compute_activations", acts)
    monkeypatch.setattr(e, "compute_statistics", stats)
    return e


def test_cache_write_back_and_reuse(tmp_path, monkeypatch):
    calls = []
    e = _fake_evaluator(monkeypatch, calls)
    p = str(tmp_path / "ref.npz")
    arr = np.random.default_rng(3).integers(0, 256, (9, 4, 4, 3), dtype=np.uint8)
    np.savez(p, arr_0=arr)
    (a0, s0), (st, sts) = ev.activations_and_statistics(e, p)
    assert calls == [9]
    with np.load(p) as z:
        assert sorted(z.files) == sorted(("arr_0",) + ev.CACHE_KEYS)
        np.testing.assert_array_equal(z["arr_0"], arr)
        np.testing.assert_array_equal(z["act"], a0)
        np.testing.assert_array_equal(z["act_s"], s0)
        np.testing.assert_array_equal(z["mu_s"], sts.mu)
        np.testing.assert_array_equal(z["sigma"], st.sigma)
    assert not [f for f in os.listdir(tmp_path) if f != "ref.npz"], "no temporary file left behind"
    (a1, s1), (st1, _) = ev.activations_and_statistics(e, p)
    assert calls == [9], "the second run reads the cached activations"
    np.testing.assert_array_equal(a1, a0)
    np.testing.assert_array_equal(st1.mu, st.mu)


def test_stored_statistics_win(tmp_path, monkeypatch):
    e = _fake_evaluator(monkeypatch, [])
    p = str(tmp_path / "ref.npz")
    np.savez(p, arr_0=np.zeros((3, 4, 4, 3), np.uint8), mu=np.ones(6), sigma=np.eye(6), mu_s=np.zeros(4), sigma_s=np.eye(4))
    (a, _), (st, sts) = ev.activations_and_statistics(e, p)
    np.testing.assert_array_equal(st.mu, np.ones(6))
    np.testing.assert_array_equal(sts.sigma, np.eye(4))
    with np.load(p) as z:
        np.testing.assert_array_equal(z["mu"], np.ones(6))     # kept, not replaced by recomputed statistics
        np.testing.assert_array_equal(z["act"], a)


def test_folder_input_is_never_written(tmp_path, monkeypatch):
    from PIL import Image
    calls = []
    e = _fake_evaluator(monkeypatch, calls)
    d = tmp_path / "imgs"
    d.mkdir()
    for i in range(5):
        Image.fromarray(np.full((4, 4, 3), i * 10, np.uint8)).save(d / f"{i}.png")
    before = {p: os.stat(d / p).st_mtime_ns for p in os.listdir(d)}
    ev.activations_and_statistics(e, str(d))
    ev.activations_and_statistics(e, str(d))
    assert calls == [5, 5]
    assert {p: os.stat(d / p).st_mtime_ns for p in os.listdir(d)} == before
    assert sorted(os.listdir(tmp_path)) == ["imgs"]


def test_write_npz_cache_keeps_compression(tmp_path):
    p = str(tmp_path / "c.npz")
    np.savez_compressed(p, arr_0=np.arange(24, dtype=np.uint8).reshape(2, 2, 2, 3))
    ev.write_npz_cache(p, {"act": np.ones((2, 3), np.float32)})
    with zipfile.ZipFile(p) as z:
        assert {i.compress_type for i in z.infolist()} == {zipfile.ZIP_DEFLATED}
    with np.load(p) as z:
        np.testing.assert_array_equal(z["act"], np.ones((2, 3)))
        np.testing.assert_array_equal(z["arr_0"], np.arange(24).reshape(2, 2, 2, 3))


# ------------------------------------------------------------------------------------------------ FIDStatistics
def test_fid_statistics_delegates():
    rng = np.random.default_rng(4)
    a, b = rng.normal(size=(50, 5)), rng.normal(size=(60, 5)) + 0.3
    s1 = ev.FIDStatistics(a.mean(0), np.cov(a, rowvar=False))
    s2 = ev.FIDStatistics(b.mean(0), np.cov(b, rowvar=False))
    assert s1.frechet_distance(s2) == fid.calculate_frechet_distance(s1.mu, s1.sigma, s2.mu, s2.sigma)


def test_evaluator_defers_the_network():
    e = ev.Evaluator(weights="/nonexistent/weights.pth", device="cpu")
    assert e._model is None
    with pytest.raises(FileNotFoundError):
        e.model
