"""FID evaluation without a GPU: the Inception state-dict loader (key / shape checks, BatchNorm folding), the Frechet distance, the
reference's folder listing and .npz reading, and where the weights are looked for (never downloaded)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _expected_shapes():
    """The conv layers of pytorch-fid's fid_inception_v3 written out from torchvision's Inception3 (name, Cin, Cout, kh, kw)."""
    rows = [("Conv2d_1a_3x3", 3, 32, 3, 3), ("Conv2d_2a_3x3", 32, 32, 3, 3), ("Conv2d_2b_3x3", 32, 64, 3, 3), ("Conv2d_3b_1x1", 64, 80, 1, 1),
            ("Conv2d_4a_3x3", 80, 192, 3, 3)]
    for b, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        rows += [(f"{b}.branch1x1", cin, 64, 1, 1), (f"{b}.branch5x5_1", cin, 48, 1, 1), (f"{b}.branch5x5_2", 48, 64, 5, 5),
                 (f"{b}.branch3x3dbl_1", cin, 64, 1, 1), (f"{b}.branch3x3dbl_2", 64, 96, 3, 3), (f"{b}.branch3x3dbl_3", 96, 96, 3, 3),
                 (f"{b}.branch_pool", cin, pf, 1, 1)]
    rows += [("Mixed_6a.branch3x3", 288, 384, 3, 3), ("Mixed_6a.branch3x3dbl_1", 288, 64, 1, 1), ("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 3),
             ("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 3)]
    for b, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        rows += [(f"{b}.branch1x1", 768, 192, 1, 1), (f"{b}.branch7x7_1", 768, c7, 1, 1), (f"{b}.branch7x7_2", c7, c7, 1, 7),
                 (f"{b}.branch7x7_3", c7, 192, 7, 1), (f"{b}.branch7x7dbl_1", 768, c7, 1, 1), (f"{b}.branch7x7dbl_2", c7, c7, 7, 1),
                 (f"{b}.branch7x7dbl_3", c7, c7, 1, 7), (f"{b}.branch7x7dbl_4", c7, c7, 7, 1), (f"{b}.branch7x7dbl_5", c7, 192, 1, 7),
                 (f"{b}.branch_pool", 768, 192, 1, 1)]
    rows += [("Mixed_7a.branch3x3_1", 768, 192, 1, 1), ("Mixed_7a.branch3x3_2", 192, 320, 3, 3), ("Mixed_7a.branch7x7x3_1", 768, 192, 1, 1),
             ("Mixed_7a.branch7x7x3_2", 192, 192, 1, 7), ("Mixed_7a.branch7x7x3_3", 192, 192, 7, 1), ("Mixed_7a.branch7x7x3_4", 192, 192, 3, 3)]
    for b, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        rows += [(f"{b}.branch1x1", cin, 320, 1, 1), (f"{b}.branch3x3_1", cin, 384, 1, 1), (f"{b}.branch3x3_2a", 384, 384, 1, 3),
                 (f"{b}.branch3x3_2b", 384, 384, 3, 1), (f"{b}.branch3x3dbl_1", cin, 448, 1, 1), (f"{b}.branch3x3dbl_2", 448, 384, 3, 3),
                 (f"{b}.branch3x3dbl_3a", 384, 384, 1, 3), (f"{b}.branch3x3dbl_3b", 384, 384, 3, 1), (f"{b}.branch_pool", cin, 192, 1, 1)]
    out = {}
    for n, cin, cout, kh, kw in rows:
        out[f"{n}.conv.weight"] = (cout, cin, kh, kw)
        for k in ("weight", "bias", "running_mean", "running_var"):
            out[f"{n}.bn.{k}"] = (cout,)
    return out


def test_key_set_and_flop_count_match_the_table():
    from ldmae_amd import fid
    assert fid.param_shapes() == _expected_shapes()
    assert len(fid.LAYERS) == 94 and len(set(fid.conv_geometries().values())) == 43
    assert abs(fid.conv_flops_per_image() / 1e9 - 11.42) < 0.01
    sd = fid.random_state_dict(3)
    assert {k: tuple(v.shape) for k, v in sd.items() if k in _expected_shapes()} == _expected_shapes()


def test_loader_rejects_missing_extra_and_misshapen_keys():
    from ldmae_amd import fid
    sd = fid.random_state_dict(0)
    fid.check_state_dict(sd)
    bad = dict(sd)
    del bad["Mixed_6c.branch7x7dbl_4.bn.running_var"]
    with pytest.raises(KeyError, match=re.escape("Mixed_6c.branch7x7dbl_4.bn.running_var")):
        fid.fold_bn(bad)
    bad = dict(sd, **{"Mixed_5b.branch9x9.conv.weight": torch.zeros(1)})
    with pytest.raises(KeyError, match=re.escape("Mixed_5b.branch9x9.conv.weight")):
        fid.fold_bn(bad)
    bad = dict(sd, **{"Mixed_7c.branch_pool.conv.weight": torch.zeros(192, 1280, 1, 1)})
    with pytest.raises(ValueError, match=re.escape("Mixed_7c.branch_pool.conv.weight")):
        fid.fold_bn(bad)
    # fc.* and num_batches_tracked are optional
    lean = {k: v for k, v in sd.items() if not k.startswith("fc.") and not k.endswith("num_batches_tracked")}
    fid.check_state_dict(lean)


def test_bn_folding_matches_conv_then_batchnorm():
    import torch.nn.functional as F
    from ldmae_amd import fid
    sd = fid.random_state_dict(1)
    folded = fid.fold_bn(sd)
    g = torch.Generator().manual_seed(2)
    for name in ("Conv2d_1a_3x3", "Mixed_6b.branch7x7_2", "Mixed_7c.branch3x3dbl_3b"):
        cin, cout, kh, kw, s, ph, pw = fid.LAYERS[name]
        x = torch.randn(2, cin, 9, 9, generator=g, dtype=torch.float64)
        ref = F.batch_norm(F.conv2d(x, sd[f"{name}.conv.weight"].double(), stride=s, padding=(ph, pw)), sd[f"{name}.bn.running_mean"].double(),
                           sd[f"{name}.bn.running_var"].double(), sd[f"{name}.bn.weight"].double(), sd[f"{name}.bn.bias"].double(), False, 0.0, 1e-3)
        w, b = folded[name]
        assert w.shape == (cout, kh, kw, cin) and w.dtype == torch.float32 and b.dtype == torch.float32
        got = F.conv2d(x, w.double().permute(0, 3, 1, 2), b.double(), stride=s, padding=(ph, pw))
        assert float((got - ref).norm() / ref.norm()) < 1e-6, name


def test_frechet_distance_closed_forms():
    from ldmae_amd.fid import calculate_frechet_distance
    rng = np.random.default_rng(0)
    a = rng.standard_normal((40, 6))
    mu, sigma = a.mean(0), np.cov(a, rowvar=False)
    assert abs(calculate_frechet_distance(mu, sigma, mu, sigma)) < 1e-9
    d1, d2 = rng.uniform(0.5, 2.0, 6), rng.uniform(0.5, 2.0, 6)
    m1, m2 = rng.standard_normal(6), rng.standard_normal(6)
    want = np.sum((m1 - m2) ** 2) + np.sum((np.sqrt(d1) - np.sqrt(d2)) ** 2)
    assert abs(calculate_frechet_distance(m1, np.diag(d1), m2, np.diag(d2)) - want) < 1e-10 * max(1.0, want)


def test_frechet_distance_singular_product_takes_the_eps_branch(capsys):
    from scipy import linalg
    from ldmae_amd.fid import calculate_frechet_distance
    # S1 S2 = [[0, 0], [1e-4, 0]] is nilpotent: its square root does not exist (sqrtm returns NaN) -> eps on the diagonals
    s1, s2 = np.array([[0.0, 0.0], [0.0, 1.0]]), np.array([[1.0, 1e-4], [1e-4, 0.0]])
    d = calculate_frechet_distance(np.zeros(2), s1, np.ones(2), s2)
    assert "singular product" in capsys.readouterr().out
    e = np.eye(2) * 1e-6
    want = 2.0 + np.trace(s1) + np.trace(s2) - 2 * np.trace(np.real(linalg.sqrtm((s1 + e) @ (s2 + e))))
    assert np.isfinite(d) and abs(d - want) < 1e-12


def test_folder_listing_and_npz_reading(tmp_path):
    from ldmae_amd import fid
    names = ["b.png", "a.jpg", "c.JPEG", "d.txt", "e.webp", "f.png", "g.tiff"]
    for n in names:
        (tmp_path / n).write_bytes(b"")
    files = [p.name for p in fid.list_images(tmp_path)]
    assert files == ["a.jpg", "b.png", "e.webp", "f.png", "g.tiff"]           # sorted, extensions of the reference (lower case)
    assert [p.name for p in fid.list_images(tmp_path, sp_len=3)] == ["a.jpg", "b.png", "e.webp"]
    mu, sigma = np.arange(3.0), np.eye(3) * 2
    np.savez(tmp_path / "s.npz", mu=mu, sigma=sigma)
    m, s = fid.compute_statistics_of_path(str(tmp_path / "s.npz"), None, 50, 2048, "cuda")
    assert np.array_equal(m, mu) and np.array_equal(s, sigma)
    # two .npz files never need the network (nor its weights)
    np.savez(tmp_path / "t.npz", mu=mu + 1, sigma=sigma)
    d = fid.calculate_fid_given_paths([str(tmp_path / "s.npz"), str(tmp_path / "t.npz")], 50, "cuda", 2048)
    assert abs(d - 3.0) < 1e-9
    with pytest.raises(RuntimeError, match="Invalid path"):
        fid.calculate_fid_given_paths([str(tmp_path / "s.npz"), str(tmp_path / "nope.npz")], 50, "cuda", 2048)


def test_weights_are_never_downloaded(tmp_path, monkeypatch):
    from ldmae_amd import fid
    monkeypatch.delenv(fid.WEIGHTS_ENV, raising=False)
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    with pytest.raises(FileNotFoundError) as e:
        fid.resolve_weights(str(tmp_path / "nope.pth"))
    msg = str(e.value)
    assert "pt_inception-2015-12-05-6726825d.pth" in msg and fid.WEIGHTS_ENV in msg and str(tmp_path / "hub") in msg
    with pytest.raises(FileNotFoundError):
        fid.InceptionFID(dims=2048, device="cuda")
    src = open(os.path.join(ROOT, "ldmae_amd", "fid.py")).read()
    assert not re.search(r"https?://|load_state_dict_from_url|load_url|urlopen|urlretrieve", src, re.I)
    # the order: argument, then the environment, then torch.hub's checkpoints directory
    (tmp_path / "hub" / "checkpoints").mkdir(parents=True)
    hub = tmp_path / "hub" / "checkpoints" / fid.WEIGHTS_NAME
    hub.write_bytes(b"x")
    assert fid.resolve_weights() == str(hub)
    env = tmp_path / "env.pth"
    env.write_bytes(b"x")
    monkeypatch.setenv(fid.WEIGHTS_ENV, str(env))
    assert fid.resolve_weights() == str(env)
    arg = tmp_path / "arg.pth"
    arg.write_bytes(b"x")
    assert fid.resolve_weights(str(arg)) == str(arg)
