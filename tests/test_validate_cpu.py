"""Held-out validation, the host side: the time sequence, the importance weights and bins against f64 closed forms, the rank partition and
merge, the refusals of the command line and of the YAML key, and the new entries in the header and the built library.  No GPU."""
import copy
import math
import os

import numpy as np
import pytest
import yaml

from ldmae_amd import validate as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "ldmae_amd/configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml")


def _cfg():
    with open(CFG) as f:
        return copy.deepcopy(yaml.safe_load(f))


def test_time_sequence_values_and_interval():
    t = V.sample_times(np.arange(6))
    assert t.dtype == np.float32
    want = [math.fmod(0.5 + i * 0.6180339887498949, 1.0) for i in range(6)]
    assert t.tolist() == [float(np.float32(w)) for w in want]
    assert t[0] == 0.5 and abs(float(t[1]) - 0.1180339887) < 1e-7 and abs(float(t[2]) - 0.7360679775) < 1e-7
    # a function of i only: any subset, any order, any batch
    idx = np.array([5, 0, 3, 2 ** 33 + 5, 3])
    sub = V.sample_times(idx)
    assert sub[0] == t[5] and sub[1] == t[0] and sub[2] == t[3] and sub[4] == t[3]
    assert sub[3] == V.sample_times([2 ** 33 + 5])[0] and 0.0 <= sub[3] < 1.0
    # the interval is an affine map of the same sequence
    lo, hi = 0.25, 0.75
    ti = V.sample_times(np.arange(1000), (lo, hi))
    u = 0.5 + np.arange(1000) * 0.6180339887498949
    assert np.array_equal(ti, (lo + (hi - lo) * (u - np.floor(u))).astype(np.float32)) and ti.min() >= lo and ti.max() <= hi
    # low discrepancy: every prefix fills ten equal bins evenly (three-distance theorem: the counts differ by a small constant)
    for n in (10, 100, 1000, 4096):
        c = np.bincount(V.bin_index(V.sample_times(np.arange(n)), 10), minlength=10)
        assert c.sum() == n and c.max() - c.min() <= 3, (n, c)
    for bad in ((0.5, 0.5), (-0.1, 1.0), (0.0, 1.5), (0.8, 0.2)):
        with pytest.raises(ValueError, match="interval"):
            V.check_interval(bad)


def test_importance_weights_and_bins_against_closed_forms():
    t = np.array([0.0, 0.1, 0.25, 0.5, 0.9, 1.0])
    w = V.lognorm_weights(t)
    assert w[0] == 0.0 and w[-1] == 0.0
    for ti, wi in zip(t[1:-1], w[1:-1]):
        z = math.log(ti / (1 - ti))
        assert wi == pytest.approx(math.exp(-z * z / 2) / math.sqrt(2 * math.pi) / (ti * (1 - ti)), rel=1e-13)
    assert w[3] == pytest.approx(4 / math.sqrt(2 * math.pi), rel=1e-14) and w[1] == pytest.approx(w[4], rel=1e-12)          # symmetric about 1/2
    # a density: it integrates to one (midpoint rule on a fine grid)
    g = (np.arange(200000) + 0.5) / 200000
    assert V.lognorm_weights(g).mean() == pytest.approx(1.0, abs=1e-6)
    assert np.array_equal(V.bin_edges(4), [0.0, 0.25, 0.5, 0.75, 1.0]) and np.allclose(V.bin_edges(5, (0.2, 0.7)), [0.2, 0.3, 0.4, 0.5, 0.6, 0.7], atol=1e-15)
    assert V.bin_index([0.0, 0.2499, 0.25, 0.75, 0.999, 1.0], 4).tolist() == [0, 0, 1, 3, 3, 3]
    assert V.bin_index([0.2, 0.45, 0.7], 5, (0.2, 0.7)).tolist() == [0, 2, 4]
    # the report: plain, per-bin and self-normalised weighted means of a known loss l(t) = t
    n = 5000
    tt = V.sample_times(np.arange(n)).astype(np.float64)
    rep = V.report(tt, tt, bins=10, use_lognorm=True)
    assert rep["num"] == n and rep["loss"] == pytest.approx(tt.mean(), rel=1e-14) and rep["sem"] == pytest.approx(tt.std(ddof=1) / math.sqrt(n), rel=1e-12)
    assert sum(r["count"] for r in rep["bins"]) == n
    for k, r in enumerate(rep["bins"]):
        sel = tt[(tt >= k / 10) & (tt < (k + 1) / 10)]
        assert r["count"] == sel.size and r["mean"] == pytest.approx(sel.mean(), rel=1e-13) and r["lo"] == pytest.approx(k / 10) and r["hi"] == pytest.approx((k + 1) / 10)
    ww = V.lognorm_weights(tt)
    assert rep["loss_train_weighted"] == pytest.approx((ww * tt).sum() / ww.sum(), rel=1e-13)
    assert rep["loss_train_weighted"] == pytest.approx(0.5, abs=5e-3)          # E t under the symmetric logit-normal
    assert "loss_train_weighted" not in V.report(tt, tt, bins=3)
    one = V.report([2.0], [0.5], bins=2)
    assert one["loss"] == 2.0 and one["sem"] is None and one["bins"][0]["mean"] is None and one["bins"][1]["count"] == 1


@pytest.mark.parametrize("world", [1, 2, 3])
def test_partition_and_merge_equal_the_single_rank_order(world):
    num = 11
    loss = lambda idx: np.sin(idx.astype(np.float64)) + 2.0          # noqa: E731
    single = V.merge_by_index([(V.rank_indices(num, 0, 1), loss(V.rank_indices(num, 0, 1)))], num)
    parts = [(V.rank_indices(num, r, world), loss(V.rank_indices(num, r, world))) for r in range(world)]
    assert all((idx % world == r).all() for r, (idx, _) in enumerate(parts))
    assert sorted(np.concatenate([i for i, _ in parts]).tolist()) == list(range(num))
    merged = V.merge_by_index(parts[::-1], num)                       # whatever order the ranks arrive in
    assert np.array_equal(merged, single) and np.array_equal(single, loss(np.arange(num)))
    if world > 1:
        with pytest.raises(ValueError, match="missing"):
            V.merge_by_index(parts[1:], num)
        with pytest.raises(ValueError, match="repeated"):
            V.merge_by_index(parts + parts[:1], num)
    with pytest.raises(ValueError, match="outside"):
        V.merge_by_index([(np.array([num]), np.array([1.0]))], num)
    with pytest.raises(ValueError, match="rank"):
        V.rank_indices(num, world, world)


def test_command_line_refusals(tmp_path, capsys):
    ck, data, stats = tmp_path / "c.pt", tmp_path / "shards", tmp_path / "latents_stats.pt"
    ck.write_bytes(b"x")
    stats.write_bytes(b"x")
    data.mkdir()
    ok = ["--config", CFG, "--ckpt", str(ck), "--data", str(data)]

    def refused(argv, text):
        with pytest.raises(SystemExit) as e:
            V.parse_args(argv)
        assert e.value.code == 2
        assert text in capsys.readouterr().err, (argv, text)

    a = V.parse_args(ok + ["--stats", str(stats), "--interval", "0.1", "0.9", "--weights", "both", "--num", "7"])
    assert a.interval == (0.1, 0.9) and a.weights == "both" and a.num == 7 and a.batch == 256 and a.seed == 0 and a.bins == 10 and a.precision == "bf16"
    assert V.parse_args(["--config", CFG, "--synthetic", "4"]).synthetic == 4
    refused(["--config", CFG, "--ckpt", str(ck)], "exactly one of --data DIR and --synthetic N")
    refused(ok + ["--synthetic", "4"], "exactly one of --data DIR and --synthetic N")
    refused(["--config", CFG, "--ckpt", "https://host/c.pt", "--data", str(data)], "downloads nothing")
    refused(["--config", CFG, "--ckpt", str(ck), "--data", "s3://bucket/shards"], "downloads nothing")
    refused(["--config", CFG, "--ckpt", str(tmp_path / "none.pt"), "--data", str(data)], "does not exist")
    refused(["--config", CFG, "--data", str(data)], "--data needs --ckpt")
    refused(["--config", CFG, "--ckpt", str(ck), "--data", str(tmp_path / "nodir")], "is not a directory")
    refused(ok + ["--stats", str(tmp_path / "nostats.pt")], "--stats")
    refused(["--config", str(tmp_path / "no.yaml"), "--synthetic", "4"], "--config")
    refused(ok + ["--sigma_rels", "0.05,0.1"], "--sigma_rels and --snapshots go together")
    refused(ok + ["--snapshots", str(data)], "--sigma_rels and --snapshots go together")
    refused(ok + ["--snapshots", str(tmp_path / "nosnaps"), "--sigma_rels", "0.05"], "is not a directory")
    refused(ok + ["--snapshots", str(data), "--sigma_rels", "0.05,0.9"], "--sigma_rels")
    refused(ok + ["--step", "8"], "--step needs --snapshots")
    refused(ok + ["--interval", "0.7", "0.2"], "--interval")
    refused(ok + ["--batch", "0"], "must be positive")
    a = V.parse_args(ok + ["--snapshots", str(data), "--sigma_rels", "0.03,0.05,0.075", "--step", "16"])
    assert a.sigma_rels == [0.03, 0.05, 0.075] and a.step == 16


def test_missing_statistics_are_refused_never_computed(tmp_path):
    import torch
    from safetensors.torch import save_file
    d = tmp_path / "valid"
    d.mkdir()
    save_file({"latents": torch.zeros(2, 8, 2, 2), "latents_flip": torch.zeros(2, 8, 2, 2), "labels": torch.zeros(2, dtype=torch.int64)},
              str(d / "latents_rank00_shard000.safetensors"))
    data = {"data_path": str(tmp_path / "train"), "latent_norm": True, "latent_multiplier": 1.0, "sample": True}
    with pytest.raises(SystemExit, match="latents_stats.pt"):
        V.ShardSource(str(d), data)
    assert os.listdir(d) == ["latents_rank00_shard000.safetensors"]               # nothing was computed or cached in the validation directory
    os.makedirs(tmp_path / "train_sample")                                        # the directory training reads: data_path + "_sample"
    torch.save({"mean": torch.full((1, 4, 1, 1), 0.5), "std": torch.full((1, 4, 1, 1), 2.0)}, tmp_path / "train_sample" / "latents_stats.pt")
    src = V.ShardSource(str(d), data)
    assert len(src) == 2 and src.sample and src.mean.tolist() == [0.5] * 4 and src.std.tolist() == [2.0] * 4
    x, y = src.read([1, 0])
    assert x.shape == (2, 8, 2, 2) and y.tolist() == [0, 0]
    plain = V.ShardSource(str(d), {"data_path": "unused", "latent_norm": False, "latent_multiplier": 0.5})
    assert plain.mean is None and not plain.sample and plain.multiplier == 0.5
    with pytest.raises(SystemExit, match="no \\*.safetensors"):
        V.ShardSource(str(tmp_path / "train_sample"), data)


def test_yaml_key():
    cfg = _cfg()
    assert V.valid_config(cfg) is None and V.training_plan(cfg, 32) == (None, None)
    cfg["data"]["valid_path"] = "/held/out"
    settings, line = V.training_plan(cfg, 32)                                      # valid_path alone: as before, the key is reported as ignored
    assert settings is None and line == "data.valid_path='/held/out' is ignored: the reference's validation pass calls an undefined evaluate()"
    cfg["train"]["valid"] = {}
    settings, line = V.training_plan(cfg, 32)
    assert settings == {"every": cfg["train"]["ckpt_every"], "num": 10000, "batch": 32, "seed": 0, "bins": 10, "weights": "both"}
    assert "Validation every 20000 steps" in line and "is ignored" not in line
    cfg["train"]["valid"] = yaml.safe_load("{every: 500, num: 2000, batch: 64, seed: 3, bins: 5, weights: ema}")
    assert V.valid_config(cfg, 32) == {"every": 500, "num": 2000, "batch": 64, "seed": 3, "bins": 5, "weights": "ema"}
    for bad, text in (({"every": 0}, "train.valid.every"), ({"num": -1}, "train.valid.num"), ({"batch": 2.5}, "train.valid.batch"),
                      ({"bins": True}, "train.valid.bins"), ({"seed": -1}, "train.valid.seed"), ({"weights": "all"}, "train.valid.weights"),
                      ({"evry": 5}, "keys out of"), ([1, 2], "must be a mapping")):
        cfg["train"]["valid"] = bad
        with pytest.raises(ValueError, match=text):
            V.valid_config(cfg, 32)
    cfg["train"]["valid"] = {"every": 2}
    del cfg["data"]["valid_path"]
    with pytest.raises(ValueError, match="train.valid needs data.valid_path"):
        V.valid_config(cfg, 32)


def test_train_driver_uses_the_plan():
    with open(os.path.join(ROOT, "ldmae_amd", "train_accum.py")) as f:
        src = f.read()
    assert "validate.training_plan(cfg, per_gpu)" in src and "validator.run(model, opt, train_steps, logger)" in src


def test_header_declares_the_entries_and_the_library_exports_them():
    import ctypes as C
    from ldmae_amd import _lib, ops
    S = _lib.SIGNATURES
    P = C.c_void_p
    assert S["ldmae_fm_valid_plan_f32"] == (C.c_int, [P, P, P, P, P, C.c_float, C.c_int, C.c_ulonglong, P, P, C.c_int, C.c_int, C.c_int, P])
    assert S["ldmae_row_mse_partials"] == (C.c_long, [C.c_int, C.c_long])
    assert S["ldmae_row_mse"] == (C.c_int, [C.c_int, P, P, P, C.c_int, C.c_long, P, P])
    lib = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in ("ldmae_fm_valid_plan_f32", "ldmae_row_mse_partials", "ldmae_row_mse"))
    fn = lib.ldmae_row_mse_partials
    fn.restype, fn.argtypes = S["ldmae_row_mse_partials"]
    assert [fn(3, m) for m in (80, 4096, 4097, 16384)] == [3, 3, 6, 12] and fn(0, 5) == 0
    assert callable(ops.fm_valid_plan) and callable(ops.row_mse)
    # both wrappers sit above conv2d_nhwc, outside the span of tests/test_ops_args_cpu.py's fixture table
    with open(ops.__file__) as f:
        text = f.read()
    assert max(text.index("def fm_valid_plan("), text.index("def row_mse(")) < text.index("def conv2d_nhwc(")
