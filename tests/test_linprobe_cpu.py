"""Linear probe / k-NN, everything that needs no GPU: the schedule, the refusals, the header, the centre table, the loader's defaults, the JSON
keys, and the f64 LARS restatement of linprobe_check.py against the golden trajectories of the reference's util/lars.py."""
import argparse
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import linprobe_check as lc
from ldmae_amd import _lib, linear_probe as lp, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ldmae_token_mean", "ldmae_bn1d_fwd", "ldmae_softmax_xent", "ldmae_lars_workspace_bytes", "ldmae_lars_norms", "ldmae_lars_step",
       "ldmae_l2_normalize", "ldmae_topk_merge", "ldmae_knn_vote")


def _args(**kw):
    return argparse.Namespace(**{**vars(lp.build_parser().parse_args([])), **kw})


# ------------------------------------------------------------------------------------------------ schedule
def test_schedule_closed_form():
    ipe, lr, mn, E, W = 7, 3.2, 0.05, 10, 3
    assert lp.lr_at(0, ipe, lr, mn, E, W) == 0.0
    assert lp.lr_at(1, ipe, lr, mn, E, W) == pytest.approx(lr * (1 / ipe) / W, rel=1e-15)
    assert lp.lr_at(W * ipe, ipe, lr, mn, E, W) == pytest.approx(lr, rel=1e-15)                    # the end of warm-up: the peak
    last = E * ipe - 1
    want = mn + (lr - mn) * 0.5 * (1 + math.cos(math.pi * (last / ipe - W) / (E - W)))
    assert lp.lr_at(last, ipe, lr, mn, E, W) == pytest.approx(want, rel=1e-15)
    assert mn < lp.lr_at(last, ipe, lr, mn, E, W) < mn + (lr - mn) * 0.01                         # one iteration short of min_lr
    mid = (W + (E - W) / 2) * ipe
    assert lp.lr_at(mid, ipe, lr, mn, E, W) == pytest.approx((lr + mn) / 2, rel=1e-12)
    assert lp.lr_at(0, ipe, lr, mn, E, 0) == lr                                                  # no warm-up: starts at the peak


def test_lr_scales_with_batch_and_accumulation():
    assert lp.scaled_lr(0.1, 256) == pytest.approx(0.1)
    assert lp.scaled_lr(0.1, 1024) == pytest.approx(0.4)
    assert lp.scaled_lr(0.1, 1024, 4) == pytest.approx(1.6)
    assert lp.scaled_lr(0.1, 16384) == pytest.approx(6.4)                                        # MAE's 16 384-image batch


def test_defaults_are_maes_recipe():
    a = lp.build_parser().parse_args([])
    assert (a.blr, a.epochs, a.warmup_epochs, a.min_lr, a.batch_size, a.accum_iter) == (0.1, 90, 10, 0.0, 1024, 1)
    assert (a.momentum, a.trust, a.weight_decay) == (0.9, 0.001, 0.0)
    assert (a.features, a.pool, a.aug, a.head_norm, a.knn, a.knn_k, a.knn_T) == ("latent", "mean", "rrc", "bn", True, 20, 0.07)
    assert (lp.BN_EPS, lp.BN_MOMENTUM, lp.HEAD_STD, lp.RRC_SCALE) == (1e-6, 0.1, 0.01, (0.08, 1.0))
    assert "data-parallel probe is out of scope" in re.sub(r"\s+", " ", lp.build_parser().format_help())


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("flag,value", [("--features", "pixels"), ("--pool", "max"), ("--aug", "none"), ("--head_norm", "ln")])
def test_parser_refuses_unknown_choices(flag, value):
    with pytest.raises(SystemExit):
        lp.build_parser().parse_args([flag, value])


def test_check_args_refuses():
    lp.check_args(_args())
    for kw, word in ((dict(features="pixels"), "--features"), (dict(pool="max"), "--pool"), (dict(knn_k=257), "TOPK_MAX_K"), (dict(knn_k=0), "--knn_k"),
                     (dict(batch_size=1), "--batch_size"), (dict(knn_T=0.0), "--knn_T")):
        with pytest.raises(ValueError, match=word):
            lp.check_args(_args(**kw))
    lp.check_args(_args(knn=False, knn_k=1000))                                                  # k is not looked at without --knn
    with pytest.raises(ValueError, match="pool"):
        lp.pool_features(None, None, "latent", "max")


def test_encode_features_refuses_unknown_source():
    from ldmae_amd.tokenizer import models_mae
    src = inspect.getsource(models_mae.MaskedAutoencoderViT.encode_features)
    assert 'raise ValueError' in src and '("encoder", "latent")' in src


def test_k_above_256_is_refused():
    assert ops.TOPK_MAX_K == 256
    with pytest.raises(ValueError, match="256"):
        ops.topk_empty(4, 257, "cpu")
    rc = _lib.load().ldmae_topk_merge(ctypes.c_void_p(16), 8, 1, 8, 0, ctypes.c_void_p(16), ctypes.c_void_p(16), 257, None)
    assert rc == -1 and "LDMAE_TOPK_MAX_K" in _lib.last_error()
    rc = _lib.load().ldmae_knn_vote(ctypes.c_void_p(16), ctypes.c_void_p(16), 1, 2, ctypes.c_void_p(16), 1, ctypes.c_void_p(16),
                                    ops.KNN_VOTE_MAX_C + 1, 0.07, ctypes.c_void_p(16), None, None)
    assert rc == -1 and "LDMAE_KNN_VOTE_MAX_C" in _lib.last_error()


def test_labels_out_of_range_are_refused_on_the_host():
    for bad in ([0, 5, 2], [0, -1, 2]):
        with pytest.raises(ValueError, match=r"labels\[1\]"):
            ops.check_labels(torch.tensor(bad), 5, "cuda")
    with pytest.raises(ValueError, match="vector"):
        ops.check_labels(torch.zeros(2, 2, dtype=torch.int64), 5, "cuda")
    with pytest.raises(ValueError, match="vector"):
        ops.check_labels(torch.zeros(3), 5, "cuda")
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.check_labels(torch.tensor([0, 1]), 5, "cpu")


def test_bn_of_one_row_is_refused():
    x = torch.zeros(1, 16)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.bn1d_fwd(x, torch.zeros(16), torch.ones(16), training=True)
    P = ctypes.c_void_p(16)
    rc = _lib.load().ldmae_bn1d_fwd(0, P, 16, P, 16, P, P, None, None, 1, 16, 1e-6, 0.1, 1, None)
    assert rc == -1 and "more than one row" in _lib.last_error()


def test_cpu_tensors_are_refused():
    x = torch.zeros(4, 16)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.token_mean(torch.zeros(2, 4, 16))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.bn1d_fwd(x, torch.zeros(16), torch.ones(16))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.softmax_xent(x, torch.tensor([0, 1, 2, 3]))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.lars_step(torch.zeros(8), torch.zeros(8), torch.zeros(8), 0.1)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.lars_norms(torch.zeros(8), torch.zeros(8))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.topk_merge(x, 0, torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.l2_normalize(x)
    if not torch.cuda.is_available():                           # the driver's own refusal is only reachable without a GPU
        with pytest.raises(RuntimeError, match="needs a GPU"):
            lp.linear_probe(_args(synthetic=8), {"data": {"image_size": 32}, "vae": {"model_name": "vmae_f8d16"}})


@pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers: only where no kernel can be launched")
@pytest.mark.parametrize("code", [1, 2, 7, -1])
def test_f32_only_entries_refuse_other_dtype_codes(code):
    P, lib = ctypes.c_void_p(16), _lib.load()
    calls = {"bn1d_fwd": lambda: lib.ldmae_bn1d_fwd(code, P, 16, P, 16, P, P, None, None, 4, 16, 1e-6, 0.1, 1, None),
             "softmax_xent": lambda: lib.ldmae_softmax_xent(code, P, 8, P, P, None, 0, P, 2, 8, 0.0, None),
             "lars_norms": lambda: lib.ldmae_lars_norms(code, P, P, 8, 0.0, P, P, None),
             "lars_step": lambda: lib.ldmae_lars_step(code, P, P, P, 8, None, 0.1, 0.0, 0.9, 0.001, None)}
    if code in (7, -1):
        calls["token_mean"] = lambda: lib.ldmae_token_mean(code, P, 16, 0, P, 2, 4, 16, None)
    for name, f in calls.items():
        rc = f()
        msg = _lib.last_error()
        assert rc == -1 and msg.startswith(name + ":") and f"dtype {code}" in msg, (name, rc, msg)


# ------------------------------------------------------------------------------------------------ header and binding
def test_header_declares_and_binds_the_new_entries():
    header = open(os.path.join(ROOT, "include", "ldmae_hip.h")).read()
    declared = set(re.findall(r"\b(ldmae_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    res, argt = _lib.SIGNATURES["ldmae_token_mean"]
    assert res is ctypes.c_int and argt == [ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_void_p]
    assert _lib.SIGNATURES["ldmae_lars_workspace_bytes"] == (ctypes.c_long, [ctypes.c_long])
    assert _lib.SIGNATURES["ldmae_lars_step"][1][5:10] == [ctypes.c_void_p] + [ctypes.c_float] * 4
    assert lib.ldmae_lars_workspace_bytes(1) == 16 and lib.ldmae_lars_workspace_bytes(4097) == 32 and lib.ldmae_lars_workspace_bytes(0) == 0
    assert f"#define LDMAE_TOPK_MAX_K {ops.TOPK_MAX_K}\n" in header and f"#define LDMAE_KNN_VOTE_MAX_C {ops.KNN_VOTE_MAX_C}\n" in header
    assert "linprobe.hip" in open(os.path.join(ROOT, "ldmae_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "ldmae_amd", "ops.py")).read()
    for name in NEW:
        assert src.count(f'"{name}"') + src.count(f".{name}(") == 1, name                      # one wrapper each


# ------------------------------------------------------------------------------------------------ loader
def test_center_table_tall_wide_square():
    from ldmae_amd.datasets.packed_images import center_table
    t = center_table(np.array([[57, 40], [40, 57], [48, 48], [41, 40], [7, 300]]))
    assert t.dtype == torch.int32 and t.tolist() == [[57, 40, 8, 0, 40, 40, 0, 0], [40, 57, 0, 8, 40, 40, 0, 0], [48, 48, 0, 0, 48, 48, 0, 0],
                                                     [41, 40, 0, 0, 40, 40, 0, 0], [7, 300, 0, 146, 7, 7, 0, 0]]
    ops.check_crop_table(torch.zeros(5, dtype=torch.int64), t, 3 * 300 * 57)                      # every box lies inside its image


def test_loader_defaults_are_unchanged():
    from ldmae_amd.datasets import packed_images as pk
    sig = inspect.signature(pk.PackedBatchLoader.__init__)
    assert sig.parameters["center"].default is False and sig.parameters["drop_last"].default is True
    assert list(sig.parameters)[-2:] == ["center", "drop_last"]                                  # appended: positional callers are untouched
    assert sig.parameters["scale"].default == (0.75, 1.0)
    src = inspect.getsource(pk.PackedBatchLoader)
    assert "center_table(ds.sizes[idx]) if self.center else draw_table(ds.sizes[idx], self.input_size, self.scale, self.ratio, g)" in src
    assert "len(order) // self.batch_size if self.drop_last else" in src


def test_synthetic_pack_round_trips(tmp_path):
    from ldmae_amd.datasets.packed_images import PackedImages
    root = lp.write_synthetic_pack(str(tmp_path / "p"), 10, 3)
    ds = PackedImages(root)
    assert len(ds) == 10 and ds.labels.tolist() == [i % 4 for i in range(10)] and len(ds.classes) == 4
    assert sorted({tuple(s) for s in ds.sizes.tolist()}) == [(40, 56), (48, 48), (56, 40)]
    again = PackedImages(lp.write_synthetic_pack(str(tmp_path / "q"), 10, 3))
    assert all(np.array_equal(ds.image(i), again.image(i)) for i in range(10))                    # seeded
    means = np.stack([ds.image(i).reshape(-1, 3).mean(0) for i in range(8)])
    assert np.array_equal(means.argmax(1)[:3], [0, 1, 2])                                        # the class fixes the colour


def test_json_keys():
    assert lp.JSON_KEYS == ("top1", "top5", "knn_top1", "knn_top5", "features", "pool", "epochs", "images")
    src = inspect.getsource(lp.linear_probe)
    body = src[src.index("res = {"):src.index('print(json.dumps({"metric": "linear_probe", **res})')]
    assert tuple(re.findall(r'"(\w+)":', body)) == lp.JSON_KEYS


# ------------------------------------------------------------------------------------------------ LARS against the reference
@pytest.mark.parametrize("case", ["main", "zero_p", "zero_update"])
def test_lars_restatement_matches_the_reference(golden, case):
    g = golden("linprobe")
    wd, momentum, trust = g[case + "_hp"]
    for which, scaled in (("w", True), ("b", False)):
        p, mu = g[f"{case}_p0_{which}"].reshape(-1), np.zeros(g[f"{case}_p0_{which}"].size)
        for s, lr in enumerate(g[case + "_lr"]):
            p, mu = lc.lars_step_ref(p, g[f"{case}_g{which}"][s].reshape(-1), mu, lr, wd, momentum, trust, scaled)
            for got, name in ((p, which), (mu, "mu_" + which)):
                want = g[f"{case}_{name}"][s].reshape(-1)
                assert np.allclose(got, want, rtol=1e-13, atol=1e-300), (case, name, s, np.abs(got - want).max())
    if case == "zero_p":
        assert not g["zero_p_p0_w"].any() and np.array_equal(g["zero_p_w"][0], -g["zero_p_lr"][0] * g["zero_p_gw"][0])      # q = 1
    if case == "zero_update":
        assert np.array_equal(g["zero_update_w"][0], g["zero_update_p0_w"]) and not g["zero_update_mu_w"][0].any()


def test_lars_bounds_are_small_and_grow(golden):
    g = golden("linprobe")
    wd, momentum, trust = g["main_hp"]
    ps, mus, eps, emus = lc.lars_trajectory_ref(g["main_p0_w"].reshape(-1), g["main_gw"].reshape(5, -1), g["main_lr"], wd, momentum, trust, True)
    assert np.allclose(ps[-1], g["main_w"][-1].reshape(-1), rtol=1e-13)
    scale = np.abs(ps[-1]).max()
    assert 0 < eps[0].max() < eps[-1].max() < 1e-4 * scale


# ------------------------------------------------------------------------------------------------ the restatements themselves
def test_rank_rule_and_topk_reference():
    l = np.array([[1.0, 3.0, 3.0, 0.5, 3.0]], dtype=np.float32)
    assert [int(lc.rank_ref(l, np.array([y]))[0]) for y in range(5)] == [3, 0, 1, 4, 2]           # ties go to the lower class
    v, i = lc.topk_ref(np.array([[0.5, 2.0, 2.0, -1.0]], dtype=np.float32), 6)
    assert i.tolist() == [[1, 2, 0, 3, -1, -1]] and v[0, :4].tolist() == [2.0, 2.0, 0.5, -1.0] and np.isneginf(v[0, 4:]).all()


def test_bn_negative_control_breaks_the_bound():
    """The mean-1e3 / std-1e-2 column of the GPU test: a one-pass E[x^2] - mean^2 in f32 leaves the bound by orders of magnitude."""
    rng = np.random.default_rng(5)
    x = (1e3 + 1e-2 * rng.standard_normal((1000, 1))).astype(np.float32)
    r = lc.bn1d_ref(x, 1e-6, np.zeros(1), np.ones(1))
    assert r["bound"].max() < 0.05 and abs(r["xhat"].std() - 1) < 1e-2
    assert (np.abs(lc.bn1d_naive_f32(x, 1e-6) - r["xhat"]) > 10 * r["bound"]).mean() > 0.5
