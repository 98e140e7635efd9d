"""Held-out validation on the GPU: the plan kernel bitwise against the composition of the paths it fuses (ops.normal, ops.latent_prologue,
ICPlan.plan), its batch invariance, row_mse against f64 with a bound derived from its summation order, the command line end to end on a tiny
DiT, the in-training hook and the EMA width sweep."""
import copy
import json
import logging
import math
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234567890ABCDEF                      # both key words of the generator in use
BIG = 2 ** 33 + 5                              # 2 * BIG needs the high counter word
T_VALUES = (0.0, 0.5, 1.0 - 2.0 ** -24)
U = 2.0 ** -24                                 # unit roundoff of f32


@pytest.fixture(scope="module")
def ops():
    from ldmae_amd import _lib, ops as o
    assert _lib.load().ldmae_arch() == b"gfx950"
    return o


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _stored(B, C, HW, sample, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 2 * C if sample else C, HW // 4, 4, generator=g)
    if sample:
        x[:, C:] = x[:, C:] * 2.0 - 1.0                                   # log-variances of both signs
        x[0, C, 0, 0], x[0, C, 0, 1] = -45.0, 33.0                        # beyond the clamp on both sides
    return x.cuda()


def _composed(ops, stored, idx, t, mean, std, mult, sample):
    """The existing paths, one after the other: the two named draws materialised per sample, the prologue kernel, ICPlan.plan in torch."""
    from ldmae_amd.transport.path import ICPlan
    B, C2, H, W = stored.shape
    C = C2 // 2 if sample else C2
    n = C * H * W
    z = torch.stack([ops.normal((n,), SEED, 2 * i, "cuda") for i in idx]).view(B, C, H, W)
    x0 = torch.stack([ops.normal((n,), SEED, 2 * i + 1, "cuda") for i in idx]).view(B, C, H, W)
    x1 = ops.latent_prologue(stored, z if sample else None, mean, std, mult, sample)
    _, xt, ut = ICPlan().plan(t, x0, x1)
    return xt, ut


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("sample", [False, True], ids=["latents", "moments"])
@pytest.mark.parametrize("B,C,HW,idx", [(3, 4, 20, [7, BIG, 0]), (2, 16, 1024, [BIG, 3])], ids=["small", "wide"])
def test_plan_is_bitwise_the_composition_of_the_existing_paths(ops, B, C, HW, idx, sample, norm):
    stored = _stored(B, C, HW, sample, 17 * B + C)
    g = torch.Generator().manual_seed(3)
    mean = (torch.randn(C, generator=g) * 0.3).cuda() if norm else None
    std = (torch.rand(C, generator=g) + 0.5).cuda() if norm else None
    mult = 0.18215 if not norm else 1.7
    for shift in range(3):                                                # every sample meets every t of {0, 0.5, 1 - 2^-24}
        t = torch.tensor([T_VALUES[(b + shift) % 3] for b in range(B)], dtype=torch.float32, device="cuda")
        xt, ut = ops.fm_valid_plan(stored, torch.tensor(idx, dtype=torch.int64, device="cuda"), t, mean, std, mult, sample, SEED)
        rxt, rut = _composed(ops, stored, idx, t, mean, std, mult, sample)
        assert xt.shape == rxt.shape == (B, C, HW // 4, 4) and xt.dtype == ut.dtype == torch.float32
        assert torch.isfinite(xt).all() and torch.isfinite(ut).all()
        assert torch.equal(_bits(xt), _bits(rxt)), (shift, int((_bits(xt) != _bits(rxt)).sum()))
        assert torch.equal(_bits(ut), _bits(rut)), (shift, int((_bits(ut) != _bits(rut)).sum()))
    # the draws are named by the index: another index, another seed give other rows; t = 0 gives x0 itself, whatever is stored
    t0 = torch.zeros(B, device="cuda")
    xa, _ = ops.fm_valid_plan(stored, torch.tensor(idx, device="cuda"), t0, mean, std, mult, sample, SEED)
    xb, _ = ops.fm_valid_plan(stored * 0, torch.tensor(idx, device="cuda"), t0, mean, std, mult, sample, SEED)
    xc, _ = ops.fm_valid_plan(stored, torch.tensor(idx, device="cuda") + 1, t0, mean, std, mult, sample, SEED)
    xd, _ = ops.fm_valid_plan(stored, torch.tensor(idx, device="cuda"), t0, mean, std, mult, sample, SEED + 1)
    assert torch.equal(xa.abs(), xb.abs()) and not torch.equal(xa, xc) and not torch.equal(xa, xd)       # 0 * x1 + x0 (the zero may carry a sign)


@pytest.mark.parametrize("sample", [False, True], ids=["latents", "moments"])
def test_plan_rows_do_not_depend_on_the_batch(ops, sample):
    C, HW = 16, 64
    stored = _stored(3, C, HW, sample, 5)
    idx = torch.tensor([11, BIG, 11], dtype=torch.int64, device="cuda")
    t = torch.tensor([0.3, 0.9, 0.3], device="cuda")
    st3 = torch.stack([stored[0], stored[1], stored[0]])                  # index 11 at positions 0 and 2
    xt3, ut3 = ops.fm_valid_plan(st3, idx, t, None, None, 1.0, sample, SEED)
    xt1, ut1 = ops.fm_valid_plan(stored[:1], idx[:1], t[:1], None, None, 1.0, sample, SEED)
    for k in (0, 2):
        assert torch.equal(_bits(xt3[k]), _bits(xt1[0])) and torch.equal(_bits(ut3[k]), _bits(ut1[0]))
    assert not torch.equal(xt3[1], xt3[0])


def test_plan_refusals(ops):
    st = torch.zeros(2, 8, 2, 3, device="cuda")
    idx, t = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(2, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.fm_valid_plan(st, idx, t)
    st = torch.zeros(2, 8, 2, 4, device="cuda")
    with pytest.raises(RuntimeError, match="fm_valid_plan idx"):
        ops.fm_valid_plan(st, idx.int(), t)
    with pytest.raises(RuntimeError, match="fm_valid_plan t"):
        ops.fm_valid_plan(st, idx, t[:1])
    with pytest.raises(RuntimeError, match="both lat_mean and lat_std"):
        ops.fm_valid_plan(st, idx, t, lat_mean=torch.zeros(4, device="cuda"))
    with pytest.raises(RuntimeError, match="fm_valid_plan lat_std"):
        ops.fm_valid_plan(st, idx, t, torch.zeros(4, device="cuda"), torch.ones(8, device="cuda"))
    with pytest.raises(RuntimeError, match="fm_valid_plan stored"):
        ops.fm_valid_plan(st[:, :7], idx, t)
    with pytest.raises(RuntimeError, match="row_mse u"):
        ops.row_mse(st, st[:, :4])
    with pytest.raises(RuntimeError, match="row_mse a"):
        ops.row_mse(st.half(), st)


def mse_bound(terms_sum, m):
    """|got - ref| <= gamma_k * ref, k = 3 + the longest chain of additions one term goes through, from the kernel's order (csrc/fm_valid.hip):
    a term carries the rounding of a - u twice (it is squared) and the rounding of its own fma: 3.  Then at most 15 further fmas of the thread's
    chain (16 elements per thread per chunk), 6 butterfly additions, 2 to join the four waves; in the fold ceil(chunks / 256) additions per
    thread, again 6 + 2; one rounding of the division by m.  gamma_k = k u / (1 - k u), u = 2^-24, applied to the sum of the (non-negative) terms."""
    chunks = -(-m // 4096)
    k = 3 + 15 + 6 + 2 + -(-chunks // 256) + 6 + 2 + 1
    return k * U / (1 - k * U) * terms_sum / m


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("m", [80, 5140, 16384])
def test_row_mse_against_f64(ops, m, dtype, offset):
    """m = 80: less than one thread group per lane; 5140: a ragged last chunk; 16384: four chunks.  offset 1: both bases one element past an
    aligned address, so every size also runs on element loads (another fixed order, the same bound)."""
    B = 3
    g = torch.Generator().manual_seed(m + offset)
    abuf = torch.zeros(B * m + 8, dtype=dtype, device="cuda")
    ubuf = torch.zeros(B * m + 8, dtype=torch.float32, device="cuda")
    a, u = abuf[offset:offset + B * m].view(B, m), ubuf[offset:offset + B * m].view(B, m)
    a.copy_(torch.randn(B, m, generator=g).to(dtype))
    u.copy_(torch.randn(B, m, generator=g) * 1.5 + 0.25)
    got = ops.row_mse(a, u)
    again = ops.row_mse(a, u)
    assert got.dtype == torch.float32 and got.shape == (B,) and torch.equal(_bits(got), _bits(again))
    terms = (a.double() - u.double()) ** 2
    ref = terms.mean(dim=1).cpu().numpy()
    bound = np.array([mse_bound(float(s), m) for s in terms.sum(dim=1).cpu()])
    err = np.abs(got.double().cpu().numpy() - ref)
    print(f"row_mse m={m} {dtype} offset={offset}: max err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), (err, bound)
    assert bool((abuf[:offset] == 0).all()) and bool((abuf[offset + B * m:] == 0).all())
    out = torch.full((B + 2,), 7.0, device="cuda")
    assert ops.row_mse(a, u, out=out[1:B + 1]).data_ptr() == out[1:].data_ptr()
    assert torch.equal(_bits(out[1:B + 1]), _bits(got)) and float(out[0]) == 7.0 and float(out[-1]) == 7.0


# ----------------------------------------------------------------------------- drivers, on the tiny DiT of the other GPU tests
def _tiny_model(monkeypatch):
    from ldmae_amd.models import lightningdit as L
    monkeypatch.setitem(L.LightningDiT_models, "LightningDiT-B/1", lambda **kw: L.LightningDiT(depth=2, hidden_size=192, patch_size=1, num_heads=3, **kw))


def _cfg(tmp_path):
    cfg = copy.deepcopy(yaml.safe_load(open(os.path.join(ROOT, "ldmae_amd/configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml"))))
    cfg["data"].update(image_size=64, num_workers=0, data_path=str(tmp_path / "feat"))
    return cfg


def _write_shards(tmp_path, n=(5, 4)):
    """Two shards of posterior moments [n, 32, 8, 8] with labels, and the TRAINING directory's statistics (data_path + '_sample')."""
    from safetensors.torch import save_file
    d = tmp_path / "held_out"
    d.mkdir()
    g = torch.Generator().manual_seed(21)
    for s, k in enumerate(n):
        lat = torch.randn(k, 32, 8, 8, generator=g)
        lat[:, 16:] = lat[:, 16:] - 2.0
        save_file({"latents": lat, "latents_flip": lat.flip(-1), "labels": torch.randint(0, 1000, (k,), generator=g)},
                  str(d / f"latents_rank00_shard{s:03d}.safetensors"))
    os.makedirs(tmp_path / "feat_sample", exist_ok=True)
    torch.save({"mean": torch.randn(1, 16, 1, 1, generator=g) * 0.1, "std": torch.rand(1, 16, 1, 1, generator=g) + 0.5},
               tmp_path / "feat_sample" / "latents_stats.pt")
    return str(d)


def _json_lines(text):
    return [ln for ln in text.splitlines() if ln.startswith("{")]


def test_command_line_end_to_end(ops, tmp_path, monkeypatch, capsys):
    import ldmae_amd.train_accum as T
    import ldmae_amd.validate as V
    _tiny_model(monkeypatch)
    cfg = _cfg(tmp_path)
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    data = _write_shards(tmp_path)
    g = torch.Generator().manual_seed(1)
    model = T.build_model(cfg)
    sd = {k: (v + 0.05 * torch.randn(v.shape, generator=g) if v.is_floating_point() and k != "pos_embed" else v.clone()) for k, v in model.state_dict().items()}
    ema = {k: (v + 0.01 * torch.randn(v.shape, generator=g) if v.is_floating_point() and k != "pos_embed" else v.clone()) for k, v in sd.items()}
    torch.save({"model": sd, "ema": ema}, tmp_path / "differ.pt")
    torch.save({"model": sd, "ema": {k: v.clone() for k, v in sd.items()}}, tmp_path / "copy.pt")
    argv = ["--config", str(tmp_path / "cfg.yaml"), "--data", data, "--batch", "4", "--seed", "5", "--bins", "4"]

    seen = []
    real = ops.row_mse

    def spy(a, u, out=None):
        r = real(a, u, out=out)
        seen.append((a.detach().clone(), u.detach().clone(), r.detach().clone()))
        return r

    monkeypatch.setattr(ops, "row_mse", spy)
    res = V.main(argv + ["--ckpt", str(tmp_path / "differ.pt"), "--weights", "both"])
    out1 = capsys.readouterr().out
    monkeypatch.setattr(ops, "row_mse", real)
    assert len(_json_lines(out1)) == 1 and json.loads(_json_lines(out1)[0]) == res
    assert "model: 9 samples, loss" in out1 and "ema: 9 samples, loss" in out1 and "expected training loss" in out1 and "t in [0.750, 1.000]" in out1
    rm, re_ = res["weights"]["model"], res["weights"]["ema"]
    assert rm["num"] == re_["num"] == 9 and len(rm["bins"]) == 4 and sum(r["count"] for r in rm["bins"]) == 9
    assert math.isfinite(rm["loss"]) and rm["sem"] > 0 and math.isfinite(rm["loss_train_weighted"])
    assert rm["loss"] != re_["loss"]                                                       # the EMA differs from the model, and so does its loss
    # the per-sample losses against mean_flat((out - ut) ** 2) in f64 from the same model outputs: batches of 4, 4, 1 for each of the two weights
    assert [a.shape[0] for a, _, _ in seen] == [4, 4, 1, 4, 4, 1]
    per = []
    for a, u, r in seen:
        terms = (a.double() - u.double()).flatten(1) ** 2
        m = terms.shape[1]
        bound = np.array([mse_bound(float(s), m) for s in terms.sum(dim=1).cpu()])
        assert (np.abs(r.double().cpu().numpy() - terms.mean(dim=1).cpu().numpy()) <= bound).all()
        per.append(r.double().cpu().numpy())
    assert rm["loss"] == float(np.concatenate(per[:3]).mean()) and re_["loss"] == float(np.concatenate(per[3:]).mean())
    # run twice: the identical JSON line; another batch size: the identical per-sample question, so the identical figures
    V.main(argv + ["--ckpt", str(tmp_path / "differ.pt"), "--weights", "both"])
    out2 = capsys.readouterr().out
    assert _json_lines(out2) == _json_lines(out1)
    res3 = V.main(["--config", str(tmp_path / "cfg.yaml"), "--data", data, "--batch", "9", "--seed", "5", "--bins", "4", "--ckpt", str(tmp_path / "differ.pt"),
                   "--weights", "both", "--precision", "fp32"])
    res4 = V.main(["--config", str(tmp_path / "cfg.yaml"), "--data", data, "--batch", "2", "--seed", "5", "--bins", "4", "--ckpt", str(tmp_path / "differ.pt"),
                   "--weights", "both", "--precision", "fp32"])
    assert res3["weights"]["model"]["loss"] == pytest.approx(res4["weights"]["model"]["loss"], rel=1e-5)
    # an EMA that is a copy of the model: equal figures; the default picks the EMA
    resc = V.main(argv + ["--ckpt", str(tmp_path / "copy.pt"), "--weights", "both"])
    assert resc["weights"]["model"] == resc["weights"]["ema"] and resc["weights"]["model"]["loss"] == rm["loss"]
    resd = V.main(argv + ["--ckpt", str(tmp_path / "differ.pt")])
    assert list(resd["weights"]) == ["ema"] and resd["weights"]["ema"] == re_
    # another seed asks another question; --num takes a prefix of the same one
    assert V.main(argv[:-4] + ["--seed", "6", "--bins", "4", "--ckpt", str(tmp_path / "differ.pt")])["weights"]["ema"]["loss"] != re_["loss"]
    resn = V.main(argv + ["--ckpt", str(tmp_path / "differ.pt"), "--weights", "model", "--num", "4"])
    assert resn["weights"]["model"]["loss"] == float(per[0].mean())
    capsys.readouterr()


class _StepLoader:
    """Batch k and the random draws of the step that consumes it are functions of k alone (as tests/test_gpu_posthoc_ema.py's loader)."""

    def __init__(self, shape, num_classes, batch):
        self.shape, self.num_classes, self.batch = shape, num_classes, batch

    def __iter__(self):
        k = 0
        while True:
            g = torch.Generator().manual_seed(9000 + k)
            x, y = torch.randn((self.batch,) + self.shape, generator=g), torch.randint(0, self.num_classes, (self.batch,), generator=g)
            k += 1
            yield x, y


def _train(tmp_path, monkeypatch, name, steps, valid_path=None, **train):
    import ldmae_amd.train_accum as T
    monkeypatch.setattr(T, "make_loader", lambda cfg, per_gpu, rank, world, synthetic: (range(1 << 10), _StepLoader((16, 8, 8), 1000, per_gpu)))
    cfg = _cfg(tmp_path)
    if valid_path is not None:
        cfg["data"]["valid_path"] = valid_path
    cfg["train"].update(global_batch_size=8, output_dir=str(tmp_path / name), exp_name="t", log_every=2, ckpt_every=100, max_steps=steps)
    cfg["train"].update(train)
    torch.manual_seed(0)
    np.random.seed(0)
    model, opt = T.do_train(cfg, synthetic=True)
    return cfg, model, opt


def test_training_hook(ops, tmp_path, monkeypatch, caplog):
    import ldmae_amd.validate as V
    _tiny_model(monkeypatch)
    data = _write_shards(tmp_path)
    slabs = []
    real = V.TrainValidator.run

    def spy(self, model, opt, step, logger):
        before = (opt.flat.params.clone(), opt.ema.clone())
        reps = real(self, model, opt, step, logger)
        slabs.append((step, before, (opt.flat.params.clone(), opt.ema.clone()), model.training, reps))
        return reps

    monkeypatch.setattr(V.TrainValidator, "run", spy)
    caplog.set_level(logging.INFO, logger="ldmae_amd.train")
    _, model, opt = _train(tmp_path, monkeypatch, "with", 4, valid_path=data, valid={"every": 2, "num": 8})
    assert [s[0] for s in slabs] == [2, 4]
    for step, before, after, training, reps in slabs:
        assert training and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(before, after)), step
        assert set(reps) == {"model", "ema"} and reps["model"]["num"] == 8
    text = caplog.text
    assert text.count("Validation Loss (model / ema):") == 2 and "(step=0000002) Validation Loss" in text and "(step=0000004) Validation Loss" in text
    assert "Validation every 2 steps" in text and "is ignored" not in text
    lines = [json.loads(ln) for ln in open(tmp_path / "with" / "t" / "validation.jsonl")]
    assert [ln["step"] for ln in lines] == [2, 4] and all(set(ln) == {"step", "seed", "model", "ema"} and len(ln["model"]["bins"]) == 10 for ln in lines)
    assert lines[1]["model"] == slabs[1][4]["model"] and lines[0]["model"]["loss"] != lines[1]["model"]["loss"]
    # the same run without train.valid: validation consumed no random stream of training and left no trace in the weights
    caplog.clear()
    slabs.clear()
    _, model0, opt0 = _train(tmp_path, monkeypatch, "without", 4)
    assert not slabs and not (tmp_path / "without" / "t" / "validation.jsonl").exists() and "Validation" not in caplog.text
    assert torch.equal(_bits(opt0.flat.params), _bits(opt.flat.params)) and torch.equal(_bits(opt0.ema), _bits(opt.ema))
    # data.valid_path alone: reported as ignored, as before
    caplog.clear()
    _train(tmp_path, monkeypatch, "ignored", 1, valid_path=data)
    assert "is ignored: the reference's validation pass calls an undefined evaluate()" in caplog.text and "Validation Loss" not in caplog.text
    assert not slabs


def test_ema_width_sweep(ops, tmp_path, monkeypatch, capsys):
    import ldmae_amd.train_accum as T
    import ldmae_amd.validate as V
    from ldmae_amd import posthoc_ema as ph
    _tiny_model(monkeypatch)
    data = _write_shards(tmp_path)
    cfg, model, opt = _train(tmp_path, monkeypatch, "run", 8, posthoc_ema={"sigma_rels": [0.05, 0.10], "snapshot_every": 2})
    snaps = str(tmp_path / "run" / "t" / "checkpoints" / "ema_snapshots")
    assert ph.read_index(snaps)["steps"] == [2, 4, 6, 8]
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    argv = ["--config", str(tmp_path / "cfg.yaml"), "--data", data, "--batch", "8", "--precision", "fp32"]
    capsys.readouterr()
    res = V.main(argv + ["--snapshots", snaps, "--sigma_rels", "0.05,0.075,0.1"])
    out = capsys.readouterr().out
    rows = [ln for ln in out.splitlines() if ln.strip().startswith("sigma_rel ")]
    assert len(rows) == 3 and sum("<- minimum" in r for r in rows) == 1 and all(" -> " in r and " +- " in r for r in rows)
    assert [r["sigma_rel"] for r in res["sweep"]] == [0.05, 0.075, 0.1] and all(r["step"] == 8 and r["num"] == 9 for r in res["sweep"])
    assert res["best_sigma_rel"] == min(res["sweep"], key=lambda r: r["loss"])["sigma_rel"] and json.loads(_json_lines(out)[0]) == res
    # the row of a stored track's width = validating that track's reconstruction directly
    sd, _ = ph.reconstruct(snaps, 0.05)
    torch.save({"ema": dict(T.build_model(cfg).state_dict(), **sd)}, tmp_path / "ema005.pt")
    direct = V.main(argv + ["--ckpt", str(tmp_path / "ema005.pt")])["weights"]["ema"]
    row = {k: v for k, v in res["sweep"][0].items() if k not in ("sigma_rel", "step", "residual_rel")}
    assert row == direct
    capsys.readouterr()
