"""Post-hoc EMA on the GPU: the fused AdamW + EMA + tracks pass and its tracks-only sibling per element against the f64 restatement of
the contract (posthoc_check.py; bounds derived there), p / m / v / ema bitwise against ldmae_adamw_ema, the f64 snapshot combination, the
whole path from optimizer steps to a reconstructed checkpoint against the brute-force average, and the train driver."""
import copy
import os
import shutil

import numpy as np
import pytest
import torch
import yaml

import posthoc_check as pc
from ldmae_amd import posthoc_ema as ph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, CANARY = 64, 12345.0
HYP = dict(lr=1e-2, beta1=0.9, beta2=0.95, eps=1e-8, ema_decay=0.9999)
NS = [1, 3, 4, 4099]          # below a vector; a scalar tail alone; one vector; more than one block (256 threads x 4) with a tail
SIGMAS = (0.05, 0.10, 0.03, 0.20)
WORST: dict = {}


@pytest.fixture(scope="module")
def ops():
    from ldmae_amd import _lib, ops as o
    assert _lib.load().ldmae_arch() == b"gfx950"
    yield o
    if WORST:
        print("\nworst |got - ref| / bound:")
        for k in sorted(WORST):
            print(f"  {k:40s} {WORST[k]:.3f}")


def _guarded(a, off=0, dtype=torch.float32):
    """A device copy of the numpy array inside a canary-filled buffer, `off` elements past a 256-byte boundary: (buffer, view)."""
    n = a.size
    buf = torch.full((GUARD + off + n + GUARD,), CANARY, dtype=dtype, device="cuda")
    view = buf[GUARD + off:GUARD + off + n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dtype))
    return buf, view


def _intact(buf, off, n):
    return bool((buf[:GUARD + off] == CANARY).all()) and bool((buf[GUARD + off + n:] == CANARY).all())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _check(key, got, ref, bound):
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), key
    r = np.abs(got - ref) / np.maximum(bound, 1e-300)
    r = np.where((bound == 0) & (got == ref), 0.0, r)
    WORST[key] = max(WORST.get(key, 0.0), float(r.max()))
    assert (np.abs(got - ref) <= bound).all(), (key, float(r.max()))


def _pad4(a):
    return np.concatenate([a, np.zeros(-a.size % 4, dtype=a.dtype)])


CASES = [dict(n=n, K=K, start=start, gscale=1.0, off=0, wd=0.0) for n in NS for K in (1, 2, 4) for start in (1, 10 ** 6)]
CASES += [dict(n=4099, K=2, start=start, gscale=0.37, off=0, wd=0.0) for start in (1, 10 ** 6)]                 # the grad_scale path
CASES += [dict(n=n, K=2, start=1, gscale=1.0, off=off, wd=0.05) for n in (3, 4099) for off in (1, 3)]          # a weight-decay span off a 16-byte boundary
CASES += [dict(n=4099, K=4, start=10 ** 6, gscale=0.5, off=2, wd=0.05)]


@pytest.mark.parametrize("c", CASES, ids=lambda c: f"n{c['n']}-K{c['K']}-t{c['start']}-g{c['gscale']}-off{c['off']}-wd{c['wd']}")
def test_adamw_ema_tracks(ops, c):
    """Five consecutive steps.  p, m, v, ema: bitwise what ldmae_adamw_ema writes on (aligned, zero-padded to a multiple of 4) copies of the
    same inputs.  Tracks: per element within the derived bound of the f64 restatement from the same f32 parameters and the same f32-rounded c;
    from step 1 the slabs start as NaN (the kernel must not read them)."""
    n, K, start, off = c["n"], c["K"], c["start"], c["off"]
    rng = np.random.default_rng(1000 * n + 10 * K + (start > 1) + off)
    f = lambda s=1.0: (s * rng.standard_normal(n)).astype(np.float32)          # noqa: E731
    p0, ema0 = f(), f()
    m0, v0 = (np.zeros(n, np.float32), np.zeros(n, np.float32)) if start == 1 else (f(0.1), (f(0.1) ** 2).astype(np.float32))
    tr0 = [np.full(n, np.nan, np.float32) if start == 1 else (p0 + f(0.05)).astype(np.float32) for _ in range(K)]
    gammas = [ph.sigma_rel_to_gamma(s) for s in SIGMAS[:K]]
    bufs = {k: _guarded(a, off) for k, a in (("p", p0), ("m", m0), ("v", v0), ("ema", ema0))}
    tbufs = [_guarded(a, off) for a in tr0]
    ref = {k: torch.from_numpy(_pad4(a)).cuda() for k, a in (("p", p0), ("m", m0), ("v", v0), ("ema", ema0))}
    thetas, css, got_tracks = [], [], []
    for s in range(5):
        t = start + s
        g = f(0.1)
        gb, gv = _guarded(g, off)
        cs = [ph.track_coef(gm, t) for gm in gammas]
        ops.adamw_ema_tracks(bufs["p"][1], gv, bufs["m"][1], bufs["v"][1], bufs["ema"][1], [tb[1] for tb in tbufs], cs, t, HYP["lr"], HYP["beta1"],
                             HYP["beta2"], HYP["eps"], c["wd"], HYP["ema_decay"], c["gscale"])
        ops.adamw_ema(ref["p"], torch.from_numpy(_pad4(g)).cuda(), ref["m"], ref["v"], ref["ema"], t, HYP["lr"], HYP["beta1"], HYP["beta2"],
                      HYP["eps"], c["wd"], HYP["ema_decay"], c["gscale"])
        for k in ("p", "m", "v", "ema"):
            assert torch.equal(_bits(bufs[k][1]), _bits(ref[k][:n])), (k, s)
            assert _intact(bufs[k][0], off, n), (k, s)
        assert _intact(gb, off, n) and torch.equal(_bits(gv), _bits(torch.from_numpy(g)))
        thetas.append(bufs["p"][1].cpu().numpy().copy())
        css.append([pc.f32(x) for x in cs])
        got_tracks.append([tb[1].cpu().numpy().copy() for tb in tbufs])
        assert all(_intact(tb[0], off, n) for tb in tbufs)
    assert not np.array_equal(thetas[0], thetas[4])
    for k in range(K):
        refs, errs = pc.track_trajectory_ref(tr0[k], thetas, [cs[k] for cs in css])
        for s in range(5):
            _check(f"tracks[t0={start}]", got_tracks[s][k], refs[s], errs[s])
        if start == 1:
            assert np.array_equal(got_tracks[0][k], thetas[0])                 # e(1) = theta(1), exactly


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", [1, 2, 4])
def test_ema_tracks_only(ops, n, K):
    """The frozen tail's sibling: the same update with no optimizer.  Steps 1..3 from NaN slabs, then 1e6..1e6+2; p is left as it was.
    Slabs on a 16-byte boundary, all one element off it (a scalar head), and the tracks off it while p is on it (not congruent: the
    all-scalar path)."""
    rng = np.random.default_rng(77 * n + K)
    gammas = [ph.sigma_rel_to_gamma(s) for s in SIGMAS[:K]]
    for off, toff in ((0, 0), (1, 1), (0, 1)):
        tr0 = [np.full(n, np.nan, np.float32) for _ in range(K)]
        tbufs = [_guarded(a, toff) for a in tr0]
        thetas, css, got = [], [], []
        for t in (1, 2, 3, 10 ** 6, 10 ** 6 + 1, 10 ** 6 + 2):
            th = rng.standard_normal(n).astype(np.float32)
            pb, pv = _guarded(th, off)
            cs = [ph.track_coef(g, t) for g in gammas]
            ops.ema_tracks_only(pv, [tb[1] for tb in tbufs], cs)
            assert torch.equal(_bits(pb), _bits(_guarded(th, off)[0]))
            thetas.append(th)
            css.append([pc.f32(x) for x in cs])
            got.append([tb[1].cpu().numpy().copy() for tb in tbufs])
            assert all(_intact(tb[0], toff, n) for tb in tbufs)
        for k in range(K):
            refs, errs = pc.track_trajectory_ref(tr0[k], thetas, [cs[k] for cs in css])
            for s in range(6):
                _check("tracks_only", got[s][k], refs[s], errs[s])


def test_track_entries_refuse_bad_arguments(ops):
    p = torch.zeros(8, device="cuda")
    t = [torch.zeros(8, device="cuda") for _ in range(5)]
    with pytest.raises(RuntimeError, match="1..4"):
        ops.ema_tracks_only(p, t, [0.5] * 5)
    with pytest.raises(RuntimeError, match="1..4"):
        ops.ema_tracks_only(p, [], [])
    with pytest.raises(RuntimeError, match="track 1"):
        ops.ema_tracks_only(p, [t[0], torch.zeros(7, device="cuda")], [0.5, 0.5])
    with pytest.raises(RuntimeError, match="track 0"):
        ops.ema_tracks_only(p, [t[0].double()], [0.5])
    for bad in (0.0, 1.5, -0.1, float("nan")):
        with pytest.raises(RuntimeError, match="coefficient"):
            ops.ema_tracks_only(p, t[:1], [bad])
    with pytest.raises(RuntimeError, match="coefficient"):
        ops.adamw_ema_tracks(p, p.clone(), p.clone(), p.clone(), p.clone(), t[:2], [0.5, 0.0], 1, 1e-3, 0.9, 0.95, 1e-8, 0.0, 0.9999)
    with pytest.raises(RuntimeError, match="snapshot_accumulate acc"):
        ops.snapshot_accumulate(p, p, 1.0)
    with pytest.raises(RuntimeError, match="snapshot_accumulate x"):
        ops.snapshot_accumulate(p.double(), t[0][:7], 1.0)
    with pytest.raises(RuntimeError, match="not finite"):
        ops.snapshot_accumulate(p.double(), p, float("inf"))
    torch.cuda.synchronize()
    assert all(bool((x == 0).all()) for x in t) and bool((p == 0).all())


@pytest.mark.parametrize("n,off", [(n, 0) for n in NS] + [(4099, 1), (3, 1)])
@pytest.mark.parametrize("terms", [1, 2, 33])
def test_snapshot_combination(ops, n, off, terms):
    """acc += coef x in f64 over 1, 2 and 33 terms with coefficients of both signs up to 4 in magnitude, then the rounding to f32: one f64
    product and one f64 addition per term, one f32 rounding at the end (posthoc_check.combine_ref)."""
    rng = np.random.default_rng(31 * n + terms + off)
    xs = [rng.standard_normal(n).astype(np.float32) for _ in range(terms)]
    coefs = [float(x) for x in rng.uniform(-4.0, 4.0, terms)]
    coefs[0] = 4.0
    if terms > 1:
        coefs[1] = -4.0
    ab, acc = _guarded(np.zeros(n), off, torch.float64)
    for x, cf in zip(xs, coefs):
        xb, xv = _guarded(x, off)
        ops.snapshot_accumulate(acc, xv, cf)
        assert _intact(xb, off, n) and torch.equal(_bits(xv), _bits(torch.from_numpy(x)))
    ref, b64, b32 = pc.combine_ref(xs, coefs)
    _check("accumulate", acc.cpu().numpy(), ref, b64)
    ob, out = _guarded(np.zeros(n, np.float32), off)
    assert ops.snapshot_finish(acc, out) is out
    _check("finish", out.cpu().numpy(), ref, b32)
    assert _intact(ab, off, n) and _intact(ob, off, n)
    assert np.array_equal(out.cpu().numpy(), acc.cpu().numpy().astype(np.float32))           # the rounding itself: to nearest
    assert torch.equal(ops.snapshot_finish(acc), out)


class _Bare(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(n, generator=torch.Generator().manual_seed(3)))


def test_end_to_end_reconstruction_against_the_brute_force_average(ops, tmp_path, capsys):
    """AdamWEMA with tracks 0.05 / 0.10 on 4099 bare parameters, seeded random gradients, 256 steps, a snapshot every 8; sigma_rel 0.075 at
    step 256 through the command line; against sum_tau w_tau theta(tau) of the recorded parameters in f64.
    Per element: |got - brute| <= ||x . W - w_r||_2 ||theta_i(1..T)||_2 (Cauchy-Schwarz over tau; W: the weights the recursion really has
    with its f32-rounded coefficients) + sum_i |x_i| (track bound of snapshot i) + the combination bound."""
    from ldmae_amd.optim import AdamWEMA
    n, T, every = 4099, 256, 8
    m = _Bare(n).cuda()
    opt = AdamWEMA(m, lr=1e-2, posthoc_sigma_rels=(0.05, 0.10))
    snaps = str(tmp_path / "snaps")
    g = torch.Generator().manual_seed(11)
    thetas = []
    for t in range(1, T + 1):
        opt.zero_grad()
        m.w.grad.copy_(torch.randn(n, generator=g) + 0.3)
        opt.step()
        thetas.append(m.w.detach().cpu().numpy().copy())
        if t % every == 0:
            opt.write_snapshot(snaps, t)
    with pytest.raises(RuntimeError, match="tracks are at step 256"):
        opt.write_snapshot(snaps, 255)
    out = str(tmp_path / "ema_0075.pt")
    assert ph.main(["--snapshots", snaps, "--sigma_rel", "0.075", "--out", out]) == 0
    text = capsys.readouterr().out
    assert "condition number" in text and "relative L2 residual" in text and "coefficients" in text
    ck = torch.load(out, map_location="cpu")
    assert set(ck["ema"]) == {"w"} and ck["ema"]["w"].dtype == torch.float32
    got = ck["ema"]["w"].numpy().astype(np.float64)
    rep = ck["posthoc_ema"]
    assert rep["step"] == T and rep["snapshots"] == 64 and rep["residual_rel"] < 2e-3

    index = ph.read_index(snaps)
    assert index["steps"] == list(range(every, T + 1, every)) and index["layout"] == [["w", 0, [n]]] and index["numel"] == opt.flat.total
    entries, rep2 = ph.plan(index, 0.075)
    assert rep2 == rep
    th = np.stack(thetas).astype(np.float64)                                   # [T, n]
    w_r = ph.discrete_weights(T, ph.sigma_rel_to_gamma(0.075))
    brute = w_r @ th
    fit = np.zeros(T)
    arith = np.zeros(n)
    files, xs = [], []
    traj = []
    for k, gm in enumerate(opt.gammas):
        cs = [pc.f32(ph.track_coef(gm, t)) for t in range(1, T + 1)]
        traj.append((cs,) + pc.track_trajectory_ref(None, thetas, cs))
    for s, k, x in entries:
        cs, refs, errs = traj[k]
        fit[:s] += x * pc.actual_weights(cs[:s])
        arith += abs(x) * errs[s - 1]
        a = np.fromfile(os.path.join(snaps, ph.snapshot_file(s, k)), dtype=np.float32)
        assert a.size == opt.flat.total and (a[n:] == 0).all()                 # the slab's alignment padding stays zero
        _check("e2e snapshot files", a[:n], refs[s - 1], errs[s - 1])
        files.append(a[:n])
        xs.append(x)
    ref_c, _, b32 = pc.combine_ref(files, xs)
    _check("e2e combination", got, ref_c, b32)
    res = float(np.linalg.norm(fit - w_r))
    assert res / float(np.linalg.norm(w_r)) == pytest.approx(rep["residual_rel"], rel=1e-3)
    bound = res * np.linalg.norm(th, axis=0) + arith + b32
    print(f"end to end: max |got - brute| {np.abs(got - brute).max():.3e}, bound {bound.min():.3e} .. {bound.max():.3e}")
    _check("e2e against brute force", got, brute, bound)
    # the classic EMA and the parameters went through the tracks entry: compare with a second optimizer that keeps no tracks
    m2 = _Bare(n).cuda()
    opt2 = AdamWEMA(m2, lr=1e-2)
    g = torch.Generator().manual_seed(11)
    for t in range(1, 9):
        opt2.zero_grad()
        m2.w.grad.copy_(torch.randn(n, generator=g) + 0.3)
        opt2.step()
    assert np.array_equal(m2.w.detach().cpu().numpy(), thetas[7]) and opt2.tracks == []
    # track state round trip
    sd = {k: ([t.clone() for t in v] if k == "tracks" else v) for k, v in opt.track_state_dict().items()}
    opt3 = AdamWEMA(_Bare(n).cuda(), lr=1e-2, posthoc_sigma_rels=(0.05, 0.10))
    opt3.load_track_state(sd)
    assert opt3.track_step == T and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(opt3.tracks, opt.tracks))
    with pytest.raises(RuntimeError, match="sigma_rels"):
        AdamWEMA(_Bare(n).cuda(), posthoc_sigma_rels=(0.05, 0.2)).load_track_state(sd)
    with pytest.raises(RuntimeError, match="different set of parameters"):
        AdamWEMA(_Bare(n + 1).cuda(), posthoc_sigma_rels=(0.05, 0.10)).load_track_state(sd)
    other = AdamWEMA(_Bare(n + 1).cuda(), posthoc_sigma_rels=(0.05, 0.10))
    other.track_step = T + 8
    with pytest.raises(RuntimeError, match="mismatched layout"):
        other.write_snapshot(snaps)


# ----------------------------------------------------------------------------- the train driver
class _StepLoader:
    """Batch k is a function of k alone, and so are the random draws of the step that consumes it (torch.manual_seed just before the batch is
    handed over; torch's and numpy's global streams): a run that starts at batch `first` sees exactly what an uninterrupted run sees from there on."""

    def __init__(self, first, shape, num_classes, batch):
        self.first, self.shape, self.num_classes, self.batch = first, shape, num_classes, batch

    def __iter__(self):
        k = self.first
        while True:
            g = torch.Generator().manual_seed(9000 + k)
            x, y = torch.randn((self.batch,) + self.shape, generator=g), torch.randint(0, self.num_classes, (self.batch,), generator=g)
            torch.manual_seed(5000 + k)
            np.random.seed(5000 + k)             # the logit-normal timesteps come from numpy's global stream (transport.sample_logit_normal)
            k += 1
            yield x, y


def _tiny_cfg(out_dir, posthoc):
    cfg = copy.deepcopy(yaml.safe_load(open(os.path.join(ROOT, "ldmae_amd/configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml"))))
    cfg["data"].update(image_size=64, num_workers=0)
    cfg["train"].update(global_batch_size=8, output_dir=str(out_dir), exp_name="t", log_every=8, ckpt_every=8, max_steps=24)
    if posthoc:
        cfg["train"]["posthoc_ema"] = {"sigma_rels": [0.05, 0.10], "snapshot_every": 8}
    return cfg


def test_train_driver_snapshots_resume_and_reconstructed_checkpoint(ops, tmp_path, monkeypatch):
    import ldmae_amd.inference as inf
    import ldmae_amd.train_accum as t
    from ldmae_amd.models import lightningdit as L
    from ldmae_amd.tokenizer import models_mae
    monkeypatch.setitem(L.LightningDiT_models, "LightningDiT-B/1", lambda **kw: L.LightningDiT(depth=2, hidden_size=192, patch_size=1, num_heads=3, **kw))
    first = [0]
    monkeypatch.setattr(t, "make_loader", lambda cfg, per_gpu, rank, world, synthetic: (range(1 << 10), _StepLoader(first[0], (16, 8, 8), 1000, per_gpu)))

    def run(name, posthoc, **train):
        cfg = _tiny_cfg(tmp_path / name, posthoc)
        cfg["train"].update(train)
        torch.manual_seed(0)
        np.random.seed(0)
        model, opt = t.do_train(cfg, synthetic=True)
        return cfg, model, opt

    cfg, model, opt = run("a", True)
    ckd = tmp_path / "a" / "t" / "checkpoints"
    snaps = ckd / "ema_snapshots"                                               # the default directory
    index = ph.read_index(str(snaps))
    assert index["steps"] == [8, 16, 24] and index["sigma_rels"] == [0.05, 0.10] and index["numel"] == opt.flat.total
    shapes = {n: list(p.shape) for n, p in model.named_parameters()}
    assert [(n, o) for n, o, _ in index["layout"]] == [(n, o) for n, o, _ in opt.layout()] and all(shapes[n] == s for n, _, s in index["layout"])
    assert "pos_embed" in shapes and not dict(model.named_parameters())["pos_embed"].requires_grad       # the frozen tail is tracked too
    assert sorted(os.listdir(snaps)) == sorted([ph.INDEX] + [ph.snapshot_file(s, k) for s in (8, 16, 24) for k in (0, 1)])
    last = [np.fromfile(snaps / ph.snapshot_file(24, k), dtype=np.float32) for k in (0, 1)]
    assert all(np.array_equal(a, tr.cpu().numpy()) for a, tr in zip(last, opt.tracks)) and not np.array_equal(last[0], last[1])
    o, k = opt.flat.offsets["pos_embed"]
    assert np.array_equal(last[0][o:o + k], model.pos_embed.detach().cpu().numpy().reshape(-1))          # a constant parameter: its own average
    cka = torch.load(ckd / "0000024.pt", map_location="cpu")
    assert set(cka) == {"model", "ema", "opt", "config", "ema_tracks"} and cka["ema_tracks"]["step"] == 24
    assert cka["ema_tracks"]["sigma_rels"] == [0.05, 0.10] and len(cka["ema_tracks"]["tracks"]) == 2

    # resumed from the step-16 checkpoint: the step-24 snapshot is the uninterrupted run's, bit for bit
    os.makedirs(tmp_path / "c" / "t" / "checkpoints")
    shutil.copy(ckd / "0000016.pt", tmp_path / "c" / "t" / "checkpoints" / "0000016.pt")
    first[0] = 16
    _, _, optc = run("c", True, resume=True)
    assert optc.track_step == 24
    snc = tmp_path / "c" / "t" / "checkpoints" / "ema_snapshots"
    assert ph.read_index(str(snc))["steps"] == [24]
    for k in (0, 1):
        assert (snc / ph.snapshot_file(24, k)).read_bytes() == (snaps / ph.snapshot_file(24, k)).read_bytes()
    ckc = torch.load(tmp_path / "c" / "t" / "checkpoints" / "0000024.pt", map_location="cpu")
    assert all(torch.equal(_bits(ckc["model"][n]), _bits(cka["model"][n])) for n in cka["model"])
    # a checkpoint written without tracks cannot continue them
    first[0] = 0
    _, modelb, optb = run("b", False)
    ckb = torch.load(tmp_path / "b" / "t" / "checkpoints" / "0000024.pt", map_location="cpu")
    assert set(ckb) == {"model", "ema", "opt", "config"} and not (tmp_path / "b" / "t" / "checkpoints" / "ema_snapshots").exists()
    assert optb.tracks == [] and "posthoc_ema" not in ckb["config"]["train"]
    for part in ("model", "ema"):                                               # tracks on never perturbed training
        assert set(ckb[part]) == set(cka[part])
        assert all(torch.equal(_bits(ckb[part][n]), _bits(cka[part][n])) for n in cka[part]), part
    os.makedirs(tmp_path / "d" / "t" / "checkpoints")
    shutil.copy(tmp_path / "b" / "t" / "checkpoints" / "0000016.pt", tmp_path / "d" / "t" / "checkpoints" / "0000016.pt")
    with pytest.raises(RuntimeError, match="no 'ema_tracks' entry"):
        run("d", True, resume=True)

    # the reconstructed checkpoint: the reference's key set, loadable by the model builder and the sampler
    out = str(tmp_path / "0000024_ema0075.pt")
    assert ph.main(["--snapshots", str(snaps), "--sigma_rel", "0.075", "--out", out, "--base", str(ckd / "0000024.pt")]) == 0
    ckr = torch.load(out, map_location="cpu")
    assert set(ckr["ema"]) == set(cka["ema"]) == set(model.state_dict()) and set(ckr["model"]) == set(cka["model"]) and ckr["config"] == cka["config"]
    assert all(ckr["ema"][n].shape == cka["ema"][n].shape and torch.isfinite(ckr["ema"][n]).all() for n in cka["ema"])
    # a width between the two tracks: close to both of them, equal to neither
    o, k = opt.flat.offsets["blocks.0.attn.qkv.weight"]
    w = ckr["ema"]["blocks.0.attn.qkv.weight"].numpy().reshape(-1).astype(np.float64)
    assert all(0 < float(np.abs(w - last[j][o:o + k]).max()) < 1e-2 for j in (0, 1))
    mdl = t.build_model(ckr["config"])
    mdl.load_state_dict(ckr["ema"])
    scfg = copy.deepcopy(cfg)
    scfg["data"].update(data_path=str(tmp_path / "feat"), latent_multiplier=1.0)
    scfg["vae"]["weight_path"] = str(tmp_path / "vmae.pth")
    scfg["sample"].update(num_sampling_steps=2, per_proc_batch_size=4, fid_num=4)
    vae = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, kl_loss_weight=True, smooth_output=True, img_size=64)
    torch.save({"model": vae.state_dict()}, scfg["vae"]["weight_path"])
    os.makedirs(str(tmp_path / "feat_sample"))
    torch.save({"mean": torch.zeros(1, 16, 1, 1), "std": torch.ones(1, 16, 1, 1)}, tmp_path / "feat_sample" / "latents_stats.pt")
    folder = inf.do_sample(scfg, out, str(tmp_path / "png"))
    assert sorted(os.listdir(folder)) == [f"{i:06d}.png" for i in range(4)]
