"""ldmae_guidance_combine (csrc/guidance.hip) per element against the f64 restatement of tests/guidance_check.py within its derived bound, on
every rule, both input types and both access paths; the bitwise properties of the contract; and sample.guidance through the tiny model of
smoke() (input 8, 16 channels, hidden 192, depth 2, f32): the tie to forward_with_cfg, to the unguided sampler, the forward counts, SDE,
dopri5 and do_sample."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guidance_check as gc     # noqa: E402

pytestmark = pytest.mark.gpu

# B, C, H, W, k: the smallest vectorised case; pass-through channels; the scalar path (HW % 4 != 0); one sample past a 4096-element pass
# of the block, on the vector path and (4099: a last group of three) on the scalar one
SHAPES = [(2, 4, 4, 4, 4), (3, 16, 8, 8, 3), (3, 5, 3, 3, 2), (2, 1, 1, 4100, 1), (2, 1, 1, 4099, 1)]
RULES = ("cfg", "rescale", "apg")
PARAMS = dict(phi=0.7, eta=0.25, norm_threshold=2.0, momentum=-0.5)
SCALE = 4.0


def draw(B, C, H, W, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * C + H * W)
    p, q, x = (torch.randn(B, C, H, W, generator=g) for _ in range(3))
    q = p + 0.3 * q                                        # a guide that is near the main prediction, as in sampling
    t = torch.rand(B, generator=g) * 0.8 + 0.1
    return p.to(dtype).cuda(), q.to(dtype).cuda(), x.cuda(), t.cuda()


def npf(t):
    return t.detach().float().cpu().numpy()


def run(rule, p, q, x, t, k, mom=None, out=None, **over):
    from ldmae_amd import ops
    kw = dict(PARAMS, **over)
    return ops.guidance_combine(rule, p, q, SCALE, k=k, x=x, t=t, phi=kw["phi"], eta=kw["eta"], norm_threshold=kw["norm_threshold"],
                                momentum=kw["momentum"] if mom is not None else 0.0, mom=mom, out=out)


def check(name, rule, got, p, q, x, t, k, m_prev=None, got_m=None, **over):
    kw = dict(PARAMS, **over)
    beta = kw["momentum"] if m_prev is not None else 0.0
    args = dict(x=npf(x), t=npf(t), phi=kw["phi"], eta=kw["eta"], r=kw["norm_threshold"], beta=beta, m_prev=None if m_prev is None else npf(m_prev))
    ref = gc.guidance_ref(rule, npf(p), npf(q), SCALE, k, **args)
    bound = gc.guidance_bound(rule, npf(p), npf(q), SCALE, k, **args)
    bound, bound_m = bound if rule == "apg" else (bound, None)
    assert np.isfinite(bound).all()
    worst = gc.worst_ratio(npf(got).astype(np.float64), ref, bound)
    print(f"{name}: worst |got - f64| / bound = {worst:.3f}")
    assert got.dtype == torch.float32 and got.shape == p.shape
    assert worst <= 1.0, name
    assert torch.equal(got[:, k:], p[:, k:].float()), "the pass-through channels are pos, bit for bit"
    if got_m is not None:
        wm = gc.worst_ratio(npf(got_m).astype(np.float64), gc.apg_ref(npf(p), npf(q), args["x"], args["t"], SCALE, k, kw["eta"], kw["norm_threshold"],
                                                                      beta, args["m_prev"])[1], bound_m)
        print(f"{name}: momentum, worst ratio {wm:.3f}")
        assert wm <= 1.0, name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("rule", RULES)
def test_rules_against_f64(rule, shape, dtype):
    B, C, H, W, k = shape
    p, q, x, t = draw(B, C, H, W, dtype)
    got = run(rule, p, q, x, t, k)
    check(f"{rule} {shape} {dtype}", rule, got, p, q, x, t, k)
    # a threshold that does not bind and one that is off take the gamma = 1 branch
    if rule == "apg":
        for r in (0.0, 1e6):
            check(f"apg r={r} {shape}", rule, run(rule, p, q, x, t, k, norm_threshold=r), p, q, x, t, k, norm_threshold=r)


@pytest.mark.parametrize("rule", RULES)
def test_misaligned_views_take_the_scalar_path_and_give_the_same_bits(rule):
    B, C, H, W, k = 3, 16, 8, 8, 3
    p, q, x, t = draw(B, C, H, W)
    want = run(rule, p, q, x, t, k)

    def shifted(a):                                        # the same values, one element off a 16-byte boundary
        buf = torch.empty(a.numel() + 1, dtype=a.dtype, device=a.device)
        v = buf[1:].view(a.shape)
        v.copy_(a)
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        return v
    for which in ("pos", "neg", "x", "all"):
        a, b, c = (shifted(v) if which in (n, "all") else v for n, v in (("pos", p), ("neg", q), ("x", x)))
        if rule != "apg" and which == "x":
            continue
        got = run(rule, a, b, c, t, k)
        check(f"{rule} misaligned {which}", rule, got, p, q, x, t, k)
        assert torch.equal(got, want), "both access paths sum in one order"
    out = shifted(torch.empty_like(p))
    assert torch.equal(run(rule, p, q, x, t, k, out=out), want) and torch.equal(out, want)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("shape", [(3, 16, 8, 8, 3), (3, 5, 3, 3, 2)], ids=["vector", "scalar"])
def test_out_may_alias_pos(rule, shape):
    B, C, H, W, k = shape
    p, q, x, t = draw(B, C, H, W)
    want = run(rule, p, q, x, t, k)
    p2 = p.clone()
    got = run(rule, p2, q, x, t, k, out=p2)
    assert got is p2 and torch.equal(p2, want)


def test_a_permuted_view_is_copied_first():
    p, q, x, t = draw(2, 4, 4, 4)
    pv = p.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)            # the layout the DiT returns: values of p, other strides
    assert not pv.is_contiguous() and torch.equal(pv, p)
    assert torch.equal(run("apg", pv, q, x, t, 4), run("apg", p, q, x, t, 4))


@pytest.mark.parametrize("shape", [(3, 16, 8, 8, 3), (3, 5, 3, 3, 2)], ids=["vector", "scalar"])
def test_three_call_momentum_sequence(shape):
    B, C, H, W, k = shape
    mom = torch.zeros(B, k * H * W, device="cuda")
    for call in range(3):
        p, q, x, t = draw(B, C, H, W, seed=call)
        before = mom.clone()
        got = run("apg", p, q, x, t, k, mom=mom)
        check(f"apg momentum call {call} {shape}", "apg", got, p, q, x, t, k, m_prev=before, got_m=mom)
        d = (p[:, :k] - q[:, :k]).reshape(B, -1)
        if call == 0:
            assert torch.equal(mom, d), "the first evaluation of a trajectory: m_prev = 0, the stored direction is p - q"
        else:
            assert not torch.equal(mom, d)
    # momentum 0 with a buffer: the direction is stored, the previous one is not read
    junk = torch.full_like(mom, float("nan"))
    p, q, x, t = draw(B, C, H, W, seed=7)
    got = run("apg", p, q, x, t, k, mom=junk, momentum=0.0)
    assert torch.equal(got, run("apg", p, q, x, t, k)) and torch.equal(junk, (p[:, :k] - q[:, :k]).reshape(B, -1))


def test_degenerate_cases():
    B, C, H, W, k = 2, 4, 4, 4, 4
    p, q, x, _ = draw(B, C, H, W)
    t5 = torch.full((B,), 0.5, device="cuda")
    # u = 0 exactly: x = -(1 - t) p with t = 0.5 -> the projection is zero, g = fma(s - 1, d, p)
    got = run("apg", p, q, -0.5 * p, t5, k, eta=0.0, norm_threshold=0.0)
    assert torch.isfinite(got).all()
    check("apg u = 0", "apg", got, p, q, -0.5 * p, t5, k, eta=0.0, norm_threshold=0.0)
    d = p - q
    assert torch.equal(got, torch.addcmul(p.double(), d.double(), torch.tensor(SCALE - 1.0, dtype=torch.float64, device="cuda")).float())
    # t = 1: the denominator of gamma is zero -> gamma = 1, no division by 1 - t anywhere
    got = run("apg", p, q, x, torch.ones(B, device="cuda"), k)
    assert torch.isfinite(got).all()
    check("apg t = 1", "apg", got, p, q, x, torch.ones(B, device="cuda"), k)
    # std(g0) = 0: p and q constant per sample -> g = g0 = fma(s, p - q, q)
    pc, qc = torch.full_like(p, 2.0), torch.full_like(p, 0.5)
    got = run("rescale", pc, qc, x, t5, k)
    assert torch.equal(got, torch.full_like(p, 0.5 + SCALE * 1.5))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rule", RULES)
def test_p_equal_q_returns_p_bit_for_bit(rule, dtype):
    for B, C, H, W, k in SHAPES[:3]:
        p, _, x, t = draw(B, C, H, W, dtype)
        got = run(rule, p, p.clone(), x, t, k)
        assert torch.equal(got, p.float()), (rule, C, H, W)


@pytest.mark.parametrize("rule", RULES)
def test_row_independence_and_repeatability(rule):
    for B, C, H, W, k in ((3, 16, 8, 8, 3), (3, 5, 3, 3, 2), (3, 1, 1, 4100, 1)):
        p, q, x, t = draw(B, C, H, W)
        mom = torch.zeros(B, k * H * W, device="cuda").normal_(generator=None) if rule == "apg" else None
        keep = None if mom is None else mom.clone()
        whole = run(rule, p, q, x, t, k, mom=None if mom is None else mom)
        again = run(rule, p, q, x, t, k, mom=None if keep is None else keep.clone())
        assert torch.equal(whole, again), "two runs give the same bits"
        for b in range(B):
            mb = None if keep is None else keep[b:b + 1].clone()
            alone = run(rule, p[b:b + 1], q[b:b + 1], x[b:b + 1], t[b:b + 1], k, mom=mb)
            assert torch.equal(alone[0], whole[b]), (rule, b, "a sample alone or in a batch: same bits")
            if mb is not None:
                assert torch.equal(mb[0], mom[b])


# ----------------------------------------------------------------------------- through the tiny model of smoke(), f32
N_CLASSES = 10


def tiny_dit(seed=0):
    from ldmae_amd.models.lightningdit import LightningDiT
    torch.manual_seed(seed)
    m = LightningDiT(input_size=8, patch_size=1, in_channels=16, hidden_size=192, depth=2, num_heads=3, num_classes=N_CLASSES,
                     class_dropout_prob=0.5, use_qknorm=True, use_swiglu=True, use_rope=True, use_rmsnorm=True)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                                  # a zero-initialised final layer would make the velocity vanish
        for n, p in m.named_parameters():
            if "adaLN_modulation" in n or n.startswith("final_layer.linear"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    m = m.cuda().eval()
    m.set_precision(torch.float32)
    return m


@pytest.fixture(scope="module")
def model():
    return tiny_dit()


def counting(m):
    """m with its forward wrapped: m.batches lists the batch size of every call."""
    m.batches = []
    inner = type(m).forward

    def forward(x, t, y=None, **kw):
        m.batches.append(len(x))
        return inner(m, x, t, y, **kw)
    m.forward = forward
    return m


def euler(steps=4):
    from ldmae_amd.transport import Sampler, create_transport
    tr = create_transport("Linear", "velocity", None, None, None)
    fn = Sampler(tr).sample_ode(sampling_method="euler", num_steps=steps + 1, atol=1e-6, rtol=1e-3)
    assert len(fn.__self__.t) == steps + 1
    return fn


def latents(model, sample_fn, guidance=None, n=4, cfg_scale=1.0):
    from ldmae_amd.inference import sample_latents
    g = torch.Generator(device="cuda").manual_seed(5)
    return sample_latents(model, sample_fn, n, cfg_scale, 0.0, torch.device("cuda"), N_CLASSES, generator=g, guidance=guidance)


def test_cfg_on_three_channels_against_forward_with_cfg(model):
    """One evaluation.  p and q are the two halves of the model's own output on the doubled batch.  torch evaluates uncond + s (cond - uncond)
    with the difference, the product and the sum rounded one by one (or the last two fused): within 2 |s| u |p - q| + u |g| of the exact value;
    the kernel within the cfg bound of guidance_check.  Each is held to its own bound against the f64 value, so they differ by at most the sum."""
    from ldmae_amd.guidance import Guidance
    g = torch.Generator().manual_seed(3)
    n, s = 4, 4.0
    x = torch.randn(n, 16, 8, 8, generator=g).cuda()
    t = torch.full((n,), 0.4, device="cuda")
    y = torch.randint(0, N_CLASSES, (n,), generator=g).cuda()
    fn = Guidance(rule="cfg", source="null_class", channels=3, scale=s, num_classes=N_CLASSES).model_fn(model)
    with torch.no_grad():
        got = fn(x, t, y)
        x2, t2, y2 = torch.cat([x, x]), torch.cat([t, t]), torch.cat([y, torch.full_like(y, N_CLASSES)])
        old = model.forward_with_cfg(x2, t2, y2, s, True, 0.1)[:n]
        both = model.forward(x2, t2, y2)
    p, q = npf(both[:n]), npf(both[n:])
    ref = gc.cfg_ref(p, q, s, 3)
    b_kernel = gc.guidance_bound("cfg", p, q, s, 3)
    P, Q = p[:, :3].astype(np.float64), q[:, :3].astype(np.float64)
    b_torch = np.zeros_like(b_kernel)
    b_torch[:, :3] = gc.SLACK * (2 * s * gc.U * np.abs(P - Q) + gc.U * np.abs(ref[:, :3]))
    wk, wt = gc.worst_ratio(npf(got), ref, b_kernel), gc.worst_ratio(npf(old), ref, b_torch)
    wd = gc.worst_ratio(npf(got), npf(old).astype(np.float64), b_kernel + b_torch)
    print(f"cfg k=3 through the model: kernel {wk:.3f}, forward_with_cfg {wt:.3f} of their bounds; kernel against forward_with_cfg {wd:.3f}")
    assert wk <= 1.0 and wt <= 1.0 and wd <= 1.0
    assert np.abs(P - Q).max() > 1e-3, "the two halves must differ, or the test shows nothing"
    assert torch.equal(got[:, 3:], old[:, 3:]) and torch.equal(got[:, 3:], both[:n, 3:])
    assert fn.calls == [1, 0]


@pytest.mark.parametrize("rule", ["cfg", "apg"])
def test_autoguidance_by_the_model_itself_is_the_unguided_sampler(model, rule):
    from ldmae_amd.guidance import Guidance
    fn = Guidance(rule=rule, source="auto", guide_ckpt="self", scale=3.0, eta=0.0, norm_threshold=2.0, momentum=-0.5 if rule == "apg" else 0.0,
                  integrator=("ODE", "euler")).model_fn(model, model)
    want, yw = latents(model, euler())
    got, yg = latents(model, euler(), guidance=fn)
    assert torch.equal(yw, yg) and got.shape == (4, 16, 8, 8) and torch.isfinite(got).all()
    assert torch.equal(got, want), "p == q: every rule returns p, so the trajectory is the unguided one bit for bit"
    assert fn.calls == [4, 4]


def test_interval_and_forward_counts():
    from ldmae_amd.guidance import Guidance
    main, guide = counting(tiny_dit()), counting(tiny_dit(seed=7))
    want, _ = latents(main, euler())
    assert main.batches == [4] * 4
    # an interval that holds no grid point: the negative model never runs and the result is the unguided one
    main.batches.clear()
    off = Guidance(rule="apg", source="auto", guide_ckpt="g", scale=3.0, interval=[2.0, 3.0]).model_fn(main, guide)
    got, _ = latents(main, euler(), guidance=off)
    assert torch.equal(got, want) and guide.batches == [] and main.batches == [4] * 4 and off.calls == [4, 0]
    # inside: auto runs each model once per evaluation on the n samples
    main.batches.clear()
    on = Guidance(rule="apg", source="auto", guide_ckpt="g", scale=3.0).model_fn(main, guide)
    got, _ = latents(main, euler(), guidance=on)
    assert main.batches == [4] * 4 and guide.batches == [4] * 4 and on.calls == [4, 4]
    assert torch.isfinite(got).all() and not torch.equal(got, want)
    # null_class runs the main model once per evaluation on the doubled batch; a half-open interval guides only the steps inside it
    main.batches.clear()
    t = [float(v) for v in euler().__self__.t]
    part = Guidance(rule="cfg", source="null_class", scale=3.0, interval=[t[1], t[3]], num_classes=N_CLASSES).model_fn(main)
    got, _ = latents(main, euler(), guidance=part)
    assert main.batches == [4, 8, 8, 4] and part.calls == [4, 0] and torch.isfinite(got).all()
    # sample_latents resets the momentum and the counts for every batch
    latents(main, euler(), guidance=part)
    assert part.calls == [4, 0]


def test_sde_and_dopri5_with_apg(model):
    from ldmae_amd.guidance import Guidance
    from ldmae_amd.transport import Sampler, create_transport
    tr = create_transport("Linear", "velocity", None, None, None)
    g = Guidance(rule="apg", source="null_class", scale=3.0, eta=0.0, norm_threshold=2.5, momentum=0.0, num_classes=N_CLASSES)
    sde = Sampler(tr).sample_sde(sampling_method="Euler", diffusion_form="sigma", num_steps=4, seed=1, keep_trajectory=False)
    got, _ = latents(model, sde, guidance=g.model_fn(model))
    assert got.shape == (4, 16, 8, 8) and got.dtype == torch.float32 and torch.isfinite(got).all()
    plain, _ = latents(model, Sampler(tr).sample_sde(sampling_method="Euler", diffusion_form="sigma", num_steps=4, seed=1, keep_trajectory=False))
    assert not torch.equal(got, plain)
    dop = Sampler(tr).sample_ode(sampling_method="dopri5", num_steps=3, atol=1e-6, rtol=1e-3)
    fn = g.model_fn(model)
    got, _ = latents(model, dop, guidance=fn)
    o = dop.__self__
    print(f"dopri5 with apg: nfe {o.nfe}, accepted {o.accepted}, rejected {o.rejected}")
    assert got.shape == (4, 16, 8, 8) and torch.isfinite(got).all() and fn.calls == [o.nfe, 0]
    # the momentum under an integrator that evaluates more than once per step is refused when the object is built
    with pytest.raises(ValueError, match="once per step"):
        Guidance(rule="apg", momentum=-0.5, integrator=("ODE", "dopri5"))


# ----------------------------------------------------------------------------- through do_sample
def _tiny_cfg(tmp_path, guidance=None):
    cfg = copy.deepcopy(yaml.safe_load(open(os.path.join(ROOT, "ldmae_amd/configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml"))))
    cfg["data"].update(image_size=64, num_workers=0, data_path=str(tmp_path / "feat"), latent_multiplier=1.0)
    cfg["train"].update(global_batch_size=8, output_dir=str(tmp_path), exp_name="t")
    cfg["vae"]["weight_path"] = str(tmp_path / "vmae.pth")
    cfg["sample"].update(sampling_method="euler", num_sampling_steps=3, per_proc_batch_size=4, fid_num=4, cfg_scale=4.0)
    if guidance:
        cfg["sample"]["guidance"] = guidance
    return cfg


def test_do_sample_writes_into_the_suffixed_folder(tmp_path, monkeypatch, capsys):
    from PIL import Image
    import ldmae_amd.inference as inf
    import ldmae_amd.train_accum as ta
    from ldmae_amd.models import lightningdit as L
    from ldmae_amd.tokenizer import models_mae
    monkeypatch.setitem(L.LightningDiT_models, "LightningDiT-B/1", lambda **kw: L.LightningDiT(depth=2, hidden_size=192, patch_size=1, num_heads=3, **kw))
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    for name in ("ckpt.pt", "early.pt"):
        dit = ta.build_model(_tiny_cfg(tmp_path))
        with torch.no_grad():
            for n, p in dit.named_parameters():
                if "adaLN_modulation" in n or n.startswith("final_layer.linear"):
                    p.copy_(torch.randn(p.shape, generator=g) * 0.02)
        torch.save({"ema": dit.state_dict(), "model": dit.state_dict()}, tmp_path / name)
    vae = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, kl_loss_weight=True, smooth_output=True, img_size=64)
    torch.save({"model": vae.state_dict()}, tmp_path / "vmae.pth")
    os.makedirs(str(tmp_path / "feat_sample"))
    torch.save({"mean": torch.randn(1, 16, 1, 1, generator=g) * 0.1, "std": torch.rand(1, 16, 1, 1, generator=g) + 0.5},
               tmp_path / "feat_sample" / "latents_stats.pt")
    cfg = _tiny_cfg(tmp_path, dict(rule="apg", source="auto", guide_ckpt=str(tmp_path / "early.pt"), scale=2.0, norm_threshold=2.5, momentum=-0.5))
    out = inf.do_sample(cfg, str(tmp_path / "ckpt.pt"))
    plain = "lightningdit-b-1-ckpt-ckpt-euler-3-interval0.10-cfg4.00-shift0.30"
    assert os.path.basename(out) == plain + "-guide-apg-auto-kall-s2.0-t0.1toinf-eta0.0-r2.5-mom-0.5-by-lightningdit-b-1-early-ema"
    assert os.path.dirname(out) == str(tmp_path / "t")
    files = sorted(os.listdir(out))
    assert files == [f"{i:06d}.png" for i in range(4)]
    ims = [np.asarray(Image.open(os.path.join(out, f))) for f in files]
    assert all(im.shape == (64, 64, 3) and im.dtype == np.uint8 and im.std() > 0 for im in ims) and len({im.tobytes() for im in ims}) == 4
    assert capsys.readouterr().out.count(inf.GUIDANCE_NOTICE) == 1
    # without the key: the folder of before, and no notice
    out0 = inf.do_sample(_tiny_cfg(tmp_path), str(tmp_path / "ckpt.pt"))
    assert os.path.basename(out0) == plain and inf.GUIDANCE_NOTICE not in capsys.readouterr().out
