"""The adaptive dopri5 ODE sampler on the GPU: every kernel of csrc/ode.hip per element against f64 on the same f32 inputs, the solver end to
end on two problems with closed forms (it must take exactly the steps of the f64 restatement of tests/test_ode_dopri5_cpu.py), then through a
tiny LightningDiT with classifier-free guidance and through do_sample.

Bounds.  u = 2^-24.  A stage out = fma(h, acc, y), acc = c_0 k_0 then m - 1 fmas, rounds m + 1 times, each rounding relative to a partial
result that is at most |y| + |h| sum |c_j k_j|: (m + 2) u (|y| + |h| sum |c_j k_j|).  The interpolant: x carries two roundings, its powers up
to 8 + 3, a coefficient 6, the product and the four additions 5: 24 u times the polynomial of absolute values.  The error ratio: the
propagated error of every quotient (err: 8 u |h| sum |e_j k_j|; tolerance: rtol * the bound of y1 + 2 u tol; quotient and square: one u each)
plus tests/gemm_check.py's blocked-sum bound acc_bound(S, K) with K the longest chain of additions of the documented fold (16 per thread, 6 + 2
per block, then ceil(blocks / 256) + 6 + 2 in the fold kernel), and one u each for the division by n and the square root.

The end-to-end trajectories are compared with the restatement within 4x the drift of the restatement run in f32 against itself in f64
(measured on the CPU: sin 2.2e-6 / 7.3e-6, lin 3.2e-6 / 4.8e-6 of max|x| for rtol 1e-3 / 1e-5; test_ode_dopri5_cpu.F32_DRIFT)."""
import copy
import math
import os

import numpy as np
import pytest
import torch
import yaml

import gemm_check as gc
import test_ode_dopri5_cpu as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = gc.U
SIZES = [1, 3, 4, 257, 4099, 65536 + 5]


def _inputs(n, seed):
    from ldmae_amd import ops
    g = torch.Generator().manual_seed(seed)
    ld = ops.ode_slab_ld(n)
    k = torch.randn(7, ld, generator=g).cuda()
    y = torch.randn(n, generator=g).cuda()
    sc = torch.tensor([0.25, 0.5, 0.0, 0.0], dtype=torch.float32).cuda()        # t, h
    return ops, y, k, sc


def _f32(vals):
    return [float(np.float32(v)) for v in vals]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("m", [1, 2, 6, 7])
def test_rk_stage_per_element(n, m):
    from ldmae_amd.transport import integrators as I
    ops, y, k, sc = _inputs(n, 100 + m)
    coef = {1: I.DP_A[1], 2: I.DP_A[2], 6: I.DP_A[6], 7: I.DP_MID}[m]
    out = torch.full((n,), float("nan"), device="cuda")
    tvec = torch.zeros(5, device="cuda")
    ops.rk_stage(y, k, coef, sc[1:2], out, sc[0:1], I.DP_C[m - 1], tvec)
    c = _f32(coef)
    K, Y, h = k[:, :n].double().cpu(), y.double().cpu(), 0.5
    terms = torch.stack([c[j] * K[j] for j in range(m)])
    ref = Y + h * terms.sum(0)
    bound = (m + 2) * U * (Y.abs() + abs(h) * terms.abs().sum(0))
    worst = gc.check(f"rk_stage m={m} n={n}", out.cpu(), ref, bound)
    print(f"rk_stage m={m} n={n}: {worst:.3f} of the bound")
    t_ref = 0.25 + float(np.float32(I.DP_C[m - 1])) * h
    assert float((tvec.double().cpu() - t_ref).abs().max()) <= 2 * U * t_ref


def _finish_ref(y, k, n, h, atol, rtol):
    """f64 y1, ratio and their bounds from the f32 inputs the kernel reads."""
    from ldmae_amd import ops
    from ldmae_amd.transport import integrators as I
    K, Y = k[:, :n].double().cpu(), y.double().cpu()
    b, e = _f32(I.DP_B), _f32(I.DP_E)
    tb = torch.stack([b[j] * K[j] for j in (0, 2, 3, 4, 5)])
    y1 = Y + h * tb.sum(0)
    by1 = 8 * U * (Y.abs() + abs(h) * tb.abs().sum(0))
    te = torch.stack([e[j] * K[j] for j in (0, 2, 3, 4, 5, 6)])
    err, berr = h * te.sum(0), 8 * U * abs(h) * te.abs().sum(0)
    tol = atol + rtol * torch.maximum(Y.abs(), y1.abs())
    q = err / tol
    bq = berr / tol + q.abs() * (rtol * by1 + 2 * U * tol) / tol + U * q.abs()
    bq2 = 2 * q.abs() * bq + bq * bq + U * q * q
    S = float((q * q).sum())
    depth = 16 + 8 + -(-ops.ode_partials(n) // 256) + 8
    bS = float(bq2.sum()) + float(gc.acc_bound(torch.tensor(S), depth))
    ratio = math.sqrt(S / n)
    bratio = bS / (2 * math.sqrt(S * n)) + 2 * U * ratio
    return y1, by1, ratio, bratio


@pytest.mark.parametrize("n", SIZES)
def test_dopri5_finish_per_element_and_ratio(n):
    ops, y, k, sc = _inputs(n, 7)
    atol, rtol = 1e-3, 1e-2
    y1 = torch.full((n,), float("nan"), device="cuda")
    partial = torch.zeros(ops.ode_partials(n), device="cuda")
    ops.dopri5_finish(y, k, sc[1:2], atol, rtol, y1, partial, sc[2:3])
    ref, by1, ratio, bratio = _finish_ref(y, k, n, 0.5, float(np.float32(atol)), float(np.float32(rtol)))
    worst = gc.check(f"dopri5_finish y1 n={n}", y1.cpu(), ref, by1)
    got = float(sc[2])
    print(f"dopri5_finish n={n}: y1 {worst:.3f} of the bound; ratio {got:.7g} (f64 {ratio:.7g}), |diff| {abs(got - ratio) / bratio:.3f} of the bound")
    assert abs(got - ratio) <= bratio
    # the same launches again: the same bits
    y1b, pb, sb = torch.empty_like(y1), torch.zeros_like(partial), torch.zeros(1, device="cuda")
    ops.dopri5_finish(y, k, sc[1:2], atol, rtol, y1b, pb, sb)
    assert torch.equal(y1, y1b) and torch.equal(partial, pb) and torch.equal(sb, sc[2:3])
    # the last stage's output IS y1 (FSAL): the stage kernel with the tableau's last row gives the same bits
    from ldmae_amd.transport import integrators as I
    ys = torch.empty_like(y1)
    ops.rk_stage(y, k, I.DP_A[6], sc[1:2], ys)
    assert torch.equal(ys, y1)


@pytest.mark.parametrize("n", SIZES)
def test_rms_norm_scaled(n):
    ops, y, k, sc = _inputs(n, 9)
    atol, rtol = 1e-6, 1e-3
    partial = torch.zeros(ops.ode_partials(n), device="cuda")
    x = k[0, :n]
    for other in (None, y):
        ops.rms_norm_scaled(x, other, atol, rtol, partial, sc[3:4])
        X, Y = x.double().cpu(), (x if other is None else other).double().cpu()
        tol = float(np.float32(atol)) + float(np.float32(rtol)) * Y.abs()
        q = X / tol
        S = float((q * q).sum())
        depth = 16 + 8 + -(-ops.ode_partials(n) // 256) + 8
        bS = float((q * q * 7 * U).sum()) + float(gc.acc_bound(torch.tensor(S), depth))      # quotient: 2 u (tolerance) + u, squared, + u
        ref = math.sqrt(S / n)
        bound = bS / (2 * math.sqrt(S * n)) + 2 * U * ref
        got = float(sc[3])
        print(f"rms_norm_scaled n={n}: {got:.7g} (f64 {ref:.7g}), |diff| {abs(got - ref) / bound:.3f} of the bound")
        assert abs(got - ref) <= bound


@pytest.mark.parametrize("n", SIZES)
def test_dopri5_interp_per_element(n):
    ops, y0, k, sc = _inputs(n, 21)
    g = torch.Generator().manual_seed(22)
    y1, ym = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    t0, h = 0.25, 0.5
    A, Bv, M, F0, F1 = y0.double().cpu(), y1.double().cpu(), ym.double().cpu(), k[0, :n].double().cpu(), k[6, :n].double().cpu()
    qa, qa_abs = 2 * h * (F1 - F0) - 8 * (Bv + A) + 16 * M, 2 * h * (F1.abs() + F0.abs()) + 8 * (Bv.abs() + A.abs()) + 16 * M.abs()
    qb, qb_abs = h * (5 * F0 - 3 * F1) + 18 * A + 14 * Bv - 32 * M, h * (5 * F0.abs() + 3 * F1.abs()) + 18 * A.abs() + 14 * Bv.abs() + 32 * M.abs()
    qc, qc_abs = h * (F1 - 4 * F0) - 11 * A - 5 * Bv + 16 * M, h * (F1.abs() + 4 * F0.abs()) + 11 * A.abs() + 5 * Bv.abs() + 16 * M.abs()
    out = torch.empty(n, device="cuda")
    for t_eval in (0.25, 0.4, 0.6180339887, 0.75):
        te = float(np.float32(t_eval))
        ops.dopri5_interp(y0, y1, ym, k, sc[1:2], sc[0:1], te, out)
        x = (te - t0) / h
        ref = A + x * h * F0 + x ** 2 * qc + x ** 3 * qb + x ** 4 * qa
        bound = 24 * U * (A.abs() + x * h * F0.abs() + x ** 2 * qc_abs + x ** 3 * qb_abs + x ** 4 * qa_abs)
        worst = gc.check(f"dopri5_interp n={n} t={t_eval}", out.cpu(), ref, bound)
        print(f"dopri5_interp n={n} t={t_eval}: {worst:.3f} of the bound")
        if t_eval == 0.25:
            assert torch.equal(out, y0)                              # exactly the step's start
        if t_eval == 0.75:
            gc.check(f"dopri5_interp n={n} at t0 + h against y1", out.cpu(), Bv, bound)


def _advance_case(ratio, accept, factor_exact):
    from ldmae_amd import ops
    t, h = float(np.float32(0.3)), float(np.float32(0.1))
    st = torch.tensor([t, h, ratio], dtype=torch.float32).cuda()
    status = torch.full((6,), float("nan"), device="cuda")
    ops.dopri5_advance(st[2:3], st[1:2], st[0:1], status)
    r = float(np.float32(ratio))
    dfac = 1.0 if r < 1 else 0.2
    factor = 10.0 if r == 0 else min(10.0, max(0.9 / r ** 0.2, dfac))
    t_new = float(np.float32(t + h)) if accept else t
    got = status.tolist()
    assert got[0] == (1.0 if accept else 0.0) and got[1] == r and got[2] == t and got[3] == h and got[4] == t_new
    assert st[0].item() == t_new and st[1].item() == got[5]
    want = h * factor
    if factor_exact:                                                 # the clamp: one f32 product
        assert got[5] == float(np.float32(want))
    else:                                                            # powf (1 ulp), the quotient and the product (1/2 ulp each) and the f32 constants: 8 u
        assert abs(got[5] - want) <= 8 * U * want, (got[5], want)
    return got[5] / h


def test_advance_ratio_zero():
    assert _advance_case(0.0, True, True) == pytest.approx(10.0, rel=1e-6)


def test_advance_accepted_step_does_not_shrink():
    assert _advance_case(0.5, True, False) > 1.0                    # 0.9 / 0.5^(1/5) = 1.034


def test_advance_rejected_step_shrinks_and_keeps_t():
    assert 0.2 < _advance_case(4.0, False, False) < 1.0             # 0.9 / 4^(1/5) = 0.682


def test_advance_growth_is_capped():
    assert _advance_case(1e-12, True, True) == pytest.approx(10.0, rel=1e-6)


# ----------------------------------------------------------------------------- the solver end to end, drift in torch (not the DiT)
def _torch_drift(problem):
    if problem == "sin":
        return lambda x, t: -x + torch.sin(5 * t).view(-1, 1, 1, 1)
    a = torch.from_numpy(R.matrix_a()).cuda()
    return lambda x, t: torch.einsum("ij,bjhw->bihw", a, x)


@pytest.mark.parametrize("problem", list(R.PROBLEMS))
@pytest.mark.parametrize("rtol,atol", R.CASES)
def test_solver_takes_the_restatements_steps(problem, rtol, atol):
    from ldmae_amd.transport.integrators import ode
    want, st = R.restated(problem, rtol, atol)
    o = ode(lambda x, t, model, **kw: model(x, t), t0=0, t1=1, sampler_type="dopri5", num_steps=11, atol=atol, rtol=rtol, timestep_shift=0.3)
    assert [float(v) for v in o.t] == R.GRID
    x0 = torch.from_numpy(R.initial_state(problem)).cuda()
    traj = o.sample(x0, _torch_drift(problem))
    torch.cuda.synchronize()
    print(f"{problem} rtol {rtol:g}: nfe {o.nfe} accepted {o.accepted} rejected {o.rejected} (restatement {st['nfe']} {st['accepted']} {st['rejected']})")
    assert traj.shape == (11,) + R.SHAPE and traj.dtype == torch.float32 and torch.equal(traj[0], x0)
    assert (o.nfe, o.accepted, o.rejected) == (st["nfe"], st["accepted"], st["rejected"])
    got = traj.double().cpu().numpy()
    ex = R.exact(problem)
    e_exact = np.abs(got - ex).reshape(11, -1).max(1)
    e_rest = np.abs(got - want).reshape(11, -1).max(1)
    print(f"   against the closed form: {e_exact.max() / (rtol * np.abs(ex).max()):.3f} rtol max|x|; against the restatement: "
          f"{e_rest.max() / np.abs(want).max():.3e} max|x| (allowed {4 * R.F32_DRIFT[(problem, rtol)]:.1e})")
    assert (e_exact <= 10 * rtol * np.abs(ex).max()).all()
    assert (e_rest <= 4 * R.F32_DRIFT[(problem, rtol)] * np.abs(want).max()).all()
    if problem == "sin":
        assert o.rejected >= 1                                       # the rejection path ran


# ----------------------------------------------------------------------------- through the model
def _tiny_dit():
    from ldmae_amd.models.lightningdit import LightningDiT
    torch.manual_seed(0)
    m = LightningDiT(input_size=8, patch_size=1, in_channels=4, hidden_size=64, depth=2, num_heads=4, num_classes=10, use_qknorm=True,
                     use_swiglu=True, use_rope=True, use_rmsnorm=True)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                                            # a zero-initialised final layer would make the drift vanish
        for n, p in m.named_parameters():
            if "adaLN_modulation" in n or n.startswith("final_layer.linear"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return m.cuda().eval()


def test_sample_ode_dopri5_through_the_model_with_cfg():
    from ldmae_amd.transport import Sampler, create_transport
    m = _tiny_dit()
    tr = create_transport("Linear", "velocity", None, None, None)
    g = torch.Generator().manual_seed(2)
    z = torch.randn(2, 4, 8, 8, generator=g).cuda()
    x0 = torch.cat([z, z])
    y = torch.tensor([3, 7, 10, 10]).cuda()
    kw = dict(y=y, cfg_scale=2.0, cfg_interval=True, cfg_interval_start=0.1)
    fn = Sampler(tr).sample_ode(sampling_method="dopri5", atol=1e-6, rtol=1e-3, num_steps=9)
    with torch.no_grad():
        traj = fn(x0, m.forward_with_cfg, **kw)
        ref = Sampler(tr).sample_ode(sampling_method="euler", atol=1e-6, rtol=1e-3, num_steps=2001)(x0, m.forward_with_cfg, **kw)[-1]
    o = fn.__self__
    print(f"dopri5 through the DiT: nfe {o.nfe} accepted {o.accepted} rejected {o.rejected}; |x - euler2001| / max|x| = "
          f"{float((traj[-1] - ref).abs().max() / ref.abs().max()):.3e}")
    assert traj.shape == (9, 4, 4, 8, 8) and torch.isfinite(traj).all() and torch.equal(traj[0], x0)
    assert float((traj[-1] - ref).abs().max()) <= 20 * 1e-3 * float(ref.abs().max())
    assert o.nfe == 1 + 6 * (o.accepted + o.rejected) + o.nfe_initial


# ----------------------------------------------------------------------------- through do_sample
def _tiny_cfg(tmp_path, method):
    cfg = copy.deepcopy(yaml.safe_load(open(os.path.join(ROOT, "ldmae_amd/configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml"))))
    cfg["data"].update(image_size=64, num_workers=0, data_path=str(tmp_path / "feat"), latent_multiplier=1.0)
    cfg["train"].update(global_batch_size=8, output_dir=str(tmp_path), exp_name="t")
    cfg["vae"]["weight_path"] = str(tmp_path / "vmae.pth")
    cfg["sample"].update(sampling_method=method, num_sampling_steps=3, per_proc_batch_size=4, fid_num=4, cfg_scale=4.0)
    return cfg


def _fixtures(tmp_path, monkeypatch):
    import ldmae_amd.train_accum as t
    from ldmae_amd.models import lightningdit as L
    from ldmae_amd.tokenizer import models_mae
    monkeypatch.setitem(L.LightningDiT_models, "LightningDiT-B/1", lambda **kw: L.LightningDiT(depth=2, hidden_size=192, patch_size=1, num_heads=3, **kw))
    torch.manual_seed(0)
    dit = t.build_model(_tiny_cfg(tmp_path, "euler"))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, p in dit.named_parameters():
            if "adaLN_modulation" in n or n.startswith("final_layer.linear"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    torch.save({"ema": dit.state_dict(), "model": dit.state_dict()}, tmp_path / "ckpt.pt")
    vae = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, kl_loss_weight=True, smooth_output=True, img_size=64)
    torch.save({"model": vae.state_dict()}, tmp_path / "vmae.pth")
    os.makedirs(str(tmp_path / "feat_sample"))
    torch.save({"mean": torch.randn(1, 16, 1, 1, generator=g) * 0.1, "std": torch.rand(1, 16, 1, 1, generator=g) + 0.5},
               tmp_path / "feat_sample" / "latents_stats.pt")


def _sample_as_before(self, x, model, **model_kwargs):
    """ode.sample as it stood before dopri5 was added (the fixed-step loop, verbatim)."""
    t = self.t.to(x.device)

    def f(tk, xk):
        return self.drift(xk, torch.ones(xk.size(0), device=xk.device) * tk, model, **model_kwargs)

    xs = [x]
    with torch.no_grad():
        for k in range(len(t) - 1):
            dt = t[k + 1] - t[k]
            if self.sampler_type == "euler":
                x = x + dt * f(t[k], x)
            elif self.sampler_type == "midpoint":
                x = x + dt * f(t[k] + dt / 2, x + dt / 2 * f(t[k], x))
            else:
                k1 = f(t[k], x)
                x = x + dt / 2 * (k1 + f(t[k + 1], x + dt * k1))
            xs.append(x)
    return torch.stack(xs)


def test_do_sample_with_dopri5_and_euler_unchanged(tmp_path, monkeypatch, capsys):
    from PIL import Image
    import ldmae_amd.inference as inf
    from ldmae_amd.transport import integrators
    _fixtures(tmp_path, monkeypatch)
    out = inf.do_sample(_tiny_cfg(tmp_path, "dopri5"), str(tmp_path / "ckpt.pt"))
    assert os.path.basename(out) == "lightningdit-b-1-ckpt-ckpt-dopri5-3-interval0.10-cfg4.00-shift0.30"
    files = sorted(os.listdir(out))
    assert files == [f"{i:06d}.png" for i in range(4)]
    ims = [np.asarray(Image.open(os.path.join(out, f))) for f in files]
    assert all(im.shape == (64, 64, 3) and im.dtype == np.uint8 and im.std() > 0 for im in ims) and len({im.tobytes() for im in ims}) == 4
    said = capsys.readouterr().out
    assert said.count("dopri5 (atol 1e-06, rtol 0.001): nfe ") == 1, said
    # euler: the PNG bytes of the fixed-step loop as it stood before this solver was added
    now = inf.do_sample(_tiny_cfg(tmp_path, "euler"), str(tmp_path / "ckpt.pt"))
    assert "euler-3" in os.path.basename(now) and "dopri5" not in capsys.readouterr().out
    monkeypatch.setattr(integrators.ode, "sample", _sample_as_before)
    before = inf.do_sample(_tiny_cfg(tmp_path, "euler"), str(tmp_path / "ckpt.pt"), out_dir=str(tmp_path / "before"))
    for f in files:
        assert open(os.path.join(now, f), "rb").read() == open(os.path.join(before, f), "rb").read(), f
