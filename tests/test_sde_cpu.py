"""The SDE sampler, host side: the f64 restatement of the Philox normal draw (known answers, stream independence, moments), the host coefficient
functions against the reference's recorded compute_diffusion / get_score_from_velocity values (tests/golden/sde.npz), the grids, the interface of
Sampler.sample_sde with every refusal, the C ABI, and the YAML / command-line handling of the sampling driver."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "ldmae_amd/configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml")
FORMS = ("constant", "SBDM", "sigma", "linear", "decreasing", "inccreasing-decreasing")

# philox4x32-10 of the Random123 distribution's kat_vectors: (counter 0, key 0) -> these four words (tests/test_likelihood_cpu.py holds all three)
KAT0 = (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
KAT2 = ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "sde.npz"))


def _from_words(words):
    u = [((w >> 9) + 0.5) * 2.0 ** -23 for w in words]
    r0, r1 = math.sqrt(-2 * math.log(u[0])), math.sqrt(-2 * math.log(u[2]))
    return [r0 * math.cos(2 * math.pi * u[1]), r0 * math.sin(2 * math.pi * u[1]), r1 * math.cos(2 * math.pi * u[3]), r1 * math.sin(2 * math.pi * u[3])]


def test_normal_first_block_is_box_muller_on_the_known_answer_words():
    from ldmae_amd.transport import probe
    z = probe.normal(7, 0, 0)
    assert z.dtype == np.float64 and z.shape == (7,)
    np.testing.assert_allclose(z[:4], _from_words(KAT0), rtol=1e-14, atol=1e-15)
    # a 64-bit seed, a counter with a non-zero high word, a block index past 2^32: the third vector, through the same word layout as rademacher
    ctr, key, want = KAT2
    words = probe.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
    assert tuple(int(w) for w in words) == want
    # every u is strictly inside (0, 1) and exact in f32: an odd multiple of 2^-24
    for w in (0, 0xffffffff, 0x1ff, 0x200):
        u = ((w >> 9) + 0.5) * 2.0 ** -23
        assert 0 < u < 1 and float(np.float32(u)) == u
    assert math.sqrt(-2 * math.log(2.0 ** -24)) == pytest.approx(math.sqrt(48 * math.log(2))) and math.sqrt(48 * math.log(2)) < 5.77


def test_normal_prefix_does_not_depend_on_n():
    from ldmae_amd.transport import probe
    a = probe.normal(4100, 3, 5)
    for n in (1, 3, 4, 5, 7, 4099):
        assert np.array_equal(a[:n], probe.normal(n, 3, 5)), n
    assert not np.array_equal(a, probe.normal(4100, 3, 6)) and not np.array_equal(a, probe.normal(4100, 4, 5))


@pytest.fixture(scope="module")
def draws():
    from ldmae_amd.transport import probe
    n = 2 ** 20
    return {sc: probe.normal(n, *sc) for sc in ((0, 0), (3, 5), (2 ** 63 + 11, 249), (3, 6))}


@pytest.mark.parametrize("sc", [(0, 0), (3, 5), (2 ** 63 + 11, 249)])
def test_normal_moments_within_five_standard_errors(draws, sc):
    z = draws[sc]
    n = z.size
    mean, var = float(z.mean()), float(z.var())
    kurt = float(((z - mean) ** 4).mean() / var ** 2)
    lag1 = float((z[:-1] * z[1:]).mean())
    print(f"seed, counter {sc}: mean {mean * math.sqrt(n):+.2f} se, variance {(var - 1) / math.sqrt(2 / n):+.2f} se, "
          f"kurtosis {(kurt - 3) / math.sqrt(96 / n):+.2f} se, lag-1 {lag1 * math.sqrt(n):+.2f} se, max |z| {np.abs(z).max():.3f}")
    assert abs(mean) < 5 / math.sqrt(n)
    assert abs(var - 1) < 5 * math.sqrt(2 / n)
    assert abs(kurt - 3) < 5 * math.sqrt(96 / n)
    assert abs(lag1) < 5 / math.sqrt(n)                               # var(z_i z_{i+1}) = 1 for independent standard normals
    assert float(np.abs(z).max()) <= math.sqrt(48 * math.log(2))


def test_normal_draws_of_two_counters_are_uncorrelated(draws):
    a, b = draws[(3, 5)], draws[(3, 6)]
    assert abs(float((a * b).mean())) < 5 / math.sqrt(a.size)


def test_diffusion_and_score_coefficients_against_the_reference_values(gold):
    from ldmae_amd.transport import path
    from ldmae_amd.transport.integrators import sde_drift_terms
    norm = float(gold["norm"])
    for form in FORMS:
        for row, key in ((0, "t_"), (1, "t2_")):
            for k, t in enumerate(gold[key + form]):
                t = float(t)                                      # the f32 grid value, exactly
                w_ref, (a_ref, b_ref) = float(gold["w_" + form][row, k]), gold["score_" + form][row, :, k]
                w = path.diffusion(t, form, norm)
                assert w == pytest.approx(w_ref, rel=1e-13, abs=1e-15), (form, t)
                a, b = path.score_from_velocity(t)
                assert a == pytest.approx(float(a_ref), rel=1e-13, abs=1e-15) and b == pytest.approx(float(b_ref), rel=1e-13), (form, t)
                al, be = sde_drift_terms(t, w)                    # drift = v + w score = (1 + w a) v + (w b) x = beta v - alpha x
                assert be == pytest.approx(1 + w_ref * float(a_ref), rel=1e-13) and al == pytest.approx(-w_ref * float(b_ref), rel=1e-13, abs=1e-15)
    assert path.diffusion(0.0, "SBDM") == math.inf
    with pytest.raises(NotImplementedError, match="Diffusion form cubic not implemented"):
        path.diffusion(0.5, "cubic")
    with pytest.raises(ValueError, match="singular at t = 1"):
        path.score_from_velocity(1.0)


def _transport(eps=1e-3):
    from ldmae_amd.transport import ModelType, PathType, Transport, WeightType
    return Transport(model_type=ModelType.VELOCITY, path_type=PathType.LINEAR, loss_type=WeightType.NONE, train_eps=eps, sample_eps=eps)


@pytest.mark.parametrize("form", FORMS)
def test_grid_and_step_coefficients(gold, form):
    """linspace(t0, t1, 6) in f32 with the reference's interval rule, and the step plan: every coefficient is the f64 formula on the reference's own
    w / score values, rounded once to f32."""
    from ldmae_amd.transport import Sampler
    tr, norm, s = _transport(), float(gold["norm"]), float(gold["last_step_size"])
    for last in (None, "Mean"):
        t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps, diffusion_form=form, sde=True, eval=True, last_step_size=0.0 if last is None else s)
        assert t0 == (1e-3 if form == "SBDM" else 0) and t1 == (1 - 1e-3 if last is None else 1 - s)
        for method in ("Euler", "Heun"):
            fn = Sampler(tr).sample_sde(sampling_method=method, diffusion_form=form, diffusion_norm=norm, last_step=last, last_step_size=s, num_steps=6)
            assert fn.sde.t.dtype == torch.float32 and np.array_equal(fn.sde.t.numpy(), gold[f"{method}/{form}/{last}/t"])
            assert float(fn.sde.dt) == float(fn.sde.t[1] - fn.sde.t[0]) and len(fn.sde.plan) == 5
    # coefficients on the grid that ends at 1 - s: the one the w_ / score_ arrays were recorded on
    r1 = lambda v: float(np.float32(v))      # noqa: E731
    w, sc, t, t2 = gold["w_" + form], gold["score_" + form], gold["t_" + form], gold["t2_" + form]
    for method in ("Euler", "Heun"):
        fn = Sampler(tr).sample_sde(sampling_method=method, diffusion_form=form, diffusion_norm=norm, last_step="Mean", last_step_size=s, num_steps=6)
        dt = float(fn.sde.dt)
        for k, c in enumerate(fn.sde.plan):
            al, be = -w[0, k] * sc[0, 1, k], 1 + w[0, k] * sc[0, 0, k]
            assert c["t"] == float(t[k]) and c["t_next"] == float(t[k + 1])
            assert c["cz"] == pytest.approx(r1(math.sqrt(2 * w[0, k] * dt)), rel=2.0 ** -23, abs=1e-30)
            if method == "Euler":
                want = dict(cx=1 - dt * al, cv=dt * be)
            else:
                al2, be2 = -w[1, k] * sc[1, 1, k], 1 + w[1, k] * sc[1, 0, k]
                assert c["t2"] == float(t2[k])
                want = dict(px=1 - dt * al, pv=dt * be, cx=1 - dt / 2 * al, cv1=dt / 2 * be, cxp=-dt / 2 * al2, cv2=dt / 2 * be2)
            for name, v in want.items():
                assert c[name] == float(np.float32(c[name])) and abs(c[name] - v) <= 2.0 ** -24 * abs(v) * (1 + 1e-6) + 1e-13 * (1 + abs(dt * al)), (name, k)
        tl = float(t[-1])
        alL, beL = -w[0, -1] * sc[0, 1, -1], 1 + w[0, -1] * sc[0, 0, -1]
        assert fn.last_coefficients == pytest.approx((r1(1 - s * alL), r1(s * beL)), rel=2.0 ** -23)
        tw = Sampler(tr).sample_sde(sampling_method=method, diffusion_form=form, last_step="Tweedie", last_step_size=s, num_steps=6).last_coefficients
        assert tw == pytest.approx((r1(1 / tl + (1 - tl) ** 2 / tl * sc[0, 1, -1]), r1((1 - tl) ** 2 / tl * sc[0, 0, -1])), rel=2.0 ** -23)
        eu = Sampler(tr).sample_sde(sampling_method=method, diffusion_form=form, last_step="Euler", last_step_size=s, num_steps=6)
        assert eu.last_coefficients == (1.0, r1(s)) and eu.model_calls == (5 if method == "Euler" else 10) + 1
        no = Sampler(tr).sample_sde(sampling_method=method, diffusion_form=form, last_step=None, num_steps=6)
        assert no.last_coefficients is None and no.model_calls == (5 if method == "Euler" else 10)


def test_check_interval_without_sde_is_unchanged():
    from ldmae_amd.transport import create_transport
    for tr in (create_transport(), _transport()):
        assert tr.check_interval(tr.train_eps, tr.sample_eps) == (0, 1)
        assert tr.check_interval(tr.train_eps, tr.sample_eps, sde=False, eval=True, reverse=False, last_step_size=0.0) == (0, 1)
        assert tr.check_interval(tr.train_eps, tr.sample_eps, sde=False, eval=True, reverse=True, last_step_size=0.04, diffusion_form="sigma") == (1, 0)
    tr = _transport(0.01)
    assert tr.check_interval(0.02, 0.01, diffusion_form="SBDM", sde=True, eval=True, last_step_size=0.04) == (0.01, 1 - 0.04)
    assert tr.check_interval(0.02, 0.01, diffusion_form="SBDM", sde=True, eval=False, last_step_size=0.0) == (0.02, 1 - 0.02)
    assert tr.check_interval(0.02, 0.01, diffusion_form="sigma", sde=True, eval=True, last_step_size=0.0) == (0, 1 - 0.01)
    assert tr.check_interval(0.02, 0.01, diffusion_form="sigma", sde=True, eval=True, reverse=True, last_step_size=0.25) == (1, 0.25)


def test_sample_sde_signature_defaults_and_refusals():
    from ldmae_amd.transport import Sampler, create_transport
    from ldmae_amd.transport.integrators import sde
    s = Sampler(create_transport())
    p = inspect.signature(s.sample_sde).parameters
    assert [(n, v.default) for n, v in p.items()] == [("sampling_method", "Euler"), ("diffusion_form", "SBDM"), ("diffusion_norm", 1.0),
                                                      ("last_step", "Mean"), ("last_step_size", 0.04), ("num_steps", 250), ("seed", 0),
                                                      ("noise", None), ("keep_trajectory", True)]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for v in p.values())
    # the no-argument call is the singular case: SBDM from t0 = 0 (create_transport forces sample_eps = 0); refused at construction, with advice
    with pytest.raises(NotImplementedError, match="SDE sampling is out of scope") as e:
        s.sample_sde()
    assert "diffusion_form='SBDM'" in str(e.value) and "sample_eps > 0" in str(e.value) and "another diffusion_form" in str(e.value)
    with pytest.raises(NotImplementedError, match="SDE sampling is out of scope"):
        s.sample_sde(diffusion_form="SBDM", sampling_method="Heun", last_step=None)
    with pytest.raises(NotImplementedError, match="diffusion_form 'cubic' is not supported"):
        s.sample_sde(diffusion_form="cubic")
    with pytest.raises(NotImplementedError, match="last_step 'Median' is not supported"):
        s.sample_sde(diffusion_form="sigma", last_step="Median")
    for bad in ("euler", "dopri5", "Midpoint"):
        with pytest.raises(NotImplementedError, match=f"sampling_method '{bad}' is not supported"):
            s.sample_sde(diffusion_form="sigma", sampling_method=bad)
    with pytest.raises(NotImplementedError, match="Euler / Heun only"):
        sde(None, lambda t: 1.0, t0=0, t1=0.96, num_steps=6, sampler_type="Milstein")
    # Heun evaluates the drift at t1; with last_step None on a sample_eps = 0 transport t1 = 1, where the score is singular
    with pytest.raises(ValueError, match="singular at t = 1"):
        s.sample_sde(diffusion_form="sigma", sampling_method="Heun", last_step=None, num_steps=6)
    fn = s.sample_sde(diffusion_form="sigma", num_steps=6)
    assert fn.calls == 0 and fn.sde.sampler_type == "Euler" and len(fn.sde.t) == 6 and float(fn.sde.t[0]) == 0 and float(fn.sde.t[-1]) == np.float32(0.96)
    assert fn.options == dict(sampling_method="Euler", diffusion_form="sigma", diffusion_norm=1.0, last_step="Mean", last_step_size=0.04, num_steps=6,
                              seed=0, keep_trajectory=True)
    with pytest.raises(RuntimeError, match="HIP device"):              # no CPU fallback
        fn(torch.zeros(2, 4, 2, 2), lambda x, t: x)
    assert fn.calls == 0
    fn.calls = 7
    assert fn.calls == 7
    # SBDM is served once the transport starts the grid at eps > 0
    ok = Sampler(_transport(1e-3)).sample_sde(num_steps=6)
    assert float(ok.sde.t[0]) == np.float32(1e-3) and ok.options["diffusion_form"] == "SBDM"


def test_abi_declares_and_binds_the_sde_entry_points():
    from ldmae_amd import _lib
    header = open(os.path.join(ROOT, "include", "ldmae_hip.h")).read()
    for name, nargs in (("ldmae_normal_f32", 5), ("ldmae_sde_combine_f32", 18)):
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\);", header)
        assert m, name + " is not declared in include/ldmae_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1 == nargs, name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
    from ldmae_amd import ops
    assert callable(ops.normal) and callable(ops.sde_combine)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.normal((4,), 0, 0, "cpu")


def _cfg(**sample):
    cfg = yaml.safe_load(open(CFG))
    cfg["sample"].update(sample)
    return cfg


def test_driver_builds_the_sde_sampler_from_the_yaml(monkeypatch):
    from ldmae_amd import inference
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cfg = _cfg(mode="SDE")
    fn = inference.build_sampler(cfg)
    assert fn.options == dict(sampling_method="Euler", diffusion_form="sigma", diffusion_norm=1.0, last_step="Mean", last_step_size=0.04,
                              num_steps=250, seed=cfg["train"]["global_seed"], keep_trajectory=False)
    assert fn.model_calls == 250 and float(fn.sde.t[0]) == 0
    monkeypatch.setenv("RANK", "3")
    monkeypatch.setenv("WORLD_SIZE", "8")
    fn = inference.build_sampler(_cfg(mode="SDE", sampling_method="HEUN", num_sampling_steps=20, diffusion_form="linear", diffusion_norm=0.5,
                                      last_step="Tweedie", last_step_size=0.02))
    assert fn.options == dict(sampling_method="Heun", diffusion_form="linear", diffusion_norm=0.5, last_step="Tweedie", last_step_size=0.02,
                              num_steps=20, seed=cfg["train"]["global_seed"] * 8 + 3, keep_trajectory=False)
    assert fn.model_calls == 2 * 19 + 1
    assert inference.build_sampler(_cfg(mode="SDE", last_step="None")).options["last_step"] is None
    assert inference.build_sampler(_cfg(mode="SDE", last_step=None)).options["last_step"] is None
    with pytest.raises(NotImplementedError, match="sampling_method 'dopri5' is not supported"):
        inference.build_sampler(_cfg(mode="SDE", sampling_method="dopri5"))
    with pytest.raises(NotImplementedError, match="Sampling mode Langevin is not supported"):
        inference.build_sampler(_cfg(mode="Langevin"))
    # SBDM: the grid starts at transport.sample_eps; the shipped YAML has null there
    with pytest.raises(NotImplementedError, match="SDE sampling is out of scope") as e:
        inference.build_sampler(_cfg(mode="SDE", diffusion_form="SBDM"))
    assert "transport.sample_eps" in str(e.value)
    cfg = _cfg(mode="SDE", diffusion_form="SBDM")
    cfg["transport"]["sample_eps"] = 0
    with pytest.raises(NotImplementedError, match="SDE sampling is out of scope"):
        inference.build_sampler(cfg)
    cfg["transport"]["sample_eps"] = 0.001
    fn = inference.build_sampler(cfg)
    assert float(fn.sde.t[0]) == np.float32(0.001) and fn.options["diffusion_form"] == "SBDM"
    # the ODE path: the bound method of the ode integrator, as before
    ode_fn = inference.build_sampler(_cfg())
    assert ode_fn.__self__.sampler_type == "euler" and len(ode_fn.__self__.t) == 250 and not hasattr(ode_fn, "model_calls")


def test_driver_flag_and_folder_names():
    from ldmae_amd import inference
    ap = inference.build_parser()
    assert ap.parse_args([]).mode is None and ap.parse_args(["--mode", "SDE"]).mode == "SDE" and ap.parse_args(["--mode", "ODE"]).mode == "ODE"
    with pytest.raises(SystemExit):
        ap.parse_args(["--mode", "sde"])
    ode_name = inference.sample_folder_name(_cfg(), "/x/ckpt/0080000.pt")
    assert ode_name == "lightningdit-b-1-ckpt-0080000-euler-250-interval0.10-cfg10.00-shift0.30"          # the reference's rule, unchanged
    assert inference.sample_folder_name(_cfg(mode="SDE"), "/x/ckpt/0080000.pt") == \
        "lightningdit-b-1-ckpt-0080000-sde-euler-250-interval0.10-cfg10.00-shift0.30"
    assert inference.sample_folder_name(_cfg(mode="SDE", sampling_method="Heun", num_sampling_steps=50), "/x/c.pt", cfg_scale=1.0) == \
        "lightningdit-b-1-ckpt-c-sde-heun-50"
    assert inference.sample_folder_name(_cfg(sampling_method="Heun", num_sampling_steps=50), "/x/c.pt", cfg_scale=1.0) == "lightningdit-b-1-ckpt-c-heun-50"
