"""Post-hoc EMA on the host: the profile mathematics, the least-squares reconstruction, the f32 form of the track update, the snapshot
index, the refusals, the YAML key and the header symbols.  No GPU."""
import json
import math
import os

import numpy as np
import pytest

import posthoc_check as pc
from ldmae_amd import posthoc_ema as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G05, G10 = ph.sigma_rel_to_gamma(0.05), ph.sigma_rel_to_gamma(0.10)


def test_sigma_rel_to_gamma_and_back():
    assert abs(G05 - 16.97) < 5e-3 and abs(G10 - 6.94) < 5e-3                  # the two shipped widths
    for s in (0.05, 0.10, 1e-3, 0.02, 0.2, 0.28, ph.SIGMA_REL_MAX * (1 - 1e-9)):
        g = ph.sigma_rel_to_gamma(s)
        assert abs(ph.gamma_to_sigma_rel(g) - s) <= 1e-12 * s + 1e-15, (s, g)
        t = s ** -2                                                            # g is a root of the cubic, and the largest real one
        assert abs(((g + 7) * g + (16 - t)) * g + (12 - t)) <= 1e-9 * (abs(g) ** 3 + t * (abs(g) + 1) + 12)
        assert g == pytest.approx(max(r.real for r in np.roots([1, 7, 16 - t, 12 - t]) if abs(r.imag) < 1e-9 * max(1, abs(r.real))), rel=1e-9, abs=1e-9)
    assert ph.sigma_rel_to_gamma(ph.SIGMA_REL_MAX * (1 - 1e-9)) == pytest.approx(0.0, abs=1e-6)      # the upper edge is gamma = 0
    assert ph.sigma_rel_to_gamma(1e-3) == pytest.approx(1e3 - 3, abs=0.01)         # towards the lower edge: gamma ~ 1 / sigma_rel - 3


@pytest.mark.parametrize("bad", [0.0, -0.05, ph.SIGMA_REL_MAX, 0.3, 1.0, float("nan"), float("inf")])
def test_sigma_rel_outside_the_range_is_refused_by_name(bad):
    with pytest.raises(ValueError, match="sigma_rel"):
        ph.sigma_rel_to_gamma(bad)


@pytest.mark.parametrize("t", [1, 2, 257, 10 ** 6])
@pytest.mark.parametrize("gamma", [G05, G10, 0.0])
def test_discrete_weights_sum_to_one(t, gamma):
    w = ph.discrete_weights(t, gamma)
    assert w.shape == (t,) and (w > 0).all()
    # t terms of rounding error each at most a few 2^-53 of a weight, summed with numpy's pairwise summation
    assert abs(float(w.sum()) - 1.0) <= (8 + math.log2(t)) * 2.0 ** -53 * 4
    assert w[-1] == pytest.approx(ph.track_coef(gamma, t), rel=1e-15)
    # and they are what the recursion gives.  The product form computes beta(s) as 1 - c_s, which for small s cancels: beta(2) = 2^-(gamma+1)
    # ~ 4e-6 comes out with a relative error of 2^-53 / 4e-6 ~ 3e-11, and a few such factors multiply
    cs = [ph.track_coef(gamma, s) for s in range(1, min(t, 300) + 1)]
    np.testing.assert_allclose(pc.actual_weights(cs), ph.discrete_weights(len(cs), gamma), rtol=1e-9, atol=0)


def test_track_coef():
    assert ph.track_coef(G05, 1) == 1.0
    assert ph.track_coef(G05, 2) == pytest.approx(1 - 0.5 ** (G05 + 1), rel=1e-14)
    assert ph.track_coef(16.97, 10 ** 6) == pytest.approx(1.797e-5, rel=1e-3)       # the issue's 1 - beta ~ 1.8e-5
    # expm1 / log1p keep full relative precision where 1 - (1 - 1/t)^(gamma+1) loses 11 digits
    assert ph.track_coef(1.0, 10 ** 6) == pytest.approx(2e-6 - 1e-12, rel=1e-14)
    with pytest.raises(ValueError):
        ph.track_coef(G05, 0)


@pytest.mark.parametrize("a,b", [((256, G05), (256, G10)), ((64, G10), (256, G05)), ((200, G05), (200, G05)), ((8, 2.0), (24, 3.5))])
def test_closed_form_inner_product_against_numerical_integration(a, b):
    closed = float(ph.inner(a[0], a[1], b[0], b[1]))
    assert closed == pytest.approx(float(ph.inner(b[0], b[1], a[0], a[1])), rel=1e-14)
    assert closed == pytest.approx(pc.integrate_inner(a[0], a[1], b[0], b[1]), rel=1e-8)


def _case(t_end=256, every=8):
    steps = [s for s in range(every, t_end + 1, every) for _ in range(2)]
    gammas = [g for _ in range(every, t_end + 1, every) for g in (G05, G10)]
    return steps, gammas


def test_target_equal_to_a_stored_profile_gives_one_hot_coefficients():
    steps, gammas = _case()
    for i in (len(steps) - 1, len(steps) - 2, 20, 1):
        x, _ = ph.solve_coefficients(steps, gammas, steps[i], gammas[i])
        want = np.zeros(len(steps))
        want[i] = 1.0
        assert np.abs(x - want).max() <= 1e-9, i


def test_fixed_reconstruction_case():
    """Snapshots every 8 steps to T = 256, tracks 0.05 / 0.10, target 0.075 at T (figures computed in f64 when the feature was specified:
    profile residual 8.6e-4 relative L2, condition number 9.5e4, max |x| 0.9; 2.2e-3 for target 0.15, 1.07e-2 for 0.03, 6.2e-3 for 0.20)."""
    steps, gammas = _case()
    res = {}
    for s in (0.075, 0.15, 0.03, 0.20):
        g = ph.sigma_rel_to_gamma(s)
        x, cond = ph.solve_coefficients(steps, gammas, 256, g)
        num, den = ph.profile_residual(steps, gammas, x, 256, g)
        res[s] = num / den
        assert abs(x.sum() - 1.0) <= 1e-12
        if s == 0.075:
            assert cond == pytest.approx(9.5e4, rel=0.02) and np.abs(x).max() == pytest.approx(0.9, abs=0.01)
        if s == 0.03:
            assert np.abs(x).max() == pytest.approx(3.7, abs=0.05)             # mixed signs, magnitude above 1: why the accumulator is f64
    print(res)
    assert res[0.075] < 2e-3
    assert res[0.075] == pytest.approx(8.6e-4, rel=0.02) and res[0.15] == pytest.approx(2.2e-3, rel=0.03)
    assert res[0.03] == pytest.approx(1.07e-2, rel=0.02) and res[0.20] == pytest.approx(6.2e-3, rel=0.02)
    # the chunked residual is the dense one
    x, _ = ph.solve_coefficients(steps, gammas, 256, ph.sigma_rel_to_gamma(0.075))
    W = np.stack([ph.discrete_weights(s, g, 1, 256) for s, g in zip(steps, gammas)])
    dense = np.linalg.norm(x @ W - ph.discrete_weights(256, ph.sigma_rel_to_gamma(0.075)))
    assert ph.profile_residual(steps, gammas, x, 256, ph.sigma_rel_to_gamma(0.075), chunk=37)[0] == pytest.approx(dense, rel=1e-9)


def test_f32_one_coefficient_form_keeps_the_fixed_point_and_the_two_coefficient_form_does_not():
    """A constant parameter at t = 1e6, gamma = 16.97, both forms iterated in numpy f32 from e = theta.  e + c (theta - e) never moves (the
    derived bound there is 0).  beta e + (1-beta) theta with beta and 1-beta rounded separately drifts towards theta (1-beta)_f32 / (1 -
    beta_f32): ~0.17 % by the issue's estimate, far outside that bound."""
    c = ph.track_coef(16.97, 10 ** 6)
    cf, bf = np.float32(c), np.float32(1.0 - c)
    theta = np.random.default_rng(0).uniform(1.0, 2.0, 64).astype(np.float32)
    one, two = theta.copy(), theta.copy()
    ref, err = theta.astype(np.float64), np.zeros(64)
    for _ in range(20000):
        one = one + cf * (theta - one)
        two = bf * two + cf * theta
        ref, err = pc.track_step_ref(ref, err, theta, float(cf))
    assert one.dtype == two.dtype == np.float32
    assert (np.abs(one.astype(np.float64) - ref) <= err).all() and (one == theta).all()
    off = np.abs(two.astype(np.float64) - ref)
    print("two-coefficient form, relative drift after 20000 steps:", float((off / theta).max()), "bound", float(err.max()))
    assert (off > err).any() and float((off / theta).max()) > 1e-3
    fixed = float(theta[0]) * float(cf) / (1.0 - float(bf))                     # its fixed point: off by (beta_f32 + c_f32 - 1) / c
    assert abs(fixed / float(theta[0]) - 1.0) > 5e-4


def test_f32_one_coefficient_form_stays_inside_the_carried_bound_away_from_the_fixed_point():
    rng = np.random.default_rng(1)
    theta0 = rng.standard_normal(257).astype(np.float32)
    e = (theta0 * np.float32(1.01)).astype(np.float32)
    ref, err = e.astype(np.float64), np.zeros(257)
    for s in range(300):
        theta = (theta0 + np.float32(1e-3) * rng.standard_normal(257).astype(np.float32)).astype(np.float32)
        cf = np.float32(ph.track_coef(G10, 40 + s))
        e = e + cf * (theta - e)
        ref, err = pc.track_step_ref(ref, err, theta, float(cf))
    assert e.dtype == np.float32 and (np.abs(e.astype(np.float64) - ref) <= err).all()
    assert float(err.max()) < 1e-5          # the bound is worth something: a few dozen ulps of the values after 300 steps


def test_combine_ref_bound_is_of_f64_size():
    rng = np.random.default_rng(2)
    xs = [rng.standard_normal(100).astype(np.float32) for _ in range(33)]
    coefs = list(rng.uniform(-4, 4, 33))
    ref, b64, b32 = pc.combine_ref(xs, coefs)
    plain = sum(c * x.astype(np.float64) for c, x in zip(coefs, xs))
    assert (np.abs(plain - ref) <= b64).all() and float(b64.max()) < 1e-12
    assert (np.abs(plain.astype(np.float32).astype(np.float64) - ref) <= b32).all()


# ----------------------------------------------------------------------------- the snapshot directory
LAYOUT = [("w", 0, (3, 5)), ("b", 64, (7,))]


def _write_dir(d, steps=(8, 16, 24), numel=128, sigma=(0.05, 0.10)):
    ix = ph.new_index(LAYOUT, numel, sigma)
    rng = np.random.default_rng(5)
    data = {}
    for s in steps:
        slabs = [rng.standard_normal(numel).astype(np.float32) for _ in sigma]
        ph.write_snapshot_files(str(d), ix, s, slabs)
        data[s] = slabs
    return ix, data


def test_snapshot_index_round_trip(tmp_path):
    ix, data = _write_dir(tmp_path)
    back = ph.read_index(str(tmp_path))
    assert back == json.load(open(tmp_path / ph.INDEX)) == ix
    assert back["format"] == ph.FORMAT and back["version"] == ph.VERSION and back["steps"] == [8, 16, 24]
    assert back["layout"] == [["w", 0, [3, 5]], ["b", 64, [7]]] and back["sigma_rels"] == [0.05, 0.10]
    assert back["gammas"] == [G05, G10]
    for s, slabs in data.items():
        for k, a in enumerate(slabs):
            m = np.memmap(tmp_path / ph.snapshot_file(s, k), dtype=np.float32, mode="r")
            assert m.shape == (128,) and (m == a).all()
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]          # everything was renamed into place
    assert ph.same_run(back, LAYOUT, 128, (0.05, 0.10)) and not ph.same_run(back, LAYOUT, 128, (0.05, 0.2))
    assert not ph.same_run(back, LAYOUT[:1], 128, (0.05, 0.10))
    text = ph.describe(back)
    assert "sigma_rel 0.05" in text and "8 .. 24" in text
    # a resumed run that repeats a step replaces it and what followed
    ph.write_snapshot_files(str(tmp_path), back, 16, data[8])
    assert ph.read_index(str(tmp_path))["steps"] == [8, 16]
    with pytest.raises(RuntimeError, match="ascend"):
        ph.write_snapshot_files(str(tmp_path), ph.read_index(str(tmp_path)), 12, data[8])


def test_refusals_by_name(tmp_path, capsys):
    with pytest.raises(RuntimeError, match="not a snapshot directory"):
        ph.read_index(str(tmp_path))
    ix, _ = _write_dir(tmp_path)
    with pytest.raises(RuntimeError, match="past the last snapshot"):
        ph.plan(ix, 0.075, step=25)
    with pytest.raises(ValueError, match="sigma_rel"):
        ph.plan(ix, 0.29)
    one = ph.new_index(LAYOUT, 128, (0.05,))
    one["steps"] = [8]
    with pytest.raises(RuntimeError, match="at least 2"):
        ph.plan(one, 0.075)
    with pytest.raises(RuntimeError, match="at least 2"):
        ph.plan(dict(one, steps=[8, 16]), 0.075, step=8)
    with pytest.raises(ValueError, match="at least 2"):
        ph.solve_coefficients([8], [G05], 8, G05)
    # unfinished: the index lists a step whose file is short or gone
    p = tmp_path / ph.snapshot_file(16, 1)
    p.write_bytes(p.read_bytes()[:-4])
    with pytest.raises(RuntimeError, match="unfinished snapshot or mismatched layout"):
        ph.read_index(str(tmp_path))
    os.remove(p)
    with pytest.raises(RuntimeError, match="unfinished snapshot or mismatched layout"):
        ph.read_index(str(tmp_path))
    assert ph.read_index(str(tmp_path), verify=False)["steps"] == [8, 16, 24]
    # mismatched layout, other format, other version
    for change, what in ((dict(layout=[["w", 120, [3, 5]]]), "mismatched layout"), (dict(format="x"), "format"), (dict(version=2), "version"),
                         (dict(steps=[16, 8]), "ascending")):
        d = tmp_path / ("bad_" + what.split()[0])
        d.mkdir()
        json.dump(dict(ix, **change), open(d / ph.INDEX, "w"))
        with pytest.raises(RuntimeError, match=what):
            ph.read_index(str(d), verify=False)
    # the command line reports them and exits non-zero, without touching the GPU
    for argv in (["--snapshots", str(tmp_path), "--sigma_rel", "0.075", "--out", str(tmp_path / "o.pt")],
                 ["--snapshots", str(tmp_path / "nothing"), "--list"],
                 ["--snapshots", str(tmp_path), "--sigma_rel", "0.3", "--out", str(tmp_path / "o.pt")],
                 ["--snapshots", str(tmp_path)]):
        assert ph.main(argv) == 2
        assert "error: posthoc_ema:" in capsys.readouterr().err
    assert not (tmp_path / "o.pt").exists()


def test_list_prints_what_a_directory_holds(tmp_path, capsys):
    _write_dir(tmp_path)
    assert ph.main(["--snapshots", str(tmp_path), "--list"]) == 0
    out = capsys.readouterr().out
    assert "3 snapshot step(s): 8 .. 24" in out and "track 1: sigma_rel 0.1" in out and "2 parameters, 128 f32 elements" in out


def test_yaml_key_parsing():
    import yaml
    from ldmae_amd.train_accum import posthoc_ema_config
    tr = yaml.safe_load("train:\n  posthoc_ema: {sigma_rels: [0.05, 0.10], snapshot_every: 500}\n")["train"]
    assert posthoc_ema_config(tr, "/x/checkpoints") == ((0.05, 0.10), 500, "/x/checkpoints/ema_snapshots")
    tr["posthoc_ema"]["dir"] = "/y"
    assert posthoc_ema_config(tr, "/x/checkpoints")[2] == "/y"
    assert posthoc_ema_config({}, "/x") is None
    for bad in ({"sigma_rels": [0.05]}, {"snapshot_every": 5}, {"sigma_rels": [], "snapshot_every": 5}, {"sigma_rels": [0.05] * 5, "snapshot_every": 5},
                {"sigma_rels": [0.05], "snapshot_every": 0}, {"sigma_rels": [0.05], "snapshot_every": 2.5}, {"sigma_rels": [0.3], "snapshot_every": 5},
                {"sigma_rels": [0.05], "snapshot_every": 5, "every": 3}, [0.05, 0.1]):
        with pytest.raises(ValueError, match="posthoc_ema|sigma_rel"):
            posthoc_ema_config({"posthoc_ema": bad}, "/x")
    # no shipped configuration sets the key: existing runs are as they were
    for ds in ("imagenet", "celeba_hq"):
        cfg = yaml.safe_load(open(os.path.join(ROOT, f"ldmae_amd/configs/{ds}/lightningdit_b_vmae_f8d16_cfg.yaml")))
        assert "posthoc_ema" not in cfg["train"]


def test_header_declares_the_entries_and_the_library_exports_them():
    import ctypes as C
    from ldmae_amd import _lib
    S = _lib.SIGNATURES
    base = S["ldmae_adamw_ema"][1]
    tr = S["ldmae_adamw_ema_tracks"][1]
    assert tr[:len(base) - 1] == base[:-1] and tr[len(base) - 1:] == [C.c_int] + [C.c_void_p] * 4 + [C.c_double] * 4 + [C.c_void_p]
    assert S["ldmae_ema_tracks_only"][1] == [C.c_void_p, C.c_long, C.c_int] + [C.c_void_p] * 4 + [C.c_double] * 4 + [C.c_void_p]
    assert S["ldmae_snapshot_accumulate"][1] == [C.c_void_p, C.c_void_p, C.c_long, C.c_double, C.c_void_p]
    assert S["ldmae_snapshot_finish"][1] == [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("ldmae_adamw_ema_tracks", "ldmae_ema_tracks_only", "ldmae_snapshot_accumulate", "ldmae_snapshot_finish"):
        assert S[name][0] is C.c_int and hasattr(lib, name)


def test_optimizer_refuses_a_width_outside_the_range_and_a_fifth_track():
    from ldmae_amd.optim import AdamWEMA
    import torch
    m = torch.nn.Linear(3, 2)
    with pytest.raises(ValueError, match="sigma_rel"):
        AdamWEMA(m, posthoc_sigma_rels=(0.05, 0.4))
    with pytest.raises(ValueError, match="at most 4"):
        AdamWEMA(m, posthoc_sigma_rels=(0.05, 0.06, 0.07, 0.08, 0.09))
    opt = AdamWEMA(m)
    assert opt.tracks == [] and opt.sigma_rels == ()
    for call in (opt.track_state_dict, lambda: opt.load_track_state({}), lambda: opt.write_snapshot("unused")):
        with pytest.raises(RuntimeError, match="keeps no post-hoc EMA tracks"):
            call()
