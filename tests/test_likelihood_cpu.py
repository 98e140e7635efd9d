"""Likelihood evaluation, host side: the numpy restatement of the Philox4x32-10 Rademacher probe against known-answer vectors, the tuple-state
paths of the ODE constructor, the C ABI, the command line's argument handling, and the refusals (no CPU fallback; nothing else un-refused)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Known-answer vectors of philox4x32 with 10 rounds from the Random123 distribution's kat_vectors (counter, key, output)
KAT = [((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    from ldmae_amd.transport import probe
    got = probe.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
    assert got.dtype == np.uint32 and tuple(int(v) for v in got) == want


def test_rademacher_restatement_reads_one_bit_per_word():
    from ldmae_amd.transport import probe
    seed, counter = 0x299f31d0a4093822, 0x85a308d3243f6a88          # key / counter words of the third vector, block index 0x0370734413198a2e
    v = 0x0370734413198a2e
    words = probe.philox4x32_10(np.array([counter & 0xffffffff, counter >> 32, v & 0xffffffff, v >> 32], dtype=np.uint32),
                                np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint32))
    assert tuple(int(w) for w in words) == KAT[2][2]
    # element i = word i % 4 of block i // 4, +1 when the top bit is set: block 0 of (seed 0, counter 0) is the first vector
    first = probe.rademacher(7, 0, 0)
    assert first.dtype == np.float32 and first[:4].tolist() == [1.0 if w >> 31 else -1.0 for w in KAT[0][2]] == [-1.0, 1.0, 1.0, 1.0]
    assert np.array_equal(probe.rademacher(4100, 3, 5)[:7], probe.rademacher(7, 3, 5))                    # a prefix, whatever n
    a, b, c = probe.rademacher(4096, 3, 5), probe.rademacher(4096, 3, 6), probe.rademacher(4096, 4, 5)
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and abs(float(a.mean())) < 5 / 64          # 5 sigma of 4096 fair signs


def test_abi_declares_and_binds_the_likelihood_entry_points():
    from ldmae_amd import _lib
    header = open(os.path.join(ROOT, "include", "ldmae_hip.h")).read()
    for name in ("ldmae_rademacher_f32", "ldmae_rowdot_partials", "ldmae_rowdot_f32", "ldmae_likelihood_finish_f32"):
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\);", header)
        assert m, name + " is not declared in include/ldmae_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
    part = _lib.load().ldmae_rowdot_partials
    assert (part(1, 1), part(3, 4096), part(3, 4097), part(0, 5)) == (1, 3, 6, 0)


def test_tuple_state_through_the_fixed_step_solvers():
    """(x, logp) through euler / heun / midpoint: both members take the method's update; x follows the plain-state result bit for bit."""
    from ldmae_amd.transport.integrators import ode
    a = torch.randn(5, 5, generator=torch.Generator().manual_seed(0)) * 0.2
    plain = lambda x, t, model, **kw: x @ a.t() * t.view(-1, 1)      # noqa: E731
    pair = lambda s, t, model, **kw: (plain(s[0], t, model), t * 2)  # noqa: E731    d logp / dt = 2 t: logp(1) = 1
    x = torch.randn(3, 5, generator=torch.Generator().manual_seed(1))
    for method, exact in (("euler", False), ("heun", True), ("midpoint", True)):
        kw = dict(t0=0, t1=1, sampler_type=method, num_steps=9, atol=1e-6, rtol=1e-3)
        xs, ls = ode(pair, **kw).sample((x, torch.zeros(3)), None)
        assert xs.shape == (9, 3, 5) and ls.shape == (9, 3) and torch.equal(xs[0], x) and float(ls[0].abs().max()) == 0
        assert torch.equal(xs, ode(plain, **kw).sample(x, None)), method
        assert abs(float(ls[-1, 0]) - 1.0) < (1e-6 if exact else 0.2), method      # second-order methods integrate 2 t exactly
    o = ode(pair, t0=0, t1=1, sampler_type="dopri5", num_steps=9, atol=1e-6, rtol=1e-3)
    with pytest.raises(RuntimeError, match="HIP device"):
        o.sample((x, torch.zeros(3)), None)
    with pytest.raises(ValueError, match=r"\(x, logp\)"):
        o.sample((x, torch.zeros(4)), None)
    with pytest.raises(ValueError, match="pair"):
        o.sample((x, torch.zeros(3), x), None)


def test_sample_ode_likelihood_signature_and_refusals():
    import inspect
    from ldmae_amd.transport import Sampler, create_transport
    s = Sampler(create_transport())
    p = inspect.signature(s.sample_ode_likelihood).parameters
    assert [(n, v.default) for n, v in p.items()] == [("sampling_method", "dopri5"), ("num_steps", 50), ("atol", 1e-6), ("rtol", 1e-3), ("seed", 0),
                                                      ("noise", None)]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for v in p.values())
    fn = s.sample_ode_likelihood()
    assert fn.ode.sampler_type == "dopri5" and len(fn.ode.t) == 50 and float(fn.ode.t[0]) == 0 and float(fn.ode.t[-1]) == 1
    with pytest.raises(RuntimeError, match="HIP device"):              # as dopri5 itself: no CPU fallback
        fn(torch.zeros(2, 4, 2, 2), lambda x, t: x)
    with pytest.raises(NotImplementedError, match="euler / heun / midpoint / dopri5"):
        s.sample_ode_likelihood(sampling_method="rk4")
    with pytest.raises(NotImplementedError, match="SDE sampling is out of scope"):      # untouched
        s.sample_sde()


def test_input_grad_only_is_off_by_default_and_restored():
    from ldmae_amd.models.lightningdit import LightningDiT
    m = LightningDiT(input_size=4, patch_size=1, in_channels=4, hidden_size=64, depth=1, num_heads=1)
    assert m._input_grad_only is False
    with m.input_grad_only() as inner:
        assert inner is m and m._input_grad_only is True
        with m.input_grad_only(False):
            assert m._input_grad_only is False
        assert m._input_grad_only is True
    with pytest.raises(ZeroDivisionError):
        with m.input_grad_only():
            1 / 0
    assert m._input_grad_only is False
    assert "_input_grad_only" not in m.state_dict()


def _cli(argv):
    import ldmae_amd.likelihood as cli
    return cli.parse_args(argv)


def test_command_line_arguments_and_refusals(tmp_path, capsys):
    cfg = os.path.join(ROOT, "ldmae_amd/configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml")
    a = _cli(["--config", cfg, "--synthetic", "4"])
    assert (a.synthetic, a.data, a.ckpt, a.batch, a.method, a.num_steps, a.atol, a.rtol, a.seed, a.precision) == \
        (4, None, None, 32, "dopri5", 50, 1e-6, 1e-3, 0, "fp32")
    (tmp_path / "c.pt").write_bytes(b"")
    a = _cli(["--config", cfg, "--data", str(tmp_path), "--ckpt", str(tmp_path / "c.pt"), "--num-images", "10", "--precision", "bf16"])
    assert a.data == str(tmp_path) and a.num_images == 10 and a.precision == "bf16"
    for argv, said in (
            (["--config", cfg], "exactly one of --data DIR and --synthetic N"),
            (["--config", cfg, "--synthetic", "4", "--data", str(tmp_path), "--ckpt", str(tmp_path / "c.pt")], "exactly one of"),
            (["--config", cfg, "--synthetic", "0"], "N >= 1"),
            (["--config", cfg, "--data", str(tmp_path)], "--data needs --ckpt"),
            (["--config", cfg, "--synthetic", "4", "--ckpt", "https://example.org/w.pt"], "downloads nothing"),
            (["--config", cfg, "--synthetic", "4", "--ckpt", str(tmp_path / "absent.pt")], "does not exist"),
            (["--config", cfg, "--data", str(tmp_path / "absent"), "--ckpt", str(tmp_path / "c.pt")], "is not a directory"),
            (["--config", str(tmp_path / "absent.yaml"), "--synthetic", "4"], "does not exist"),
            (["--config", cfg, "--synthetic", "4", "--batch", "0"], "must be positive"),
            (["--synthetic", "4"], "--config")):
        with pytest.raises(SystemExit) as e:
            _cli(argv)
        assert e.value.code == 2 and said in capsys.readouterr().err, argv


def test_command_line_refuses_to_run_without_a_device(monkeypatch):
    import ldmae_amd.likelihood as cli
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = os.path.join(ROOT, "ldmae_amd/configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml")
    with pytest.raises(SystemExit, match="needs a HIP device"):
        cli.main(["--config", cfg, "--synthetic", "2"])
