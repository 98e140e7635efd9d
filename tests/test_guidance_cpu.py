"""sample.guidance without a GPU: parsing and defaults, every refusal (all of them when the object is built), the momentum / integrator rule,
the folder-name suffix, and that nothing changes while the key is absent."""
import copy
import ctypes
import math
import os
import sys

import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ldmae_amd import _lib, inference as inf, ops          # noqa: E402
from ldmae_amd.guidance import KEYS, Guidance              # noqa: E402

IMAGENET = os.path.join(ROOT, "ldmae_amd", "configs", "imagenet", "lightningdit_b_vmae_f8d16_cfg.yaml")
CELEBA = os.path.join(ROOT, "ldmae_amd", "configs", "celeba_hq", "lightningdit_b_vmae_f8d16_cfg.yaml")


def config(path=IMAGENET, **guidance):
    c = yaml.safe_load(open(path))
    if guidance:
        c['sample']['guidance'] = guidance
    return c


# ----------------------------------------------------------------------------- parsing and defaults
def test_the_key_is_absent_from_the_shipped_configurations():
    for path in (IMAGENET, CELEBA):
        c = config(path)
        assert 'guidance' not in c['sample'] and Guidance.from_config(c) is None


def test_defaults_come_from_the_cfg_keys():
    c = config(rule="cfg")
    g = Guidance.from_config(c)
    assert (g.rule, g.source, g.channels) == ("cfg", "null_class", "all")
    assert g.scale == c['sample']['cfg_scale'] == 10.0
    assert g.interval == (c['sample']['cfg_interval_start'], math.inf) == (0.10, math.inf)
    assert (g.phi, g.eta, g.norm_threshold, g.momentum) == (0.7, 0.0, 0.0, 0.0)
    assert g.guide_model_type == c['model']['model_type'] and g.guide_weights == "ema" and g.guide_ckpt is None
    assert g.k(16) == 16
    c['sample'].pop('cfg_interval_start')
    assert Guidance.from_config(c).interval == (0.0, math.inf)


def test_every_key_is_read():
    g = Guidance.from_config(config(rule="apg", source="auto", channels=3, scale=2.5, interval=[0.2, 0.8], phi=0.5, eta=0.25, norm_threshold=7.5,
                                    momentum=-0.5, guide_ckpt="ckpts/0020000.pt", guide_model_type="LightningDiT-B/2", guide_weights="model"))
    assert (g.rule, g.source, g.channels, g.scale, g.interval) == ("apg", "auto", 3, 2.5, (0.2, 0.8))
    assert (g.phi, g.eta, g.norm_threshold, g.momentum) == (0.5, 0.25, 7.5, -0.5)
    assert (g.guide_ckpt, g.guide_model_type, g.guide_weights) == ("ckpts/0020000.pt", "LightningDiT-B/2", "model")
    assert g.k(16) == 3
    assert set(KEYS) == {"rule", "source", "channels", "scale", "interval", "phi", "eta", "norm_threshold", "momentum", "guide_ckpt",
                         "guide_model_type", "guide_weights"}


def test_direct_construction():
    g = Guidance(rule="rescale", scale=4.0, channels=3, phi=1.0)
    assert (g.rule, g.scale, g.channels, g.phi, g.interval) == ("rescale", 4.0, 3, 1.0, (0.0, math.inf))


# ----------------------------------------------------------------------------- refusals, all at construction
@pytest.mark.parametrize("guidance, needle", [
    (dict(rule="cfgpp"), "rule 'cfgpp'"),
    (dict(rule="cfg", source="self"), "source 'self'"),
    (dict(rule="cfg", sclae=3.0), "unknown key(s) 'sclae'"),
    (dict(rule="cfg", channels=0), "channels 0"),
    (dict(rule="cfg", channels=17), "channels 17"),
    (dict(rule="cfg", channels="first"), "channels 'first'"),
    (dict(rule="rescale", phi=1.5), "phi 1.5"),
    (dict(rule="rescale", phi=-0.1), "phi -0.1"),
    (dict(rule="apg", norm_threshold=-1.0), "norm_threshold -1.0"),
    (dict(rule="cfg", interval=[0.5, 0.1]), "interval"),
    (dict(rule="cfg", interval=0.3), "interval"),
    (dict(rule="cfg", source="auto"), "guide_ckpt"),
    (dict(rule="cfg", source="auto", guide_ckpt="g.pt", guide_weights="best"), "guide_weights 'best'"),
    (dict(rule="cfg", momentum=0.5), "only rule apg"),
])
def test_refusals_by_name(guidance, needle):
    with pytest.raises(ValueError) as e:
        Guidance.from_config(config(**guidance))
    assert needle in str(e.value) and "sample.guidance" in str(e.value)


def test_a_non_mapping_is_refused():
    c = config()
    c['sample']['guidance'] = "apg"
    with pytest.raises(ValueError, match="a mapping"):
        Guidance.from_config(c)


def test_null_class_needs_classes_and_the_advice_names_auto():
    with pytest.raises(ValueError) as e:
        Guidance.from_config(config(CELEBA, rule="cfg", scale=2.0))
    assert "num_classes == 1" in str(e.value) and "source: auto" in str(e.value)
    g = Guidance.from_config(config(CELEBA, rule="cfg", scale=2.0, source="auto", guide_ckpt="output/checkpoints/0020000.pt"))
    assert g.source == "auto"


class FakeModel:
    def __init__(self, channels=16, size=8, classes=10, out_channels=None):
        self.in_channels, self.out_channels = channels, out_channels or channels
        self.x_embedder = type("E", (), {"img_size": (size, size)})()
        self.y_embedder = type("Y", (), {"num_classes": classes})()


def test_model_fn_refusals_happen_before_sampling():
    auto = Guidance(rule="cfg", source="auto", guide_ckpt="g.pt", scale=2.0)
    with pytest.raises(ValueError, match="needs the guide model"):
        auto.model_fn(FakeModel())
    with pytest.raises(ValueError, match="latent shape"):
        auto.model_fn(FakeModel(), FakeModel(size=4))
    with pytest.raises(ValueError, match="latent shape"):
        auto.model_fn(FakeModel(), FakeModel(channels=4))
    with pytest.raises(ValueError, match="learn_sigma"):
        auto.model_fn(FakeModel(out_channels=32), FakeModel())
    with pytest.raises(ValueError, match="unconditional"):
        Guidance(rule="cfg", scale=2.0).model_fn(FakeModel(classes=1))
    with pytest.raises(ValueError, match="channels 17"):
        Guidance(rule="cfg", scale=2.0, channels=17).model_fn(FakeModel())
    fn = auto.model_fn(FakeModel(), FakeModel())
    assert callable(fn) and callable(fn.reset) and fn.calls == [0, 0] and fn.guidance is auto


def test_do_sample_refuses_before_anything_is_loaded(tmp_path):
    """No checkpoint, no tokenizer and no device exist here: the refusal comes first, also when the folder is given."""
    with pytest.raises(ValueError, match="guide_ckpt"):
        inf.do_sample(config(rule="cfg", source="auto"), "missing.pt", out_dir=str(tmp_path))
    with pytest.raises(ValueError, match="source: auto"):
        inf.do_sample(config(CELEBA, rule="apg"), "missing.pt")
    with pytest.raises(NotImplementedError, match="demo"):
        inf.do_sample(config(rule="cfg"), "missing.pt", demo=True)


# ----------------------------------------------------------------------------- momentum needs one evaluation per step
@pytest.mark.parametrize("mode, method, ok", [("ODE", "euler", True), ("SDE", "euler", True), ("SDE", "Euler", True), ("ODE", "heun", False),
                                              ("ODE", "midpoint", False), ("ODE", "dopri5", False), ("SDE", "heun", False)])
def test_momentum_and_integrator(mode, method, ok):
    c = config(rule="apg", momentum=-0.5)
    c['sample'].update(mode=mode, sampling_method=method)
    if ok:
        assert Guidance.from_config(c).momentum == -0.5
    else:
        with pytest.raises(ValueError) as e:
            Guidance.from_config(c)
        assert "momentum" in str(e.value) and "once per step" in str(e.value)
    c['sample']['guidance']['momentum'] = 0.0           # without momentum every integrator is accepted
    assert Guidance.from_config(c).momentum == 0.0


def test_sample_latents_checks_the_sampler_of_a_directly_built_object():
    """Built without `integrator`, the rule is applied against the sampling function, before anything is drawn (no device exists here)."""
    from ldmae_amd.transport import Sampler, create_transport
    sampler = Sampler(create_transport("Linear", "velocity", None, None, None))
    fn = Guidance(rule="apg", source="auto", guide_ckpt="g.pt", scale=2.0, momentum=-0.5).model_fn(FakeModel(), FakeModel())
    for kw in (dict(sampling_method="heun"), dict(sampling_method="dopri5")):
        with pytest.raises(ValueError, match="once per step"):
            inf.sample_latents(FakeModel(), sampler.sample_ode(num_steps=3, **kw), 2, 1.0, 0.0, "cpu", guidance=fn)
    with pytest.raises(ValueError, match="once per step"):
        inf.sample_latents(FakeModel(), sampler.sample_sde(sampling_method="Heun", diffusion_form="sigma", num_steps=3), 2, 1.0, 0.0, "cpu", guidance=fn)
    fn.guidance.check_sampler(sampler.sample_ode(sampling_method="euler", num_steps=3))
    fn.guidance.check_sampler(sampler.sample_sde(sampling_method="Euler", diffusion_form="sigma", num_steps=3))


# ----------------------------------------------------------------------------- folder names
BASE = dict(rule="apg", source="null_class", channels="all", scale=4.0, interval=[0.1, 0.9], eta=0.0, norm_threshold=5.0, momentum=-0.5)
VARIANTS = [dict(rule="cfg", momentum=0.0), dict(rule="rescale", momentum=0.0), dict(channels=3), dict(channels=16), dict(scale=4.5), dict(interval=[0.2, 0.9]),
            dict(interval=[0.1, 0.8]), dict(eta=0.5), dict(norm_threshold=2.5), dict(momentum=-0.25), dict(momentum=0.0),
            dict(source="auto", guide_ckpt="ck/0020000.pt"), dict(source="auto", guide_ckpt="ck/0040000.pt"),
            dict(source="auto", guide_ckpt="ck/0020000.pt", guide_weights="model"),
            dict(source="auto", guide_ckpt="ck/0020000.pt", guide_model_type="LightningDiT-B/2")]


def test_folder_suffix_is_deterministic_and_distinct_per_parameter():
    ck = "output/checkpoints/0080000.pt"
    plain = inf.sample_folder_name(config(), ck)
    names = [inf.sample_folder_name(config(**BASE), ck)]
    assert names[0] == inf.sample_folder_name(config(**copy.deepcopy(BASE)), ck)
    assert names[0].startswith(plain + "-guide-apg-nullclass-kall-") and "/" not in names[0] and names[0] == names[0].lower()
    for v in VARIANTS:
        names.append(inf.sample_folder_name(config(**dict(BASE, **v)), ck))
    assert len(set(names)) == len(names), sorted(names)
    # the parameters of rescale
    a, b = (inf.sample_folder_name(config(rule="rescale", phi=phi), ck) for phi in (0.7, 0.75))
    assert a != b and "phi0.7" in a
    # values that agree to two decimals still get folders of their own
    a, b = (inf.sample_folder_name(config(rule="cfg", scale=s), ck) for s in (4.0, 4.001))
    assert a != b


# ----------------------------------------------------------------------------- nothing changes without the key
def test_without_the_key_names_parser_and_sampler_are_as_before():
    c = config()
    assert inf.sample_folder_name(c, "output/checkpoints/0080000.pt") == "lightningdit-b-1-ckpt-0080000-euler-250-interval0.10-cfg10.00-shift0.30"
    assert inf.sample_folder_name(config(CELEBA), "a/0060000.pt") == "lightningdit-b-1-ckpt-0060000-euler-250"
    a = inf.build_parser().parse_args([])
    assert (a.guidance_rule, a.guidance_source, a.guidance_channels, a.guide_ckpt) == (None, None, None, None)
    assert inf.apply_guidance_flags(c, a) is c
    fn = inf.build_sampler(c)
    assert fn.__self__.sampler_type == "euler" and not hasattr(fn, "guidance")
    import inspect
    p = inspect.signature(inf.sample_latents).parameters
    assert p["guidance"].default is None and list(p)[-1] == "guidance"


def test_flags_override_the_yaml():
    a = inf.build_parser().parse_args(["--guidance_rule", "apg", "--guidance_source", "auto", "--guidance_channels", "3", "--guide_ckpt", "g.pt"])
    c = inf.apply_guidance_flags(config(rule="cfg", eta=0.5), a)
    assert c['sample']['guidance'] == dict(rule="apg", eta=0.5, source="auto", channels=3, guide_ckpt="g.pt")
    a = inf.build_parser().parse_args(["--guidance_rule", "rescale", "--guidance_channels", "all"])
    c = inf.apply_guidance_flags(config(), a)
    assert c['sample']['guidance'] == dict(rule="rescale", channels="all") and Guidance.from_config(c).rule == "rescale"
    with pytest.raises(SystemExit):
        inf.apply_guidance_flags(config(), inf.build_parser().parse_args(["--guidance_channels", "three"]))


# ----------------------------------------------------------------------------- the native entry and its wrapper
def test_symbol_in_header_library_and_makefile():
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.SIGNATURES["ldmae_guidance_combine"] == (I, [I, I, P, P, P, P, P, P, I, I, I, I, F, F, F, F, F, P])
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ldmae_guidance_combine")
    assert "guidance.hip" in open(os.path.join(ROOT, "ldmae_amd", "csrc", "Makefile")).read()
    header = open(os.path.join(ROOT, "include", "ldmae_hip.h")).read()
    assert all(f"#define LDMAE_GUIDE_{n} {v}" in header for n, v in (("CFG", 0), ("RESCALE", 1), ("APG", 2)))
    assert ops.GUIDANCE_RULES == {"cfg": 0, "rescale": 1, "apg": 2}


def Z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


@pytest.mark.parametrize("kw, needle", [
    (dict(rule="cfgpp"), "guidance_combine rule"),
    (dict(k=0), "guidance_combine k"),
    (dict(k=5), "guidance_combine k"),
    (dict(rule="rescale", phi=1.5), "guidance_combine phi"),
    (dict(rule="apg", norm_threshold=-1.0), "guidance_combine norm_threshold"),
    (dict(rule="apg", mom=Z(2, 63)), "guidance_combine mom"),
    (dict(rule="apg", momentum=0.5), "guidance_combine mom"),
    (dict(rule="apg", x=None), "needs the state x"),
    (dict(neg=Z(2, 8, 4, 4)), "learn_sigma"),
    (dict(rule="apg", x=Z(2, 8, 4, 4)), "learn_sigma"),
    (dict(neg=Z(2, 4, 4, 4, dtype=torch.bfloat16)), "guidance_combine neg: dtype"),
    (dict(pos=Z(2, 4, 4, 4, dtype=torch.float16), neg=Z(2, 4, 4, 4, dtype=torch.float16)), "guidance_combine pos: dtype"),
    (dict(out=Z(2, 4, 4, 4, dtype=torch.bfloat16)), "guidance_combine out: dtype"),
    (dict(rule="apg", t=Z(3)), "guidance_combine t: shape"),
])
def test_wrapper_refusals_by_name(kw, needle):
    args = dict(rule="cfg", pos=Z(2, 4, 4, 4), neg=Z(2, 4, 4, 4), scale=2.0, k=4, x=Z(2, 4, 4, 4), t=Z(2))
    args.update(kw)
    with pytest.raises(RuntimeError) as e:
        ops.guidance_combine(**args)
    assert needle in str(e.value)


def test_a_well_formed_call_stops_only_at_the_device():
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.guidance_combine("apg", Z(2, 4, 4, 4), Z(2, 4, 4, 4), 2.0, k=3, x=Z(2, 4, 4, 4), t=Z(2), mom=Z(2, 48), momentum=-0.5)
