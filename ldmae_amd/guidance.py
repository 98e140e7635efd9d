"""Guidance rules of the sampler, the opt-in YAML key sample.guidance: classifier-free guidance on ALL latent channels
(or the first k), CFG-rescale (Lin et al. 2024), adaptive projected guidance (APG, Sadat et al. 2024) and autoguidance (Karras et al. 2024:
the negative prediction comes from a weaker model -- an earlier checkpoint, a post-hoc EMA reconstruction, a smaller model -- so it needs no
null class).  The rule itself is one HIP launch (ops.guidance_combine, csrc/guidance.hip; the contract is in include/ldmae_hip.h).

    sample:
      guidance:
        rule: cfg | rescale | apg
        source: null_class | auto        # auto = autoguidance with a second model
        channels: all | <int>            # default all; 3 = the reference's behaviour
        scale: <float>                   # default sample.cfg_scale
        interval: [lo, hi]               # guided when lo <= t < hi; default [sample.cfg_interval_start or 0, inf]
        phi: 0.7                         # rescale
        eta: 0.0                         # apg
        norm_threshold: 0.0              # apg; 0 = off
        momentum: 0.0                    # apg
        guide_ckpt: <path>               # source auto
        guide_model_type: <name>         # default model.model_type
        guide_weights: ema | model       # default ema

Without the key nothing here runs: sample_latents(cfg_scale=...) and LightningDiT.forward_with_cfg stay as they are.  What any of these rules
does to FID has not been measured (no trained checkpoint is available to this project)."""
from __future__ import annotations

import math

import torch

RULES = ("cfg", "rescale", "apg")
SOURCES = ("null_class", "auto")
KEYS = ("rule", "source", "channels", "scale", "interval", "phi", "eta", "norm_threshold", "momentum", "guide_ckpt", "guide_model_type",
        "guide_weights")
# the integrators that evaluate the model exactly once per step: the only ones under which "the previous evaluation" is the previous step
ONE_EVAL_PER_STEP = (("ODE", "euler"), ("SDE", "euler"))


def integrator_of(cfg):
    """(mode, method in lower case) of a YAML's sample section."""
    s = cfg['sample']
    return str(s.get('mode', 'ODE')), str(s.get('sampling_method', 'euler')).lower()


def integrator_of_sampler(sample_fn):
    """(mode, method in lower case) of a function returned by Sampler.sample_ode / sample_sde, or None when it is neither."""
    solver = getattr(sample_fn, "__self__", None)
    if hasattr(solver, "sampler_type"):
        return "ODE", solver.sampler_type.lower()
    if hasattr(sample_fn, "sde"):
        return "SDE", sample_fn.sde.sampler_type.lower()
    return None


class Guidance:
    """One guidance setting, checked when it is built.  num_classes / in_channels (when given) let the refusals that need the model happen
    here and not in the middle of sampling; integrator = (mode, method), e.g. ("ODE", "euler")."""

    def __init__(self, rule="cfg", source="null_class", channels="all", scale=1.0, interval=(0.0, math.inf), phi=0.7, eta=0.0,
                 norm_threshold=0.0, momentum=0.0, guide_ckpt=None, guide_model_type=None, guide_weights="ema", num_classes=None,
                 in_channels=None, integrator=None):
        if rule not in RULES:
            raise ValueError(f"sample.guidance.rule {rule!r}: one of {', '.join(RULES)}")
        if source not in SOURCES:
            raise ValueError(f"sample.guidance.source {source!r}: one of {', '.join(SOURCES)}")
        if channels != "all" and (isinstance(channels, bool) or not isinstance(channels, int) or channels < 1
                                  or (in_channels is not None and channels > in_channels)):
            raise ValueError(f"sample.guidance.channels {channels!r}: 'all' or an integer in 1 .. in_channels"
                             + (f" = {in_channels}" if in_channels is not None else ""))
        if guide_weights not in ("ema", "model"):
            raise ValueError(f"sample.guidance.guide_weights {guide_weights!r}: 'ema' or 'model'")
        interval = tuple(float(v) for v in interval) if isinstance(interval, (list, tuple)) else interval
        if not (isinstance(interval, tuple) and len(interval) == 2 and interval[0] <= interval[1]):
            raise ValueError(f"sample.guidance.interval {interval!r}: [lo, hi] with lo <= hi (guided when lo <= t < hi)")
        scale, phi, eta, norm_threshold, momentum = (float(v) for v in (scale, phi, eta, norm_threshold, momentum))
        if not 0.0 <= phi <= 1.0:
            raise ValueError(f"sample.guidance.phi {phi!r}: a value in [0, 1]")
        if norm_threshold < 0.0:
            raise ValueError(f"sample.guidance.norm_threshold {norm_threshold!r} must not be negative (0 = off)")
        if source == "null_class" and num_classes == 1:
            raise ValueError("sample.guidance.source null_class: the model is unconditional (data.num_classes == 1), it has no null class to guide "
                             "against; use source: auto (autoguidance with an earlier checkpoint or a smaller model, guide_ckpt)")
        if source == "auto" and not guide_ckpt:
            raise ValueError("sample.guidance.source auto: guide_ckpt (the checkpoint of the guiding model) is missing")
        if momentum != 0.0 and rule != "apg":
            raise ValueError(f"sample.guidance.momentum {momentum!r}: only rule apg has a momentum")
        if momentum != 0.0 and integrator is not None:
            self.check_integrator(momentum, integrator)
        self.rule, self.source, self.channels, self.scale, self.interval = rule, source, channels, scale, interval
        self.phi, self.eta, self.norm_threshold, self.momentum = phi, eta, norm_threshold, momentum
        self.guide_ckpt, self.guide_model_type, self.guide_weights, self.num_classes = guide_ckpt, guide_model_type, guide_weights, num_classes

    @staticmethod
    def check_integrator(momentum, integrator):
        mode, method = integrator[0], str(integrator[1]).lower()
        if momentum != 0.0 and (mode, method) not in ONE_EVAL_PER_STEP:
            raise ValueError(f"sample.guidance.momentum {momentum!r} with {mode} {method}: the momentum is the previous STEP's direction, so the "
                             "integrator must evaluate the model exactly once per step: ODE euler or SDE Euler (heun, midpoint and dopri5 evaluate "
                             "more than once, dopri5 also rejects steps); set momentum: 0.0 or change sample.sampling_method")

    def check_sampler(self, sample_fn):
        """The same rule for an object built without `integrator`, against the sampling function itself (sample_latents, before it draws)."""
        integrator = integrator_of_sampler(sample_fn)
        if integrator is not None:
            self.check_integrator(self.momentum, integrator)

    @classmethod
    def from_config(cls, cfg):
        """The Guidance of a YAML's sample.guidance, or None when the key is absent (nothing changes then)."""
        s = cfg['sample']
        g = s.get('guidance')
        if g is None:
            return None
        if not isinstance(g, dict):
            raise ValueError(f"sample.guidance: a mapping of {', '.join(KEYS)} expected, got {g!r}")
        unknown = sorted(set(g) - set(KEYS))
        if unknown:
            raise ValueError(f"sample.guidance: unknown key(s) {', '.join(map(repr, unknown))}; the keys are {', '.join(KEYS)}")
        kw = dict(g)
        kw.setdefault('scale', s.get('cfg_scale', 1.0))
        kw.setdefault('interval', [s.get('cfg_interval_start') or 0.0, math.inf])
        kw.setdefault('guide_model_type', cfg['model']['model_type'])
        return cls(num_classes=cfg['data'].get('num_classes'), in_channels=cfg['model'].get('in_chans', 4), integrator=integrator_of(cfg), **kw)

    def k(self, C):
        k = C if self.channels == "all" else self.channels
        if not 1 <= k <= C:
            raise ValueError(f"sample.guidance.channels {self.channels!r}: 'all' or an integer in 1 .. in_channels = {C}")
        return k

    def rule_params(self):
        """The parameters the rule reads, in a fixed order (name, value)."""
        return {"cfg": (), "rescale": (("phi", self.phi),),
                "apg": (("eta", self.eta), ("r", self.norm_threshold), ("mom", self.momentum))}[self.rule]

    def folder_suffix(self):
        """Deterministic, and distinct whenever two settings differ in the rule, the source, k, the scale, the interval, a parameter of the rule
        or the guide: repr() of a float is its shortest round-trip form, so different values give different text."""
        lo, hi = self.interval
        parts = [f"-guide-{self.rule}-{self.source.replace('_', '')}-k{self.channels}-s{self.scale!r}-t{lo!r}to{hi!r}"]
        parts += [f"-{n}{v!r}" for n, v in self.rule_params()]
        if self.source == "auto":
            parts.append(f"-by-{self.guide_model_type}-{str(self.guide_ckpt).split('/')[-1].rsplit('.', 1)[0]}-{self.guide_weights}")
        return "".join(parts).replace('/', '-').lower()

    def check_guide(self, model, guide):
        """A guide must produce the main model's latent shape: refused here, before sampling."""
        a = (model.in_channels, tuple(model.x_embedder.img_size))
        b = (guide.in_channels, tuple(guide.x_embedder.img_size))
        if a != b:
            raise ValueError(f"sample.guidance: the guide's latent shape (channels, size) = {b} differs from the main model's {a}")

    def model_fn(self, model, guide=None):
        """fn(x, t, y) -> the guided velocity [n, C, H, W] f32 on the UN-doubled batch.  Inside the interval (lo <= t[0] < hi, read on the host as
        forward_with_cfg's gate is): null_class runs the model once on cat([x, x]) with labels cat([y, null]); auto runs model(x, t, y) and
        guide(x, t, y).  Outside it the negative forward is not run and fn returns the model's own output.  fn.reset() clears the APG momentum
        (a new trajectory); fn.calls counts (main, negative) forwards since the last reset."""
        from . import ops
        if getattr(model, "out_channels", model.in_channels) != model.in_channels:
            raise ValueError("sample.guidance: learn_sigma models (out_channels != in_channels) are not supported")
        null = self.num_classes if self.num_classes is not None else getattr(getattr(model, "y_embedder", None), "num_classes", None)
        if self.source == "auto":
            if guide is None:
                raise ValueError("sample.guidance.source auto: Guidance.model_fn needs the guide model")
            self.check_guide(model, guide)
        elif null is None or null == 1:
            raise ValueError("sample.guidance.source null_class: the model is unconditional (num_classes == 1) or its class count is unknown; "
                             "use source: auto")
        k = self.k(model.in_channels)
        lo, hi = self.interval
        state = {"mom": None}

        def fn(x, t, y=None, **kw):
            if not lo <= float(t[0]) < hi:
                fn.calls[0] += 1
                return model.forward(x, t, y)
            n = len(x)
            if self.source == "auto":
                pos, neg = model.forward(x, t, y), guide.forward(x, t, y)
                fn.calls[0] += 1
                fn.calls[1] += 1
            else:
                both = model.forward(torch.cat([x, x], 0), torch.cat([t, t], 0), torch.cat([y, torch.full_like(y, null)], 0))
                pos, neg = both[:n], both[n:]
                fn.calls[0] += 1
            if self.rule != "apg":
                return ops.guidance_combine(self.rule, pos, neg, self.scale, k=k, phi=self.phi)
            mom = None
            if self.momentum != 0.0:
                if state["mom"] is None or state["mom"].shape[0] != n:
                    state["mom"] = torch.zeros(n, k * x[0, 0].numel(), dtype=torch.float32, device=x.device)
                mom = state["mom"]
            return ops.guidance_combine("apg", pos, neg, self.scale, k=k, x=x.float(), t=t.float(), eta=self.eta,
                                        norm_threshold=self.norm_threshold, momentum=self.momentum, mom=mom)

        def reset():
            state["mom"] = None
            fn.calls = [0, 0]

        fn.reset = reset
        fn.guidance = self
        fn.calls = [0, 0]
        return fn
