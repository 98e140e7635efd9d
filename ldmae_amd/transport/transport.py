"""Transport objective + samplers (reference: LDMAE/transport/transport.py)."""
import contextlib
import enum

import numpy as np
import torch as th

from . import path
from .integrators import ode, sde, sde_drift_terms, SDE_METHODS, _f32
from .utils import mean_flat


class ModelType(enum.Enum):
    NOISE = enum.auto()
    SCORE = enum.auto()
    VELOCITY = enum.auto()


class PathType(enum.Enum):
    LINEAR = enum.auto()
    GVP = enum.auto()
    VP = enum.auto()


class WeightType(enum.Enum):
    NONE = enum.auto()
    VELOCITY = enum.auto()
    LIKELIHOOD = enum.auto()


class _DispersiveFn(th.autograd.Function):
    """L = log mean_ij exp(-||z_i - z_j||^2 / (K tau)) of z [B, K] f32 (ops.dispersive_fwd; the contract is in include/ldmae_hip.h).  The forward
    leaves C [B, B]; the backward is dz = g C z (ops.dispersive_bwd) with the upstream gradient g read on the host: it is the loss weight over
    the accumulation steps, a number the driver already holds, and one scalar read per step where the tapped block's backward is about to
    start anyway."""

    @staticmethod
    def forward(ctx, z, tau):
        from .. import ops
        loss, C = ops.dispersive_fwd(z, tau)
        ctx.save_for_backward(z, C)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        from .. import ops
        z, C = ctx.saved_tensors
        return ops.dispersive_bwd(C, z, float(g)), None


def dispersive_options(opt, depth, *, per_gpu_batch=None, use_checkpoint=False, where="dispersive"):
    """The option {weight: 0.5, tau: 0.5, block: <int>} of the Dispersive Loss, checked -> {'weight', 'tau', 'block'}, or None for None.  block
    (counted from 0) defaults to depth // 4.  Refused by name: an unknown key, weight < 0, tau <= 0, a block outside 0 .. depth - 1, a per-GPU
    batch of 1 (the loss of a single sample is the constant 0) and use_checkpoint (LightningDiT.tap_block)."""
    if opt is None:
        return None
    if not isinstance(opt, dict) or set(opt) - {"weight", "tau", "block"}:
        raise ValueError(f"{where} must be a mapping with the keys weight, tau and block (all optional); got {opt!r}")

    def number(key, default):
        v = opt.get(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float("inf"), float("-inf")):
            raise ValueError(f"{where}.{key} must be a finite number; got {v!r}")
        return float(v)

    weight, tau = number("weight", 0.5), number("tau", 0.5)
    if weight < 0:
        raise ValueError(f"{where}.weight must not be negative; got {weight!r}")
    if tau <= 0:
        raise ValueError(f"{where}.tau must be > 0; got {tau!r}")
    block = opt.get("block", depth // 4)
    if isinstance(block, bool) or not isinstance(block, int) or not 0 <= block < depth:
        raise ValueError(f"{where}.block must be an integer in 0 .. {depth - 1} (depth {depth}, counted from 0); got {block!r}")
    if per_gpu_batch is not None and per_gpu_batch < 2:
        raise ValueError(f"{where} needs a per-GPU batch of at least 2 (the term is computed per rank and micro-batch; one sample has no pair); "
                         f"got {per_gpu_batch}")
    if use_checkpoint:
        raise ValueError(f"{where} with model.use_checkpoint: true is not supported (LightningDiT.tap_block needs the block output of the forward)")
    return {"weight": weight, "tau": tau, "block": block}


class Transport:
    def __init__(self, *, model_type, path_type, loss_type, train_eps, sample_eps, use_cosine_loss=False, use_lognorm=False,
                 partitial_train=None, partial_ratio=1.0, shift_lg=False, dispersive=None):
        """dispersive (not a reference option): None, or {'tau': ..., 'block': ...} (and 'weight', which the driver applies): training_losses
        then runs the model under LightningDiT.tap_block(block) and adds terms['disp_loss'], the Dispersive Loss of that block's output."""
        self.dispersive = dispersive
        self.loss_type, self.model_type = loss_type, model_type
        if path_type != PathType.LINEAR or model_type != ModelType.VELOCITY:
            raise NotImplementedError("ldmae_amd Transport: linear path + velocity prediction only (SURVEY.md 2.1 #7)")
        self.path_sampler = path.ICPlan()
        self.train_eps, self.sample_eps = train_eps, sample_eps
        self.use_cosine_loss, self.use_lognorm = use_cosine_loss, use_lognorm
        self.partitial_train, self.partial_ratio, self.shift_lg = partitial_train, partial_ratio, shift_lg

    def prior_logp(self, z):
        n = int(np.prod(z.shape[1:]))
        return -n / 2.0 * np.log(2 * np.pi) - th.sum(z.flatten(1) ** 2, dim=1) / 2.0

    def check_interval(self, train_eps, sample_eps, *, diffusion_form="SBDM", sde=False, reverse=False, eval=False,
                       last_step_size=0.0):
        """transport.py:84-111 for the velocity model on the linear path: the whole unit interval, except for the SDE sampler, which starts at
        eps under the SBDM diffusion (infinite at t = 0) and stops one last step short of 1 (at 1 - eps when last_step_size is 0)."""
        t0, t1 = 0, 1
        if sde:
            eps = sample_eps if eval else train_eps
            t0 = eps if diffusion_form == "SBDM" else 0
            t1 = 1 - eps if last_step_size == 0 else 1 - last_step_size
        return (1 - t0, 1 - t1) if reverse else (t0, t1)

    def sample_logit_normal(self, mu, sigma, size=1):
        """transport.py:113-123.  The reference calls scipy.stats.norm.rvs with no random_state, i.e.
        numpy's GLOBAL RandomState; `mu + sigma * standard_normal(size)` consumes that stream identically."""
        z = mu + sigma * np.random.standard_normal(size)
        return th.tensor(1 / (1 + np.exp(-z)), dtype=th.float32)

    def sample_in_range(self, mu, sigma, target_size, range_min=0, range_max=0.5):
        out = []
        while len(out) < target_size:
            s = self.sample_logit_normal(mu, sigma, size=target_size)
            out.extend(s[(s >= range_min) & (s <= range_max)])
        return th.tensor(out[:target_size])

    def sample(self, x1, sp_timesteps=None, shifted_mu=0):
        """transport.py:136-166: x0 on x1's device RNG, t on the host (numpy for logit-normal)."""
        x0 = th.randn_like(x1)
        t0, t1 = self.check_interval(self.train_eps, self.sample_eps)
        B = x1.shape[0]
        if not self.use_lognorm:
            if self.partitial_train is not None and th.rand(1) < self.partial_ratio:
                t = th.rand((B,)) * (self.partitial_train[1] - self.partitial_train[0]) + self.partitial_train[0]
            else:
                t = th.rand((B,)) * (t1 - t0) + t0
        elif not self.shift_lg:
            if self.partitial_train is not None and th.rand(1) < self.partial_ratio:
                t = self.sample_in_range(0, 1, B, range_min=self.partitial_train[0], range_max=self.partitial_train[1])
            else:
                t = self.sample_logit_normal(0, 1, size=B) * (t1 - t0) + t0
        else:
            assert self.partitial_train is None, "Shifted lognormal distribution is not compatible with partial training"
            t = self.sample_logit_normal(shifted_mu, 1, size=B) * (t1 - t0) + t0
        if sp_timesteps is not None:
            t = th.rand((B,)) * (sp_timesteps[1] - sp_timesteps[0]) + sp_timesteps[0]
        # host-drawn t -> device through pinned memory, asynchronously: a pageable .to(device) makes torch synchronise the stream, i.e. the
        # host waits for the whole previous step and the GPU then idles (~1 ms per step) while the next step's first kernels are launched
        if x1.is_cuda and not t.is_cuda:
            t = t.to(x1.dtype).pin_memory().to(x1.device, non_blocking=True)
        else:
            t = t.to(x1)
        return t, x0, x1

    def training_losses(self, model, x1, model_kwargs=None, sp_timesteps=None, shifted_mu=0):
        """transport.py:169-215."""
        model_kwargs = model_kwargs or {}
        t, x0, x1 = self.sample(x1, sp_timesteps, shifted_mu)
        t, xt, ut = self.path_sampler.plan(t, x0, x1)
        if self.dispersive is None:
            out = model(xt, t, **model_kwargs)
            z = None
        else:
            owner = getattr(model, "__self__", model)                       # model may be a bound method
            if not hasattr(owner, "tap_block"):
                raise RuntimeError("ldmae_amd Transport: dispersive needs a model with tap_block (LightningDiT); got " + type(owner).__name__)
            with owner.tap_block(self.dispersive['block']):
                out = model(xt, t, **model_kwargs)
                z = owner.tapped
        assert out.size() == xt.size()
        terms = {'pred': out}
        if z is not None:                                                   # a scalar, on the f32 tap: outside the autocast region
            with th.autocast(device_type="cuda", enabled=False):
                terms['disp_loss'] = _DispersiveFn.apply(z.reshape(z.shape[0], -1), self.dispersive['tau'])
        terms['loss'] = mean_flat((out - ut) ** 2)
        if self.use_cosine_loss:
            terms['cos_loss'] = mean_flat(1 - th.nn.functional.cosine_similarity(out, ut, dim=1))
        return terms

    def get_drift(self):
        """transport.py:217-245, velocity model: the drift of the probability-flow ODE is the model output itself."""
        def body_fn(x, t, model, **kw):
            out = model(x, t, **kw)
            assert out.shape == x.shape, "Output shape from ODE solver must match input shape"
            return out
        return body_fn


class Sampler:
    """transport.py:270-502: the ODE sampler, the SDE sampler and likelihood evaluation."""

    def __init__(self, transport):
        self.transport = transport
        self.drift = transport.get_drift()

    def sample_ode(self, *, sampling_method="dopri5", num_steps=50, atol=1e-6, rtol=1e-3, reverse=False, timestep_shift=0.0):
        drift = (lambda x, t, model, **kw: self.drift(x, th.ones_like(t) * (1 - t), model, **kw)) if reverse else self.drift
        t0, t1 = self.transport.check_interval(self.transport.train_eps, self.transport.sample_eps, sde=False, eval=True,
                                               reverse=reverse, last_step_size=0.0)
        return ode(drift=drift, t0=t0, t1=t1, sampler_type=sampling_method, num_steps=num_steps, atol=atol, rtol=rtol,
                   timestep_shift=timestep_shift).sample

    def sample_sde(self, *, sampling_method="Euler", diffusion_form="SBDM", diffusion_norm=1.0, last_step="Mean", last_step_size=0.04,
                   num_steps=250, seed=0, noise=None, keep_trajectory=True):
        """transport.py:336-396: a function (init, model, **model_kwargs) -> the list of the num_steps states after each step, the last one
        produced by `last_step` at t1 (None / "Mean" / "Tweedie" / "Euler"); with keep_trajectory=False a list holding only that last state.
        Euler-Maruyama or Heun (integrators.sde) under the diffusion coefficient w(t) = path.diffusion(t, diffusion_form, diffusion_norm).

        Where this departs from the reference: the network runs ONCE per drift evaluation (the reference's drift(x, t) + w score(x, t) calls it
        twice; for a velocity model on the linear path the score is affine in (v, x), so the SDE drift is beta v - alpha x, sde_drift_terms);
        every step is one HIP launch with host-computed coefficients; and the noise is a named draw: step k of call number c of the returned
        function draws normal(seed, (c << 32) | k) (Philox4x32-10, generated inside the step kernel), so a sample is a function of
        (init, seed, call index).  fn.calls is that call index: readable and resettable.  noise(k, shape) -> tensor replaces the draw (tests).

        The default form SBDM is infinite at t = 0, and a Transport from create_transport has sample_eps = 0, so t0 = 0: the reference then
        returns non-finite samples; here that combination is refused when the sampler is built."""
        if sampling_method not in SDE_METHODS:
            raise NotImplementedError(f"ldmae_amd Sampler: SDE sampling_method {sampling_method!r} is not supported: 'Euler' or 'Heun'")
        if diffusion_form not in path.DIFFUSION_FORMS:
            raise NotImplementedError(f"ldmae_amd Sampler: diffusion_form {diffusion_form!r} is not supported: one of "
                                      + ", ".join(repr(f) for f in path.DIFFUSION_FORMS))
        if last_step not in (None, "Mean", "Tweedie", "Euler"):
            raise NotImplementedError(f"ldmae_amd Sampler: last_step {last_step!r} is not supported: None, 'Mean', 'Tweedie' or 'Euler'")
        if last_step is None:
            last_step_size = 0.0
        t0, t1 = self.transport.check_interval(self.transport.train_eps, self.transport.sample_eps, diffusion_form=diffusion_form, sde=True,
                                               eval=True, reverse=False, last_step_size=last_step_size)
        if diffusion_form == "SBDM" and not t0:
            raise NotImplementedError("ldmae_amd Sampler: SDE sampling is out of scope for diffusion_form='SBDM' with t0 == 0: the SBDM diffusion "
                                      "(1-t)^2 / t + (1-t) is infinite there and the samples would not be finite.  Build the Transport with "
                                      "sample_eps > 0 (create_transport forces 0 for the velocity model; in the YAML driver set "
                                      "transport.sample_eps), or choose another diffusion_form, e.g. 'sigma' (SURVEY.md 2.1 #7)")

        def w(t):
            return path.diffusion(t, diffusion_form, diffusion_norm)

        _sde = sde(self.drift, w, t0=t0, t1=t1, num_steps=num_steps, sampler_type=sampling_method, seed=seed, noise=noise,
                   keep_trajectory=keep_trajectory)
        # the last step at t1 (f32, as the reference's th.ones * t1): x' = lx x + lv v
        tl, s = float(_sde.t[-1]), float(last_step_size)
        if last_step == "Mean":
            al, be = sde_drift_terms(tl, w(tl))
            last = (_f32(1 - s * al, "1 - s alpha at t1"), _f32(s * be, "s beta at t1"))
        elif last_step == "Tweedie":                       # x / t + (1-t)^2 / t score, score = a v + b x
            a, b = path.score_from_velocity(tl)
            last = (_f32(1 / tl + (1 - tl) ** 2 / tl * b, "the Tweedie x coefficient"), _f32((1 - tl) ** 2 / tl * a, "the Tweedie v coefficient"))
        elif last_step == "Euler":
            last = (1.0, _f32(s, "last_step_size"))
        else:
            last = None

        def _sample(init, model, **model_kwargs):
            from .. import ops
            if not init.is_cuda:
                raise RuntimeError("ldmae_amd sample_sde: the draw and the steps are HIP kernels: the state must be on a HIP device (no CPU "
                                   "fallback); got " + str(init.device))
            _sde.calls = _sample.calls
            xs = _sde.sample(init, model, **model_kwargs)
            _sample.calls = _sde.calls
            x = xs[-1]
            if last is not None:
                with th.no_grad():
                    ts = th.full((x.size(0),), tl, dtype=th.float32, device=x.device)
                    v = self.drift(x, ts, model, **model_kwargs).float().contiguous()
                    x = ops.sde_combine((x, v), last, x if not keep_trajectory else th.empty_like(x))
            if not keep_trajectory:
                return [x]
            xs.append(x)
            assert len(xs) == num_steps, "Samples does not match the number of steps"
            return xs

        _sample.calls = 0
        _sample.sde = _sde
        _sample.options = dict(sampling_method=sampling_method, diffusion_form=diffusion_form, diffusion_norm=diffusion_norm, last_step=last_step,
                               last_step_size=last_step_size, num_steps=num_steps, seed=seed, keep_trajectory=keep_trajectory)
        _sample.last_coefficients = last
        _sample.model_calls = (num_steps - 1) * (2 if sampling_method == "Heun" else 1) + (last is not None)
        return _sample

    def sample_ode_likelihood(self, *, sampling_method="dopri5", num_steps=50, atol=1e-6, rtol=1e-3, seed=0, noise=None):
        """transport.py:445-502: a function (x, model, **model_kwargs) -> (logp, z).  The probability-flow ODE is integrated from data to noise
        (time reversed: t -> 1 - t, state derivative -v) on the augmented state (x, logp); d logp / dt is Hutchinson's estimate eps^T (dv/dx) eps
        of the divergence with a fresh Rademacher eps per drift evaluation, and logp = prior_logp(z) - delta_logp.

        Where this departs from the reference: the network runs ONCE per drift evaluation -- v and the vector-Jacobian product eps^T dv/dx come
        from the same forward (the reference runs it a second time for v) -- and eps is a named draw: ops.rademacher (Philox4x32-10) keyed by
        `seed` with the evaluation index as the counter, so a likelihood is a function of (x, seed).  noise(nfe_index, shape) -> a +-1 tensor
        replaces the draw (tests).  A model with an input-gradient-only backward (LightningDiT.input_grad_only) is evaluated in that mode: no
        parameter gradient is computed."""
        from .. import ops
        calls = [0]

        def _likelihood_drift(state, t, model, **model_kwargs):
            x, _ = state
            idx, calls[0] = calls[0], calls[0] + 1
            eps = noise(idx, x.shape).to(x) if noise is not None else ops.rademacher(x.shape, seed, idx, x.device)
            t = th.ones_like(t) * (1 - t)
            with th.enable_grad():
                xg = x.detach().requires_grad_(True)
                v = self.drift(xg, t, model, **model_kwargs)
                (vjp,) = th.autograd.grad(v, xg, grad_outputs=eps.contiguous())
            return -v.detach(), ops.rowdot(vjp.contiguous(), eps.contiguous())

        t0, t1 = self.transport.check_interval(self.transport.train_eps, self.transport.sample_eps, sde=False, eval=True, reverse=False,
                                               last_step_size=0.0)
        _ode = ode(drift=_likelihood_drift, t0=t0, t1=t1, sampler_type=sampling_method, num_steps=num_steps, atol=atol, rtol=rtol)

        def _sample_fn(x, model, **model_kwargs):
            if not x.is_cuda:
                raise RuntimeError("ldmae_amd likelihood: the probe, its reductions and the solver are HIP kernels: the state must be on a HIP "
                                   "device (no CPU fallback); got " + str(x.device))
            calls[0] = 0
            x = x.float().contiguous()
            owner = getattr(model, "__self__", model)                       # model may be a bound method (forward / forward_with_cfg)
            mode = owner.input_grad_only() if hasattr(owner, "input_grad_only") else contextlib.nullcontext()
            with mode:
                zs, deltas = _ode.sample((x, th.zeros(x.size(0), dtype=th.float32, device=x.device)), model, **model_kwargs)
            z, delta = zs[-1].contiguous(), deltas[-1].contiguous()
            logp = ops.likelihood_finish(ops.rowdot(z), delta, z[0].numel())     # prior_logp(z) - delta_logp in one launch
            return logp, z

        _sample_fn.ode = _ode                                               # nfe / accepted / rejected of the last call
        return _sample_fn
