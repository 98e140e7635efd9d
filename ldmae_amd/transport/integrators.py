"""ODE integrators on the sampler's shifted grid (reference: LDMAE/transport/integrators.py:77-125, which hands `sampler_type` to
torchdiffeq.odeint).  No torchdiffeq here: the fixed-step solvers (euler / heun / midpoint) are written out, and the adaptive `dopri5` follows
torchdiffeq's published algorithm (rk_common.py / dopri5.py) with its own arithmetic in HIP kernels (csrc/ode.hip).  The SDE integrator (class
`sde`, reference integrators.py:8-75: Euler-Maruyama / Heun) is at the end of the file: one HIP launch between two model evaluations."""
import torch as th


def shifted_grid(t0, t1, num_steps, timestep_shift):
    """linspace, then t -> s t / (1 + (s-1) t) when s > 0 (integrators.py:92-101)."""
    t = th.linspace(t0, t1, num_steps)
    if timestep_shift > 0:
        t = th.tensor([(timestep_shift * tn) / (1 + (timestep_shift - 1) * tn) for tn in t])
    return t


METHODS = ("euler", "heun", "midpoint", "dopri5")

# Dormand-Prince 5(4) (Dormand & Prince 1980; the constants torchdiffeq's dopri5.py uses, Shampine's dense-output midpoint weights included)
DP_C = (0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0)
DP_A = ((),
        (1 / 5,),
        (3 / 40, 9 / 40),
        (44 / 45, -56 / 15, 32 / 9),
        (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
        (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656),
        (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84))
DP_B = (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0.0)
DP_E = (35 / 384 - 1951 / 21600, 0.0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720, -2187 / 6784 + 12231 / 42400, 11 / 84 - 649 / 6300,
        -1 / 60)
DP_MID = (6025192743 / 30085553152 / 2, 0.0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2, 187940372067 / 1594534317056 / 2,
          -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2)
DP_SAFETY, DP_IFACTOR, DP_DFACTOR, DP_ORDER = 0.9, 10.0, 0.2, 5


class ode:
    def __init__(self, drift, *, t0, t1, sampler_type, num_steps, atol, rtol, timestep_shift=0.0, max_num_steps=2 ** 31 - 1):
        assert t0 < t1, "ODE sampler has to be in forward time"
        self.drift = drift
        self.t = shifted_grid(t0, t1, num_steps, timestep_shift)
        self.atol, self.rtol = atol, rtol
        self.sampler_type = sampler_type.lower()
        if self.sampler_type not in METHODS:
            raise NotImplementedError(f"ldmae_amd: ODE solvers euler / heun / midpoint / dopri5 only, got {sampler_type}")
        self.max_num_steps = max_num_steps
        self.nfe = self.accepted = self.rejected = 0            # set by sample() (dopri5)

    def sample(self, x, model, **model_kwargs):
        """Returns the stacked trajectory [len(t), ...] like odeint; callers take [-1] (inference.py:287).  x may be the tuple (x, logp) of
        likelihood evaluation (logp [B] f32): the drift then maps ((x, logp), t, model) to the pair of derivatives, and the result is the
        tuple of the two stacked trajectories, as odeint returns it."""
        if isinstance(x, (tuple, list)):
            return self._sample_augmented(tuple(x), model, **model_kwargs)
        if self.sampler_type == "dopri5":
            return self._sample_dopri5(x, model, **model_kwargs)
        t = self.t.to(x.device)

        def f(tk, xk):
            return self.drift(xk, th.ones(xk.size(0), device=xk.device) * tk, model, **model_kwargs)

        xs = [x]
        with th.no_grad():
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
        return th.stack(xs)

    def _sample_augmented(self, state, model, **model_kwargs):
        """The tuple state (x, logp).  torchdiffeq flattens the tuple into ONE vector of n + B elements, with one tolerance per element and the
        RMS norm over that whole vector; so does this: dopri5 runs on slab rows of n + B floats (x first, logp behind it), with the kernels and
        the controller of the plain state.  The fixed-step methods apply their update to both members."""
        if len(state) != 2:
            raise ValueError("ode.sample: a tuple state is the pair (x, logp)")
        x, logp = state
        if logp.shape != (x.shape[0],) or logp.dtype != th.float32 or x.dtype != th.float32:
            raise ValueError(f"ode.sample: (x, logp) needs f32 x and f32 logp of shape [{x.shape[0]}], got {x.dtype} and {tuple(logp.shape)} {logp.dtype}")
        if self.sampler_type == "dopri5":
            return self._sample_dopri5(x, model, logp=logp, **model_kwargs)
        t = self.t.to(x.device)

        def f(tk, s):
            return self.drift(s, th.ones(x.size(0), device=x.device) * tk, model, **model_kwargs)

        def step(s, c, d):
            return tuple(a + c * b for a, b in zip(s, d))

        s, out = (x, logp), [(x, logp)]
        with th.no_grad():
            for k in range(len(t) - 1):
                dt = t[k + 1] - t[k]
                if self.sampler_type == "euler":
                    s = step(s, dt, f(t[k], s))
                elif self.sampler_type == "midpoint":
                    s = step(s, dt, f(t[k] + dt / 2, step(s, dt / 2, f(t[k], s))))
                else:
                    k1 = f(t[k], s)
                    k2 = f(t[k + 1], step(s, dt, k1))
                    s = step(s, dt / 2, tuple(a + b for a, b in zip(k1, k2)))
                out.append(s)
        return th.stack([o[0] for o in out]), th.stack([o[1] for o in out])

    def _sample_dopri5(self, x, model, logp=None, **model_kwargs):
        """Adaptive Dormand-Prince 5(4) with FSAL from t[0] to t[-1], controlled as torchdiffeq controls it: the error ratio is the RMS over the
        WHOLE state tensor (all samples, both CFG halves) of err / (atol + rtol max(|y0|, |y1|)); a step is accepted when it is <= 1; the next
        step is h min(10, max(0.9 / ratio^(1/5), 1 if accepted else 0.2)); the first step comes from the Hairer-Norsett-Wanner rule under the
        same norm.  The trajectory at the grid points is the quartic interpolant of the accepted step that covers them.  A step is never clipped
        to a grid point: the last one may pass t[-1] (the result there is interpolated), so the model IS evaluated slightly beyond t[-1], as
        under the reference.  Sets self.nfe / accepted / rejected.

        Everything between two model evaluations is one HIP launch (ops.rk_stage / dopri5_finish / dopri5_advance / dopri5_interp); t, h and
        the ratio stay on the device and the host reads one 6-float record per attempted step (the only synchronisation of the solver).

        logp (the augmented state of _sample_augmented): the state vector is x flattened followed by logp, n = x.numel() + B; the drift is handed
        (x, logp) and its two results go to k[s, :x.numel()] and k[s, x.numel():n].  Returns the pair of trajectories."""
        import numpy as np
        from .. import ops
        if not x.is_cuda:
            raise RuntimeError("ldmae_amd dopri5: the solver's kernels need the state on a HIP device (no CPU fallback); got " + str(x.device))
        grid = [float(v) for v in self.t.to(th.float32)]
        shape, nx, dev = x.shape, x.numel(), x.device
        n = nx if logp is None else nx + logp.numel()
        ld = ops.ode_slab_ld(n)
        traj = th.empty((len(grid),) + (tuple(shape) if logp is None else (n,)), dtype=th.float32, device=dev)
        if logp is None:
            traj[0].copy_(x)
        k = th.empty(7, ld, dtype=th.float32, device=dev)
        ybuf = th.empty(4, ld, dtype=th.float32, device=dev)
        y, y1, ytmp, ymid = (ybuf[i, :n] for i in range(4))
        if logp is None:
            y.copy_(x.reshape(-1))
        else:
            y[:nx].copy_(x.reshape(-1))
            y[nx:].copy_(logp)
            traj[0].copy_(y)
        partial = th.empty(ops.ode_partials(n), dtype=th.float32, device=dev)
        # device scalars: t, h, ratio, the constant 1, the status record of dopri5_advance (6), the norms of the starting-step rule (4)
        st = th.tensor([grid[0], 0.0, 0.0, 1.0] + [0.0] * 10, dtype=th.float32, device=dev)
        t_dev, h_dev, ratio_dev, one_dev, status, d_dev = st[0:1], st[1:2], st[2:3], st[3:4], st[4:10], st[10:14]
        tvec = th.full((shape[0],), grid[0], dtype=th.float32, device=dev)
        self.nfe = self.accepted = self.rejected = 0

        def f(yin, slot):
            if logp is None:
                out = self.drift(yin.view(shape), tvec, model, **model_kwargs)
                k[slot, :n].view(shape).copy_(out)
            else:
                dx, dlogp = self.drift((yin[:nx].view(shape), yin[nx:]), tvec, model, **model_kwargs)
                k[slot, :nx].view(shape).copy_(dx)
                k[slot, nx:n].copy_(dlogp)
            self.nfe += 1

        with th.no_grad():
            f(y, 0)
            # starting step (Hairer, Norsett & Wanner II.4): d0 = |y0|, d1 = |f0|, one trial Euler step of h0, d2 = |f1 - f0| / h0
            ops.rms_norm_scaled(y, None, self.atol, self.rtol, partial, d_dev[0:1])
            ops.rms_norm_scaled(k[0, :n], y, self.atol, self.rtol, partial, d_dev[1:2])
            ops.dopri5_initial_step(d_dev, 0, h_dev)
            ops.rk_stage(y, k, (1.0,), h_dev, ytmp, t_dev, 1.0, tvec)
            f(ytmp, 1)
            ops.rk_stage(k[1, :n], k, (-1.0,), one_dev, ymid)                       # f1 - f0, exactly
            ops.rms_norm_scaled(ymid, y, self.atol, self.rtol, partial, d_dev[2:3])
            ops.dopri5_initial_step(d_dev, 1, h_dev)
            self.nfe_initial = 1
            t_end, fsal_pending, have_mid = grid[0], False, False
            for i in range(1, len(grid)):
                steps = 0
                while grid[i] > t_end:
                    if steps >= self.max_num_steps:
                        raise RuntimeError(f"dopri5: max_num_steps ({self.max_num_steps}) exceeded before t = {grid[i]}")
                    if fsal_pending:                                                   # first same as last: k7 of the accepted step
                        k[0].copy_(k[6])
                        fsal_pending = False
                    for s in range(1, 7):
                        ops.rk_stage(y, k, DP_A[s], h_dev, ytmp, t_dev, DP_C[s], tvec)
                        f(ytmp, s)
                    ops.dopri5_finish(y, k, h_dev, self.atol, self.rtol, y1, partial, ratio_dev)
                    ops.dopri5_advance(ratio_dev, h_dev, t_dev, status)
                    acc, _, t_was, h_was, t_now, _ = status.tolist()                   # the one synchronising read of the step
                    if not np.float32(t_was) + np.float32(h_was) > np.float32(t_was):
                        raise RuntimeError(f"dopri5: underflow in the step size (t = {t_was}, h = {h_was})")
                    steps += 1
                    if acc:
                        self.accepted += 1
                        y, y1 = y1, y                                                   # y: the new state, y1: the step's start
                        t_end, fsal_pending, have_mid = t_now, True, False
                    else:
                        self.rejected += 1
                if not have_mid:                                                        # status[2], status[3]: start and size of the accepted step
                    ops.rk_stage(y1, k, DP_MID, status[3:4], ymid)
                    have_mid = True
                dst = traj[i].view(-1) if n % 4 == 0 else ytmp                         # the kernel stores 16 bytes at a time: aligned rows only
                ops.dopri5_interp(y1, y, ymid, k, status[3:4], status[2:3], grid[i], dst)
                if n % 4:
                    traj[i].view(-1).copy_(dst)
        if logp is not None:
            return traj[:, :nx].reshape((len(grid),) + tuple(shape)), traj[:, nx:].contiguous()
        return traj


SDE_METHODS = ("Euler", "Heun")


def _f32(v, what):
    """One rounding of a host f64 coefficient to f32, as a Python float; a coefficient that is not finite is an error, not a sample."""
    import numpy as np
    with np.errstate(over="ignore"):
        r = float(np.float32(v))
    if not np.isfinite(r):
        raise ValueError(f"ldmae_amd sde: the coefficient {what} is not finite ({v}); the grid touches a singular point of the diffusion form")
    return r


def sde_drift_terms(t, w):
    """(alpha, beta) of the reference's SDE drift v + w score = beta v - alpha x for a velocity model on the linear path: the score is
    (t v - x) / var with var = (1-t)^2 + t (1-t) (path.score_from_velocity), so alpha = w / var and beta = 1 + w t / var.  Host f64."""
    from .path import score_from_velocity
    a, b = score_from_velocity(t)
    return -w * b, 1 + w * a


class sde:
    """Euler-Maruyama / Heun on the fixed grid linspace(t0, t1, num_steps) (reference: integrators.py:8-75) for a velocity model on the linear
    path.  The reference's constructor keywords; where it takes the SDE drift and the diffusion as tensor functions, this takes

        drift      (x, t, model, **kw) -> v, the model's velocity (Transport.get_drift()): ONE model call per drift evaluation,
        diffusion  t -> w(t), the diffusion coefficient at one time on the host (f64),

    and builds the SDE drift beta v - alpha x from them (sde_drift_terms).  Every step is then a fixed linear combination of at most four
    tensors plus a multiple of a standard-normal draw: one ops.sde_combine launch between two model evaluations, with coefficients computed
    here in f64 from the f32 grid values, rounded once to f32 and passed by value.  The loop reads nothing back from the device.

    seed / noise / keep_trajectory: the draw of step k of call number c is normal(seed, (c << 32) | k), generated inside the kernel;
    noise(k, shape) -> tensor replaces it; keep_trajectory=False updates two buffers in place and returns only the last state."""

    def __init__(self, drift, diffusion, *, t0, t1, num_steps, sampler_type, seed=0, noise=None, keep_trajectory=True):
        assert t0 < t1, "SDE sampler has to be in forward time"
        if sampler_type not in SDE_METHODS:
            raise NotImplementedError(f"ldmae_amd: SDE samplers Euler / Heun only, got {sampler_type!r}")
        if num_steps < 2:
            raise ValueError(f"ldmae_amd sde: num_steps must be at least 2, got {num_steps}")
        self.num_timesteps = num_steps
        self.t = th.linspace(t0, t1, num_steps)
        self.dt = self.t[1] - self.t[0]
        self.drift, self.diffusion, self.sampler_type = drift, diffusion, sampler_type
        self.seed, self.noise, self.keep_trajectory = seed, noise, keep_trajectory
        self.calls = 0
        self.plan = [self.step_coefficients(k) for k in range(num_steps - 1)]       # raises here, not mid-loop, on a singular grid

    def step_coefficients(self, k):
        """The f32 coefficients of step k as a dict.  Euler: x' = cx x + cv v + cz z.  Heun: xhat = x + cz z; xp = px xhat + pv v1;
        x' = cx xhat + cv1 v1 + cxp xp + cv2 v2, with v1 = model(xhat, t), v2 = model(xp, t2), t2 = t + dt in f32 as the reference adds it."""
        import math
        import numpy as np
        t, dt = float(self.t[k]), float(self.dt)
        w = self.diffusion(t)
        al, be = sde_drift_terms(t, w)
        c = {"t": t, "t_next": float(self.t[k + 1]), "cz": _f32(math.sqrt(2 * w * dt), f"sqrt(2 w dt) at t = {t}")}
        if self.sampler_type == "Euler":
            c.update(cx=_f32(1 - dt * al, f"1 - dt alpha at t = {t}"), cv=_f32(dt * be, f"dt beta at t = {t}"))
            return c
        t2 = float(np.float32(t) + np.float32(dt))
        al2, be2 = sde_drift_terms(t2, self.diffusion(t2))
        c.update(t2=t2, px=_f32(1 - dt * al, f"1 - dt alpha at t = {t}"), pv=_f32(dt * be, f"dt beta at t = {t}"),
                 cx=_f32(1 - dt / 2 * al, f"1 - dt/2 alpha at t = {t}"), cv1=_f32(dt / 2 * be, f"dt/2 beta at t = {t}"),
                 cxp=_f32(-dt / 2 * al2, f"dt/2 alpha at t = {t2}"), cv2=_f32(dt / 2 * be2, f"dt/2 beta at t = {t2}"))
        return c

    def sample(self, init, model, **model_kwargs):
        """The num_steps - 1 states after each step, as a list (the reference's return value), or [last state] with keep_trajectory=False."""
        from .. import ops
        if not init.is_cuda:
            raise RuntimeError("ldmae_amd sde: the draw and the step are HIP kernels: the state must be on a HIP device (no CPU fallback); got "
                               + str(init.device))
        call, self.calls = self.calls, self.calls + 1
        shape, dev = init.shape, init.device
        x = init.float().contiguous()
        if not self.keep_trajectory:
            x = x.clone() if x.data_ptr() == init.data_ptr() else x              # updated in place below: never the caller's tensor
        tvec = th.full((shape[0],), self.plan[0]["t"], dtype=th.float32, device=dev)
        heun = self.sampler_type == "Heun"
        xp = th.empty_like(x) if heun else None
        xhat = th.empty_like(x) if heun and self.keep_trajectory else None

        def f(xin):
            return self.drift(xin, tvec, model, **model_kwargs).float().contiguous()

        def draw(k):
            """Keyword arguments of the noise term of step k: a given tensor, or the (seed, counter) of the inline draw."""
            if self.noise is not None:
                z = self.noise(k, shape).to(device=dev, dtype=th.float32).contiguous()
                if z.shape != shape:
                    raise ValueError(f"ldmae_amd sde: noise({k}, {tuple(shape)}) returned shape {tuple(z.shape)}")
                return {"z": z}
            return {"seed": self.seed, "counter": (call << 32) | k}

        samples = []
        with th.no_grad():
            for k, c in enumerate(self.plan):
                out = th.empty_like(x) if self.keep_trajectory else x
                if not heun:
                    v = f(x)
                    ops.sde_combine((x, v), (c["cx"], c["cv"]), out, noise_coef=c["cz"], t_next=c["t_next"], t_out=tvec, **draw(k))
                else:
                    xh = xhat if self.keep_trajectory else x
                    ops.sde_combine((x,), (1.0,), xh, noise_coef=c["cz"], **draw(k))
                    v1 = f(xh)
                    ops.sde_combine((xh, v1), (c["px"], c["pv"]), xp, t_next=c["t2"], t_out=tvec)
                    v2 = f(xp)
                    ops.sde_combine((xh, v1, xp, v2), (c["cx"], c["cv1"], c["cxp"], c["cv2"]), out, t_next=c["t_next"], t_out=tvec)
                x = out
                if self.keep_trajectory:
                    samples.append(x)
        return samples if self.keep_trajectory else [x]
