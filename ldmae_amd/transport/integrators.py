"""ODE integrators on the sampler's shifted grid (reference: LDMAE/transport/integrators.py:77-125, which hands `sampler_type` to
torchdiffeq.odeint).  No torchdiffeq here: the fixed-step solvers (euler / heun / midpoint) are written out, and the adaptive `dopri5` follows
torchdiffeq's published algorithm (rk_common.py / dopri5.py) with its own arithmetic in HIP kernels (csrc/ode.hip)."""
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
