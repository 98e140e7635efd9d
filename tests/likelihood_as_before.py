"""The code paths tests/test_gpu_likelihood.py pins as unchanged, restated VERBATIM (but for one import statement, marked) as they stood before likelihood evaluation was added: the
backward passes of the three LightningDiT autograd Functions (the input-gradient-only mode must leave the training path's launches alone) and
ode._sample_dopri5 on a plain (non-tuple) state.  The test installs them in place of the current ones and compares bits.  Not a test module."""
import torch
import torch as th

from ldmae_amd import ops
from ldmae_amd.models.lightningdit import _FUSED_QKN_BWD, _dmod_times_w, _dw_into_grad, _qk_layernorm_bwd, _unpad_swiglu_grads      # noqa: F401
from ldmae_amd.transport.integrators import DP_A, DP_C, DP_MID      # noqa: F401


# ----------------------------------------------------------------------------- models/lightningdit.py: _PatchEmbedFn / _DiTBlockFn / _FinalLayerFn .backward
def _patch_embed_backward_as_before(ctx, g):
    tok, w2d = ctx.saved_tensors
    g = g.contiguous()
    dtok = ops.gemm_nt(g, ops.cast_weight(w2d, torch.float32, True, False)[1]) if ctx.needs_input_grad[0] else None
    if not ctx.lowp and g.dtype == torch.float32 and tok.dtype == torch.float32 and ops.thin_ok(g.shape[1], tok.shape[1]):
        dw, db = ops.thin_tn(g, tok)            # weight and bias gradient in ONE pass over the 805-MB gradient
        return dtok, dw, db, None, None, None
    dw = ops.gemm_tn(ops.cast(g, torch.bfloat16), tok) if ctx.lowp else ops.gemm_tn(g, tok)
    return dtok, dw, ops.colsum(g), None, None, None


def _block_backward_as_before(ctx, gout):
    (x2, sc, cos, sin, mod, rstd1, xm1, qkv, q, k, v, o, lse, y1, xmid, rstd2, xm2, h12, hid, y2,
     n1w, qnw, knw, n2w, adaw, WqkvT, WpT, W12T, W3T) = ctx.saved_tensors[:29]
    qk_saved = ctx.saved_tensors[29:] if ctx.qk_ln else None
    B, N, D, H, hd, eps, dtype = ctx.dims
    M = B * N
    # f32 residual-stream gradient.  `inplace` (set by LightningDiT.forward for its own block chain, where a block output
    # feeds only the next block / final layer, whose backward allocates the buffer handed to us): accumulate IN PLACE in
    # that buffer -- no 805 MB copy per block.  Otherwise (a block called on its own, or with hooks tapping its output) the
    # incoming gradient may be shared with another consumer and must not be modified: work on a private copy.
    dx = gout.contiguous().view(M, D)
    if not ctx.inplace and dx.data_ptr() == gout.data_ptr():
        dx = dx.clone()
    chain, idx = ctx.chain, ctx.idx
    # column chunk of each modulation vector in mod / dmod: (shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp), :246; no shifts with wo_shift, :242
    c_sh1, c_s1, c_g1, c_sh2, c_s2, c_g2 = (0, 1, 2, 3, 4, 5) if ctx.nmod == 6 else (None, 0, 1, None, 2, 3)
    col = lambda t_, c_: None if c_ is None else t_[:, c_ * D:(c_ + 1) * D]      # noqa: E731
    s1, g1, s2, g2 = col(mod, c_s1), col(mod, c_g1), col(mod, c_s2), col(mod, c_g2)
    sg = ops.SideGemms(dx.device, enabled=dtype == torch.bfloat16)      # weight gradients: off the critical path
    # ---- MLP branch
    pre = chain.pre.pop(idx, None) if chain is not None else None
    if pre is not None and pre[0] == dx.data_ptr():      # the next member's backward already gated this dx (see _GradChain)
        _, dy2, db3, dmod = pre
    else:
        dmod = chain.dmod(idx, mod) if chain is not None else torch.empty(mod.shape, dtype=mod.dtype, device=mod.device)
        dy2, db3 = ops.gate_bwd(dx, y2, g2, col(dmod, c_g2), N, dtype, with_bias=True)   # bias grads where dy is produced
    qkvw_p, pw_p, w12_p, w3_p = ctx.wparams
    notify = []
    dW3, r = _dw_into_grad(sg, dy2, hid, w3_p, ctx.direct); notify.append((r, w3_p))
    if ctx.swiglu:
        dh12, db12 = ops.gemm_nt_swiglu_bwd(dy2, W3T, h12, with_bias=True)
    else:                            # timm Mlp: fc2's input gradient through the tanh-GELU backward; fc1's bias gradient = its column sums
        dh12 = ops.gelu_tanh_bwd(ops.gemm_nt(dy2, W3T), h12)
        db12 = ops.colsum(dh12)
    dW12, r = _dw_into_grad(sg, dh12, xm2, w12_p, ctx.direct); notify.append((r, w12_p))
    dxm2 = ops.gemm_nt(dh12, W12T)
    # norm2 backward and the attention branch's gate backward in one pass (the updated dx is consumed from registers)
    dn2, dy1, dbp = ops.rmsnorm_modulate_bwd_gate(dxm2, xmid, n2w, s2, rstd2, dx, col(dmod, c_sh2), col(dmod, c_s2),
                                                  y1, g1, col(dmod, c_g1), N, dtype)
    # ---- attention branch
    dWp, r = _dw_into_grad(sg, dy1, o.view(M, D), pw_p, ctx.direct); notify.append((r, pw_p))
    do = ops.gemm_nt(dy1, WpT)
    dqnb = dknb = None
    if qk_saved is not None:         # nn.LayerNorm QK-norm (composed path)
        dq, dk, dv = ops.attention_bwd(q, k, v, o, do, lse, hd ** -0.5)
        dqkv, dqn, dqnb, dkn, dknb, dbqkv = _qk_layernorm_bwd(dq, dk, dv, qk_saved, qnw, knw, cos, sin, B, N, H, hd, dtype)
    elif v is None and hd in (64, 128) and N % 64 == 0 and _FUSED_QKN_BWD:      # QK-norm / RoPE backward inside the attention backward's epilogues: no head-major dq / dk
        dqkv, dqn, dkn, dbqkv = ops.attention_bwd_pv_qknorm(q, k, qkv, o, do, lse, hd ** -0.5, qnw, knw, cos, sin, eps)
    elif v is None:
        dq, dk, dqkv = ops.attention_bwd_pv(q, k, qkv, o, do, lse, hd ** -0.5)          # dv lands in the v slot of dqkv
        dqkv, dqn, dkn, dbqkv = ops.qknorm_rope_bwd(dq, dk, None, qkv, qnw, knw, cos, sin, B, N, H, hd, eps, with_bias=True, dqkv=dqkv)
    else:
        dq, dk, dv = ops.attention_bwd(q, k, v, o, do, lse, hd ** -0.5)
        dqkv, dqn, dkn, dbqkv = ops.qknorm_rope_bwd(dq, dk, dv, qkv, qnw, knw, cos, sin, B, N, H, hd, eps, with_bias=True)
    dqkv = dqkv.view(M, 3 * D)
    dWqkv, r = _dw_into_grad(sg, dqkv, xm1, qkvw_p, ctx.direct); notify.append((r, qkvw_p))
    dxm1 = ops.gemm_nt(dqkv, WqkvT)
    if chain is not None:
        dn1 = chain.norm_bwd(idx, dxm1, x2, n1w, s1, rstd1, dx, col(dmod, c_sh1), col(dmod, c_s1), N, dtype)
    else:
        dn1 = ops.rmsnorm_modulate_bwd(dxm1, x2, n1w, s1, rstd1, dx, col(dmod, c_sh1), col(dmod, c_s1), N)
    # ---- adaLN: per block in f32, or (batched) nothing here -- block 0, the last to run, returns the shared dmod buffer for mod_all
    dmod_all = None
    if ctx.batched_ada:
        dadaw = dadab = dsc = None
        if idx == 0:
            dmod_all = chain.dmod_all
    else:
        dadaw, dadab = ops.gemm_tn(dmod, sc), ops.colsum(dmod)
        dsc = _dmod_times_w(dmod, adaw)
    if ctx.hs is not None:                         # padded SwiGLU hidden: hand autograd the real units' rows / columns
        dW12, db12, dW3 = _unpad_swiglu_grads(dW12, db12, dW3, *ctx.hs)
    sg.join()
    # the eight small gradients of the block (norm weights, biases, QK-norm weights): with `direct`, ONE launch adds them into their .grad
    # views instead of one AccumulateGrad add each
    small = [dn1, dbqkv, dqn, dkn, dbp, dn2, db12, db3, dqnb, dknb]
    if ctx.sparams is not None:
        pairs = [(p_, g_) for p_, g_ in zip(ctx.sparams, small) if p_ is not None]      # use_qknorm=False: no q_norm / k_norm weights
        if all(g_ is not None and p_.grad is not None and p_.grad.dtype == torch.float32 and p_.grad.is_contiguous() and p_.grad.shape == g_.shape
               for p_, g_ in pairs):
            ops.multi_add_([p_.grad for p_, _ in pairs], [g_ for _, g_ in pairs])
            notify.extend((getattr(p_, "_ldmae_grad_ready", None), p_) for p_, _ in pairs)
            dn1 = dbqkv = dqn = dkn = dbp = dn2 = db12 = db3 = dqnb = dknb = None
    for r, p_ in notify:          # gradients written straight into .grad: tell the reducer (no-op without one)
        if r is not None:
            r(p_)
    return (dx.view(B, N, D), dsc, None, None, None, None, None, None, None, None, None, None, dmod_all, None,
            dn1, dWqkv, dbqkv, dqn, dkn, dqnb, dknb, dWp, dbp, dn2, dW12, db12, dW3, db3, dadaw, dadab)


def _final_layer_backward_as_before(ctx, gout):
    x2, sc, mod, rstd, xf, nw, lw, adaw = ctx.saved_tensors
    B, N, D, dtype = ctx.dims
    M = B * N
    g = gout.contiguous().view(M, -1)
    ga = ops.cast(g, dtype)
    dlw, dlb = ops.gemm_tn(ga, xf), ops.colsum(g)
    if g.dtype == torch.float32 and ops.thin_ok(lw.shape[1], lw.shape[0]):                        # K = p*p*C = 16 / 32: ldmae_thin_nt
        dxf = ops.thin_nt(g, lw.float().t().contiguous(), out_dtype=dtype)
    else:
        dxf = ops.gemm_nt(g, ops.cast_weight(lw, torch.float32, True, False)[1], out_dtype=dtype)     # f32 MFMA
    dx = torch.empty(M, D, dtype=torch.float32, device=g.device)     # written, not accumulated into: no 805 MB memset + read
    dmod = torch.empty_like(mod)
    if ctx.chain is not None:
        dnw = ctx.chain.norm_bwd(ctx.idx, dxf, x2, nw, mod[:, D:], rstd, dx, dmod[:, :D], dmod[:, D:], N, dtype, accumulate=False)
    else:
        dnw = ops.rmsnorm_modulate_bwd(dxf, x2, nw, mod[:, D:], rstd, dx, dmod[:, :D], dmod[:, D:], N, accumulate=False)
    dadaw, dadab = ops.gemm_tn(dmod, sc), ops.colsum(dmod)
    dsc = _dmod_times_w(dmod, adaw)
    return dx.view(B, N, D), dsc, None, None, None, None, dnw, dlw, dlb, dadaw, dadab



# ----------------------------------------------------------------------------- transport/integrators.py: ode._sample_dopri5
def _sample_dopri5_as_before(self, x, model, **model_kwargs):
    """Adaptive Dormand-Prince 5(4) with FSAL from t[0] to t[-1], controlled as torchdiffeq controls it: the error ratio is the RMS over the
    WHOLE state tensor (all samples, both CFG halves) of err / (atol + rtol max(|y0|, |y1|)); a step is accepted when it is <= 1; the next
    step is h min(10, max(0.9 / ratio^(1/5), 1 if accepted else 0.2)); the first step comes from the Hairer-Norsett-Wanner rule under the
    same norm.  The trajectory at the grid points is the quartic interpolant of the accepted step that covers them.  A step is never clipped
    to a grid point: the last one may pass t[-1] (the result there is interpolated), so the model IS evaluated slightly beyond t[-1], as
    under the reference.  Sets self.nfe / accepted / rejected.

    Everything between two model evaluations is one HIP launch (ops.rk_stage / dopri5_finish / dopri5_advance / dopri5_interp); t, h and
    the ratio stay on the device and the host reads one 6-float record per attempted step (the only synchronisation of the solver)."""
    import numpy as np
    from ldmae_amd import ops                                          # the one changed line: the original is a relative import
    if not x.is_cuda:
        raise RuntimeError("ldmae_amd dopri5: the solver's kernels need the state on a HIP device (no CPU fallback); got " + str(x.device))
    grid = [float(v) for v in self.t.to(th.float32)]
    shape, n, dev = x.shape, x.numel(), x.device
    ld = ops.ode_slab_ld(n)
    traj = th.empty((len(grid),) + tuple(shape), dtype=th.float32, device=dev)
    traj[0].copy_(x)
    k = th.empty(7, ld, dtype=th.float32, device=dev)
    ybuf = th.empty(4, ld, dtype=th.float32, device=dev)
    y, y1, ytmp, ymid = (ybuf[i, :n] for i in range(4))
    y.copy_(x.reshape(-1))
    partial = th.empty(ops.ode_partials(n), dtype=th.float32, device=dev)
    # device scalars: t, h, ratio, the constant 1, the status record of dopri5_advance (6), the norms of the starting-step rule (4)
    st = th.tensor([grid[0], 0.0, 0.0, 1.0] + [0.0] * 10, dtype=th.float32, device=dev)
    t_dev, h_dev, ratio_dev, one_dev, status, d_dev = st[0:1], st[1:2], st[2:3], st[3:4], st[4:10], st[10:14]
    tvec = th.full((shape[0],), grid[0], dtype=th.float32, device=dev)
    self.nfe = self.accepted = self.rejected = 0

    def f(yin, slot):
        out = self.drift(yin.view(shape), tvec, model, **model_kwargs)
        k[slot, :n].view(shape).copy_(out)
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
    return traj
