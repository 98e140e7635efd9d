"""Likelihood evaluation on the GPU: the Rademacher probe and the row reductions of csrc/ode.hip, the augmented state (x, logp) through the
solvers, the input-gradient-only backward of the LightningDiT, and Sampler.sample_ode_likelihood / the command line end to end.

Bounds.  u = 2^-24.
rowdot: a term a_j b_j is rounded into its thread's fma chain (at most 16 links), then passes the block sum (6 butterfly steps + 2) and the fold
(ceil(chunks / 256) links in a thread, 6 + 2 in the block): k = 16 + 8 + ceil(chunks / 256) + 8 roundings at most, each relative to a partial sum
bounded by sum |a_j b_j|: |got - f64| <= gamma_k sum |a b|, gamma_k = k u / (1 - k u).
Linear field (test_tuple_state_linear_field): an accepted step has an error estimate of RMS <= 1 in units of atol + rtol max(|y0|, |y1|) over the
N = n + B elements of the flattened state, so no element's estimate exceeds sqrt(N) (atol + rtol max|y|); the estimate is that of the embedded 4th
order solution, which bounds the propagated 5th order one for steps in the asymptotic range (h ||A|| < 1 here).  Local errors of `accepted` steps
add up, each amplified over the rest of the unit interval by at most exp(||A||_inf) (x' = -x A^T; the logp row has a constant derivative and is
amplified by 1): |global error| <= accepted sqrt(N) (atol + rtol max|y|) exp(||A||_inf).  The interpolation to t = 1 inside the last step is of
the same order and inside the same estimate (the trajectory is the quartic of the accepted step).  f32 rounding of the
state (a few u |y| per stage) is four orders below rtol = 1e-3 and is not added."""
import copy
import json
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


# ----------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 1024, 1025, 4100])
def test_rademacher_is_the_numpy_restatement(n):
    from ldmae_amd import ops
    from ldmae_amd.transport import probe
    draws = {}
    for seed in (0, 0x123456789ABCDEF):
        for counter in (0, 7):
            got = ops.rademacher((n,), seed, counter, "cuda").cpu().numpy()
            want = probe.rademacher(n, seed, counter)
            assert got.dtype == np.float32 and np.array_equal(got, want), (n, seed, counter)
            assert set(np.unique(got)) <= {-1.0, 1.0}
            draws[(seed, counter)] = got
    if n >= 1023:                                                    # 2^-1023 that two independent draws agree everywhere
        assert not np.array_equal(draws[(0, 0)], draws[(0, 7)]) and not np.array_equal(draws[(0, 0)], draws[(0x123456789ABCDEF, 0)])
    # a destination that is only 4-byte aligned takes the element-store path: the same signs
    buf = torch.zeros(n + 2, device="cuda")
    from ldmae_amd._lib import call, ptr, stream
    call("ldmae_rademacher_f32", ptr(buf[1:]), n, 0, 7, stream())
    assert np.array_equal(buf[1:n + 1].cpu().numpy(), draws[(0, 7)]) and float(buf[0]) == 0 and float(buf[n + 1]) == 0


@pytest.mark.parametrize("B,m", [(1, 1), (2, 3), (3, 1024), (2, 4097), (5, 16 * 8 * 8)])
@pytest.mark.parametrize("offset", [0, 1])
def test_rowdot_against_f64(B, m, offset):
    """offset 1: the base is 4 bytes past a 16-byte boundary; (2, 3) and (2, 4097): the second row starts off the boundary in any case."""
    from ldmae_amd import ops
    g = torch.Generator().manual_seed(100 * B + m)
    a = torch.randn(B * m + offset, generator=g).cuda()[offset:].view(B, m)
    b = torch.randn(B * m + offset, generator=g).cuda()[offset:].view(B, m)
    chunks = -(-m // 4096)
    k = 16 + 8 + -(-chunks // 256) + 8
    gamma = k * U / (1 - k * U)
    for x, y in ((a, b), (a, None)):
        got = ops.rowdot(x, y)
        again = ops.rowdot(x, y)
        y = x if y is None else y
        ref = (x.double() * y.double()).sum(1).cpu()
        bound = gamma * (x.double() * y.double()).abs().sum(1).cpu()
        err = (got.double().cpu() - ref).abs()
        print(f"rowdot B={B} m={m} offset={offset}: worst {float((err / bound).max()):.3f} of the bound")
        assert got.shape == (B,) and (err <= bound).all()
        assert torch.equal(got, again)


def test_likelihood_finish_is_the_f32_formula():
    from ldmae_amd import ops
    g = torch.Generator().manual_seed(5)
    s, d = (torch.rand(7, generator=g) * 2000).cuda(), torch.randn(7, generator=g).cuda()
    c = torch.tensor(-1024 / 2.0 * math.log(2 * math.pi), dtype=torch.float32).cuda()
    assert torch.equal(ops.likelihood_finish(s, d, 1024), (c - s / 2.0) - d)


# ----------------------------------------------------------------------------- solver: the plain state is untouched
def test_plain_state_solvers_give_the_bits_of_the_earlier_code():
    """tests/test_gpu_ode_dopri5.py's first case (x' = -x + sin 5t, rtol 1e-3): dopri5 against ode._sample_dopri5 as it stood before the tuple
    state (tests/likelihood_as_before.py), the fixed-step methods against that file's loop."""
    import likelihood_as_before as before
    import test_gpu_ode_dopri5 as G
    from ldmae_amd.transport.integrators import ode
    rtol, atol = R.CASES[0]
    drift = lambda x, t, model, **kw: model(x, t)      # noqa: E731
    x0 = torch.from_numpy(R.initial_state("sin")).cuda()
    f = G._torch_drift("sin")
    o = ode(drift, t0=0, t1=1, sampler_type="dopri5", num_steps=11, atol=atol, rtol=rtol, timestep_shift=0.3)
    now = o.sample(x0, f)
    stats = (o.nfe, o.accepted, o.rejected)
    was = before._sample_dopri5_as_before(o, x0, f)
    assert torch.equal(now, was) and stats == (o.nfe, o.accepted, o.rejected)
    for method in ("euler", "heun", "midpoint"):
        s = ode(drift, t0=0, t1=1, sampler_type=method, num_steps=11, atol=atol, rtol=rtol, timestep_shift=0.3)
        assert torch.equal(s.sample(x0, f), G._sample_as_before(s, x0, f)), method


# ----------------------------------------------------------------------------- solver: the tuple state on a linear field
def _matrix6():
    m = np.random.RandomState(3).standard_normal((6, 6))
    return (0.3 * m / np.abs(m).sum(1).max()).astype(np.float32)          # ||A||_inf = 0.3


class _Linear(torch.nn.Module):
    """v(x, t) = x A^T: divergence tr(A), Jacobian A for every x and t."""

    def __init__(self):
        super().__init__()
        self.register_buffer("a", torch.from_numpy(_matrix6()))

    def forward(self, x, t):
        return x @ self.a.t()


@pytest.mark.parametrize("method", ["dopri5", "heun"])
def test_tuple_state_linear_field(method):
    from scipy.linalg import expm
    from ldmae_amd.transport import Sampler, create_transport
    A = _matrix6().astype(np.float64)
    model = _Linear().cuda()
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(3, 6, generator=g) + 2.0).cuda()
    eps = (torch.randint(0, 2, (3, 6), generator=g).float() * 2 - 1).cuda()
    seen = []

    def noise(i, shape):
        seen.append(i)
        return eps

    atol, rtol = 1e-6, 1e-3
    fn = Sampler(create_transport()).sample_ode_likelihood(sampling_method=method, num_steps=5, atol=atol, rtol=rtol, noise=noise)
    logp, z = fn(x, model)
    o = fn.ode
    E, X = eps.double().cpu().numpy(), x.double().cpu().numpy()
    quad = np.einsum("bi,ij,bj->b", E, A, E)                          # eps^T A eps, constant in time: its integral over [0, 1]
    z_ref = X @ expm(-A).T
    m = 6
    delta = -(logp.double().cpu().numpy() - (-m / 2 * math.log(2 * math.pi) - (z.double().cpu().numpy() ** 2).sum(1) / 2))
    assert seen == list(range(len(seen))) and logp.shape == (3,) and z.shape == (3, 6)
    if method == "dopri5":
        assert len(seen) == o.nfe and o.accepted >= 1
        N = 3 * 6 + 3
        ymax = max(np.abs(X).max() * math.exp(0.3), np.abs(quad).max())
        bound = o.accepted * math.sqrt(N) * (atol + rtol * ymax) * math.exp(0.3)      # see the module docstring
    else:                                                             # Heun, 4 steps of 1/4: local error h^3 / 6 |A^3 x| per step, amplified as above; exact on logp
        bound = 4 * (0.25 ** 3) / 6 * (0.3 ** 3) * np.abs(X).max() * math.exp(0.3) * math.exp(0.3) + 64 * U * np.abs(X).max()
    ez, ed = np.abs(z.double().cpu().numpy() - z_ref).max(), np.abs(delta - quad).max()
    print(f"{method}: nfe {o.nfe} accepted {o.accepted} rejected {o.rejected}; |z - expm(-A) x| {ez:.3e}, |delta - eps^T A eps| {ed:.3e}, bound {bound:.3e}")
    assert ez <= bound and ed <= bound + 16 * U * (m / 2 * math.log(2 * math.pi) + (z_ref ** 2).sum(1).max())


def test_hutchinson_estimate_covers_the_trace():
    """256 seeded draws (one Euler step of a batch of 256: delta_logp[b] = eps_b^T A eps_b): the mean within 4 standard errors of tr(A)."""
    from ldmae_amd.transport import Sampler, create_transport
    model = _Linear().cuda()
    x = torch.ones(256, 6).cuda()
    fn = Sampler(create_transport()).sample_ode_likelihood(sampling_method="euler", num_steps=2, seed=11)
    logp, z = fn(x, model)
    est = -(logp.double() - (-3 * math.log(2 * math.pi) - (z.double() ** 2).sum(1) / 2)).cpu().numpy()
    tr = float(np.trace(_matrix6().astype(np.float64)))
    se = est.std(ddof=1) / math.sqrt(256)
    print(f"Hutchinson: mean {est.mean():.5f} +- {se:.5f}, tr(A) = {tr:.5f}")
    assert se > 0 and abs(est.mean() - tr) <= 4 * se


# ----------------------------------------------------------------------------- the LightningDiT
def _dit(zero_final=False):
    """The smallest configuration that runs every branch: depth 2, hidden 128, 2 heads of 64 (the fused QK-norm attention backward), 64 tokens of
    16 channels, a SwiGLU hidden size off the 128 grid (341: the padded path)."""
    from ldmae_amd.models.lightningdit import LightningDiT
    torch.manual_seed(0)
    m = LightningDiT(input_size=8, patch_size=1, in_channels=16, hidden_size=128, depth=2, num_heads=2, num_classes=10, use_qknorm=True,
                     use_swiglu=True, use_rope=True, use_rmsnorm=True)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                                            # the zero-initialised adaLN / final layer would hide everything
        for n, p in m.named_parameters():
            if "adaLN_modulation" in n or (n.startswith("final_layer.linear") and not zero_final):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return m.cuda().eval()


def _inputs(B, seed=2):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 16, 8, 8, generator=g).cuda(), torch.rand(B, generator=g).cuda(), torch.randint(0, 10, (B,), generator=g).cuda(),
            torch.randn(B, 16, 8, 8, generator=g).cuda())


def _call(m, how, x, t, y):
    if how == "forward":
        return m(x, t, y)
    return m.forward_with_cfg(x, t, torch.cat([y[:len(y) // 2], torch.full_like(y[:len(y) // 2], 10)]), 2.0, True, 0.1)


@pytest.mark.parametrize("how", ["forward", "forward_with_cfg"])
@pytest.mark.parametrize("prec,B", [("f32", 2), ("bf16", 2), ("bf16", 8)])
def test_input_only_backward_gives_the_bits_of_the_full_backward(how, prec, B):
    """B = 8 under bf16: the batched adaLN GEMM (B = 2 keeps the per-block f32 one)."""
    from ldmae_amd import ops
    m = _dit()
    B = B * 2 if how == "forward_with_cfg" else B
    x, t, y, g = _inputs(B)
    ac = lambda: torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec == "bf16")      # noqa: E731
    xa = x.clone().requires_grad_(True)
    with ac():
        out = _call(m, how, xa, t, y)
    out.backward(g)
    assert all(p.grad is not None for n, p in m.named_parameters() if p.requires_grad and "y_embedder" not in n and "t_embedder" not in n)
    for frozen in (False, True):
        m.zero_grad(set_to_none=True)
        m.requires_grad_(not frozen)
        m.pos_embed.requires_grad_(False)
        xb = x.clone().requires_grad_(True)
        with m.input_grad_only(), ac():
            out2 = _call(m, how, xb, t, y)
        ops.launch_counts(reset=True)
        (dx,) = torch.autograd.grad(out2, xb, g)
        counts = ops.launch_counts()
        assert torch.equal(out2, out) and torch.equal(dx, xa.grad), (frozen, float((dx - xa.grad).abs().max()))
        assert counts["tn_bf16"] == counts["tn_f32"] == counts["tn_f16"] == 0, counts      # no weight-gradient GEMM
        assert all(p.grad is None for p in m.parameters())
    assert m._input_grad_only is False                               # the context restored the default


def test_input_only_backward_leaves_preset_grads_alone():
    m = _dit()
    x, t, y, g = _inputs(2)
    for p in m.parameters():
        if p.requires_grad:
            p.grad = torch.full_like(p, 3.0)
    xb = x.clone().requires_grad_(True)
    with m.input_grad_only():
        m(xb, t, y).backward(g)
    assert xb.grad is not None and float(xb.grad.abs().sum()) > 0
    assert all(torch.equal(p.grad, torch.full_like(p, 3.0)) for p in m.parameters() if p.requires_grad)


@pytest.mark.parametrize("prec,B", [("f32", 2), ("bf16", 8)])
def test_input_only_graph_keeps_the_full_layout_without_the_weight_gradient_operands(prec, B):
    """One saved-tensor layout for both modes: under input_grad_only() a block node has the 29 slots of the full mode, and those that only
    the parameter gradients read -- SiLU(c), xm1, xm2, hid, the adaLN weight (slots 1, 6, 16, 18, 24) -- hold None, so nothing is kept alive
    for them."""
    from test_gpu_resnorm_fused import _block_nodes
    m = _dit()
    x, t, y, _ = _inputs(B)
    with m.input_grad_only(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec == "bf16"):
        out = m(x.clone().requires_grad_(True), t, y)
    nodes = _block_nodes(out.grad_fn)
    assert len(nodes) == 2
    for n in nodes:
        sv = n.saved_tensors
        assert len(sv) == 29
        assert [i for i, s in enumerate(sv) if s is None] == sorted([1, 6, 16, 18, 24] + ([10] if prec == "bf16" else []))      # (bf16: no head-major v, slot 10)
        assert sv[0].shape == (B * 64, 128) and sv[13].shape == (B * 64, 128) and sv[15].shape == (B * 64,)
        # nor through the node's attributes: the zero-padded f32 copies of w12 / w3 (SwiGLU width 341 here) are not held for the backward
        assert n.wparams is None and n.sparams is None and n.direct is False


def test_block_gradients_are_returned_by_argument_name():
    import inspect
    from ldmae_amd.models import lightningdit as L
    params = list(inspect.signature(L._DiTBlockFn.forward).parameters)
    assert params[0] == "ctx" and params[-1] == "gemm_precision"      # forward-only: never reaches a backward
    assert len(L._BLOCK_ARGS) == 31 and list(L._BLOCK_ARGS) == params[1:-1]
    assert set(L._BLOCK_SMALL) <= set(L._BLOCK_ARGS)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_training_backward_is_the_earlier_code_path(prec, monkeypatch):
    """Mode off: dx and every parameter gradient of a training-style backward have the bits of the three backward passes as they stood before
    the mode was added (tests/likelihood_as_before.py; the one None they gain answers the new, unused, flag argument)."""
    import likelihood_as_before as before
    from ldmae_amd.models import lightningdit as L
    m = _dit().train()
    x, t, y, g = _inputs(2)

    def step():
        m.zero_grad(set_to_none=True)
        xa = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec == "bf16"):
            out = m(xa, t, y)
        ((out - g) ** 2).mean().backward()
        return xa.grad, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    dx_now, grads_now = step()
    for cls, fn in ((L._PatchEmbedFn, before._patch_embed_backward_as_before), (L._DiTBlockFn, before._block_backward_as_before),
                    (L._FinalLayerFn, before._final_layer_backward_as_before)):
        monkeypatch.setattr(cls, "backward", staticmethod(lambda ctx, gr, fn=fn: tuple(fn(ctx, gr)) + (None,)))
    dx_was, grads_was = step()
    assert torch.equal(dx_now, dx_was) and grads_now.keys() == grads_was.keys() and len(grads_now) > 30
    for n in grads_now:
        assert torch.equal(grads_now[n], grads_was[n]), n


def test_vjp_is_the_central_finite_difference():
    """eps^T dv/dx along 4 random unit directions d against (F(x + h d) - F(x - h d)) / 2h, F = sum(out * eps), h = 1 (a perturbation of 0.02
    per element), f32.  Bound: the CPU oracle's own finite-difference error at the same h on the same weights, inputs, eps and directions,
    measured with oracle/dit.py evaluated in f64 (parameters, inputs and products in f64; its f32 frequency / rotation tables stay as they are)
    against its autograd gradient: 2.03e-6, 1.26e-5, 2.62e-5, 2.80e-5 for the four directions (the same oracle in f32: 5.3e-6 .. 3.0e-5, so
    at this h the truncation term dominates the rounding of F, |F| ~ 14, u |F| ~ 1e-6).  Allowed: 4 x the worst, 1.12e-4, against
    directional derivatives of the order of 0.2."""
    m = _dit().requires_grad_(False)
    x, t, y, _ = _inputs(2)
    g = torch.Generator().manual_seed(3)
    eps = (torch.randint(0, 2, x.shape, generator=g).float() * 2 - 1).cuda()
    ds = [torch.randn(x.shape, generator=g) for _ in range(4)]
    ds = [(d / d.norm()).cuda() for d in ds]
    xg = x.clone().requires_grad_(True)
    with m.input_grad_only():
        (vjp,) = torch.autograd.grad(m(xg, t, y), xg, eps)
    h = 1.0
    with torch.no_grad():
        for i, d in enumerate(ds):
            fd = (float((m(x + h * d, t, y).double() * eps).sum()) - float((m(x - h * d, t, y).double() * eps).sum())) / (2 * h)
            an = float((vjp.double() * d.double()).sum())
            print(f"direction {i}: vjp . d = {an:.6f}, central difference {fd:.6f}, |diff| {abs(fd - an):.2e} (allowed 1.12e-4)")
            assert abs(fd - an) <= 4 * 2.80e-5


# ----------------------------------------------------------------------------- end to end
def test_likelihood_through_the_dit_is_a_function_of_the_seed():
    from ldmae_amd.transport import Sampler, create_transport
    m = _dit().requires_grad_(False)
    x, _, y, _ = _inputs(2)
    s = Sampler(create_transport())
    runs = []
    for seed in (5, 5, 6):
        fn = s.sample_ode_likelihood(num_steps=2, seed=seed)
        logp, z = fn(x, m.forward, y=y)
        runs.append((logp, z, (fn.ode.nfe, fn.ode.accepted, fn.ode.rejected)))
    print(f"logp {runs[0][0].tolist()} (seed 6: {runs[2][0].tolist()}); nfe / accepted / rejected {runs[0][2]}")
    assert runs[0][0].shape == (2,) and runs[0][0].dtype == torch.float32 and torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    assert not torch.equal(runs[0][0], runs[2][0])                   # another seed, another probe
    assert runs[0][2][0] == 2 + 6 * (runs[0][2][1] + runs[0][2][2])
    assert all(p.grad is None for p in m.parameters())


@pytest.mark.parametrize("method", ["heun", "dopri5"])
def test_zero_velocity_returns_the_prior(method):
    """A zeroed final layer: v = 0 and eps^T J = 0 exactly.  A fixed-step method then returns z == x bit for bit and logp is the f32 formula
    c - sumsq / 2 on the kernel's sums of squares.  Under dopri5 the state at t = 1 is the quartic interpolant of the last accepted step, and that
    polynomial does not reproduce a constant state exactly in f32 (its coefficients -8 (y + y) + 16 y, 18 y + 14 y - 32 y, -11 y - 5 y + 16 y
    cancel only up to the roundings of 18 y, 14 y, 11 y, 5 y and of the sums: at most 3 roundings of values below 32 |y| each, so |coefficient|
    <= 96 u |y|, times x^2 + x^3 + x^4 <= 3, plus the 4 additions: |z - x| <= 300 u |x|; about one element in ten moves by an ulp).  That
    arithmetic is the plain sampler's and is pinned bit for bit, so dopri5 is held to this bound instead; delta_logp is exactly 0 either way."""
    from ldmae_amd import ops
    from ldmae_amd.transport import Sampler, create_transport
    m = _dit(zero_final=True).requires_grad_(False)
    x, _, y, _ = _inputs(2)
    tr = create_transport()
    logp, z = Sampler(tr).sample_ode_likelihood(sampling_method=method, num_steps=3, seed=1)(x, m.forward, y=y)
    c = torch.tensor(-1024 / 2.0 * math.log(2 * math.pi), dtype=torch.float32).cuda()
    assert torch.equal(logp, c - ops.rowdot(z) / 2.0)               # the f32 formula on the kernel's sums of squares, delta = 0 exactly
    if method == "heun":
        assert torch.equal(z, x)
        zerr = 0.0
    else:
        zerr = 300 * U
        moved = (z != x).float().mean()
        print(f"dopri5, zero velocity: {float(moved):.3f} of the elements moved, worst {float(((z - x).abs() / x.abs()).max() / U):.2f} u |x|")
        assert ((z - x).abs() <= zerr * x.abs()).all()
    k = 16 + 8 + 1 + 8                                               # against Transport.prior_logp(x) (torch's summation order): two sums, each within gamma_k
    want = tr.prior_logp(x)
    ss = (x.double() ** 2).sum((1, 2, 3))
    assert ((logp - want).abs().double() <= (2 * k * U + 2.5 * zerr) * ss / 2 + 2 * U * want.abs().double()).all()


def test_command_line_on_synthetic_latents(tmp_path, monkeypatch, capsys):
    import ldmae_amd.likelihood as cli
    from ldmae_amd.models import lightningdit as L
    cfg = copy.deepcopy(yaml.safe_load(open(os.path.join(ROOT, "ldmae_amd/configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml"))))
    cfg["data"].update(image_size=64)
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    monkeypatch.setitem(L.LightningDiT_models, "LightningDiT-B/1", lambda **kw: L.LightningDiT(depth=2, hidden_size=128, patch_size=1, num_heads=2, **kw))
    res = cli.main(["--config", str(tmp_path / "cfg.yaml"), "--synthetic", "4", "--batch", "4", "--num-steps", "2"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == res
    assert res["images"] == 4 and math.isfinite(res["bits_per_dim"]) and res["bits_per_dim_sem"] > 0 and res["nfe"] == 2 + 6 * (res["accepted"] + res["rejected"])
    # untrained weights (no --ckpt): a zero velocity, so the N(0, I) latents score the entropy of the prior up to sampling noise
    assert abs(res["bits_per_dim"] - 0.5 * math.log2(2 * math.pi * math.e)) < 0.2
