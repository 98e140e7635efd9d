"""The SDE sampler on the GPU: the Philox normal draw and the step kernel of csrc/ode.hip per element against f64, Sampler.sample_sde against the
reference's own f64 trajectories (tests/golden/sde.npz), the number of model calls, and the sampler end to end through a tiny LightningDiT.

Bounds.  U = 2^-24 (the unit roundoff of f32; one ulp of a value y is at most 2 U |y|).

The draw  z = fl(r c),  r = sqrt(-2 ln u_a),  c = cos or sin of theta = 2 pi u_b,  u exact in f32.  Allowances for the device's math library, stated
here and not measured: logf within 2 ulp, sqrtf within 1 ulp, sinf / cosf within 2 ulp.
  theta:  fl(fl(2 pi) u) carries two roundings: |d theta| <= 2 U theta  (theta < 2 pi, so at most 4 pi U = 12.6 U);
  c:      |d c| <= |d theta| + 2 ulp <= 2 U theta + 4 U             (|sin'|, |cos'| <= 1; |c| <= 1);
  r:      -2 ln u within 2 ulp = 4 U relative (the factor 2 is exact), halved by the root, plus the root's own ulp (2 U): 4 U relative;
  z:      |d z| <= r |d c| + |z| (4 U + U)                           (the product's rounding is the last U)
so per element  |z_gpu - z_f64| <= [r (2 theta + 4) + 5 |z|] U (1 + 1e-3): at most 5.77 (12.6 + 4 + 5) U = 7.4e-6 at the largest r, about 1e-6
for a typical element.  (A numpy f32 emulation of the same specification is off by at most 1.8e-6.)

The step  out = sum_{j<m} c_j x_j + c_z z:  fl(c_0 x_0), then one fma per further term, the noise term last: m roundings, each relative to a
partial sum bounded by S = sum |c_j x_j| + |c_z z|, so |out - f64| <= gamma_m S <= (m + 2) U S (the issue's bound; gamma_m = m U / (1 - m U)).
With the draw generated in the kernel the f64 value is taken on probe.normal, and the draw's bound times |c_z| is added."""
import math
import os

import numpy as np
import pytest
import torch

import gemm_check as gc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = gc.U
NS = [1, 3, 4, 5, 4095, 4096, 4097, 8193]          # the scalar tail alone, the float4 body, the 1024-item block edge, three blocks
FORMS = ("constant", "SBDM", "sigma", "linear", "decreasing", "inccreasing-decreasing")
LASTS = (None, "Mean", "Tweedie", "Euler")


def _draw_bound(n, seed, counter):
    """(z in f64, the per-element bound of the module docstring) for the draw (seed, counter)."""
    from ldmae_amd.transport import probe
    z = probe.normal(n, seed, counter)
    s, c = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    v = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.stack([np.full_like(v, c & 0xFFFFFFFF), np.full_like(v, c >> 32), v & np.uint64(0xFFFFFFFF), v >> np.uint64(32)], -1)
    u = ((probe.philox4x32_10(ctr, np.array([s & 0xFFFFFFFF, s >> 32], dtype=np.uint64)) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    r = np.repeat(np.sqrt(-2 * np.log(u[:, 0::2])), 2, axis=-1).reshape(-1)[:n]              # r of (u0, u1) for values 0, 1; of (u2, u3) for 2, 3
    theta = np.repeat(2 * np.pi * u[:, 1::2], 2, axis=-1).reshape(-1)[:n]
    return z, (r * (2 * theta + 4) + 5 * np.abs(z)) * U * (1 + 1e-3)


# ----------------------------------------------------------------------------- the draw
@pytest.mark.parametrize("n", NS)
def test_normal_against_the_f64_restatement(n):
    from ldmae_amd import ops
    worst = 0.0
    for seed, counter in ((0, 0), (3, 5), (0xFEDCBA9876543210, (7 << 32) | 249)):        # a 64-bit seed, a counter with a non-zero high word
        got = ops.normal((n,), seed, counter, "cuda")
        again = ops.normal((n,), seed, counter, "cuda")
        want, bound = _draw_bound(n, seed, counter)
        err = np.abs(got.double().cpu().numpy() - want)
        worst = max(worst, float(err.max()))
        print(f"normal n={n} seed={seed:#x} counter={counter:#x}: worst |err| {err.max():.3e}, worst err / bound {float((err / bound).max()):.3f}, "
              f"largest bound {bound.max():.3e}")
        assert got.dtype == torch.float32 and got.shape == (n,) and torch.equal(got, again)
        assert (err <= bound).all()
        assert float(got.abs().max()) <= math.sqrt(48 * math.log(2)) * (1 + 8 * U)
        # a destination that is only 4-byte aligned takes the element-store path: the same bits, nothing written outside
        buf = torch.zeros(n + 2, device="cuda")
        ops.normal(None, seed, counter, "cuda", out=buf[1:n + 1])
        assert torch.equal(buf[1:n + 1], got) and float(buf[0]) == 0 and float(buf[n + 1]) == 0
    if n >= 4095:
        a, b = ops.normal((n,), 3, 5, "cuda"), ops.normal((n,), 3, 6, "cuda")
        assert not torch.equal(a, b) and abs(float(a.mean())) < 5 / math.sqrt(n)


# ----------------------------------------------------------------------------- the step kernel
def _inputs(n, m, seed):
    g = torch.Generator().manual_seed(seed)
    ins = [(torch.randn(n, generator=g) * (1 + j)).cuda() for j in range(m)]
    coef = [float(np.float32(c)) for c in (torch.randn(m, generator=g) * 1.5).tolist()]
    nc = float(np.float32(0.37 + 0.1 * m))
    z = torch.randn(n, generator=g).cuda()
    return ins, coef, nc, z


def _f64(ins, coef, nc=0.0, z=None):
    """(sum_j c_j x_j, S = sum |c_j x_j|) in f64 on the CPU, plus the noise term when z (f64 numpy or tensor) is given."""
    acc = sum(c * x.double().cpu().numpy() for c, x in zip(coef, ins))
    S = sum(abs(c) * np.abs(x.double().cpu().numpy()) for c, x in zip(coef, ins))
    if z is not None:
        zz = z.double().cpu().numpy() if torch.is_tensor(z) else z
        acc, S = acc + nc * zz, S + abs(nc) * np.abs(zz)
    return acc, S


@pytest.mark.parametrize("m", [1, 2, 3, 4])
@pytest.mark.parametrize("n", NS)
def test_sde_combine_against_f64(n, m):
    from ldmae_amd import ops
    ins, coef, nc, z = _inputs(n, m, 1000 * m + n)
    seed, counter = 0x1234567890ABCDEF, (3 << 32) | 17
    new = lambda: torch.full((n,), float("nan"), device="cuda")      # noqa: E731
    mean_ref, mean_S = _f64(ins, coef)
    worst = {}
    for mode in ("none", "tensor", "philox"):
        kw = {"none": {}, "tensor": dict(noise_coef=nc, z=z), "philox": dict(noise_coef=nc, seed=seed, counter=counter)}[mode]
        if mode == "philox":
            zd, zb = _draw_bound(n, seed, counter)
            ref, S = _f64(ins, coef, nc, zd)
            extra = abs(nc) * zb
        else:
            ref, S = _f64(ins, coef, nc, z if mode == "tensor" else None)
            extra = 0.0
        for with_mean in (False, True):
            mean = new() if with_mean else None
            out = ops.sde_combine(ins, coef, new(), mean_out=mean, **kw)
            err = np.abs(out.double().cpu().numpy() - ref)
            bound = (m + 2) * U * S + extra
            worst[mode] = max(worst.get(mode, 0.0), float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (mode, with_mean, float(err.max()))
            if with_mean:                                            # the sum without the noise term
                merr = np.abs(mean.double().cpu().numpy() - mean_ref)
                assert (merr <= (m + 2) * U * mean_S).all(), (mode, float(merr.max()))
                assert torch.equal(out, ops.sde_combine(ins, coef, new(), **kw))          # the second output changes nothing in the first
                if mode == "none":
                    assert torch.equal(out, mean)
            assert torch.equal(out, ops.sde_combine(ins, coef, new(), mean_out=new() if with_mean else None, **kw))       # two runs, the same bits
        base = ops.sde_combine(ins, coef, new(), **kw)
        if mode == "philox":                                         # the draw in the kernel == ldmae_normal_f32, then the tensor form
            drawn = ops.normal((n,), seed, counter, "cuda")
            assert torch.equal(base, ops.sde_combine(ins, coef, new(), noise_coef=nc, z=drawn))
        # in place: the output is one of the inputs (or z); the same bits as out of place
        for j in range(m):
            cp = [t.clone() for t in ins]
            assert torch.equal(ops.sde_combine(cp, coef, cp[j], **kw), base), (mode, "out is input", j)
            assert all(torch.equal(cp[i], ins[i]) for i in range(m) if i != j)
        if mode == "tensor":
            zc = z.clone()
            assert torch.equal(ops.sde_combine(ins, coef, zc, noise_coef=nc, z=zc), base)
        cp = [t.clone() for t in ins]
        mean = cp[m - 1] if m > 1 else new()                         # the mean over the last input, the result over the first
        got = ops.sde_combine(cp, coef, cp[0], mean_out=mean, **kw)
        assert torch.equal(got, base) and (np.abs(mean.double().cpu().numpy() - mean_ref) <= (m + 2) * U * mean_S).all()
    print(f"sde_combine n={n} m={m}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("nt", [1, 257])
def test_sde_combine_fills_the_time_vector(nt):
    from ldmae_amd import ops
    ins, coef, nc, z = _inputs(4097, 2, 7)
    tbuf = torch.full((nt + 2,), -1.0, device="cuda")
    tv = float(np.float32(0.384))
    out = ops.sde_combine(ins, coef, torch.empty(4097, device="cuda"), noise_coef=nc, z=z, t_next=tv, t_out=tbuf[1:nt + 1])
    assert torch.equal(out, ops.sde_combine(ins, coef, torch.empty(4097, device="cuda"), noise_coef=nc, z=z))
    assert (tbuf[1:nt + 1] == tv).all() and float(tbuf[0]) == -1 and float(tbuf[nt + 1]) == -1


def test_sde_combine_refuses_overlap_and_misalignment():
    from ldmae_amd import ops
    n = 64
    buf = torch.zeros(4 * n, device="cuda")
    a, b, o = buf[0:n], buf[n:2 * n], buf[2 * n:3 * n]
    ok = ops.sde_combine((a, b), (1.0, 2.0), o)
    assert float(ok.abs().sum()) == 0
    for what, call in (
            ("partial overlap with an input", lambda: ops.sde_combine((a, b), (1.0, 2.0), buf[4:4 + n])),
            ("partial overlap with z", lambda: ops.sde_combine((a,), (1.0,), buf[n + 8:2 * n + 8], noise_coef=1.0, z=b)),
            ("mean partially over an input", lambda: ops.sde_combine((a, b), (1.0, 2.0), o, mean_out=buf[n - 4:2 * n - 4])),
            ("out is mean_out", lambda: ops.sde_combine((a, b), (1.0, 2.0), o, mean_out=o)),
            ("misaligned input", lambda: ops.sde_combine((buf[1:n + 1], b), (1.0, 2.0), o)),
            ("misaligned out", lambda: ops.sde_combine((a, b), (1.0, 2.0), buf[2 * n + 1:3 * n + 1])),
            ("misaligned z", lambda: ops.sde_combine((a,), (1.0,), o, noise_coef=1.0, z=buf[n + 2:2 * n + 2])),
            ("t_out inside an input", lambda: ops.sde_combine((a, b), (1.0, 2.0), o, t_next=0.5, t_out=buf[8:12]))):
        with pytest.raises(RuntimeError, match=r"ldmae_sde_combine_f32 failed \(rc="):
            call()
    with pytest.raises(RuntimeError, match="1 to 4 inputs"):
        ops.sde_combine((a, a, a, a, a), (1.0,) * 5, o)
    from ldmae_amd._lib import call, ptr, stream
    cf = (__import__("ctypes").c_float * 4)(1.0, 0.0, 0.0, 0.0)
    for mode, z in ((3, None), (1, None), (0, b)):                   # an unknown mode; z missing; z given without the tensor mode
        with pytest.raises(RuntimeError, match="sde_combine"):
            call("ldmae_sde_combine_f32", ptr(a), None, None, None, cf, 1, ptr(z), 1.0, mode, 0, 0, ptr(o), None, n, 0.0, None, 0, stream())
    assert float(buf.abs().sum()) == 0                               # nothing was launched


# ----------------------------------------------------------------------------- the sampler against the reference's trajectories
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "sde.npz"))


class _Toy:
    """v = tanh(x W) (1 + t) + b of tests/golden/make_golden_sde.py on the device, in f32 elementwise arithmetic; keeps what it saw."""

    def __init__(self, gold):
        self.W, self.b = torch.from_numpy(gold["W"]).cuda(), torch.from_numpy(gold["b"]).cuda()
        self.calls = []

    def __call__(self, x, t):
        assert not torch.is_grad_enabled()
        h = torch.tanh((x.unsqueeze(2) * self.W.view(1, *self.W.shape, 1, 1)).sum(1))
        v = h * (1 + t).view(-1, 1, 1, 1) + self.b.view(1, -1, 1, 1)
        self.calls.append((x.clone(), t.clone(), v.clone()))
        return v


def _transport(eps):
    from ldmae_amd.transport import ModelType, PathType, Transport, WeightType
    return Transport(model_type=ModelType.VELOCITY, path_type=PathType.LINEAR, loss_type=WeightType.NONE, train_eps=eps, sample_eps=eps)


def _step_floors(fn, method, calls, draws, has_last):
    """The combine bound of each trajectory point's LAST launch, max over elements: (m + 2) U (sum |c_j x_j| + |c_z z|) on what the run saw."""
    mx = lambda terms: float(sum(abs(c) * t.double().abs() for c, t in terms).max())      # noqa: E731
    floors = []
    for k, c in enumerate(fn.sde.plan):
        if method == "Euler":
            x, _, v = calls[k]
            floors.append(4 * U * mx([(c["cx"], x), (c["cv"], v), (c["cz"], draws[k])]))
        else:
            (xh, _, v1), (xp, _, v2) = calls[2 * k], calls[2 * k + 1]
            floors.append(6 * U * mx([(c["cx"], xh), (c["cv1"], v1), (c["cxp"], xp), (c["cv2"], v2)]))
    if has_last:
        x, _, v = calls[-1]
        floors.append(4 * U * mx([(fn.last_coefficients[0], x), (fn.last_coefficients[1], v)]))
    else:
        floors.append(floors[-1])                                    # last_step None repeats the last state
    return floors


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("method", ["Euler", "Heun"])
def test_sample_sde_against_the_reference_trajectories(gold, method, form):
    """Every stored case: the recorded draws through noise=, the toy model on the device, each trajectory point against the reference's f64 run.
    Allowed per point: 4 x the reference's own f32 - f64 deviation there (the rearranged coefficient algebra is a different, equally rounded,
    f32 evaluation), and never less than the combine bound of that step.  Also the number of model calls and the times they were made at."""
    from ldmae_amd.transport import Sampler
    tr = _transport(float(gold["sample_eps"]))
    draws = [torch.from_numpy(d).cuda() for d in gold["draws"]]
    x0 = torch.from_numpy(gold["x0"]).cuda()
    for last in LASTS:
        case = f"{method}/{form}/{last}"
        model, asked = _Toy(gold), []
        fn = Sampler(tr).sample_sde(sampling_method=method, diffusion_form=form, diffusion_norm=float(gold["norm"]), last_step=last,
                                    last_step_size=float(gold["last_step_size"]), num_steps=6,
                                    noise=lambda k, shape: (asked.append((k, tuple(shape))), draws[k])[1])
        xs = fn(x0, model)
        assert isinstance(xs, list) and len(xs) == 6 and all(x.shape == x0.shape and x.dtype == torch.float32 for x in xs)
        assert asked == [(k, tuple(x0.shape)) for k in range(5)] and torch.equal(x0, torch.from_numpy(gold["x0"]).cuda())
        # one model call per drift evaluation, at the grid's times
        per = 1 if method == "Euler" else 2
        assert len(model.calls) == 5 * per + (last is not None) == fn.model_calls, case
        t = gold[case + "/t"]
        want_t = [float(t[k]) if per == 1 or i == 0 else float(t[k] + (t[1] - t[0])) for k in range(5) for i in range(per)] + [float(t[-1])] * (last is not None)
        assert [c[1].tolist() for c in model.calls] == [[w] * 3 for w in want_t], case
        if last is None:
            assert xs[-1] is xs[-2] or torch.equal(xs[-1], xs[-2])
        floors = _step_floors(fn, method, model.calls, draws, last is not None)
        ref, dev = gold[case + "/traj"], gold[case + "/dev"]
        ratios = []
        for k in range(6):
            err = float(np.abs(xs[k].double().cpu().numpy() - ref[k]).max())
            allowed = max(4 * float(dev[k]), floors[k])
            ratios.append(err / allowed)
        print(f"{case:40s} err / allowed per point " + " ".join(f"{r:.2f}" for r in ratios) + f"   (worst {max(ratios):.2f}; |x| up to {np.abs(ref).max():.1f})")
        assert max(ratios) <= 1.0, (case, ratios)
        # keep_trajectory=False: the same last state, in place on the sampler's own buffers
        fn2 = Sampler(tr).sample_sde(sampling_method=method, diffusion_form=form, diffusion_norm=float(gold["norm"]), last_step=last,
                                     last_step_size=float(gold["last_step_size"]), num_steps=6, noise=lambda k, shape: draws[k], keep_trajectory=False)
        only = fn2(x0, _Toy(gold))
        assert len(only) == 1 and torch.equal(only[-1], xs[-1]) and torch.equal(x0, torch.from_numpy(gold["x0"]).cuda()), case


def test_default_draw_is_a_function_of_seed_and_call_index(gold):
    """Without noise=: step k of call c draws normal(seed, (c << 32) | k) inside the kernel -- the same bits as the tensor form on ops.normal."""
    from ldmae_amd import ops
    from ldmae_amd.transport import Sampler
    tr, x0 = _transport(1e-3), torch.from_numpy(gold["x0"]).cuda()
    for method in ("Euler", "Heun"):
        fn = Sampler(tr).sample_sde(sampling_method=method, diffusion_form="sigma", num_steps=6, seed=77)
        a, b = fn(x0, _Toy(gold)), fn(x0, _Toy(gold))
        assert fn.calls == 2 and not torch.equal(a[-1], b[-1])        # the second call draws with another counter
        fn.calls = 0
        assert all(torch.equal(p, q) for p, q in zip(a, fn(x0, _Toy(gold))))
        named = Sampler(tr).sample_sde(sampling_method=method, diffusion_form="sigma", num_steps=6,
                                       noise=lambda k, shape: ops.normal(shape, 77, (1 << 32) | k, "cuda"))
        assert all(torch.equal(p, q) for p, q in zip(b, named(x0, _Toy(gold))))
        other = Sampler(tr).sample_sde(sampling_method=method, diffusion_form="sigma", num_steps=6, seed=78)(x0, _Toy(gold))
        assert not torch.equal(other[0], a[0])


# ----------------------------------------------------------------------------- end to end through a tiny LightningDiT
def _dit():
    from ldmae_amd.models.lightningdit import LightningDiT
    torch.manual_seed(0)
    m = LightningDiT(input_size=8, patch_size=1, in_channels=16, hidden_size=128, depth=2, num_heads=2, num_classes=10, use_qknorm=True,
                     use_swiglu=True, use_rope=True, use_rmsnorm=True)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                                            # the zero-initialised adaLN / final layer would make every output zero
        for n, p in m.named_parameters():
            if "adaLN_modulation" in n or n.startswith("final_layer.linear"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return m.cuda().eval()


def test_sde_through_the_sampling_driver_with_guidance():
    from ldmae_amd import ops
    from ldmae_amd.inference import sample_latents
    from ldmae_amd.transport import Sampler, create_transport
    m, dev, n = _dit(), torch.device("cuda"), 8                      # 8: half and doubled batch both take the batched bf16 adaLN path
    s = Sampler(create_transport())

    def run(fn, start=0.3):
        fn.calls = 0
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return sample_latents(m, fn, n, 4.0, start, dev, 10, generator=torch.Generator(device="cuda").manual_seed(5))

    fn = s.sample_sde(diffusion_form="sigma", num_steps=6, seed=5, keep_trajectory=False)
    halves, fulls = [], []
    orig_fwd, orig_cfg = m.forward, m.forward_with_cfg
    m.forward = lambda x, tt, y: (halves.append(len(x)), orig_fwd(x, tt, y))[1]
    m.forward_with_cfg = lambda *a, **k: (fulls.append(len(a[0])), orig_cfg(*a, **k))[1]
    (lat, y), (lat2, y2) = run(fn), run(fn)
    m.forward, m.forward_with_cfg = orig_fwd, orig_cfg
    assert lat.shape == (n, 16, 8, 8) and lat.dtype == torch.float32 and torch.isfinite(lat).all()
    assert torch.equal(lat, lat2) and torch.equal(y, y2)                                  # a function of (init, seed, call index)
    # per run: t = 0 and 0.192 lie below the interval start 0.3 -> two calls on the conditional half; forward_with_cfg (which calls forward on the
    # doubled batch itself) for the other three steps and the last one
    assert halves.count(n) == 2 * 2 and fulls == [2 * n] * 4 * 2 and halves.count(2 * n) == len(fulls) and fn.model_calls == 6
    lat3, _ = run(s.sample_sde(diffusion_form="sigma", num_steps=6, seed=6, keep_trajectory=False))
    assert not torch.equal(lat, lat3)
    # the conditional-half shortcut against forward_with_cfg on the doubled batch at every step: the kept half, bit for bit
    g = torch.Generator(device="cuda").manual_seed(5)
    z = torch.randn(n, 16, 8, 8, device="cuda", generator=g)
    yy = torch.randint(0, 10, (n,), device="cuda", generator=g)
    fn.calls = 0
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ref = fn(torch.cat([z, z]), m.forward_with_cfg, y=torch.cat([yy, torch.full((n,), 10, device="cuda")]), cfg_scale=4.0, cfg_interval=True,
                 cfg_interval_start=0.3)[-1][:n]
    assert torch.equal(y, yy) and torch.equal(lat, ref)

    # every step satisfies its formula: named draws, the model's outputs captured
    for method in ("Euler", "Heun"):
        seen, zs = [], {}

        def noise(k, shape):
            zs[k] = ops.normal(shape, 9, k, "cuda")
            return zs[k]

        inner = s.sample_sde(sampling_method=method, diffusion_form="sigma", num_steps=6, noise=noise)
        traj = []

        def outer(zin, model, **kw):
            def cap(x, t, **k2):
                assert not torch.is_grad_enabled()
                out = model(x, t, **k2)
                seen.append((x.clone(), t.clone(), out.float().clone()))
                return out
            traj.append(zin.clone())
            traj.extend(inner(zin, cap, **kw))
            return traj

        out, _ = run(outer)
        assert torch.equal(out, traj[-1][:n]) and torch.isfinite(out).all() and len(traj) == 7 and len(seen) == inner.model_calls
        d64 = lambda t: t.double()      # noqa: E731
        worst = 0.0
        for k, c in enumerate(inner.sde.plan):
            if method == "Euler":
                x, t, v = seen[k]
                assert torch.equal(x, traj[k]) and (t == c["t"]).all()
                terms = [(c["cx"], x), (c["cv"], v), (c["cz"], zs[k])]
                bound_m = 2
            else:
                (xh, t1, v1), (xp, t2, v2) = seen[2 * k], seen[2 * k + 1]
                assert (t1 == c["t"]).all() and (t2 == np.float32(c["t2"])).all()
                hat = d64(traj[k]) + c["cz"] * d64(zs[k])
                assert ((d64(xh) - hat).abs() <= 3 * U * (d64(traj[k]).abs() + abs(c["cz"]) * d64(zs[k]).abs())).all()
                pred = c["px"] * d64(xh) + c["pv"] * d64(v1)
                assert ((d64(xp) - pred).abs() <= 4 * U * (abs(c["px"]) * d64(xh).abs() + abs(c["pv"]) * d64(v1).abs())).all()
                terms = [(c["cx"], xh), (c["cv1"], v1), (c["cxp"], xp), (c["cv2"], v2)]
                bound_m = 4
            want = sum(cf * d64(tt) for cf, tt in terms)
            S = sum(abs(cf) * d64(tt).abs() for cf, tt in terms)
            err = (d64(traj[k + 1]) - want).abs()
            worst = max(worst, float((err / ((bound_m + 2) * U * S)).max()))
            assert (err <= (bound_m + 2) * U * S).all(), (method, k)
        x, t, v = seen[-1]
        lx, lv = inner.last_coefficients
        assert torch.equal(x, traj[-2]) and (t == np.float32(0.96)).all()
        S = abs(lx) * d64(x).abs() + abs(lv) * d64(v).abs()
        assert ((d64(traj[-1]) - (lx * d64(x) + lv * d64(v))).abs() <= 4 * U * S).all()
        print(f"{method} through the DiT with guidance: worst step error / bound {worst:.3f}")
