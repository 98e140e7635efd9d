"""The attention checker checked (CPU only): tests/attn_check.py must accept correct kernel arithmetic and reject small faults.

`emulate_fwd` / `emulate_bwd` redo the kernels' arithmetic in torch: tiles of 64 keys, q (k) scaled by c32 and rounded to the operand type,
f32 scores, the running maximum with the threshold-6 wave-uniform rescale rule (or a static shift), p rounded to the operand type for P.V,
the f32 row sum of the unrounded p (of the rounded p at head dims 16 / 72), one rounding of the output; the backward likewise.

Worst |err| / bound the emulation reaches over head dims 16, 64, 72 x N 40, 200, 256 x both input families (measured here, against the
reference arithmetic, never against a device; test_emulation_passes_the_bounds prints them):

    dtype   o      lse    dq     dk     dv
    bf16    0.81   0.72   0.87   0.89   0.93
    fp16    0.58   0.63   0.80   0.80   0.77
    f32     0.032  0.064  0.065  0.051  0.074

Planted faults (test_planted_faults): each is rejected by the bound while the whole-tensor norm the old suite uses stays under its
tolerance -- except where stated:
  * NaN / unwritten (canary) element: the norm is NaN, which the old `rel_err < tol` also fails; listed for completeness.
  * p TRUNCATED instead of rounded in P.V: rejected on peaked rows only.  Truncation is one-sided with a relative error in [0, 2^-7), mean
    0.69 * 2^-8; the honest bound allows 2^-8 for the rounding of p plus the output's half ulp.  Where one key carries a row its chop shows and
    the element is out; on flat rows the chops average below 2^-8 in every sum (lse at head dims 16 / 72 included) and no element can be shown
    wrong (test_truncated_p_is_rejected_only_on_peaked_rows asserts the numbers).
"""
import math

import pytest
import torch

import attn_check as ac
from conftest import rel_err

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
OLD_TOL = {BF16: (2e-2, 3e-2), F16: (2e-2, 3e-2), F32: (2e-5, 1e-4)}       # (forward, backward) of tests/test_gpu_kernels.py
_CANARY = {BF16: (torch.int16, 0x7FDE), F16: (torch.int16, 0x7E5A), F32: (torch.int32, 0x7FC0DEAD)}


def _round(x, dtype, trunc=False):
    """f32 -> operand type -> f32.  trunc: chop instead of round to nearest (the planted fault)."""
    if dtype == F32:
        return x
    if not trunc:
        return x.to(dtype).float()
    drop = 16 if dtype == BF16 else 13
    return (x.view(torch.int32) >> drop << drop).view(F32)


def emulate_fwd(q, k, v, scale, shift=None, trunc_p=False, drop=None, unmask_last=False):
    """-> (o [B,H,N,hd] in dtype, lse f32).  drop = (b, h, wave, tile): that 64-key tile is skipped for rows 32 wave .. 32 wave + 31.
    unmask_last: the LAST row sees one padding key (a copy of row N - 1 of k / v) with score 0 in its last tile."""
    dtype, (B, H, N, hd) = q.dtype, q.shape
    kind = ac.kind_of(dtype, hd)
    c = torch.tensor(ac.c32(scale), dtype=F32)
    lsum = kind == "mfma16" and hd % 32 != 0
    Qf = q.float() if kind == "f32" else (q.float() * c).to(dtype).float()
    nt = (N + 63) // 64
    acc = torch.zeros(B, H, N, hd)
    l = torch.zeros(B, H, N)
    static = shift is not None
    ms = torch.as_tensor(shift, dtype=F32).expand(B, H, N).clone() if static else torch.zeros(B, H, N)
    pad = (-N) % 32
    for kt in range(nt):
        Kt, Vt = k[:, :, kt * 64:(kt + 1) * 64].float(), v[:, :, kt * 64:(kt + 1) * 64].float()
        s = Qf @ Kt.transpose(-1, -2)
        if kind == "f32":
            s = s * c
        if unmask_last and kt == nt - 1:
            extra = torch.full((B, H, N, 1), -math.inf)
            extra[:, :, N - 1] = 0.0
            s = torch.cat([s, extra], -1)
            Vt = torch.cat([Vt, v[:, :, N - 1:N].float()], 2)
        if not static:
            if kt == 0:
                ms = s.amax(-1)
            elif kind != "mfma16":
                new = torch.maximum(ms, s.amax(-1))
                alpha = torch.exp2(ms - new)
                l, acc, ms = l * alpha, acc * alpha[..., None], new
            else:
                mx = (s - ms[..., None]).amax(-1)
                trig = torch.nn.functional.pad(mx > ac.RESCALE_THR, (0, pad)).view(B, H, -1, 32).any(-1, keepdim=True).expand(-1, -1, -1, 32)
                d = torch.where(trig.reshape(B, H, -1)[..., :N], mx.clamp(min=0.0), torch.zeros_like(mx))
                alpha = torch.exp2(-d)
                l, acc, ms = l * alpha, acc * alpha[..., None], ms + d
        p = torch.exp2(s - ms[..., None])
        if drop is not None and drop[3] == kt:
            b_, h_, w_, _ = drop
            p[b_, h_, 32 * w_:32 * w_ + 32] = 0.0
        pr = _round(p, dtype, trunc_p)
        l = l + (pr if lsum else p).sum(-1)
        acc = acc + pr @ Vt
    o = (acc * (1.0 / l)[..., None]).to(dtype)
    lse = (ms + torch.log2(l)) * torch.tensor(0.6931471805599453, dtype=F32)
    return o, lse


def emulate_bwd(q, k, v, o, do, lse, scale, delta_from_next=None):
    """-> dq, dk, dv in dtype.  delta_from_next = (b, h, wave): those 32 rows use the delta of the row after them."""
    dtype, (B, H, N, hd) = q.dtype, q.shape
    kind = ac.kind_of(dtype, hd)
    c, sc = torch.tensor(ac.c32(scale), dtype=F32), torch.tensor(ac.s32(scale), dtype=F32)
    lse2 = (lse.float() * torch.tensor(1.4426950408889634, dtype=F32))[..., None]
    Q, K, V, O, dO = (t.float() for t in (q, k, v, o, do))
    delta = (dO * O).sum(-1, keepdim=True)
    if delta_from_next is not None:
        b_, h_, w_ = delta_from_next
        delta = delta.clone()
        delta[b_, h_, 32 * w_:32 * w_ + 32] = delta[b_, h_, 32 * w_ + 1:32 * w_ + 33].clone()
    dP = dO @ V.transpose(-1, -2) - delta
    if kind == "mfma16":
        sq = (Q * c).to(dtype).float() @ K.transpose(-1, -2) - lse2
        sk = Q @ (K * c).to(dtype).float().transpose(-1, -2) - lse2
    else:
        sq = sk = (Q @ K.transpose(-1, -2)) * c - lse2
    pq, pk = torch.exp2(sq), torch.exp2(sk)
    dq = ((_round(pq * dP, dtype) @ K) * sc).to(dtype)
    dk = ((_round(pk * dP, dtype).transpose(-1, -2) @ Q) * sc).to(dtype)
    dv = (_round(pk, dtype).transpose(-1, -2) @ dO).to(dtype)
    return dq, dk, dv


def _case(dtype, hd, N, family, B=2, H=3, seed=None):
    q, k, v, do = ac.make_inputs(B, H, N, hd, dtype, family, seed if seed is not None else hd * 1000 + N)
    scale = hd ** -0.5
    f = ac.fwd_ref(q, k, v, scale)
    assert f["finite"], "the f64 reference must stay finite"
    o_in, lse_in = f["o"].to(dtype), f["lse"].float()
    b = ac.bwd_ref(q, k, v, o_in, do, lse_in, scale)
    assert all(bool(torch.isfinite(b[n]).all()) for n in ("dq", "dk", "dv", "bdq", "bdk", "bdv"))
    return dict(q=q, k=k, v=v, do=do, scale=scale, f=f, b=b, o_in=o_in, lse_in=lse_in)


def _check_fwd(c, o, lse):
    return ac.check("o", o, c["f"]["o"], c["f"]["bo"]), ac.check("lse", lse, c["f"]["lse"], c["f"]["bl"])


def _check_bwd(c, dq, dk, dv):
    return tuple(ac.check(n, g, c["b"][n], c["b"]["b" + n]) for n, g in (("dq", dq), ("dk", dk), ("dv", dv)))


WORST: dict = {}


@pytest.mark.parametrize("family", ["unit", "peaked"])
@pytest.mark.parametrize("N", [40, 200, 256])
@pytest.mark.parametrize("hd", [16, 64, 72])
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "fp16", "f32"])
def test_emulation_passes_the_bounds(dtype, hd, N, family):
    c = _case(dtype, hd, N, family)
    if family == "peaked":
        rowmax = c["f"]["s2"].amax(-1)
        assert float(rowmax.max()) >= 30 and float(rowmax.median()) >= 12 and float(c["f"]["smax"].max()) < 60
    o, lse = emulate_fwd(c["q"], c["k"], c["v"], c["scale"])
    ratios = _check_fwd(c, o, lse) + _check_bwd(c, *emulate_bwd(c["q"], c["k"], c["v"], c["o_in"], c["do"], c["lse_in"], c["scale"]))
    for name, r in zip(("o", "lse", "dq", "dk", "dv"), ratios):
        key = (str(dtype)[6:], name)
        WORST[key] = max(WORST.get(key, 0.0), r)
    print("err/bound o lse dq dk dv:", " ".join(f"{r:.3f}" for r in ratios))
    # old-style norms of the same results: correct arithmetic sits well inside the old tolerances too
    assert rel_err(o, c["f"]["o"]) < OLD_TOL[dtype][0]


def test_bounds_are_not_vacuous():
    """Runs after the sweep above (file order): every output's worst err / bound over the sweep is above 1e-2, else the bound is too loose."""
    if not WORST:
        pytest.skip("needs test_emulation_passes_the_bounds in the same run")
    print({k: round(v, 3) for k, v in sorted(WORST.items())})
    for key, r in WORST.items():
        assert 1e-2 < r <= 1.0, (key, r)


def test_static_shift_emulation_passes(dtype=BF16):
    """A static shift (any true bound up to 50) instead of the running maximum: same bound with M = the shift (bf16 only: the others take none)."""
    for family, shift in (("unit", 12.0), ("peaked", 49.5)):
        c = _case(dtype, 64, 200, family)
        assert float(c["f"]["smax"].max()) <= shift
        f = ac.fwd_ref(c["q"], c["k"], c["v"], c["scale"], shift=shift)
        o, lse = emulate_fwd(c["q"], c["k"], c["v"], c["scale"], shift=shift)
        ac.check("o", o, f["o"], f["bo"])
        ac.check("lse", lse, f["lse"], f["bl"])


def _rejected(fn):
    try:
        fn()
    except ac.BoundError:
        return True
    return False


def test_planted_faults():
    """Each fault: rejected by the bound, accepted by the old norm tolerance (the gap this closes)."""
    tol_f, tol_b = OLD_TOL[BF16]
    # -- one query row blended half and half with its neighbour (a full swap needs N >= 1024 at B H = 6 to hide in the norm)
    c = _case(BF16, 64, 256, "unit", B=2, H=4)
    o, lse = emulate_fwd(c["q"], c["k"], c["v"], c["scale"])
    bad = o.clone()
    bad[1, 2, 77] = (0.5 * (o[1, 2, 77].float() + o[1, 2, 78].float())).to(BF16)
    assert rel_err(bad, c["f"]["o"]) < tol_f and _rejected(lambda: _check_fwd(c, bad, lse))
    # -- a whole row swapped, at the benchmark's N = 1024
    c4 = _case(BF16, 16, 1024, "unit", B=2, H=6)
    o4, lse4 = emulate_fwd(c4["q"], c4["k"], c4["v"], c4["scale"])
    bad = o4.clone()
    bad[0, 3, 500] = o4[0, 3, 501]
    assert rel_err(bad, c4["f"]["o"]) < tol_f and _rejected(lambda: _check_fwd(c4, bad, lse4))
    # -- one element 4 ulp off, where the output's own spacing is largest against the bound (peaked rows: |O| is about sum P |v|)
    cp = _case(BF16, 64, 200, "peaked")
    op, lsep = emulate_fwd(cp["q"], cp["k"], cp["v"], cp["scale"])
    u = ac.ulp(cp["f"]["o"], BF16)
    idx = torch.unravel_index(torch.argmax(u / cp["f"]["bo"]), u.shape)
    assert 3 * float(u[idx]) > float(cp["f"]["bo"][idx])        # 4 ulp minus the emulation's own half ulp stays outside
    bad = op.clone()
    bad[idx] = (op[idx].float() + 4 * float(u[idx])).to(BF16)
    assert rel_err(bad, cp["f"]["o"]) < tol_f and _rejected(lambda: _check_fwd(cp, bad, lsep))
    # -- NaN and an unwritten (canary) element: the old norm is NaN there, which `< tol` fails as well
    for bits in (None, _CANARY[BF16][1]):
        bad = o.clone()
        if bits is None:
            bad[0, 0, 3, 5] = float("nan")
        else:
            bad.view(torch.int16)[0, 0, 3, 5] = bits
        assert _rejected(lambda: _check_fwd(c, bad, lse)) and not rel_err(bad, c["f"]["o"]) < tol_f
    # -- the last row of a ragged N with one padding key unmasked
    cr = _case(BF16, 64, 40, "unit")
    o_r, lse_r = emulate_fwd(cr["q"], cr["k"], cr["v"], cr["scale"], unmask_last=True)
    assert rel_err(o_r, cr["f"]["o"]) < tol_f and rel_err(lse_r, cr["f"]["lse"]) < 2e-3
    assert _rejected(lambda: ac.check("o", o_r, cr["f"]["o"], cr["f"]["bo"])) and _rejected(lambda: ac.check("lse", lse_r, cr["f"]["lse"], cr["f"]["bl"]))
    # -- one 64-key tile dropped for one 32-row wave
    o_d, lse_d = emulate_fwd(c4["q"], c4["k"], c4["v"], c4["scale"], drop=(1, 0, 3, 2))
    assert rel_err(o_d, c4["f"]["o"]) < tol_f and rel_err(lse_d, c4["f"]["lse"]) < 2e-3
    assert _rejected(lambda: ac.check("o", o_d, c4["f"]["o"], c4["f"]["bo"])) and _rejected(lambda: ac.check("lse", lse_d, c4["f"]["lse"], c4["f"]["bl"]))
    # -- lse of one head off by log(1 + 2^-6)
    bad = lse.clone()
    bad[1, 1] += math.log1p(2.0 ** -6)
    assert rel_err(bad, c["f"]["lse"]) < 2e-3 and _rejected(lambda: ac.check("lse", bad, c["f"]["lse"], c["f"]["bl"]))
    # -- head dim 72: column 71 taken from the padded zero column (for one wave's rows)
    c72 = _case(BF16, 72, 256, "unit")
    o72, lse72 = emulate_fwd(c72["q"], c72["k"], c72["v"], c72["scale"])
    bad = o72.clone()
    bad[0, 1, 64:96, 71] = 0
    assert rel_err(bad, c72["f"]["o"]) < tol_f and _rejected(lambda: _check_fwd(c72, bad, lse72))
    # -- backward: a correct lse, but one wave's rows use the delta of the row after them (dv does not depend on delta)
    good = emulate_bwd(c["q"], c["k"], c["v"], c["o_in"], c["do"], c["lse_in"], c["scale"])
    _check_bwd(c, *good)
    dq, dk, dv = emulate_bwd(c["q"], c["k"], c["v"], c["o_in"], c["do"], c["lse_in"], c["scale"], delta_from_next=(1, 2, 1))
    assert torch.equal(dv, good[2])
    for got, name in ((dq, "dq"), (dk, "dk")):
        assert rel_err(got, c["b"][name]) < tol_b
    assert _rejected(lambda: ac.check("dq", dq, c["b"]["dq"], c["b"]["bdq"]))
    assert _rejected(lambda: ac.check("dk", dk, c["b"]["dk"], c["b"]["bdk"]))
    cb = _case(BF16, 64, 200, "peaked")
    good = emulate_bwd(cb["q"], cb["k"], cb["v"], cb["o_in"], cb["do"], cb["lse_in"], cb["scale"])
    _check_bwd(cb, *good)
    # -- backward outputs: one element 4 ulp off, NaN
    for name, g in zip(("dq", "dk", "dv"), good):
        u = ac.ulp(cb["b"][name], BF16)
        idx = torch.unravel_index(torch.argmax(u / cb["b"]["b" + name]), u.shape)
        assert 3 * float(u[idx]) > float(cb["b"]["b" + name][idx]), name
        bad = g.clone()
        bad[idx] = (g[idx].float() + 4 * float(u[idx])).to(BF16)
        assert rel_err(bad, cb["b"][name]) < tol_b and _rejected(lambda: ac.check(name, bad, cb["b"][name], cb["b"]["b" + name]))
        bad = g.clone()
        bad[0, 0, 0, 0] = float("nan")
        assert _rejected(lambda: ac.check(name, bad, cb["b"][name], cb["b"]["b" + name]))


def test_planted_faults_f32():
    """The f32 kernels' old tolerances (2e-5 forward, 1e-4 backward) hide the same faults at their own scale."""
    tol_f, tol_b = OLD_TOL[F32]
    c = _case(F32, 64, 256, "unit", B=2, H=4)
    o, lse = emulate_fwd(c["q"], c["k"], c["v"], c["scale"])
    bad = o.clone()
    bad[1, 2, 77, :8] = o[1, 2, 77, :8] * (1 + 2e-3)                     # eight elements of one row off by 2e-3 relative
    assert rel_err(bad, c["f"]["o"]) < tol_f and _rejected(lambda: _check_fwd(c, bad, lse))
    bad = lse.clone()
    bad[1, 1, 5] += 1e-4
    assert rel_err(bad, c["f"]["lse"]) < 1e-5 and _rejected(lambda: ac.check("lse", bad, c["f"]["lse"], c["f"]["bl"]))
    good = emulate_bwd(c["q"], c["k"], c["v"], c["o_in"], c["do"], c["lse_in"], c["scale"])
    _check_bwd(c, *good)
    for name, g in zip(("dq", "dk", "dv"), good):
        bad = g.clone()
        i = torch.unravel_index(torch.argmax(g.abs()), g.shape)
        bad[i] = g[i] * (1 + 1e-3)
        assert rel_err(bad, c["b"][name]) < tol_b and _rejected(lambda: ac.check(name, bad, c["b"][name], c["b"]["b" + name]))


def test_truncated_p_is_rejected_only_on_peaked_rows():
    """p chopped instead of rounded for the P.V product: one-sided, relative error in [0, 2^-7) with mean ln 2 * 2^-8 = 0.69 * 2^-8; the honest
    bound allows 2^-8 for the rounding of p plus the output's own half ulp (2^-9 .. 2^-8 relative).
    Peaked rows (one key carries the row): the output inherits that key's chop, and where it exceeds 2^-8 + 2 * half an ulp the element is out:
    REJECTED.  Flat rows (unit family): the chops average to 0.69 * 2^-8 < 2^-8 in every sum, also in lse at head dim 16 whose row sum adds the
    chopped p, so the fault stays inside the bound and is NOT rejectable per element; it still stands out against the correct emulation
    (err / bound of lse at least 1.5 times larger and above 0.6).  The old norm accepts both."""
    c = _case(BF16, 64, 200, "peaked")
    o, lse = emulate_fwd(c["q"], c["k"], c["v"], c["scale"], trunc_p=True)
    assert rel_err(o, c["f"]["o"]) < 2e-2 and rel_err(lse, c["f"]["lse"]) < 2e-3
    assert _rejected(lambda: ac.check("o", o, c["f"]["o"], c["f"]["bo"]))
    c = _case(BF16, 16, 256, "unit")
    good = _check_fwd(c, *emulate_fwd(c["q"], c["k"], c["v"], c["scale"]))
    o, lse = emulate_fwd(c["q"], c["k"], c["v"], c["scale"], trunc_p=True)
    assert rel_err(o, c["f"]["o"]) < 2e-2 and rel_err(lse, c["f"]["lse"]) < 2e-3
    bad = _check_fwd(c, o, lse)                      # passes: inside the bound
    print(f"head dim 16, flat rows, truncated p: err / bound o {bad[0]:.3f} lse {bad[1]:.3f}; correct emulation o {good[0]:.3f} lse {good[1]:.3f}")
    assert bad[1] > 1.5 * good[1] and bad[1] > 0.6


def test_qknorm_operator_is_the_autograd_of_the_front_end():
    """attn_check.qknorm_bwd_op against autograd of rope(rmsnorm(x) * w) in f64; its absolute form dominates it."""
    g = torch.Generator().manual_seed(3)
    B, H, N, hd = 1, 2, 8, 64
    x = torch.randn(B, H, N, hd, generator=g, dtype=torch.float64, requires_grad=True)
    w = 1 + 0.1 * torch.randn(hd, generator=g, dtype=torch.float64)
    ang = torch.rand(N, hd // 2, generator=g, dtype=torch.float64) * 6.28
    cos, sin = ang.cos().repeat_interleave(2, 1), ang.sin().repeat_interleave(2, 1)
    n = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6) * w
    rot = torch.stack([-n[..., 1::2], n[..., 0::2]], -1).reshape(n.shape)
    y = n * cos + rot * sin
    gy = torch.randn(B, H, N, hd, generator=g, dtype=torch.float64)
    y.backward(gy)
    out, _ = ac.qknorm_bwd_op(gy, x.detach(), w, cos, sin, 1e-6)
    assert rel_err(out, x.grad) < 1e-12
    up, _ = ac.qknorm_bwd_op(gy.abs(), x.detach(), w, cos, sin, 1e-6, absolute=True)
    assert bool((up >= out.abs() * (1 - 1e-12)).all())


def test_wrapper_route_predicate():
    """ops.attention_fwd_qkv takes the key-norm pass + bounded kernel iff bf16, hd <= 32, N >= 512 and B H N^2 >= the threshold: pinned on the
    device (test_gpu_attention_paths.py::test_wrapper_route) because the wrapper decides inline; here only the documented default."""
    import ldmae_amd.ops as ops
    assert ops.BOUNDED_ATTENTION_MIN_SCORES == 1 << 31 or "LDMAE_BOUNDED_ATTN_MIN" in __import__("os").environ
