"""tests/eval_check.py without a device: f32 restatements of the evaluation kernels' arithmetic pass their bounds at the shapes of
tests/test_gpu_eval_paths.py, planted faults fail them, the case tables reach every host predicate, and the precision / recall cases leave
(almost) no flag undecided."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import eval_check as ec
import test_gpu_eval_paths as T

F32, F16, F64 = torch.float32, torch.float16, torch.float64


def _fails(fn):
    with pytest.raises((ec.BoundError, AssertionError)):
        fn()


def _both(values, what):
    assert {bool(v) for v in values} == {True, False}, f"{what}: not both taken and not taken"


def _all(seen, wanted, what):
    assert set(wanted) <= set(seen), f"{what}: missing {sorted(set(wanted) - set(seen), key=str)}"


def _by(cases, name):
    return next(c for c in cases if c["name"] == name)


# ----------------------------------------------------------------------------- convolution
def conv_f32(c, x, w, b, drop_tap=False, skip_last_k=False, anchor_end=False):
    """The convolution in f32, tap by tap (another order than the kernel's: the bound holds for every order).  Faults: drop the tap that reads
    pixel (0, 0) for output (0, 0); zero the last 16-wide K step; anchor the windows at the far edge (padding on the wrong side)."""
    B, H, W, Cin = x.shape
    kh, kw, sh, sw, ph, pw = c["kh"], c["kw"], c["sh"], c["sw"], c["ph"], c["pw"]
    Ho, Wo = ec.conv_out(H, W, kh, kw, sh, sw, ph, pw)
    ry, rx = ((H + 2 * ph - kh) % sh, (W + 2 * pw - kw) % sw) if anchor_end else (0, 0)
    xp = Fn.pad(x, (0, 0, pw, pw + kw, ph, ph + kh))
    wk = w.reshape(w.shape[0], -1).clone()
    if skip_last_k:
        K = wk.shape[1]
        wk[:, (K - 1) // 16 * 16:] = 0
    wk = wk.view_as(w)
    out = torch.zeros(B, Ho, Wo, w.shape[0])
    for ky in range(kh):
        for kx in range(kw):
            patch = xp[:, ry + ky:ry + ky + sh * Ho:sh, rx + kx:rx + kx + sw * Wo:sw, :]
            t = patch @ wk[:, ky, kx, :].T
            if drop_tap and ky == ph and kx == pw:
                t[:, 0, 0, :] = 0
            out = out + t
    if b is not None:
        out = out + b
    return out.clamp_min(0) if c["relu"] else out


@pytest.mark.parametrize("c", T.CONV, ids=T._ids(T.CONV))
def test_conv_restatement_and_faults(c):
    x, w, b = T.conv_inputs(c)
    ref, bound, _ = T.conv_reference(c)
    assert ec.finite(ref, bound) and ref.shape[:3] == (c["B"],) + ec.conv_out(c["H"], c["W"], c["kh"], c["kw"], c["sh"], c["sw"], c["ph"], c["pw"])
    ec.check(c["name"], conv_f32(c, x, w, b), ref, bound)
    c0 = dict(c, relu=0)
    ref0, bound0, _ = ec.conv_ref(x, w, b, c["sh"], c["sw"], c["ph"], c["pw"], 0)
    _fails(lambda: ec.check(c["name"], conv_f32(c0, x, w, b, drop_tap=True), ref0, bound0))
    _fails(lambda: ec.check(c["name"], conv_f32(c0, x, w, b, skip_last_k=True), ref0, bound0))
    if (c["H"] + 2 * c["ph"] - c["kh"]) % c["sh"] or (c["W"] + 2 * c["pw"] - c["kw"]) % c["sw"]:
        _fails(lambda: ec.check(c["name"], conv_f32(c0, x, w, b, anchor_end=True), ref0, bound0))


def test_conv_wrong_side_case_exists():
    assert any(c["sh"] == 2 and (c["H"] + 2 * c["ph"] - c["kh"]) % 2 for c in T.CONV)


# ----------------------------------------------------------------------------- pools
def pool_f32(x, k, s, p, mode, div_k2=False, pad_zero_wins=False):
    t, m = ec._windows(x.double(), k, s, p, 0.0 if (mode == 1 or pad_zero_wins) else -math.inf)
    t = t.float()
    if mode == 0:
        return t.max(-1).values
    acc = torch.zeros_like(t[..., 0])
    for j in range(k * k):                                          # in-image taps in order; an out-of-image tap adds an exact 0
        acc = acc + t[..., j]
    n = torch.full_like(acc, float(k * k)) if div_k2 else m.sum(-1).float().expand_as(acc)
    return acc / n


@pytest.mark.parametrize("c", T.POOL, ids=T._ids(T.POOL))
def test_pool_restatement_and_faults(c):
    x = T.pool_inputs(c)
    k, s, p = c["k"], c["s"], c["p"]
    if c["mode"] == 0:
        want = ec.maxpool_exact(x, k, s, p)
        assert torch.equal(pool_f32(x, k, s, p, 0), want)
        assert torch.equal(want, Fn.max_pool2d(x.permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1))
        if c["neg"]:
            assert not torch.equal(pool_f32(x, k, s, p, 0, pad_zero_wins=True), want)
    else:
        ref, bound = ec.avgpool_ref(x, k, s, p)
        assert torch.allclose(ref, Fn.avg_pool2d(x.double().permute(0, 3, 1, 2), k, s, p, count_include_pad=False).permute(0, 2, 3, 1), atol=1e-12)
        ec.check(c["name"], pool_f32(x, k, s, p, 1), ref, bound)
        if p > 0:
            _fails(lambda: ec.check(c["name"], pool_f32(x, k, s, p, 1, div_k2=True), ref, bound))


@pytest.mark.parametrize("c", T.GAP, ids=T._ids(T.GAP))
def test_global_avgpool_restatement(c):
    x = 0.5 + torch.randn(c["B"], c["HW"], c["C"], generator=T._gen("gap" + c["name"]))
    s = torch.zeros(c["B"], c["C"])
    for j in range(c["HW"]):
        s = s + x[:, j]
    ref, bound = ec.global_avgpool_ref(x)
    ec.check(c["name"], s / float(c["HW"]), ref, bound)
    if c["HW"] > 1:
        _fails(lambda: ec.check(c["name"], s / float(c["HW"] - 1), ref, bound))


# ----------------------------------------------------------------------------- pre-processing
def fid_preprocess_f32(img, Ho, Wo, no_half=False):
    """fid_preprocess_kernel in numpy float32 (unfused)."""
    f = np.float32
    B, H, W, _ = img.shape
    def axis(n_in, n_out):
        sc = f(n_in) / f(n_out)
        o = np.arange(n_out, dtype=np.float32)
        s = np.maximum(sc * (o + f(0.5)) - (f(0) if no_half else f(0.5)), f(0))
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        i1 = i0 + (i0 < n_in - 1)
        l1 = np.clip(s - i0.astype(np.float32), f(0), f(1))
        return i0, i1, l1, f(1) - l1
    y0, y1, ly1, ly0 = axis(H, Ho)
    x0, x1, lx1, lx0 = axis(W, Wo)
    V = img.astype(np.float32) / f(255)
    ly0, ly1, lx0, lx1 = ly0[None, :, None, None], ly1[None, :, None, None], lx0[None, None, :, None], lx1[None, None, :, None]
    v = ly0 * (lx0 * V[:, y0][:, :, x0] + lx1 * V[:, y0][:, :, x1]) + ly1 * (lx0 * V[:, y1][:, :, x0] + lx1 * V[:, y1][:, :, x1])
    return torch.from_numpy(v * f(2) - f(1))


@pytest.mark.parametrize("c", T.FIDPRE, ids=T._ids(T.FIDPRE))
def test_fid_preprocess_restatement_and_fault(c):
    img = T.image_u8(c, "fidpre")
    ref, bound = ec.fid_preprocess_ref(img, c["Ho"], c["Wo"])
    want = Fn.interpolate(img.double().permute(0, 3, 1, 2) / 255, (c["Ho"], c["Wo"]), mode="bilinear", align_corners=False) * 2 - 1
    assert torch.allclose(ref, want.permute(0, 2, 3, 1), atol=1e-5)      # the definition (ATen takes the scale in f64 here: a loose cross-check)
    assert float(bound.max()) < 2e-5
    ec.check(c["name"], fid_preprocess_f32(img.numpy(), c["Ho"], c["Wo"]), ref, bound)
    if (c["H"], c["W"]) != (1, 1):
        _fails(lambda: ec.check(c["name"], fid_preprocess_f32(img.numpy(), c["Ho"], c["Wo"], no_half=True), ref, bound))


@pytest.mark.parametrize("c", T.ADMPRE, ids=T._ids(T.ADMPRE))
def test_adm_preprocess_restatement_and_fault(c):
    img = T.image_u8(c, "admpre")
    got = ec.adm_preprocess_f32(img.numpy(), c["Ho"], c["Wo"])
    # the definition in f64 (TF1 legacy resize), from the f32 scale: the f32 restatement is within a few roundings of it
    B, H, W, _ = img.shape
    sy = torch.arange(c["Ho"], dtype=F64) * float(np.float32(H) / np.float32(c["Ho"]))
    sx = torch.arange(c["Wo"], dtype=F64) * float(np.float32(W) / np.float32(c["Wo"]))
    y0, x0 = sy.floor().long().clamp_max(H - 1), sx.floor().long().clamp_max(W - 1)
    y1, x1 = (y0 + 1).clamp_max(H - 1), (x0 + 1).clamp_max(W - 1)
    yl, xl = (sy - sy.floor())[None, :, None, None], (sx - sx.floor())[None, None, :, None]
    I = img.double()
    top = I[:, y0][:, :, x0] + (I[:, y0][:, :, x1] - I[:, y0][:, :, x0]) * xl
    bot = I[:, y1][:, :, x0] + (I[:, y1][:, :, x1] - I[:, y1][:, :, x0]) * xl
    want = ((top + (bot - top) * yl) - 128) / 128
    tol = 2 * ec.U * (255 * 40 + 255 * 6) / 128                      # coordinate roundings (|s| < 40) and six roundings of values <= 255
    assert float((torch.from_numpy(got).double() - want).abs().max()) <= tol
    if (c["H"], c["W"]) != (c["Ho"], c["Wo"]) and (c["H"], c["W"]) != (1, 1):
        assert not np.array_equal(ec.adm_preprocess_f32(img.numpy(), c["Ho"], c["Wo"], half_pixel=True), got)
    if c["name"] == "clamp_last":                                    # the last outputs' upper tap is held at in - 1
        assert int(y0.max()) == H - 1 and int(x0.max()) == W - 1


# ----------------------------------------------------------------------------- f64 reductions
@pytest.mark.parametrize("c", T.STATS, ids=T._ids(T.STATS))
def test_fid_stats_restatement_and_fault(c):
    f1, _, shift, s0, c0 = T.stats_inputs(c)
    Y = f1.double().numpy() - shift.double().numpy()
    r = ec.fid_stats_ref(f1.numpy(), shift.numpy(), s0.numpy(), c0.numpy())
    acc_s, acc_c = np.zeros(c["D"]), np.zeros((c["D"], c["D"]))
    for i in range(c["n"]):
        acc_s, acc_c = acc_s + Y[i], acc_c + np.outer(Y[i], Y[i])
    ec.check64("sum", s0.numpy() + acc_s, *r["sum"])
    ec.check64("cross", c0.numpy() + acc_c, *r["cross"])
    Yf = (f1 - shift).numpy()                                       # the subtraction in f32: one f32 rounding per term must fail
    if c["n"] > 1:
        _fails(lambda: ec.check64("cross", c0.numpy() + Yf.astype(np.float64).T @ Yf.astype(np.float64), *r["cross"]))


@pytest.mark.parametrize("c", T.SQN, ids=T._ids(T.SQN))
def test_row_sqnorms_restatement_and_fault(c):
    x = torch.randn(c["M"], c["D"], generator=T._gen("sqn" + c["name"]))
    ref, bound = ec.row_sqnorms_ref(x)
    ec.check(c["name"], (x.double() ** 2).sum(-1).float(), ref, bound)
    if c["D"] >= 63:
        _fails(lambda: ec.check(c["name"], (x * x).cumsum(-1)[:, -1] * (1 + 2.0 ** -22), ref, bound))


@pytest.mark.parametrize("c", T.LOGITS, ids=T._ids(T.LOGITS))
def test_logits_restatement_and_fault(c):
    u, w = T.logits_inputs(c)
    ref, bound = ec.logits_ref(u, w)
    ec.check(c["name"], u @ w.T, ref, bound)
    D = c["D"]
    if D > 1:                                                       # the last K step dropped
        _fails(lambda: ec.check(c["name"], u[:, :(D - 1) // 16 * 16 or 1] @ w[:, :(D - 1) // 16 * 16 or 1].T, ref, bound))


# ----------------------------------------------------------------------------- k-NN radii and flags
def dist_f32(u, nu, v, nv):
    return ((nu[:, None] - 2.0 * (u @ v.T)) + nv[None, :]).clamp_min(0.0)


@pytest.mark.parametrize("c", T.KNN, ids=T._ids(T.KNN))
def test_knn_restatement_and_fault(c):
    x, nrm = T.knn_inputs(c)
    d, e = ec.pair_dist(x, nrm, x, nrm)
    lo, hi = ec.knn_interval(d, e, c["nhood"])
    assert ec.finite(lo, hi) and bool((lo <= hi).all())
    srt = dist_f32(x, nrm, x, nrm).sort(-1).values
    idx = torch.tensor(c["nhood"])
    ec.check_interval(c["name"], srt[:, idx], lo, hi)
    if max(c["nhood"]) > 1:                                          # radii taken one place too low
        _fails(lambda: ec.check_interval(c["name"], srt[:, (idx - 1).clamp_min(0)], lo, hi))
    # the interval is tight: its half width stays within the rounding errors of |x|^2-sized quantities
    assert float(((hi - lo) / (1 + nrm.double()[:, None])).max()) < 64 * c["D"] * ec.U


def flags_f32(u, nu, ru, v, nv, rv, strict=False):
    d = dist_f32(u, nu, v, nv)
    cmp = torch.lt if strict else torch.le
    return cmp(d[:, :, None], rv[None, :, :]).any(1).int(), cmp(d[:, :, None], ru[:, None, :]).any(0).int()


@pytest.mark.parametrize("c", T.PRF, ids=T._ids(T.PRF))
def test_pr_flags_reference_decides_and_fault(c):
    u, nu, ru, v, nv, rv = T.pr_inputs(c)
    u1, u0, v1, v0 = T.pr_reference(c)
    cap = 0.0 if c["kind"] == "int" else 0.01
    gu, gv = flags_f32(u, nu, ru, v, nv, rv)
    und_u, und_v = ec.check_flags(c["name"] + " u_in", gu, u1, u0, cap), ec.check_flags(c["name"] + " v_in", gv, v1, v0, cap)
    print(f"{c['name']}: undecided {und_u:.4f} / {und_v:.4f}; ones {float(u1.double().mean()):.2f} / {float(v1.double().mean()):.2f}")
    if c["kind"] == "far":
        assert bool(u0.all()) and bool(v0.all())
    else:
        for one, zero, what in ((u1, u0, "u_in"), (v1, v0, "v_in")):
            assert bool(one.any()) and bool(zero.any()), f"{c['name']} {what}: the decided flags do not take both values"
    if c["kind"] == "int":
        assert bool((u1 ^ u0).all()) and bool((v1 ^ v0).all())
        su, sv = flags_f32(u, nu, ru, v, nv, rv, strict=True)       # `<` where the kernel says `<=`: the ties d == r decide
        if c["M"] > 10:                                             # (the 5 x 3 case has no flag that a tie alone decides)
            _fails(lambda: (ec.check_flags(c["name"], su, u1, u0, 0.0), ec.check_flags(c["name"], sv, v1, v0, 0.0)))


# ----------------------------------------------------------------------------- softmax + Inception Score sums
def softmax_is_f32(x, split, cross_split=False, nan_log=False):
    M, C = x.shape
    E = torch.exp(x - x.max(-1, keepdim=True).values)
    p = E / E.sum(-1, keepdim=True)
    pd = p.double()
    with np.errstate(all="ignore"):
        h = (pd * pd.log()).nan_to_num(nan=math.nan if nan_log else 0.0).sum(-1)
    ns, cps = (M + split - 1) // split, (split + 127) // 128
    S = torch.zeros(ns, C, dtype=F64)
    for s in range(ns):
        for q in range(cps):
            r0 = s * split + q * 128
            r1 = min(r0 + 128, M) if cross_split else min(r0 + 128, s * split + split, M)
            if r1 > r0:
                S[s] += pd[r0:r1].sum(0)
    return p, h, S


@pytest.mark.parametrize("c", T.IS_CASES, ids=T._ids(T.IS_CASES))
def test_softmax_is_restatement_and_faults(c):
    x = T.is_inputs(c)
    ref = ec.softmax_is_ref(x, c["split"])
    p, h, S = softmax_is_f32(x, c["split"])
    assert ec.finite(*ref["p"])
    ec.check(c["name"] + " p", p, *ref["p"])
    ec.check64(c["name"] + " h", h.numpy(), *ref["h"])
    ec.check64(c["name"] + " S", S.numpy(), *ref["S"])
    assert float(np.max(ref["h"][1])) < 1e-4 and float(np.max(ref["S"][1])) < 1e-4      # the bounds stay those of f32 roundings
    if c["C"] > 1:
        assert float(p[0, c["C"] // 2]) == 0.0
        _fails(lambda: ec.check64(c["name"] + " h", softmax_is_f32(x, c["split"], nan_log=True)[1].numpy(), *ref["h"]))
    ns = (c["M"] + c["split"] - 1) // c["split"]
    if c["split"] % 128 and ns > 1:
        _fails(lambda: ec.check64(c["name"] + " S", softmax_is_f32(x, c["split"], cross_split=True)[2].numpy(), *ref["S"]))


def test_softmax_is_cases_reach_the_chunk_edges():
    S = T.IS_CASES
    _all({c["M"] for c in S}, (1, 127, 128, 129, 300), "M")
    _all({c["C"] for c in S}, (1, 255, 256, 257, 1008), "C")
    _all({c["split"] for c in S}, (1, 100, 128, 129), "split")
    assert any(c["split"] > c["M"] for c in S)
    assert any(c["split"] > 128 and c["split"] % 128 and c["M"] > c["split"] for c in S), "a split above one chunk with a partly filled last chunk"


# ----------------------------------------------------------------------------- LPIPS pre-processing, quantiser
@pytest.mark.parametrize("c", T.LPREP, ids=T._ids(T.LPREP))
def test_lpips_prep_restatement_and_fault(c):
    a, b = T.lprep_inputs(c)
    x = torch.cat([a, b], 0).permute(0, 2, 3, 1)
    sh, sc = torch.tensor(ec.LP_SHIFT, dtype=F32), torch.tensor(ec.LP_SCALE, dtype=F32)
    y = (x - sh) / sc
    ec.check(c["name"], y, *ec.lpips_prep_ref(a, b, F32))
    ec.check(c["name"], y.clamp(-65504, 65504).half(), *ec.lpips_prep_ref(a, b, F16))
    _fails(lambda: ec.check(c["name"], (x - sh) * (1 / sc), *ec.lpips_prep_ref(a, b, F32)))      # a reciprocal multiply is not the division
    _fails(lambda: ec.check(c["name"], y.half(), *ec.lpips_prep_ref(a, b, F16)))                    # no saturation: inf
    assert (2 * c["B"] * c["H"] * c["W"]) % 256 or c["name"] == "B3_16x16"


@pytest.mark.parametrize("c", T.QZ, ids=T._ids(T.QZ))
def test_quantizer_restatement_and_fault(c):
    dec, _ = T.qz_inputs(c)
    q = ec.quantize_f32(dec.numpy())
    want = torch.clamp(127.5 * dec + 128.0, 0, 255).to(torch.uint8).numpy()        # the expression as torch evaluates it
    assert np.array_equal(q, want)
    if c["kind"] == "rand" and dec.numel() > 100:
        assert not np.array_equal(ec.quantize_f32(dec.numpy(), nearest=True), q)
    a = np.arange(256, dtype=np.uint8)[None, :]
    assert int(ec.sse_exact(a, a[:, ::-1].copy())[0]) == sum((i - (255 - i)) ** 2 for i in range(256))


# ----------------------------------------------------------------------------- LPIPS head, SSIM
def lpips_layer_f32(f, lw, old, B, eps_inside=False):
    f = f.float()
    a, c = f[:B], f[B:]
    s0, s1 = (a * a).sum(-1, keepdim=True), (c * c).sum(-1, keepdim=True)
    if eps_inside:
        r0, r1 = 1.0 / (s0 + 1e-10).sqrt(), 1.0 / (s1 + 1e-10).sqrt()
    else:
        r0, r1 = 1.0 / (s0.sqrt() + 1e-10), 1.0 / (s1.sqrt() + 1e-10)
    dx = a * r0 - c * r1
    d = (lw * dx * dx).sum(-1)
    return old + (d.double().sum(-1) / f.shape[1]).float()


@pytest.mark.parametrize("c", T.LPL, ids=T._ids(T.LPL))
def test_lpips_layer_restatement_and_fault(c):
    f, lw, old = T.lpl_inputs(c)
    ref, bound = T.lpl_reference(c)
    assert ec.finite(ref, bound) and float(bound.max()) < 2e-5
    got = lpips_layer_f32(f, lw, old, c["B"])
    ec.check(c["name"], got, ref, bound)
    if c["equal"]:
        assert torch.equal(got, old)
    elif c["h"] * c["w"] in (7, 391, 513):
        _fails(lambda: ec.check(c["name"], lpips_layer_f32(f, lw, old, c["B"], eps_inside=True), ref, bound))


def ssim_f32(X, Y, lo, hi, dr, crop=True, clamp=True):
    """ssim_tile_kernel's shifted formulation in f32, tile by tile.  Faults: reflect-padded and averaged over the whole image; no clamp."""
    f = np.float32
    B, C, H, W = X.shape
    c1, c2 = ec.ssim_consts(dr)
    d = (torch.arange(11, dtype=F32) - 5) / 1.5
    g = torch.exp(-(d * d) / 2)
    g = g / g.sum()
    x, y = X.reshape(B * C, H, W), Y.reshape(B * C, H, W)
    if clamp:
        x, y = x.clamp(f(lo), f(hi)), y.clamp(f(lo), f(hi))
    if not crop:
        x, y = Fn.pad(x[None], (5, 5, 5, 5), mode="reflect")[0], Fn.pad(y[None], (5, 5, 5, 5), mode="reflect")[0]
        H, W = H + 10, W + 10
    def blur(q):
        return (((q.unfold(2, 11, 1) * g).sum(-1)).unfold(1, 11, 1) * g).sum(-1)
    tot = torch.zeros(B * C, dtype=F64)
    for oy0 in range(5, H - 5, 32):
        for ox0 in range(5, W - 5, 32):
            y1, x1 = min(oy0 + 37, H), min(ox0 + 37, W)
            shx, shy = x[:, oy0, ox0][:, None, None], y[:, oy0, ox0][:, None, None]
            xs, ys = x[:, oy0 - 5:y1, ox0 - 5:x1] - shx, y[:, oy0 - 5:y1, ox0 - 5:x1] - shy
            m0, m1, m2, m3, m4 = (blur(q) for q in (xs, ys, xs * xs, ys * ys, xs * ys))
            vx, vy, cxy = (m2 - m0 * m0).clamp_min(0), (m3 - m1 * m1).clamp_min(0), m4 - m0 * m1
            mx, my = m0 + shx, m1 + shy
            sm = ((2 * (mx * my) + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
            tot += sm.sum((1, 2)).double()
    return (tot.reshape(B, C).sum(-1) / (C * (H - 10) * (W - 10))).float()


@pytest.mark.parametrize("c", T.SSIM, ids=T._ids(T.SSIM))
def test_ssim_restatement_and_faults(c):
    X, Y = T.ssim_inputs(c)
    ref, bound = T.ssim_reference(c)
    assert ec.finite(ref, bound) and float(bound.max()) < 1e-4
    assert torch.allclose(ref, ec.ssim_plain(X, Y, c["lo"], c["hi"], c["dr"]), atol=1e-9), "the shifted reference is not the definition"
    got = ssim_f32(X, Y, c["lo"], c["hi"], c["dr"])
    ec.check(c["name"], got, ref, bound)
    if c["kind"] == "const":
        assert torch.equal(got, torch.ones(c["B"]))
    if c["kind"] == "rand":
        _fails(lambda: ec.check(c["name"], ssim_f32(X, Y, c["lo"], c["hi"], c["dr"], crop=False), ref, bound))
        if T.ssim_clamp_active(c):
            _fails(lambda: ec.check(c["name"], ssim_f32(X, Y, c["lo"], c["hi"], c["dr"], clamp=False), ref, bound))


# ----------------------------------------------------------------------------- the tables reach every host predicate
def test_case_names_are_unique():
    for tab in (T.CONV, T.POOL, T.GAP, T.FIDPRE, T.ADMPRE, T.STATS, T.SQN, T.LOGITS, T.KNN, T.PRF, T.IS_CASES, T.LPREP, T.QZ, T.LPL, T.SSIM):
        names = [c["name"] for c in tab]
        assert len(names) == len(set(names))


def test_case_table_covers_every_predicate():
    # ---- convolution: `vec`, by each of its five reasons alone
    V = [T.conv_vec_reasons(c) for c in T.CONV]
    assert any(all(v.values()) for v in V), "no vector case"
    for r in ("cin", "xoff", "ldx", "x_al", "w_al"):
        assert any(not v[r] and all(v[k] for k in v if k != r) for v in V), f"conv: no case that is scalar because of {r} alone"
    _all({c["Cin"] for c in T.CONV if all(T.conv_vec_reasons(c).values())}, (4, 8, 12, 16, 20, 32), "conv vector Cin")
    _all({c["Cin"] for c in T.CONV}, (3, 5), "conv scalar Cin")
    _all({c["Cout"] for c in T.CONV}, (1, 63, 64, 65, 96), "conv Cout")
    _all({(c["kh"], c["kw"]) for c in T.CONV}, ((1, 1), (3, 3), (1, 7), (7, 1), (5, 5)), "conv kernels")
    _both([c["relu"] for c in T.CONV], "conv relu")
    _both([c["bias"] for c in T.CONV], "conv bias given")
    for vec in (True, False):
        sub = [c for c in T.CONV if all(T.conv_vec_reasons(c).values()) == vec]
        _both([c["relu"] for c in sub], f"conv vec={vec} relu")
        _both([c["bias"] for c in sub], f"conv vec={vec} bias")
    Ms = [T.conv_M(c) for c in T.CONV]
    assert 1 in Ms and 128 in Ms and any(1 < m < 128 for m in Ms) and any(m > 128 and m % 128 for m in Ms)
    assert any(T.conv_M(c) < 128 and c["B"] == 2 for c in T.CONV), "one partly filled tile spanning two images"
    assert any(c["sh"] != c["sw"] for c in T.CONV) and any(c["ph"] != c["pw"] for c in T.CONV)
    assert any(c["sh"] == 2 and (c["H"] + 2 * c["ph"] - c["kh"]) % 2 for c in T.CONV)
    assert any(c["kh"] > c["H"] for c in T.CONV), "a kernel larger than the unpadded image"
    assert any(c["ldx"] > c["Cin"] and c["ldo"] > c["Cout"] for c in T.CONV), "input and output slices"
    # a 16-wide K step that spans several taps (Cin < 16) on the vector path
    assert {4, 8, 12} <= {c["Cin"] for c in T.CONV if all(T.conv_vec_reasons(c).values()) and c["kh"] * c["kw"] > 1}
    # ---- pools
    _both([c["mode"] for c in T.POOL], "pool mode")
    for m in (0, 1):
        _all({(c["k"], c["s"], c["p"]) for c in T.POOL if c["mode"] == m}, ((3, 1, 1), (3, 2, 0), (1, 1, 0), (2, 2, 0), (5, 1, 2)), f"pool mode {m} (k, s, p)")
        _all({c["C"] for c in T.POOL if c["mode"] == m}, (1, 65), f"pool mode {m} C")
        assert any(T.pool_total(c) % 256 for c in T.POOL if c["mode"] == m) and any(c["ldx"] > c["C"] and c["ldo"] > c["C"] for c in T.POOL if c["mode"] == m)
        assert any(T.pool_total(c) > 256 for c in T.POOL if c["mode"] == m), "more than one block"
    assert all(c["H"] != c["W"] for c in T.POOL) and any(c["neg"] and c["mode"] == 0 and c["p"] > 0 for c in T.POOL)
    _all({c["HW"] for c in T.GAP}, (1, 64, 289), "global_avgpool HW")
    # ---- statistics, norms
    _all({c["D"] for c in T.STATS}, (1, 63, 64, 65, 200), "fid_stats D")
    _all({n for c in T.STATS for n in (c["n"], c["n2"])}, (1, 15, 16, 17, 50), "fid_stats n")
    _all({c["M"] for c in T.SQN}, (1, 4, 5), "row_sqnorms M")
    _all({c["D"] for c in T.SQN}, (1, 63, 64, 65, 2023), "row_sqnorms D")
    # ---- launch_pairwise: `vec`, by each of its three reasons alone, for each epilogue
    tabs = dict(logits=[T.pair_vec_reasons(c["D"], c["uoff"], c["woff"]) for c in T.LOGITS],
                knn=[T.pair_vec_reasons(c["D"], c["off"], c["off"]) for c in T.KNN], pr=[T.pair_vec_reasons(c["D"], c["off"], c["off"]) for c in T.PRF])
    for name, V in tabs.items():
        assert any(all(v.values()) for v in V), f"{name}: no vector case"
        assert any(not v["d"] and v["u_al"] and v["v_al"] for v in V), f"{name}: no case that is scalar because of D alone"
        assert any(v["d"] and not (v["u_al"] and v["v_al"]) for v in V), f"{name}: no case that is scalar because of a pointer alone"
    assert any(v["d"] and not v["u_al"] and v["v_al"] for v in tabs["logits"]) and any(v["d"] and v["u_al"] and not v["v_al"] for v in tabs["logits"])
    _all({c["M"] for c in T.LOGITS}, (1, 127, 128, 129, 300), "logits M")
    _all({c["N"] for c in T.LOGITS}, (1, 63, 64, 65, 130), "logits N")
    _all({c["D"] for c in T.LOGITS}, (1, 3, 4, 15, 16, 17, 20, 36), "logits D")
    # ---- knn_radii / pr_flags: nsplit below, at and above the column-tile count
    for c in T.KNN + T.PRF:
        ct, ns = T.col_tiles(c["N"]), T.nsplit_set(c["N"])
        assert ct in ns and any(n > ct for n in ns) and 1 in ns and 2 in ns
    assert any(any(n < T.col_tiles(c["N"]) for n in T.nsplit_set(c["N"])) for c in T.KNN)
    assert any(any(n < T.col_tiles(c["N"]) for n in T.nsplit_set(c["N"])) for c in T.PRF)
    # a split count that does not divide the tile count: the last split is short (tps * nsplit > tiles)
    assert any(T.col_tiles(c["N"]) % n for c in T.KNN + T.PRF for n in T.nsplit_set(c["N"]) if n < T.col_tiles(c["N"]))
    _all({c["N"] for c in T.KNN}, (8, 65, 129, 200), "knn N")
    _all({c["D"] for c in T.KNN}, (3, 7, 20, 36), "knn D")
    _all({k for c in T.KNN for k in c["nhood"]}, range(8), "knn index")
    _all({len(c["nhood"]) for c in T.KNN}, (1, 8), "knn nk")
    assert any(c["N"] == max(c["nhood"]) + 1 for c in T.KNN)
    _all({(c["M"], c["N"]) for c in T.PRF}, ((131, 70), (131, 150), (257, 193), (5, 3), (300, 129)), "pr shapes")
    _all({len(c["nhood"]) for c in T.PRF}, (1, 2, 8), "pr nk")
    _all({c["kind"] for c in T.PRF}, ("gauss", "int", "far"), "pr kinds")
    assert any(c["M"] < 128 and c["N"] < 64 for c in T.PRF), "padded rows and columns"
    # ---- quantiser: the block cap
    _both([T.qz_capped(c["H"] * c["W"]) for c in T.QZ], "qz_blocks cap (recon_quantize_psnr)")
    _both([T.qz_capped(3 * c["H"] * c["W"]) for c in T.QZ], "qz_blocks cap (sse_u8)")
    _all({c["H"] * c["W"] for c in T.QZ}, (1, 255, 1025, 513 * 513), "quantiser HW")
    # ---- lpips_layer: each C for each T, the chunk cap; SSIM: the tile raggedness and the clamp
    _all({(c["C"], c["T"]) for c in T.LPL}, {(C, t) for C in (64, 128, 256, 512) for t in (F32, F16)}, "lpips_layer C x T")
    for t in (F32, F16):
        _both([T.lpips_capped(c["h"] * c["w"]) for c in T.LPL if c["T"] == t], f"lpips_chunks cap, {t}")
        assert any(T.lpips_capped(c["h"] * c["w"]) and c["C"] == 64 for c in T.LPL if c["T"] == t)
        _both([c["equal"] for c in T.LPL if c["T"] == t], f"equal halves, {t}")
    _all({c["h"] * c["w"] for c in T.LPL}, (1, 7, 391, 513), "lpips_layer HW")
    _all({c["H"] for c in T.SSIM}, (11, 12, 42, 43, 75), "ssim H")
    _all({c["W"] for c in T.SSIM}, (11, 12, 42, 43, 75), "ssim W")
    _all({c["C"] for c in T.SSIM}, (1, 3), "ssim C")
    _both([T.ssim_clamp_active(c) for c in T.SSIM if c["kind"] == "rand"], "ssim clamp active")
    assert len({c["dr"] for c in T.SSIM}) >= 2 and {"const", "negconst"} <= {c["kind"] for c in T.SSIM}
    assert any(c["B"] == 1 for c in T.LPREP) and all(c["H"] != c["W"] for c in T.LPREP[:2])
