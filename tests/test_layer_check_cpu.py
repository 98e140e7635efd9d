"""CPU checks of tests/layer_check.py and of the case tables of tests/test_gpu_layer_paths.py (no GPU needed).

  - f32 emulations of every family layer_check.py bounds, in torch, over three summation associations (sequential, pairwise, 16 lanes then a
    butterfly) and fused / unfused multiply-adds: each must sit inside the bound with zero excluded elements, through the same `check`
    the device tests call;
  - planted faults (a wrong formula evaluated in f64, so the only error IS the fault): each must be rejected by the bound;
  - test_case_table_covers_every_predicate: each host predicate restated as a function of the case's shape is both taken and not taken
    by the device tables, and every template instantiation is reached.
"""
import math

import pytest
import torch
import torch.nn.functional as Fn

import layer_check as lc
import test_gpu_layer_paths as T

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
ASSOC = ("seq", "pair", "lanes")
EPS = 1e-6


def _g(seed):
    return torch.Generator().manual_seed(seed)


def ssum(t, dim, assoc):
    """f32 sum along `dim` in the given association -> (sum, depth of the longest chain of additions)."""
    t = t.movedim(dim, 0)
    n = t.shape[0]

    def pair(u):
        p = 1 << max(math.ceil(math.log2(u.shape[0])), 0)
        u = torch.cat([u, torch.zeros((p - u.shape[0],) + u.shape[1:], dtype=u.dtype)])
        while u.shape[0] > 1:
            u = u[0::2] + u[1::2]
        return u[0], max(int(math.log2(p)), 1)

    def seq(u):
        acc = u[0].clone()
        for i in range(1, u.shape[0]):
            acc = acc + u[i]
        return acc, max(u.shape[0] - 1, 1)

    if assoc == "seq":
        return seq(t)
    if assoc == "pair":
        return pair(t)
    pad = (-n) % 16
    u = torch.cat([t, torch.zeros((pad,) + t.shape[1:], dtype=t.dtype)]).view((-1, 16) + t.shape[1:])
    a, d1 = seq(u)
    b, d2 = pair(a)
    return b, d1 + d2


def madd(a, b, c, fma):
    """a * b + c with one rounding (fused) or two."""
    return (a.double() * b.double() + c.double()).float() if fma else a * b + c


def ok(name, got, ref, bound):
    assert lc.finite(ref, bound)
    return lc.check(name, got, ref, bound)


def bad(name, got, ref, bound):
    assert lc.finite(ref, bound)
    with pytest.raises(lc.BoundError):
        lc.check(name, got, ref, bound)


# ----------------------------------------------------------------------------- LayerNorm
def emu_ln_fwd(x, w, b, assoc, fma):
    D = x.shape[1]
    invD = torch.tensor(1.0 / D, dtype=F32)
    s, d1 = ssum(x, 1, assoc)
    mu = s * invD
    c = x - mu[:, None]
    v, d2 = ssum(c * c, 1, assoc)
    rs = (v * invD + torch.tensor(EPS, dtype=F32)).double().rsqrt().float()
    return madd(c * rs[:, None], w, b, fma), mu, rs, d1, d2


def _ln_inputs(M, D, fam, seed):
    g = _g(seed)
    x = torch.randn(M, D, generator=g)
    if fam == "offset":
        x = 100.0 + x
    elif fam == "tiny":
        x = 1e-3 * x
    return x, 1 + 0.3 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g), g


LN_SHAPES = ((18, 4, "unit"), (5, 196, "offset"), (37, 388, "unit"), (5, 1280, "offset"), (1, 772, "unit"), (18, 192, "tiny"))


@pytest.mark.parametrize("fma", (False, True))
@pytest.mark.parametrize("assoc", ASSOC)
def test_emulation_layernorm_fwd_inside_bounds(assoc, fma):
    for i, (M, D, fam) in enumerate(LN_SHAPES):
        x, w, b, _ = _ln_inputs(M, D, fam, 10 + i)
        y, mu, rs, d1, d2 = emu_ln_fwd(x, w, b, assoc, fma)
        for Tt in T.TYPES:
            ref = lc.ln_fwd_ref(x, w, b, EPS, Tt, d_mean=d1, d_var=d2 + 1)         # + 1: the product of an unfused c * c term
            ok("y", y.to(Tt), *ref["y"])
        ok("mean", mu, *ref["mean"])
        ok("rstd", rs, *ref["rstd"])


def _ln_stats(x):
    xd = x.double()
    mean = xd.mean(-1)
    return mean.float(), (((xd - mean[:, None]) ** 2).mean(-1) + EPS).rsqrt().float()


def emu_ln_bwd(g, x, w, mean, rstd, dx0, dw0, db0, beta, assoc, fma):
    D = x.shape[1]
    invD = torch.tensor(1.0 / D, dtype=F32)
    gf = g.float()
    xh = (x - mean[:, None]) * rstd[:, None]
    gy = gf * w
    s1, d1 = ssum(gy, 1, assoc)
    s2, d2 = ssum(gy * xh, 1, assoc)
    s1, s2 = s1 * invD, s2 * invD
    inner = madd(-xh, s2[:, None], gy - s1[:, None], fma)
    dx = madd(rstd[:, None], inner, dx0, fma)
    dw, dc = ssum(gf * xh, 0, assoc)
    db, _ = ssum(gf, 0, assoc)
    if beta:
        dw, db = dw + dw0, db + db0
    return dx, dw, db, max(d1, d2) + 1, dc + 2


@pytest.mark.parametrize("fma", (False, True))
@pytest.mark.parametrize("assoc", ASSOC)
def test_emulation_layernorm_bwd_inside_bounds(assoc, fma):
    for i, (M, D, fam) in enumerate(LN_SHAPES):
        for Tt in T.TYPES:
            x, w, _, g = _ln_inputs(M, D, fam, 30 + i)
            mean, rstd = _ln_stats(x)
            go = torch.randn(M, D, generator=g).to(Tt)
            dx0, dw0, db0 = torch.randn(M, D, generator=g), torch.randn(D, generator=g), torch.randn(D, generator=g)
            beta = float(i % 2)
            dx, dw, db, dr, dc = emu_ln_bwd(go, x, w, mean, rstd, dx0, dw0, db0, beta, assoc, fma)
            ref = lc.ln_bwd_ref(go, x, w, mean, rstd, dx0, dw0, db0, beta, d_row=dr, d_col=dc)
            ok("dx", dx, *ref["dx"])
            ok("dx_cast", dx.to(Tt), *ref["dx_cast"])
            ok("dw", dw, *ref["dw"])
            ok("db", db, *ref["db"])


def test_planted_faults_layernorm():
    # forward, rows of spread 1e-3 (eps matters), offset rows (the centre matters) and D = 196 (a partly filled last chunk)
    x, w, b, _ = _ln_inputs(18, 192, "tiny", 50)
    X, W, B_ = x.double(), w.double(), b.double()
    xc = X - X.mean(-1, keepdim=True)
    ref = lc.ln_fwd_ref(x, w, b, EPS, F32)
    ok("sane", (xc * ((xc ** 2).mean(-1, keepdim=True) + EPS).rsqrt() * W + B_).float(), *ref["y"])
    bad("eps omitted", (xc * (xc ** 2).mean(-1, keepdim=True).rsqrt() * W + B_).float(), *ref["y"])
    bad("eps omitted: rstd", (xc ** 2).mean(-1).rsqrt().float(), *ref["rstd"])
    x, w, b, _ = _ln_inputs(5, 196, "offset", 51)
    X, W, B_ = x.double(), w.double(), b.double()
    xc = X - X.mean(-1, keepdim=True)
    ref = lc.ln_fwd_ref(x, w, b, EPS, F32)
    bad("variance about zero", (xc * ((X ** 2).mean(-1, keepdim=True) + EPS).rsqrt() * W + B_).float(), *ref["y"])
    m192 = X[:, :192].mean(-1, keepdim=True)
    c192 = X - m192
    bad("last chunk left out of the statistics", (c192 * ((c192[:, :192] ** 2).mean(-1, keepdim=True) + EPS).rsqrt() * W + B_).float(), *ref["y"])
    bad("last chunk left out: mean", m192[:, 0].float(), *ref["mean"])
    # backward
    x, w, _, g = _ln_inputs(37, 196, "unit", 52)
    mean, rstd = _ln_stats(x)
    go, dx0, z = torch.randn(37, 196, generator=g), torch.randn(37, 196, generator=g), torch.zeros(196)
    ref = lc.ln_bwd_ref(go, x, w, mean, rstd, dx0, z, z, 0.0)
    G, W, rs = go.double(), w.double(), rstd.double()[:, None]
    xh, gy = (x.double() - mean.double()[:, None]) * rs, go.double() * w.double()
    s1, s2 = gy.mean(-1, keepdim=True), (gy * xh).mean(-1, keepdim=True)
    ok("sane", (dx0.double() + rs * (gy - s1 - xh * s2)).float(), *ref["dx"])
    bad("- s1 dropped", (dx0.double() + rs * (gy - xh * s2)).float(), *ref["dx"])
    bad("dx not accumulated", (rs * (gy - s1 - xh * s2)).float(), *ref["dx"])
    bad("dw and db swapped: dw", G.sum(0).float(), *ref["dw"])
    bad("dw and db swapped: db", (G * xh).sum(0).float(), *ref["db"])
    bad("one partial row dropped: dw", (G * xh)[1:].sum(0).float(), *ref["dw"])
    old = torch.randn(196, generator=g)
    ref1 = lc.ln_bwd_ref(go, x, w, mean, rstd, dx0, old, old, 1.0)
    ok("sane beta", (old.double() + G.sum(0)).float(), *ref1["db"])
    bad("beta ignored: db", G.sum(0).float(), *ref1["db"])
    bad("beta ignored: dw", (G * xh).sum(0).float(), *ref1["dw"])


# ----------------------------------------------------------------------------- colsum, restore, thin GEMMs, label embedding
@pytest.mark.parametrize("assoc", ASSOC)
def test_emulation_sums_inside_bounds(assoc):
    g = _g(60)
    for Tt in T.TYPES:                                        # colsum
        x, old = torch.randn(300, 12, generator=g).to(Tt), torch.randn(12, generator=g)
        s, d = ssum(x.float(), 0, assoc)
        ok("colsum", s, *lc.colsum_ref(x, None, d))
        ok("colsum beta", s + old, *lc.colsum_ref(x, old, d + 1))
    B, L, keep, D = 3, 17, 5, 68                              # restore_tokens_bwd
    ids = torch.stack([torch.randperm(L, generator=g) for _ in range(B)])
    go = torch.randn(B, L, D, generator=g)
    s, d = ssum(go[ids >= keep], 0, assoc)
    dx, (rm, bm) = lc.restore_bwd_ref(go, ids, keep, d)
    ok("dmask", s, rm, bm)
    for b in range(B):
        for l in range(L):
            if ids[b, l] < keep:
                assert torch.equal(dx[b, ids[b, l]], go[b, l])
    for fma in (False, True):                                 # thin GEMMs
        M, N, K, rpb = 140, 12, 16, 52
        t, w, bias, pos = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g), torch.randn(rpb, N, generator=g)
        if fma:
            acc = bias[None].expand(M, N).clone()
            for k in range(K):
                acc = madd(t[:, k, None], w[None, :, k], acc, True)
        else:
            acc, _ = ssum(t[:, None, :] * w[None], 2, assoc)
            acc = acc + bias
        out = acc + pos[torch.arange(M) % rpb]
        for Tt in (F32, BF16):
            ok("thin_nt", out.to(Tt), *lc.thin_nt_ref(t, w, bias, pos, rpb, Tt))
        gg, w0, b0 = torch.randn(M, N, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
        if fma:
            dw, d = torch.zeros(N, K), M
            for m in range(M):
                dw = madd(gg[m, :, None], t[m][None], dw, True)
        else:
            dw, d = ssum(gg[:, :, None] * t[:, None, :], 0, assoc)
        db, d2 = ssum(gg, 0, assoc)
        (rw, bw), (rb, bb) = lc.thin_tn_ref(gg, t, w0, b0, max(d, d2) + 1)
        ok("thin_tn dW", dw + w0, rw, bw)
        ok("thin_tn dbias", db + b0, rb, bb)
    Bn, D = 300, 20                                           # label_embed_bwd
    y, drop = torch.randint(0, 8, (Bn,), generator=g), (torch.rand(Bn, generator=g) < 0.3).to(torch.uint8)
    go, old = torch.randn(Bn, D, generator=g), torch.randn(13, D, generator=g)
    rows = lc.label_rows(y, drop, 12)
    got = old.clone()
    for r in rows.unique().tolist():
        s, _ = ssum(go[rows == r], 0, assoc)
        got[r] = old[r] + s
    ref, bound = lc.label_bwd_ref(go, y, drop, old, 12)
    ok("dtable", got, ref, bound)
    assert float(bound[8:12].abs().max()) == 0.0 and torch.equal(got[8:12], old[8:12])


def test_planted_faults_sums():
    g = _g(61)
    x, old = torch.randn(300, 12, generator=g), torch.randn(12, generator=g)
    X = x.double()
    ok("sane", X.sum(0).float(), *lc.colsum_ref(x))
    bad("one partial row dropped", X[:-1].sum(0).float(), *lc.colsum_ref(x))
    bad("beta ignored", X.sum(0).float(), *lc.colsum_ref(x, old))
    bad("a gap column read", (X.sum(0) + X[:, :1].sum(0)).float(), *lc.colsum_ref(x))
    B, L, keep, D = 4, 64, 16, 68
    ids = torch.stack([torch.randperm(L, generator=g) for _ in range(B)])
    go = torch.randn(B, L, D, generator=g)
    _, (rm, bm) = lc.restore_bwd_ref(go, ids, keep)
    rows = go.view(B * L, D)[(ids >= keep).view(-1)].double()
    ok("sane", rows.sum(0).float(), rm, bm)
    grp = torch.arange(B * L)[(ids >= keep).view(-1)] % 16
    bad("mask-token gradient missing one row group", rows[grp != 5].sum(0).float(), rm, bm)
    M, N, K, rpb = 392, 12, 16, 52
    t, w, bias, pos = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g), torch.randn(128, N, generator=g)
    ref, bound = lc.thin_nt_ref(t, w, bias, pos[:rpb], rpb, F32)
    base = t.double() @ w.double().T + bias.double()
    ok("sane", (base + pos.double()[torch.arange(M) % rpb]).float(), ref, bound)
    bad("pos row m % 128", (base + pos.double()[torch.arange(M) % 128]).float(), ref, bound)
    bad("bias dropped", (base - bias.double() + pos.double()[torch.arange(M) % rpb]).float(), ref, bound)
    gg, w0 = torch.randn(M, N, generator=g), torch.randn(N, K, generator=g)
    (rw, bw), (rb, bb) = lc.thin_tn_ref(gg, t, w0, None)
    bad("thin_tn: beta ignored", (gg.double().T @ t.double()).float(), rw, bw)
    bad("thin_tn: one chunk dropped", (w0.double() + gg.double()[8:].T @ t.double()[8:]).float(), rw, bw)
    bad("thin_tn: dbias with a row dropped", gg.double()[1:].sum(0).float(), rb, bb)


# ----------------------------------------------------------------------------- conv3x3
def _conv_terms(x, w):
    """-> terms [B, Cout, Cin * 9, H * W] of the direct convolution."""
    B, C, H, W = x.shape
    cols = Fn.unfold(x, 3, padding=1)                         # [B, C * 9, H W]
    return cols[:, None] * w.reshape(C, C * 9)[None, :, :, None]


@pytest.mark.parametrize("fma", (False, True))
@pytest.mark.parametrize("assoc", ASSOC)
def test_emulation_conv3x3_inside_bounds(assoc, fma):
    g = _g(70)
    for (B, C, H, W) in ((2, 3, 5, 4), (1, 3, 1, 8), (2, 1, 4, 10), (1, 4, 3, 5)):
        x, w, b, go = torch.randn(B, C, H, W, generator=g), torch.randn(C, C, 3, 3, generator=g), torch.randn(C, generator=g), torch.randn(B, C, H, W, generator=g)
        if fma:
            terms, acc = _conv_terms(x.double(), w.double()), b.view(1, C, 1).expand(B, C, H * W).clone()
            for k in range(C * 9):
                acc = (terms[:, :, k] + acc.double()).float()
            out = acc
        else:
            s, _ = ssum(_conv_terms(x, w), 2, assoc)
            out = s + b.view(1, C, 1)
        ok("out", out.view(B, C, H, W), *lc.conv_ref(x, w, b))
        ref = lc.conv_bwd_ref(go, x, w, True, ssum(torch.zeros(B * H * W), 0, assoc)[1])
        wt = w.flip(2, 3).transpose(0, 1).contiguous()        # the input-gradient form: taps transposed AND mirrored
        s, _ = ssum(_conv_terms(go, wt), 2, assoc)
        ok("dx", s.view(B, C, H, W), *ref["dx"])
        cols = Fn.unfold(x, 3, padding=1)                     # [B, C * 9, HW]
        tw = (go.view(B, C, 1, H * W) * cols[:, None]).permute(0, 3, 1, 2).reshape(B * H * W, C, C * 9)
        s, _ = ssum(tw, 0, assoc)
        ok("dw", s.view(C, C, 3, 3), *ref["dw"])
        s, _ = ssum(go.permute(0, 2, 3, 1).reshape(-1, C), 0, assoc)
        ok("db", s, *ref["db"])


def test_planted_faults_conv3x3():
    g = _g(71)
    B, C, H, W = 2, 3, 5, 8
    x, w, b, go = torch.randn(B, C, H, W, generator=g), torch.randn(C, C, 3, 3, generator=g), torch.randn(C, generator=g), torch.randn(B, C, H, W, generator=g)
    X, Wd, G = x.double(), w.double(), go.double()
    ref, bound = lc.conv_ref(x, w, b)
    ok("sane", Fn.conv2d(X, Wd, b.double(), padding=1).float(), ref, bound)
    # the left / right neighbour taken across a row end: pad the FLATTENED rows instead of each row
    flat = Fn.pad(X.reshape(B, C, H * W), (1, 1))
    wrap = torch.stack([flat[:, :, 0:H * W], flat[:, :, 1:H * W + 1], flat[:, :, 2:H * W + 2]], -1).view(B, C, H, W, 3)   # [.., dx]
    rows = Fn.pad(wrap, (0, 0, 0, 0, 1, 1))                                                                             # zero rows above / below
    out = b.double().view(1, C, 1, 1) + sum(torch.einsum("bchw,oc->bohw", rows[:, :, dy:dy + H, :, dx], Wd[:, :, dy, dx]) for dy in range(3) for dx in range(3))
    bad("neighbour across a row end", out.float(), ref, bound)
    bad("bias dropped", Fn.conv2d(X, Wd, None, padding=1).float(), ref, bound)
    rb = lc.conv_bwd_ref(go, x, w)
    ok("sane dx", Fn.conv2d(G, Wd.flip(2, 3).transpose(0, 1), padding=1).float(), *rb["dx"])
    bad("taps transposed but not mirrored", Fn.conv2d(G, Wd.transpose(0, 1), padding=1).float(), *rb["dx"])
    bad("taps mirrored but not transposed", Fn.conv2d(G, Wd.flip(2, 3), padding=1).float(), *rb["dx"])
    dw = rb["dw"][0]
    bad("dw taps mirrored", dw.flip(2, 3).float(), *rb["dw"])
    bad("dw channels swapped", dw.transpose(0, 1).float(), *rb["dw"])
    bad("db of one pixel less", (G.sum((0, 2, 3)) - G[0, :, 0, 0]).float(), *rb["db"])


# ----------------------------------------------------------------------------- MAE loss, latent prologue
@pytest.mark.parametrize("assoc", ASSOC)
def test_emulation_mae_loss_and_latent_inside_bounds(assoc):
    g = _g(80)
    for (B, C, H, W, p) in ((2, 3, 16, 48, 4), (1, 1, 16, 16, 8), (1, 3, 32, 16, 16)):
        x, t = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
        mask = (torch.rand(B, (H // p) * (W // p), generator=g) < 0.75).float()
        m = lc._pixel_mask(mask, B, C, H, W, p).float()
        d = x - t
        am, d1 = ssum((m * (d * d)).view(-1), 0, assoc)
        av, _ = ssum(((1 - m) * (d * d)).view(-1), 0, assoc)
        ok("sums", torch.stack([am, av]), *lc.mae_loss_fwd_ref(x, t, mask, p, d1))
        coef = torch.tensor([0.37, -1.3])
        k = 2 * (coef[0] * m + coef[1] * (1 - m))
        ok("dpred", k * d, *lc.mae_loss_bwd_ref(x, t, mask, coef, p))
    lat, mu, sd = 3 * torch.randn(2, 16, 8, generator=g), torch.randn(16, generator=g), 0.5 + torch.rand(16, generator=g)
    ok("latent", ((lat - mu[None, :, None]) / sd[None, :, None]) * torch.tensor(0.7), *lc.latent_ref(lat, mu, sd, 0.7))
    ok("latent plain", lat * torch.tensor(0.7), *lc.latent_ref(lat, None, None, 0.7))


def test_planted_faults_mae_loss_and_latent():
    g = _g(81)
    B, C, H, W, p = 2, 3, 16, 48, 4
    x, t = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    mask = (torch.rand(B, (H // p) * (W // p), generator=g) < 0.5).float()
    d2 = (x.double() - t.double()) ** 2
    m = lc._pixel_mask(mask, B, C, H, W, p)
    ref, bound = lc.mae_loss_fwd_ref(x, t, mask, p, 20)
    ok("sane", torch.stack([(m * d2).sum(), ((1 - m) * d2).sum()]), ref, bound)
    # the mask indexed with H / p patches per row where W / p is meant
    yy, xx = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None].expand(H, W)
    idx = ((yy // p) * (H // p) + xx // p).clamp(max=mask.shape[1] - 1)
    mh = mask.double()[:, idx][:, None].expand(B, C, H, W)
    bad("mask indexed with H", torch.stack([(mh * d2).sum(), ((1 - mh) * d2).sum()]), ref, bound)
    coef = torch.tensor([0.37, -1.3])
    rb, bb = lc.mae_loss_bwd_ref(x, t, mask, coef, p)
    d = x.double() - t.double()
    ok("sane bwd", (2 * (0.37 * m + float(coef[1]) * (1 - m)) * d).float(), rb, bb + 1e-7 * rb.abs())       # 0.37 is not an f32: allow its rounding
    bad("bwd: mask indexed with H", (2 * (float(coef[0]) * mh + float(coef[1]) * (1 - mh)) * d).float(), rb, bb)
    bad("bwd: factor 2 dropped", ((float(coef[0]) * m + float(coef[1]) * (1 - m)) * d).float(), rb, bb)
    lat, mu, sd = 3 * torch.randn(2, 16, 8, generator=g), torch.randn(16, generator=g), 0.5 + torch.rand(16, generator=g)
    ref, bound = lc.latent_ref(lat, mu, sd, 0.7)
    L_, MU, SD = lat.double(), mu.double()[None, :, None], sd.double()[None, :, None]
    ok("sane", ((L_ - MU) / SD * lc.f32(0.7)).float(), ref, bound)
    bad("reciprocal of std in bf16-class precision", ((L_ - MU) * (1 / SD).to(BF16).double() * lc.f32(0.7)).float(), ref, bound)
    bad("multiplier dropped", ((L_ - MU) / SD).float(), ref, bound)


# ----------------------------------------------------------------------------- AdamW
HYP = T.HYP


def emu_adamw(p, g, m, v, ema, a, fma):
    t = lambda k: torch.tensor(a[k], dtype=F32)               # noqa: E731
    gj = g if a["gscale"] == 1.0 else g * t("gscale")
    p = p * t("decay_mul")
    m = madd(t("w1"), gj - m, m, fma)
    v = madd(t("w2"), gj * gj, v * t("beta2"), fma)
    denom = v.sqrt() / t("bc2_sqrt") + t("eps")
    p = madd(t("neg_step"), m / denom, p, fma)
    out = dict(p=p, m=m, v=v)
    if ema is not None:
        out["ema"] = madd(t("ema_a"), p, ema * t("ema_d"), fma)
    return out


@pytest.mark.parametrize("fma", (False, True))
def test_emulation_adamw_inside_bounds(fma):
    g = _g(90)
    n = 4160
    for gs, wd, use_ema, steps in ((1.0, 0.0, True, (1,)), (2.0 ** -7, 0.05, True, (1, 2, 3)), (1.0, 0.05, False, (10000,)), (2.0 ** -7, 0.0, False, (2,))):
        first = steps[0] == 1
        p0, g0 = torch.randn(n, generator=g), torch.randn(n, generator=g) / gs
        g0[::7] = 0.0
        m0 = torch.zeros(n) if first else 0.1 * torch.randn(n, generator=g)
        v0 = torch.zeros(n) if first else 0.01 * torch.rand(n, generator=g)
        e0 = torch.randn(n, generator=g) if use_ema else None
        cur, state = dict(p=p0, m=m0, v=v0, ema=e0), None
        for s in steps:
            a = lc.adam_scalars(s, HYP["lr"], HYP["beta1"], HYP["beta2"], HYP["eps"], wd, HYP["ema_decay"], gs)
            cur = emu_adamw(cur["p"], g0, cur["m"], cur["v"], cur.get("ema"), a, fma)
            out = lc.adamw_ref(p0, g0, m0, v0, e0, a, state)
            state = (out["p"], out["m"], out["v"], out.get("ema"))
            for k, fl in out.items():
                ok(f"{k}@{s}", cur[k], fl.v, fl.e)
    e, p = torch.randn(1003, generator=g), torch.randn(1003, generator=g)
    ok("ema_only", madd(torch.tensor(lc.f32(1 - 0.9999), dtype=F32), p, e * torch.tensor(0.9999, dtype=F32), fma), *lc.ema_ref(e, p, 0.9999))


def _adam_f64(p, g, m, v, ema, a, g2scale=True):
    P, G, M_, V = p.double(), g.double(), m.double(), v.double()
    gj = G * a["gscale"]
    P = P * a["decay_mul"]
    M_ = M_ + a["w1"] * (gj - M_)
    V = V * a["beta2"] + a["w2"] * (gj * gj if g2scale else G * G)
    P = P + a["neg_step"] * (M_ / (V.sqrt() / a["bc2_sqrt"] + a["eps"]))
    return dict(p=P.float(), m=M_.float(), v=V.float(), ema=(ema.double() * a["ema_d"] + a["ema_a"] * P).float())


def test_planted_faults_adamw():
    g = _g(91)
    n, gs, wd, step = 512, 2.0 ** -7, 0.05, 3
    p0, g0 = torch.randn(n, generator=g), torch.randn(n, generator=g) / gs
    m0, v0, e0 = 0.1 * torch.randn(n, generator=g), 0.01 * torch.rand(n, generator=g), torch.randn(n, generator=g)
    args = (HYP["lr"], HYP["beta1"], HYP["beta2"], HYP["eps"], wd, HYP["ema_decay"], gs)
    a = lc.adam_scalars(step, *args)
    ref = lc.adamw_ref(p0, g0, m0, v0, e0, a)
    good = _adam_f64(p0, g0, m0, v0, e0, a)
    for k in ref:
        ok("sane " + k, good[k], ref[k].v, ref[k].e)
    bad("decay_mul omitted", _adam_f64(p0, g0, m0, v0, e0, dict(a, decay_mul=1.0))["p"], ref["p"].v, ref["p"].e)
    bad("gscale applied to g but not to g^2", _adam_f64(p0, g0, m0, v0, e0, a, g2scale=False)["v"], ref["v"].v, ref["v"].e)
    prev = lc.adam_scalars(step - 1, *args)
    wrong = _adam_f64(p0, g0, m0, v0, e0, dict(a, bc2_sqrt=prev["bc2_sqrt"], neg_step=prev["neg_step"]))
    bad("bias correction of step - 1", wrong["p"], ref["p"].v, ref["p"].e)
    bad("bias correction of step - 1: ema", wrong["ema"], ref["ema"].v, ref["ema"].e)
    bad("ema of the old p", (e0.double() * a["ema_d"] + a["ema_a"] * p0.double()).float(), ref["ema"].v, ref["ema"].e)
    re, be = lc.ema_ref(e0, p0, 0.9999)
    bad("ema_only: weights swapped", (e0.double() * lc.f32(1 - 0.9999) + lc.f32(0.9999) * p0.double()).float(), re, be)



# ----------------------------------------------------------------------------- activations, timestep embedding, latent sampling
def _f(c):
    return torch.tensor(c, dtype=F32)


def _exp32(x):
    """exp of an f32 argument, correctly rounded: inside every measured constant."""
    return x.double().exp().float()


def _erf32(x, dtype):
    return torch.special.erf(x.double()).float()              # erff for every type (csrc/common.h erf_act): correctly rounded here


def _sig32(a):
    return 1 / (1 + _exp32(-a))


def _tanh32(u):
    return 1 - 2 / (_exp32(2 * u) + 1)


def test_emulation_activations_inside_bounds():
    g = _g(120)
    for Tt in T.TYPES:
        x, go = T._act_args(2000, 12.0, g, Tt), torch.randn(2000, generator=g).to(Tt)
        v, gf = x.float(), go.float()
        e = _erf32(v * _f(lc.R2), Tt)
        ok("gelu", (0.5 * v * (1 + e)).to(Tt), *lc.gelu_fwd_ref(x))
        ok("gelu bwd", (gf * (0.5 * (1 + e) + v * (_f(lc.RPI) * _exp32(-0.5 * v * v)))).to(Tt), *lc.gelu_bwd_ref(go, x))
        if Tt == F16:
            continue
        t = _tanh32(_f(lc.KT) * (v + _f(0.044715) * v * v * v))
        ok("gelu_tanh", (0.5 * v * (1 + t)).to(Tt), *lc.gelu_tanh_fwd_ref(x))
        d = 0.5 * (1 + t) + 0.5 * v * (1 - t * t) * _f(lc.KT) * (1 + _f(0.134145) * v * v)
        ok("gelu_tanh bwd", (gf * d).to(Tt), *lc.gelu_tanh_bwd_ref(go, x))
        h, gh = T._act_args(37 * 48, 90.0, g, Tt).view(37, 48), torch.randn(37, 24, generator=g).to(Tt)
        a, b, gg = h[:, :24].float(), h[:, 24:].float(), gh.float()
        sg = _sig32(a)
        ok("swiglu", (a * sg * b).to(Tt), *lc.swiglu_fwd_ref(h))
        ok("swiglu bwd", torch.cat([gg * b * sg * (1 + a * (1 - sg)), gg * a * sg], 1).to(Tt), *lc.swiglu_bwd_ref(gh, h))
        xs, gs = T._act_args(2000, 90.0, g), torch.randn(2000, generator=g)
        ss = 1 / (1 + _exp32(-xs))
        ok("silu", (xs / (1 + _exp32(-xs))).to(Tt), *lc.silu_fwd_ref(xs, Tt))
        ok("silu bwd", gs * ss * (1 + xs * (1 - ss)), *lc.silu_bwd_ref(gs, xs))
    tt = torch.tensor([0.0, 0.25, 1.0, 1000.0])
    for dim, mp in ((2, 1e4), (3, 1e4), (256, 1e4), (257, 100.0)):
        half = dim // 2
        j = torch.arange(half, dtype=F32)
        freq = _exp32(-torch.log(_f(mp).double()).float() * j / half)
        a = tt[:, None] * freq
        out = torch.cat([a.double().cos().float(), a.double().sin().float(), torch.zeros(4, dim - 2 * half)], 1)
        ok("timestep", out, *lc.timestep_ref(tt, dim, mp))
    for fma in (False, True):
        mom, noise = 3 * torch.randn(2, 32, 8, generator=g), torch.randn(2, 16, 8, generator=g)
        mom[:, 16:] = 12 * torch.randn(2, 16, 8, generator=g)
        mom[:, 16:, 0], mom[:, 16:, 1], mom[:, 16:, 2], mom[:, 16:, 3] = -30.0, 20.0, -45.0, 33.0
        mu, sd = torch.randn(16, generator=g), 0.5 + torch.rand(16, generator=g)
        v = madd(_exp32(0.5 * mom[:, 16:].clamp(-30, 20)), noise, mom[:, :16], fma)
        ok("latent sample", ((v - mu[None, :, None]) / sd[None, :, None]) * _f(0.7), *lc.latent_sample_ref(mom, noise, mu, sd, 0.7))
        ok("latent sample plain", v * _f(0.7), *lc.latent_sample_ref(mom, noise, None, None, 0.7))


def test_planted_faults_activations():
    g = _g(121)
    x, go = T._act_args(2000, 12.0, g), torch.randn(2000, generator=g)
    X, G = x.double(), go.double()
    cdf, pdf = 0.5 * (1 + torch.special.erf(X * lc.R2)), lc.RPI * torch.exp(-0.5 * X * X)
    rf, rb = lc.gelu_fwd_ref(x), lc.gelu_bwd_ref(go, x)
    ok("sane", (X * cdf).float(), *rf)
    ok("sane bwd", (G * (cdf + X * pdf)).float(), *rb)
    bad("gelu bwd: pdf term dropped", (G * cdf).float(), *rb)
    th = torch.tanh(lc.KT * (X + 0.044715 * X ** 3))
    tf, tb = lc.gelu_tanh_fwd_ref(x), lc.gelu_tanh_bwd_ref(go, x)
    ok("sane tanh", (0.5 * X * (1 + th)).float(), *tf)
    dth = 0.5 * (1 + th) + 0.5 * X * (1 - th * th) * lc.KT * (1 + 3 * 0.044715 * X * X)
    ok("sane tanh bwd", (G * dth).float(), *tb)
    bad("exact GELU where the tanh form is meant", (X * cdf).float(), *tf)
    bad("tanh GELU where the exact form is meant", (0.5 * X * (1 + th)).float(), *rf)
    bad("tanh bwd: the cubic's derivative dropped", (G * (0.5 * (1 + th) + 0.5 * X * (1 - th * th) * lc.KT)).float(), *tb)
    h, gh = T._act_args(37 * 48, 90.0, g).view(37, 48), torch.randn(37, 24, generator=g)
    A, B_, GG = h[:, :24].double(), h[:, 24:].double(), gh.double()
    S = torch.sigmoid(A)
    da, db = GG * B_ * S * (1 + A * (1 - S)), GG * A * S
    rs = lc.swiglu_bwd_ref(gh, h)
    ok("sane swiglu", (A * S * B_).float(), *lc.swiglu_fwd_ref(h))
    ok("sane swiglu bwd", torch.cat([da, db], 1).float(), *rs)
    bad("swiglu bwd: the two halves swapped", torch.cat([db, da], 1).float(), *rs)
    bad("swiglu: gate on the other half", (B_ * torch.sigmoid(B_) * A).float(), *lc.swiglu_fwd_ref(h))
    xs, gs = T._act_args(2000, 90.0, g), torch.randn(2000, generator=g)
    XS = xs.double()
    SS = torch.sigmoid(XS)
    ok("sane silu", (XS * SS).float(), *lc.silu_fwd_ref(xs, F32))
    bad("silu bwd: x (1 - s) term dropped", (gs.double() * SS).float(), *lc.silu_bwd_ref(gs, xs))
    tt = torch.tensor([0.0, 0.25, 1.0, 1000.0])
    ref, bound = lc.timestep_ref(tt, 256, 1e4)
    wrong, _ = lc.timestep_ref(tt, 256, 1e4, wrong_div=256)
    ok("sane timestep", ref.float(), ref, bound)
    bad("timestep: j / dim", wrong.float(), ref, bound)
    bad("timestep: cos and sin swapped", torch.cat([ref[:, 128:], ref[:, :128]], 1).float(), ref, bound)
    mom, noise = 3 * torch.randn(2, 32, 8, generator=g), torch.randn(2, 16, 8, generator=g)
    mom[:, 16:, 0], mom[:, 16:, 1], mom[:, 16:, 2], mom[:, 16:, 3] = -30.0, 20.0, -45.0, 33.0
    ref, bound = lc.latent_sample_ref(mom, noise, None, None, 0.7)
    noclamp, _ = lc.latent_sample_ref(mom, noise, None, None, 0.7, clamp=False)
    ok("sane latent", ref.float(), ref, bound)
    bad("latent: logvar not clamped", noclamp.float(), ref, bound)
    r16 = lambda t: t.to(BF16).double()                       # noqa: E731
    for name, (r, bd) in (("gelu", rf), ("gelu bwd", rb), ("gelu_tanh", tf), ("gelu_tanh bwd", tb), ("swiglu bwd", rs), ("silu", lc.silu_fwd_ref(xs, F32)),
                          ("silu bwd", lc.silu_bwd_ref(gs, xs)), ("timestep", lc.timestep_ref(tt, 256, 1e4))):
        bad(name + ": bf16 result", r16(r).float(), r, bd)
    for Tt in (BF16, F16):
        xh = x.to(Tt)
        r, bd = lc.gelu_fwd_ref(xh)
        ok("sane 16-bit", r.to(Tt), r, bd)
        bad("gelu: two-ulp flip", _flip2(r.to(Tt)), r, bd)


# ----------------------------------------------------------------------------- 16-bit flips and bf16 intermediates
def _flip2(t):
    """Every element moved by two ulps of its 16-bit type."""
    return (t.view(torch.int16) + 2).view(t.dtype)


def test_two_ulp_flip_of_a_16bit_output_is_rejected():
    g = _g(100)
    x, w, b, _ = _ln_inputs(18, 196, "unit", 100)
    for Tt in (BF16, F16):
        ref, bound = lc.ln_fwd_ref(x, w, b, EPS, Tt)["y"]
        y = ref.to(Tt)
        ok("sane", y, ref, bound)
        bad("ln y", _flip2(y), ref, bound)
        mean, rstd = _ln_stats(x)
        go, dx0, z = torch.randn(18, 196, generator=g).to(Tt), torch.randn(18, 196, generator=g), torch.zeros(196)
        ref, bound = lc.ln_bwd_ref(go, x, w, mean, rstd, dx0, z, z, 0.0)["dx_cast"]
        bad("ln dx_cast", _flip2(ref.to(Tt)), ref, bound)
    t, wt = torch.randn(40, 16, generator=g), torch.randn(12, 16, generator=g)
    ref, bound = lc.thin_nt_ref(t, wt, None, None, 0, BF16)
    bad("thin_nt", _flip2(ref.to(BF16)), ref, bound)


def test_bf16_intermediates_are_rejected_for_every_f32_output():
    """The f64 reference with ONE intermediate (or the result) rounded to bf16 must fall outside every f32 bound."""
    g = _g(101)
    r16 = lambda t: t.to(BF16).double()                       # noqa: E731
    x, w, b, _ = _ln_inputs(18, 196, "unit", 101)
    ref = lc.ln_fwd_ref(x, w, b, EPS, F32)
    X = x.double()
    xc = X - X.mean(-1, keepdim=True)
    rs = ((xc ** 2).mean(-1, keepdim=True) + EPS).rsqrt()
    bad("ln y: bf16 rstd", (xc * r16(rs) * w.double() + b.double()).float(), *ref["y"])
    bad("ln mean", r16(X.mean(-1)).float(), *ref["mean"])
    bad("ln rstd", r16(rs[:, 0]).float(), *ref["rstd"])
    mean, rstd = _ln_stats(x)
    go, dx0, z = torch.randn(18, 196, generator=g), torch.randn(18, 196, generator=g), torch.zeros(196)
    rb = lc.ln_bwd_ref(go, x, w, mean, rstd, dx0, z, z, 0.0)
    for k in ("dx", "dw", "db"):
        bad("ln " + k, r16(rb[k][0]).float(), *rb[k])
    xx = torch.randn(300, 12, generator=g)
    rc_, bc = lc.colsum_ref(xx)
    bad("colsum", r16(rc_).float(), rc_, bc)
    t, wt, gg = torch.randn(140, 16, generator=g), torch.randn(12, 16, generator=g), torch.randn(140, 12, generator=g)
    rn, bn = lc.thin_nt_ref(t, wt, None, None, 0, F32)
    bad("thin_nt", r16(rn).float(), rn, bn)
    (rw, bw), (rb2, bb2) = lc.thin_tn_ref(gg, t)
    bad("thin_tn dW", r16(rw).float(), rw, bw)
    bad("thin_tn dbias", r16(rb2).float(), rb2, bb2)
    cx, cw, cb, cg = torch.randn(2, 3, 5, 8, generator=g), torch.randn(3, 3, 3, 3, generator=g), torch.randn(3, generator=g), torch.randn(2, 3, 5, 8, generator=g)
    r, bd = lc.conv_ref(cx, cw, cb)
    bad("conv out", r16(r).float(), r, bd)
    for k, (r, bd) in lc.conv_bwd_ref(cg, cx, cw).items():
        bad("conv " + k, r16(r).float(), r, bd)
    mask = torch.tensor([[1.0, 0.0], [0.0, 1.0]])
    r, bd = lc.mae_loss_fwd_ref(cx[:, :, :4], cg[:, :, :4], mask, 4, 12)
    bad("mae sums", r16(r), r, bd)
    r, bd = lc.mae_loss_bwd_ref(cx[:, :, :4], cg[:, :, :4], mask, torch.tensor([0.37, -1.3]), 4)
    bad("mae dpred", r16(r).float(), r, bd)
    lat, mu, sd = 3 * torch.randn(2, 16, 8, generator=g), torch.randn(16, generator=g), 0.5 + torch.rand(16, generator=g)
    r, bd = lc.latent_ref(lat, mu, sd, 0.7)
    bad("latent", r16(r).float(), r, bd)
    n = 512
    p0, g0, m0, v0, e0 = (torch.randn(n, generator=g), torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g), 0.01 * torch.rand(n, generator=g),
                          torch.randn(n, generator=g))
    out = lc.adamw_ref(p0, g0, m0, v0, e0, lc.adam_scalars(3, HYP["lr"], HYP["beta1"], HYP["beta2"], HYP["eps"], 0.05, HYP["ema_decay"], 1.0))
    for k, fl in out.items():
        bad("adamw " + k, r16(fl.v).float(), fl.v, fl.e)
    y, old, go = torch.randint(0, 8, (70,), generator=g), torch.randn(13, 20, generator=g), torch.randn(70, 20, generator=g)
    r, bd = lc.label_bwd_ref(go, y, None, old, 12)
    bad("dtable", torch.where(bd > 0, r16(r), r).float(), r, bd)


# ----------------------------------------------------------------------------- references against torch / numpy definitions
def test_references_follow_the_definitions():
    g = _g(110)
    x, w, b, _ = _ln_inputs(18, 196, "unit", 110)
    ref = lc.ln_fwd_ref(x, w, b, EPS, F32)
    want = Fn.layer_norm(x.double(), (196,), w.double(), b.double(), EPS)
    assert float((ref["y"][0] - want).abs().max()) < 1e-12
    # the LayerNorm backward against autograd in f64
    xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
    bd = b.double().requires_grad_()
    go = torch.randn(18, 196, generator=g)
    Fn.layer_norm(xd, (196,), wd, bd, EPS).backward(go.double())
    mean, rstd = _ln_stats(x)
    z = torch.zeros(196)
    rb = lc.ln_bwd_ref(go, x, w, mean, rstd, torch.zeros(18, 196), z, z, 0.0)
    assert float((rb["dx"][0] - xd.grad).abs().max()) < 1e-5            # mean / rstd are the f32-rounded ones
    assert float((rb["dw"][0] - wd.grad).abs().max()) < 1e-4 and float((rb["db"][0] - bd.grad).abs().max()) < 1e-12
    # conv backward against autograd
    cx, cw, cg = torch.randn(2, 3, 5, 8, generator=g).double().requires_grad_(), torch.randn(3, 3, 3, 3, generator=g).double().requires_grad_(), \
        torch.randn(2, 3, 5, 8, generator=g)
    Fn.conv2d(cx, cw, None, padding=1).backward(cg.double())
    rb = lc.conv_bwd_ref(cg, cx.detach(), cw.detach())
    assert float((rb["dx"][0] - cx.grad).abs().max()) < 1e-12 and float((rb["dw"][0] - cw.grad).abs().max()) < 1e-12
    # the MAE loss against the patchified form of models_mae.py forward_loss
    B, C, H, W, p = 2, 3, 16, 48, 4
    pr, im = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    mask = (torch.rand(B, (H // p) * (W // p), generator=g) < 0.5).float()
    patch = lambda t: t.double().view(B, C, H // p, p, W // p, p).permute(0, 2, 4, 3, 5, 1).reshape(B, -1, p * p * C)     # noqa: E731
    per = ((patch(pr) - patch(im)) ** 2).sum(-1)
    ref, _ = lc.mae_loss_fwd_ref(pr, im, mask, p, 10)
    assert abs(float(ref[0] - (per * mask.double()).sum())) < 1e-9 and abs(float(ref[1] - (per * (1 - mask.double())).sum())) < 1e-9
    # AdamW against torch.optim.AdamW in f64 (scalars differ by their f32 rounding only)
    p0, g0 = torch.randn(64, generator=g), torch.randn(64, generator=g)
    pp = p0.double().clone().requires_grad_()
    opt = torch.optim.AdamW([pp], lr=HYP["lr"], betas=(HYP["beta1"], HYP["beta2"]), eps=HYP["eps"], weight_decay=0.05)
    state = None
    for s in (1, 2, 3):
        pp.grad = g0.double().clone()
        opt.step()
        out = lc.adamw_ref(p0, g0, torch.zeros(64), torch.zeros(64), None, lc.adam_scalars(s, HYP["lr"], HYP["beta1"], HYP["beta2"], HYP["eps"], 0.05, 0.0, 1.0),
                           state)
        state = (out["p"], out["m"], out["v"], None)
    assert float((out["p"].v - pp.detach()).abs().max()) < 1e-6          # 3 steps x the f32 rounding (6e-8) of decay_mul and step size; one step moves p by 2e-4
    # random masking: -0.0 and +0.0 are equal keys, ordered by index
    r, m, k = lc.masking_ref(torch.tensor([[0.0, -0.0, 0.0, -0.0, -1.0]]), 2)
    assert r.tolist() == [[1, 2, 3, 4, 0]] and k.tolist() == [[4, 0]] and m.tolist() == [[0.0, 1.0, 1.0, 1.0, 0.0]]


# ----------------------------------------------------------------------------- the device tables
def _both(values, what):
    assert set(values) == {False, True}, f"{what}: only {set(values)} in the table"


def _all(values, want, what):
    assert set(values) >= set(want), f"{what}: {set(want) - set(values)} not reached"


def test_case_table_covers_every_predicate():
    # ---- layernorm_fwd
    F = T.LN_FWD
    _all({(T.ln_nv_class(c["D"]), c["T"]) for c in F}, {(n, t) for n in (3, 6, 12, 16, 20) for t in T.TYPES}, "ln_fwd NV x type")
    _all({c["D"] for c in F}, T.LN_D, "ln_fwd D")
    for n in (3, 6, 12, 16, 20):
        _both([T.ln_partial_chunk(c["D"]) for c in F if T.ln_nv_class(c["D"]) == n], f"ln_fwd NV{n}: partly filled last chunk")
    _both([c["mean"] for c in F], "ln_fwd mean given")
    _both([c["rstd"] for c in F], "ln_fwd rstd given")
    _both([c["M"] == 1 for c in F], "ln_fwd M = 1")
    _both([c["M"] % 16 == 0 for c in F] + [True], "ln_fwd M % 16")
    assert any(c["M"] % 16 for c in F)
    _both([T.ln_fwd_capped(c["M"]) for c in F], "ln_fwd 4096-workgroup cap")
    assert any(T.ln_fwd_capped(c["M"]) and c["M"] > 4096 * 16 and c["M"] % 16 for c in F), "the cap's second pass is not ragged"
    _both([c["fam"] == "offset" for c in F], "ln_fwd offset rows")
    # ---- layernorm_bwd
    Bk = T.LN_BWD
    _all({(T.ln_nv_class(c["D"]), c["T"]) for c in Bk}, {(n, t) for n in (3, 6, 12, 16, 20) for t in T.TYPES}, "ln_bwd NV x type")
    _all({c["D"] for c in Bk}, T.LN_D, "ln_bwd D")
    _both([c["M"] < 128 for c in Bk], "ln_bwd M < 128")
    _both([c["M"] % 128 == 0 for c in Bk], "ln_bwd M % 128")
    _both([c["M"] % 16 == 0 for c in Bk], "ln_bwd M % 16")
    G = [T.ln_bwd_groups(c["M"]) for c in Bk]
    assert any(g_ < 64 for g_ in G) and any(g_ > 64 and g_ % 64 for g_ in G), "ln_reduce: G below / above 64"
    _both([c["beta_w"] == 1.0 for c in Bk], "ln_bwd beta_w")
    _all({(c["T"], c["cast"]) for c in Bk}, {(BF16, True), (F16, True), (BF16, False), (F16, False), (F32, False)}, "ln_bwd dx_cast")
    assert not any(c["cast"] and c["T"] == F32 for c in Bk)
    assert any(c["D"] == 1280 and 32 * c["D"] * 4 == 160 * 1024 for c in Bk), "the 160-KiB launch"
    _all({(T.ln_nv_class(c["D"]), c["beta_w"]) for c in Bk}, {(n, b) for n in (3, 6, 12, 16, 20) for b in (0.0, 1.0)}, "ln_bwd NV x beta_w")
    # ---- colsum
    Cs = T.COLSUM
    _all({c["T"] for c in Cs}, T.TYPES, "colsum dtype")
    _all({T.colsum_rows(c["M"], c["N"]) for c in Cs}, (8, 16, 32, 64, 128, 256), "colsum_rows ladder")
    Gs = [T.colsum_groups(c["M"], c["N"]) for c in Cs]
    assert any(g_ == 1 for g_ in Gs) and any(1 < g_ < 256 for g_ in Gs) and any(g_ >= 256 for g_ in Gs), "colsum G"
    _all({c["N"] for c in Cs}, (4, 12, 200, 1024, 1028, 2304), "colsum N")
    nc = [T.colsum_last_ncol4(c["N"]) for c in Cs]
    assert any(256 // n > 1 and 256 % n == 0 for n in nc) and any(256 // n > 1 and 256 % n for n in nc) and any(n == 256 for n in nc), "colsum nsub"
    assert any(c["N"] > 1024 and T.colsum_last_ncol4(c["N"]) == 1 for c in Cs), "a one-float4 last column block"
    _both([c["gap"] > 0 for c in Cs], "colsum ldx > N")
    _both([c["beta"] == 1.0 for c in Cs], "colsum beta")
    _all({(c["T"], c["gap"] > 0) for c in Cs}, {(t, True) for t in T.TYPES}, "colsum ldx > N per dtype")
    # ---- restore_tokens
    R = T.RESTORE
    _all({c["D"] for c in R}, (4, 68, 192, 196, 384, 388, 512), "restore D")
    for n in (3, 6, 8):
        _both([c["D"] % 64 != 0 for c in R if T.rt_nv_class(c["D"]) == n], f"restore NV{n}: partial chunk")
    _both([c["keep"] == 1 for c in R], "restore keep = 1")
    _both([c["keep"] == c["L"] for c in R], "restore keep = L")
    assert any(c["keep"] == c["L"] and c["dmask"] for c in R), "keep = L with the mask-token gradient"
    _both([c["dmask"] for c in R], "restore dmask_token given")
    _both([T.rt_capped(c["B"], c["L"]) for c in R], "restore 2048-workgroup cap")
    assert any(c["B"] * c["L"] == 32768 + 19 for c in R)
    # ---- thin GEMMs
    N_ = T.THIN_NT
    _all({(c["K"], c["T"], c["pos"]) for c in N_}, {(k, t, p_) for k in (16, 32) for t in (F32, BF16) for p_ in (False, True)}, "thin_nt instantiations")
    _both([c["bias"] for c in N_], "thin_nt bias")
    _all({c["M"] for c in N_}, (5, 128, 128 * 3 + 8), "thin_nt M")
    _all({c["N"] for c in N_}, (4, 772, 1028), "thin_nt N")
    assert any(c["pos"] and 128 % c["rpb"] and c["M"] > c["rpb"] for c in N_), "rows_per_batch that does not divide 128"
    _both([c["N"] > 1024 for c in N_], "thin_nt second column block")
    Tn = T.THIN_TN
    _all({c["K"] for c in Tn}, (16, 32), "thin_tn K")
    _all({c["M"] for c in Tn}, (5, 512, 512 * 2 + 8, 512 * 65 + 3), "thin_tn M")
    _all({c["N"] for c in Tn}, (4, 260, 772), "thin_tn N")
    ch = [T.thin_chunks(c["M"]) for c in Tn]
    assert 1 in ch and any(1 < k <= 64 for k in ch) and any(k > 64 and k % 64 for k in ch), "thin_tn chunks"
    _both([c["dbias"] for c in Tn], "thin_tn dbias")
    _both([c["beta"] == 1.0 for c in Tn], "thin_tn beta")
    _both([c["N"] > 256 for c in Tn], "thin_tn second column block")
    # ---- conv3x3
    Cf, Cb = T.CONV_FWD, T.CONV_BWD
    for tab, what in ((Cf, "conv3x3"), (Cb, "conv3x3_bwd")):
        _both([T.conv_rgb(c["C"], c["W"], c["xoff"], c["ooff"]) for c in tab], what + " rgb kernel")
        gen = [c for c in tab if not T.conv_rgb(c["C"], c["W"], c["xoff"], c["ooff"]) and c["dx"]]
        assert any(c["C"] == 3 and c["W"] % 4 and not c["xoff"] and not c["ooff"] for c in gen), what + ": generic for W % 4 alone"
        assert any(c["C"] == 3 and c["W"] % 4 == 0 and c["xoff"] and not c["ooff"] for c in gen), what + ": generic for the input pointer alone"
        assert any(c["C"] == 3 and c["W"] % 4 == 0 and c["ooff"] and not c["xoff"] for c in gen), what + ": generic for the output pointer alone"
        assert any(T.conv_rgb(c["C"], c["W"], c["xoff"], c["ooff"]) and c["W"] == 4 for c in tab) and any(c["H"] == 1 for c in tab)
    _all({c["C"] for c in Cf}, (1, 2, 3, 4), "conv3x3 C")
    assert all(c["C"] == 3 for c in Cb)
    _both([c["bias"] for c in Cf], "conv3x3 b given")
    assert {T.conv_rgb(c["C"], c["W"], c["xoff"], c["ooff"]) for c in Cf if not c["bias"]} == {False, True}, "b NULL on both kernels"
    _both([c["dx"] for c in Cb], "conv3x3_bwd dx given")
    _both([T.conv_bwd_capped(c["B"], c["H"], c["W"]) for c in Cb], "CONV_BWD_G cap")
    assert any(c["B"] * c["H"] * c["W"] == 256 * 1024 + 256 * 3 + 5 for c in Cb)
    # ---- MAE loss
    Ml = T.MAE_LOSS
    _all({c["p"] for c in Ml}, (4, 8, 16), "mae_loss p")
    _both([c["H"] != c["W"] for c in Ml], "mae_loss H != W")
    assert any(c["H"] > c["W"] for c in Ml) and any(c["H"] < c["W"] for c in Ml)
    _all({c["C"] for c in Ml}, (1, 3), "mae_loss C")
    _all({c["mask"] for c in Ml}, ("rand", "all1", "all0"), "mae_loss masks")
    _both([c["B"] * c["C"] * c["H"] * c["W"] // 4 > 524288 for c in Ml], "mae_loss cap")
    # ---- latent prologue (sample = 0)
    Lt = T.LATENT
    _both([c["norm"] for c in Lt], "latent mean / std given")
    _all({c["C"] for c in Lt}, (1, 16), "latent C")
    _all({c["HW"] for c in Lt}, (4, 1024, 1028), "latent HW")
    # ---- activations
    Ac = T.ACT
    _all({(c["kind"], c["T"]) for c in Ac}, {("gelu", t) for t in T.TYPES} | {("gelu_tanh", F32), ("gelu_tanh", BF16)}, "gelu kinds x dtypes")
    for kind in ("gelu", "gelu_tanh"):
        ns = [c["n"] for c in Ac if c["kind"] == kind]
        assert 1 in ns and any(n % 256 for n in ns) and any(T.ew_capped(n) for n in ns) and not all(T.ew_capped(n) for n in ns), kind
    Sw = T.SWIGLU
    _all({c["T"] for c in Sw}, (F32, BF16), "swiglu dtype")
    assert any(c["M"] == 1 and c["Hs"] == 8 for c in Sw) and any((c["M"] * c["Hs"] // 8) % 256 for c in Sw)
    _both([T.ew_capped(c["M"] * c["Hs"] // 8) for c in Sw], "swiglu cap")
    _all({(c["T"], c["n"]) for c in T.SILU}, {(t, n) for t in (F32, BF16) for n in T.ACT_N}, "silu dtype x n")
    _both([T.ew_capped(n) for n in T.ACT_N], "elementwise cap")
    assert 1 in T.ACT_N and any(n % 256 for n in T.ACT_N)
    edge = T._act_args(64, 90.0, _g(2))
    assert bool((edge == 0).any()) and float(edge.abs().max()) == 90.0 and bool(((edge != 0) & (edge.abs() < 1e-20)).any())
    Ls = T.LATENT_S
    _both([c["norm"] for c in Ls], "latent (sample) mean / std given")
    _all({c["C"] for c in Ls}, (1, 16), "latent (sample) C")
    _all({c["HW"] for c in Ls}, (4, 1024, 1028), "latent (sample) HW")
    # ---- AdamW, EMA
    Ad = T.ADAMW
    _both([c["ema"] for c in Ad], "adamw ema given")
    _all({c["gs"] for c in Ad}, (1.0, 2.0 ** -7), "adamw grad_scale")
    _all({c["wd"] for c in Ad}, (0.0, 0.05), "adamw weight_decay")
    _all({s for c in Ad for s in c["steps"]}, (1, 2, 10000), "adamw steps")
    assert any(len(c["steps"]) == 3 for c in Ad), "three consecutive steps"
    _all({c["n"] for c in Ad}, (4, 4096 + 64), "adamw n")
    _both([T.ew_capped(c["n"] // 4) for c in Ad], "adamw cap")
    _both([T.ew_capped(c["n"]) for c in T.EMA_ONLY], "ema_only cap")
    assert any(c["n"] == 1 for c in T.EMA_ONLY) and any(c["n"] % 256 for c in T.EMA_ONLY)
    # ---- label embedding
    Le = T.LABEL
    _all({c["drop"] for c in Le}, ("null", "mixed", "all"), "label drop")
    _all({c["B"] for c in Le}, (1, 70, 256, 300), "label B")
    _all({c["D"] for c in Le}, (4, 192, 300), "label D")
    _all({T.label_passes(c["B"]) for c in Le}, (1, 2), "label ballot passes")
    # ---- bit-exact kernels
    Mk = T.MASKING
    _all({c["L"] for c in Mk}, (1, 2, 3, 200, 255, 256, 257, 4096), "masking L")
    assert any(c["keep"] == 0 for c in Mk) and any(c["keep"] == 1 for c in Mk) and any(c["keep"] == c["L"] > 1 for c in Mk)
    _all(T.MASK_ROWS, ("ties", "all_equal", "negative", "signed_zero"), "masking rows")
    nz = T.masking_noise(200, _g(1))
    assert bool((nz[4] == 0).any()) and bool(torch.signbit(nz[4][nz[4] == 0]).any()) and not bool(torch.signbit(nz[4][nz[4] == 0]).all())
    assert bool((nz[3] < 0).any()) and nz[2].unique().numel() == 1 and nz[1].unique().numel() <= 8
    Pg = T.PATCH
    _all({(c["p"], c["C"]) for c in Pg}, {(p_, c_) for p_ in (1, 2, 8, 16) for c_ in (3, 4)}, "patch_gather p x C")
    _all({c["T"] for c in Pg}, (F32, BF16), "patch_gather dtype")
    _all({c["D"] for c in Pg}, (4, 192, 516), "patch_gather D")
    assert any(c["keep"] == 1 for c in Pg)
    Ca = T.CAST
    _all({(c["src"], c["dst"], c["n"]) for c in Ca}, {(s, d, n) for s, d in T.CAST_PAIRS for n in (1, 7, 8, 9, 1003)}, "cast pairs x n")
    _both([T.ew_capped(c["n"] // 8 + 1) for c in Ca], "cast cap")
    St = T.CAST_STACK
    _all({c["count"] for c in St}, (1, 3, 64), "cast_stack count")
    _all({c["T"] for c in St}, (F32, BF16), "cast_stack dtype")
    assert any(c["n"] == 8 for c in St)
    _both([(c["n"] // 8 + 255) // 256 > 1024 for c in St], "cast_stack cap")
    Cw = T.CAST_WEIGHT
    _all({(T.cw64(c["R"], c["C"], c["doff"]), c["T"]) for c in Cw}, {(k, t) for k in (False, True) for t in T.TYPES}, "cast_weight kernel x type")
    k32 = [c for c in Cw if not T.cw64(c["R"], c["C"], c["doff"])]
    assert any(c["R"] % 64 and c["C"] % 64 == 0 and not c["doff"] for c in k32) and any(c["C"] % 64 and c["R"] % 64 == 0 and not c["doff"] for c in k32)
    assert any(c["doff"] == 8 and c["R"] % 64 == 0 and c["C"] % 64 == 0 for c in k32), "32-tile kernel for the destination offset alone"
    assert any(c["R"] == 1 for c in Cw) and any(c["C"] == 1 for c in Cw) and any(c["R"] < 32 and c["C"] < 32 and c["R"] > 1 and c["C"] > 1 for c in Cw)
    for k in (False, True):
        _both([c["dst"] for c in Cw if T.cw64(c["R"], c["C"], c["doff"]) == k], f"cast_weight dst given (64-tile {k})")
        _both([c["dstT"] for c in Cw if T.cw64(c["R"], c["C"], c["doff"]) == k], f"cast_weight dstT given (64-tile {k})")
    Ma = T.MULTI_ADD
    _all({len(c["lens"]) for c in Ma}, (1, 32), "multi_add count")
    assert any({1, 255, 256, 65536 + 1} <= set(c["lens"]) for c in Ma), "multi_add mixed lengths"
    Ts = T.TIMESTEP
    _all({c["dim"] for c in Ts}, (2, 3, 256, 257), "timestep dim")
    assert len({c["mp"] for c in Ts}) >= 2 and any((c["B"] * (c["dim"] // 2)) % 256 for c in Ts)
    # ---- the refusal table names every refusal the suite promises
    for need in ("layernorm_fwd D % 4", "layernorm_fwd D > 1280", "layernorm_bwd_cast f32 dx_cast", "restore_tokens_bwd D > 512",
                 "restore_tokens_bwd dmask without workspace", "latent_prologue mean only", "latent_prologue std only", "latent_prologue sample without noise",
                 "thin_tn beta 0.5", "thin_tn short workspace", "cast misaligned src", "cast bf16 -> f16", "adamw_ema n % 4", "adamw_ema step 0",
                 "conv3x3_bwd C = 4", "mae_loss_fwd p % 4", "mae_loss_fwd p not dividing H"):
        assert need in T.REFUSED
