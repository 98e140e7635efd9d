"""The bounds of tests/row_check.py pass and bite (CPU only).

A plain torch f32 emulation of each row kernel of csrc/elementwise.hip and csrc/qk_rope.hip rounds where the kernel rounds.  It runs with two associations of
every sum (sequential; pairwise halves, as the wave butterflies pair lanes) and with products contracted into the following add (that one
product-add in f64, rounded once) or not.  The row mean of the LayerNorm form is the one sum whose bound depends on the association
(row_check.py R4: NCH + 9 roundings deep), so it is always summed pairwise, whose depth log2(D) <= 8 + NCH is within that count.

  - the emulation is inside every bound at every (dtype, D or hd) class of the GPU case tables, with zero excluded elements;
  - for every 16-bit output a stored element moved by 2 ulp is rejected (first, last, a random interior element); for every f32 output the
    emulation with every f32 intermediate rounded to bf16 is rejected;
  - every planted fault (an emulation with exactly one defect) raises BoundError;
  - the GPU case tables reach every dispatch predicate, taken and not taken.

Worst err / bound of the emulation over all classes and the four (association, contraction) variants:
  norm forward:   rstd 0.34; y 1.00 (bf16), 0.22 (f32, RMS), 0.12 (f32, LayerNorm form)
  norm backward:  dx 0.63 (RMS), 0.17 (LayerNorm form); dy 1.00 (bf16), 0.76 (f32); dshift 0.22, dscale 0.24, dw 0.15, dgate 0.12, dbias 0.12
  gate_bwd:       dy 1.00 (bf16), 0.99 (f32: one rounding, and the bound is that rounding); dgate 0.23; dbias 0.11
  QK forward:     q | k 1.00 (bf16), 0.30 (f32, norm), 0.83 (f32, RoPE only)
  QK backward:    slots 1.00 (bf16), 0.07 (f32); dwq / dwk 0.06
  rope:           1.00 (bf16), 0.89 (f32)
"""
import math

import pytest
import torch

import row_check as rc
import test_gpu_row_paths as T

F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-6
WORST: dict = {}
VARIANTS = [("tree", False), ("seq", False), ("tree", True), ("seq", True)]


class Em:
    """f32 arithmetic, one rounding per operation.  lowp: every intermediate rounded to bf16 as well."""

    def __init__(self, assoc="tree", fma=False, lowp=False, fault=None):
        self.assoc, self.fuse, self.lowp, self.fault = assoc, fma, lowp, fault

    def r(self, t):
        t = t.float()
        return t.bfloat16().float() if self.lowp else t

    def mul(self, a, b):
        return self.r(a * b)

    def add(self, a, b):
        return self.r(a + b)

    def sub(self, a, b):
        return self.r(a - b)

    def div(self, a, b):
        return self.r(a / b)

    def fma(self, a, b, c):
        if self.fuse:
            return self.r((a.double() * b.double() + torch.as_tensor(c).double()).float())
        return self.add(self.mul(a, b), c)

    def tree(self, t):
        n = 1 << max(0, (t.shape[-1] - 1).bit_length())
        t = torch.nn.functional.pad(t, (0, n - t.shape[-1]))
        while n > 1:
            n //= 2
            t = self.add(t[..., :n], t[..., n:])
        return t[..., 0]

    def sum(self, t, dim=-1):
        t = t.movedim(dim, -1)
        if self.assoc == "tree":
            return self.tree(t)
        acc = t[..., 0]
        for i in range(1, t.shape[-1]):
            acc = self.add(acc, t[..., i])
        return acc

    def dot(self, a, b, dim=-1):
        a, b = torch.broadcast_tensors(a, b)
        a, b = a.movedim(dim, -1), b.movedim(dim, -1)
        if self.assoc == "seq" and self.fuse:
            acc = self.mul(a[..., 0], b[..., 0])
            for i in range(1, a.shape[-1]):
                acc = self.fma(a[..., i], b[..., i], acc)
            return acc
        return self.sum(self.mul(a, b))

    def rsqrt(self, t):
        return self.r(torch.rsqrt(t))


@pytest.fixture(scope="module", autouse=True)
def _report():
    """The table of the module docstring, printed at module teardown (pytest -s)."""
    yield
    for k in sorted(WORST):
        print(f"  {k:32s} {WORST[k]:.3f}")


def _rows(v, rpb, M):
    return None if v is None else v.float().repeat_interleave(rpb, 0)


def _colsum(E, term_a, term_b, groups, old=None):
    """sum over the rows of each group of term_a * term_b (term_b None: term_a alone), the product contracted into the add if E says so."""
    D = term_a.shape[-1]
    a = term_a.reshape(groups, -1, D)
    s = E.sum(a, 1) if term_b is None else E.dot(a, term_b.reshape(groups, -1, D), 1)
    return s if old is None else E.add(old.float(), s)


# ----------------------------------------------------------------------------- emulations
def em_norm_fwd(E, x, w, shift, scale, rpb, eps, center, Tout):
    M, D = x.shape
    f = E.fault
    xc = x
    if center:
        mean = E.div(E.tree(x), float(D))[:, None]
        xc = E.sub(x, mean)
        ss = E.dot(xc, xc)
        if f == "center_var_e2":                               # E[x^2] - mean^2 in f32
            ss = E.mul(E.sub(E.div(E.dot(x, x), float(D)), E.mul(mean[:, 0], mean[:, 0])), float(D))
    else:
        ss = E.dot(x, x)
    den = float(256 * rc.nch(D)) if f == "div_256nch" else float(D)
    arg = E.div(ss, den)
    rs = E.rsqrt(arg if f == "eps_omitted" else E.add(arg, eps))[:, None]
    rstd = rs[:, 0].clone()
    if f == "rstd_neighbour":
        rs = rs.roll(1, 0)
    y = E.mul(xc, rs)
    if w is not None:
        y = E.mul(y, w)
    sc, sh = _rows(scale, rpb, M), _rows(shift, rpb, M)
    if f == "mod_next_sample":                                 # the last row of every sample takes the next sample's vectors
        idx = torch.arange(M)
        idx[rpb - 1::rpb] = (idx[rpb - 1::rpb] + 1) % M
        sc, sh = (None if sc is None else sc[idx]), (None if sh is None else sh[idx])
    if sc is not None:
        sc1 = sc if f == "scale_no_one" else E.add(sc, 1.0)
        y = E.fma(y, sc1, sh) if (sh is not None) else E.mul(y, sc1)
    elif sh is not None:
        y = E.add(y, sh)
    if f == "last_chunk_unnormalised":
        y[:, -4:] = x[:, -4:]
    if f == "last_chunk_unwritten":
        y[:, -4:] = math.nan
    return dict(y=y.to(Tout), rstd=rstd)


def em_norm_bwd(E, dout, x, w, scale, rstd, rpb, center, dx_old, dw_old, y, gate):
    M, D = x.shape
    B, f, Tg = M // rpb, E.fault, dout.dtype
    g, rs = dout.float(), rstd.float()[:, None]
    xc = E.sub(x, E.div(E.tree(x), float(D))[:, None]) if center else x
    nv = E.mul(xc, rs)
    wv = torch.ones(D) if w is None else w.float()
    sc1 = E.add(_rows(scale, rpb, M), 1.0)
    dy_ = E.mul(g, sc1)
    dn = E.mul(dy_, wv)
    dot = E.div(E.dot(dn, nv), float(D))[:, None]
    d = E.sub(dn, E.mul(nv, dot)) if not E.fuse else E.fma(-nv, dot, dn)
    if center and f != "no_msum":
        d = E.sub(d, E.div(E.sum(dn), float(D))[:, None])
    d0 = E.mul(d, rs)
    acc = dx_old is not None
    if f == "beta_as_overwrite":
        acc = False
    if f == "beta_as_accumulate":
        acc, dx_old = True, torch.ones(M, D)
    dx = E.add(dx_old.float(), d0) if acc else d0
    out = dict(dx=dx)

    def per_sample(a, b):
        if f == "drop_last_partial":                           # the last quarter of every sample's rows: its last partial
            k = rpb - max(1, rpb // 4)
            a = a.reshape(B, rpb, D)[:, :k].reshape(-1, D)
            b = None if b is None else b.reshape(B, rpb, D)[:, :k].reshape(-1, D)
        s = _colsum(E, a, b, B)
        return s.roll(1, 0) if f == "partials_next_sample" else s

    out["dshift"] = per_sample(g, None)
    out["dscale"] = per_sample(g, E.mul(nv, wv))
    if w is not None:
        out["dw"] = _colsum(E, dy_, nv, 1, dw_old)[0]
    if gate is not None:
        out["dy"] = E.mul(dx, _rows(gate, rpb, M)).to(Tg)
        out["dgate"] = per_sample(d0 if f == "dgate_pre_accumulate" else dx, y.float())
        out["dbias"] = _colsum(E, out["dy"].float(), None, 1)[0]
    return out


def em_gate_bwd(E, dx, y, gate, rpb, Tg):
    M, D = dx.shape
    dy = (dx if gate is None else E.mul(dx, _rows(gate, rpb, M))).to(Tg)
    out = dict(dy=dy, dbias=_colsum(E, dy.float(), None, 1)[0])
    if y is not None:
        out["dgate"] = _colsum(E, dx, y.float(), M // rpb)
    return out


def em_rope(E, t, cos, sin, transposed=False):
    f = E.fault
    if f == "table_row_next":
        cos, sin = cos.roll(-1, 0), sin.roll(-1, 0)
    te, to = t[..., 0::2], t[..., 1::2]
    if f == "pair_swapped":
        te, to = to, te
    ce, co, se, so = cos[:, 0::2], cos[:, 1::2], sin[:, 0::2], sin[:, 1::2]
    if f == "sin_sign":
        se, so = -se, -so
    if transposed != (f == "adjoint_as_forward"):
        oe, oo = E.fma(te, ce, E.mul(to, so)), E.fma(to, co, -E.mul(te, se))
    else:
        oe, oo = E.fma(te, ce, -E.mul(to, se)), E.fma(to, co, E.mul(te, so))
    return torch.stack([oe, oo], -1).reshape(t.shape)


def em_qk_fwd(E, qkv, w2, cos, sin, eps, mode):
    """qkv [B,N,3,H,hd] -> q, k [B,H,N,hd] in the dtype of qkv."""
    f, Tq = E.fault, qkv.dtype
    hd = qkv.shape[-1]
    out = []
    for s in range(2):
        src = 2 if (f == "k_at_v_offset" and s == 1) else s
        x = qkv[:, :, src].permute(0, 2, 1, 3).float()
        if mode == "norm":
            ss = E.dot(x, x)
            if f == "rowsum_neighbour":                         # the lane-group sum runs over a neighbouring item's lanes as well
                ss = E.add(ss, ss.flatten().roll(-1).reshape(ss.shape))
            rs = E.rsqrt(E.add(E.div(ss, float(hd)), eps))[..., None]
            w = w2[1 - s] if f == "wk_on_q" else w2[s]
            x = E.mul(E.mul(x, rs), w.float())
        out.append(em_rope(E, x, cos, sin).to(Tq))
    return out


def em_qk_bwd(E, g, x, w, cos, sin, eps):
    """One slot: g, x [B,H,N,hd] -> (stored slot [f32, before the rounding to T], per-item weight-gradient terms)."""
    hd = g.shape[-1]
    t = em_rope(E, g.float(), cos, sin, transposed=True)
    if w is None:
        return t, None
    xf = x.float()
    rs = E.rsqrt(E.add(E.div(E.dot(xf, xf), float(hd)), eps))[..., None]
    n = E.mul(xf, rs)
    dn = E.mul(t, w.float())
    m = E.div(E.dot(dn, n), float(hd))[..., None]
    o = E.mul(E.fma(-n, m, dn), rs)
    return o, (t, n)


# ----------------------------------------------------------------------------- inputs and checks
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rec(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)
    return r


def norm_fwd_case(D, Tout, center=False, shift=True, scale=True, fam="unit", rpb=6, B=2, seed=1):
    g = _gen(seed + D)
    M = B * rpb
    x = T._row_input(M, D, fam, g)
    x[M // 2] = 0.0
    w = None if center else 1 + 0.1 * torch.randn(D, generator=g)
    sh = 0.3 * torch.randn(B, D, generator=g) if shift else None
    sc = 0.3 * torch.randn(B, D, generator=g) if scale else None
    return dict(x=x, w=w, shift=sh, scale=sc, rpb=rpb, center=center, T=Tout)


def check_norm_fwd(c, got, key=None):
    ref = rc.norm_fwd_ref(c["x"], c["w"], c["shift"], c["scale"], c["rpb"], EPS, c["center"], c["T"])
    assert rc.finite(*ref.values())
    r1 = rc.check("y", got["y"], ref["y"], ref["by"])
    r2 = rc.check("rstd", got["rstd"], ref["rstd"], ref["brstd"])
    if key:
        _rec(f"{key}:y", r1), _rec(f"{key}:rstd", r2)


def run_norm_fwd(c, E):
    return em_norm_fwd(E, c["x"], c["w"], c["shift"], c["scale"], c["rpb"], EPS, c["center"], c["T"])


def norm_bwd_case(D, Tg, center=False, gate=False, bx=0, bw=0, fam="unit", rpb=8, B=2, seed=2):
    g = _gen(seed + D)
    M = B * rpb
    x = T._row_input(M, D, "ln" if center else fam, g)
    dout = torch.randn(M, D, generator=g)
    if fam == "hot":
        rc.hot(dout, g)
    c = dict(dout=dout.to(Tg), x=x, w=None if center else 1 + 0.1 * torch.randn(D, generator=g), scale=0.3 * torch.randn(B, D, generator=g),
             rpb=rpb, center=center, dx_old=torch.randn(M, D, generator=g) if bx else None,
             dw_old=torch.randn(D, generator=g) if bw and not center else None,
             y=torch.randn(M, D, generator=g).to(Tg) if gate else None, gate=1 + 0.1 * torch.randn(B, D, generator=g) if gate else None)
    c["rstd"] = rc.row_stats(x, EPS, center)[2][:, 0].float()
    return c


def run_norm_bwd(c, E):
    return em_norm_bwd(E, c["dout"], c["x"], c["w"], c["scale"], c["rstd"], c["rpb"], c["center"], c["dx_old"], c["dw_old"], c["y"], c["gate"])


def check_norm_bwd(c, got, key=None, only=None):
    ref = rc.norm_bwd_ref(c["dout"], c["x"], c["w"], c["scale"], c["rstd"], c["rpb"], c["center"], c["dx_old"], c["dw_old"], c["y"], c["gate"])
    for n in got:
        if only and n not in only:
            continue
        if n == "dbias":
            r = rc.stored_colsum("dbias", got["dbias"], got["dy"])
        else:
            assert rc.finite(*ref[n])
            r = rc.check(n, got[n], *ref[n])
        if key:
            _rec(f"{key}:{n}", r)


def qk_case(hd, Tq, mode="norm", B=1, N=6, H=2, seed=3):
    g = _gen(seed + hd)
    cos, sin = rc.tables(N, hd, g)
    qkv = torch.stack([rc.hot(torch.randn(B, N, H, hd, generator=g), g, 1, 8.0) for _ in range(3)], 2).to(Tq)
    qkv[0, N // 2, :2, H - 1] = 0
    return dict(qkv=qkv, w=1 + 0.1 * torch.randn(2, hd, generator=g), cos=cos, sin=sin, mode=mode, T=Tq,
                grads=[torch.randn(B, H, N, hd, generator=g).to(Tq) for _ in range(2)])


def check_qk_fwd(c, got, key=None):
    for s, n in enumerate(("q", "k")):
        x = c["qkv"][:, :, s].permute(0, 2, 1, 3)
        ref, b = rc.qk_fwd_ref(x, c["w"][s] if c["mode"] == "norm" else None, c["cos"], c["sin"], EPS, c["T"])
        assert rc.finite(ref, b)
        r = rc.check(n, got[s], ref, b)
        if key:
            _rec(f"{key}:{n}", r)


def run_qk_bwd(c, E):
    """-> (dq slot, dk slot) in T, dw [2, hd] or None"""
    slots, dw = [], []
    for s in range(2):
        x = c["qkv"][:, :, s].permute(0, 2, 1, 3)
        o, tn = em_qk_bwd(E, c["grads"][s], x, c["w"][s] if c["mode"] == "norm" else None, c["cos"], c["sin"], EPS)
        slots.append(o.to(c["T"]))
        if tn is not None:
            hd = o.shape[-1]
            dw.append(_colsum(E, tn[0].reshape(-1, hd), tn[1].reshape(-1, hd), 1)[0])
    return slots, (torch.stack(dw) if dw else None)


def check_qk_bwd(c, slots, dw, key=None):
    for s, n in enumerate(("dq", "dk")):
        norm = c["mode"] == "norm"
        x = c["qkv"][:, :, s].permute(0, 2, 1, 3) if norm else None
        w = c["w"][s] if norm else None
        ref, b = rc.qk_bwd_ref(c["grads"][s], x, w, c["cos"], c["sin"], EPS, c["T"])
        assert rc.finite(ref, b)
        r = rc.check(n + "-slot", slots[s], ref, b)
        if key:
            _rec(f"{key}:{n}-slot", r)
        if norm:
            ref, b = rc.qk_dw_ref(c["grads"][s], x, w, c["cos"], c["sin"], EPS)
            assert rc.finite(ref, b)
            r = rc.check("dw" + n[1], dw[s], ref, b)
            if key:
                _rec(f"{key}:dw", r)


# ----------------------------------------------------------------------------- the emulation is inside the bounds
FWD_CLASSES = sorted({(c["D"], _t, c["center"], c["shift"], c["scale"], c["fam"]) for c in T.NORM_FWD for _t in [c["dtype"]]}, key=str)
BWD_CLASSES = sorted({(c["D"], c["dtype"], c["form"] == "ln", c["gate"]) for c in T.NORM_BWD}, key=str)
QK_CLASSES = sorted({(c["hd"], c["dtype"], c["mode"]) for c in T.QK_FWD + T.QK_BWD if c["mode"] != "plain"}, key=str)


@pytest.mark.parametrize("assoc,fma", VARIANTS)
def test_emulation_norm_fwd_inside_bounds(assoc, fma):
    for D, Tout, center, shift, scale, fam in FWD_CLASSES:
        c = norm_fwd_case(D, Tout, center, shift, scale, fam)
        check_norm_fwd(c, run_norm_fwd(c, Em(assoc, fma)), f"norm_fwd[{'ln' if center else 'rms'},{T._tn(Tout)}]")


@pytest.mark.parametrize("assoc,fma", VARIANTS)
def test_emulation_norm_bwd_inside_bounds(assoc, fma):
    for i, (D, Tg, center, gate) in enumerate(BWD_CLASSES):
        for rpb in (5, 8):
            c = norm_bwd_case(D, Tg, center, gate, bx=(i + rpb) % 2, bw=i % 2, fam="hot" if i % 3 == 0 else "unit", rpb=rpb)
            check_norm_bwd(c, run_norm_bwd(c, Em(assoc, fma)), f"norm_bwd[{'ln' if center else 'rms'},{T._tn(Tg)}]")


@pytest.mark.parametrize("assoc,fma", VARIANTS)
def test_emulation_gate_bwd_inside_bounds(assoc, fma):
    for D, Tg, gate in sorted({(c["D"], c["dtype"], c["gate"]) for c in T.GATE_BWD}, key=str):
        g = _gen(50 + D)
        M, rpb = 12, 6
        dx, y = rc.hot(torch.randn(M, D, generator=g), g), torch.randn(M, D, generator=g).to(Tg)
        gt = 1 + 0.1 * torch.randn(2, D, generator=g) if gate else None
        got = em_gate_bwd(Em(assoc, fma), dx, y if gate else None, gt, rpb, Tg)
        ref = rc.gate_bwd_ref(dx.double(), torch.zeros(M, D, dtype=torch.float64), y if gate else None, gt, rpb, Tg)
        key = f"gate_bwd[{T._tn(Tg)}]"
        _rec(key + ":dy", rc.check("dy", got["dy"], *ref["dy"]))
        if gate:
            _rec(key + ":dgate", rc.check("dgate", got["dgate"], *ref["dgate"]))
        _rec(key + ":dbias", rc.stored_colsum("dbias", got["dbias"], got["dy"]))


@pytest.mark.parametrize("assoc,fma", VARIANTS)
def test_emulation_qk_inside_bounds(assoc, fma):
    for hd, Tq, mode in QK_CLASSES:
        c = qk_case(hd, Tq, mode)
        E = Em(assoc, fma)
        check_qk_fwd(c, em_qk_fwd(E, c["qkv"], c["w"], c["cos"], c["sin"], EPS, mode), f"qk_fwd[{T._tn(Tq)},{mode}]")
        check_qk_bwd(c, *run_qk_bwd(c, E), key=f"qk_bwd[{T._tn(Tq)},{mode}]")


@pytest.mark.parametrize("fma", [False, True])
def test_emulation_rope_inside_bounds(fma):
    for hd, Tr, tr in sorted({(c["hd"], c["dtype"], c["transposed"]) for c in T.ROPE}, key=str):
        g = _gen(70 + hd)
        cos, sin = rc.tables(6, hd, g)
        t = torch.randn(3, 6, hd, generator=g).to(Tr)
        got = em_rope(Em("tree", fma), t.float(), cos, sin, bool(tr)).to(Tr)
        ref, fn = rc.rope_ref(t.double(), cos, sin, bool(tr))
        _rec(f"rope[{T._tn(Tr)}]:out", rc.check("rope", got, ref, rc.stored(ref, fn, Tr)))


# ----------------------------------------------------------------------------- non-vacuity
def _flips(t):
    """t (16-bit) with one element moved by 2 ulp: first, last, a random interior element."""
    n = t.numel()
    for i in (0, n - 1, int(torch.randint(1, n - 1, (1,), generator=_gen(n)))):
        bits = t.clone().flatten().view(torch.int16)
        bits[i] += 2                                              # 2 ulp away in magnitude (the sign bit is untouched)
        yield i, bits.view(t.dtype).reshape(t.shape)


def test_two_ulp_flip_of_a_16bit_output_is_rejected():
    E = Em()
    for center, fam in ((False, "hot"), (True, "ln")):
        c = norm_fwd_case(192, BF16, center, fam=fam)
        got = run_norm_fwd(c, E)
        for i, y in _flips(got["y"]):
            with pytest.raises(rc.BoundError):
                check_norm_fwd(c, dict(got, y=y))
    c = norm_bwd_case(192, BF16, gate=True, bx=1, fam="hot")
    got = run_norm_bwd(c, E)
    for i, dy in _flips(got["dy"]):
        with pytest.raises(rc.BoundError):
            check_norm_bwd(c, dict(got, dy=dy), only=("dy",))
    for hd in (8, 72):
        for mode in ("norm", "rope"):
            c = qk_case(hd, BF16, mode)
            q, k = em_qk_fwd(E, c["qkv"], c["w"], c["cos"], c["sin"], EPS, mode)
            slots, dw = run_qk_bwd(c, E)
            for i, k2 in _flips(k):
                with pytest.raises(rc.BoundError):
                    check_qk_fwd(c, [q, k2])
            for i, s2 in _flips(slots[0]):
                with pytest.raises(rc.BoundError):
                    check_qk_bwd(c, [s2, slots[1]], dw)
    g = _gen(9)
    cos, sin = rc.tables(6, 64, g)
    t = torch.randn(2, 6, 64, generator=g).to(BF16)
    for tr in (False, True):
        ref, fn = rc.rope_ref(t.double(), cos, sin, tr)
        for i, o in _flips(em_rope(E, t.float(), cos, sin, tr).to(BF16)):
            with pytest.raises(rc.BoundError):
                rc.check("rope", o, ref, rc.stored(ref, fn, BF16))


def _rejected(fn):
    with pytest.raises(rc.BoundError):
        fn()


def test_bf16_intermediates_are_rejected_for_every_f32_output():
    E = Em(lowp=True)
    for center in (False, True):
        c = norm_fwd_case(192, F32, center, fam="ln" if center else "unit")
        got = run_norm_fwd(c, E)
        ref = rc.norm_fwd_ref(c["x"], c["w"], c["shift"], c["scale"], c["rpb"], EPS, center, F32)
        _rejected(lambda: rc.check("y", got["y"], ref["y"], ref["by"]))
        _rejected(lambda: rc.check("rstd", got["rstd"], ref["rstd"], ref["brstd"]))
        c = norm_bwd_case(192, F32, center, gate=True, bx=1, bw=1)
        got = run_norm_bwd(c, E)
        for n in got:
            if n != "dbias":
                _rejected(lambda: check_norm_bwd(c, got, only=(n,)))
        _rejected(lambda: rc.stored_colsum("dbias", got["dbias"], run_norm_bwd(c, Em())["dy"]))
    for hd in (16, 72):
        c = qk_case(hd, F32)
        q, k = em_qk_fwd(E, c["qkv"], c["w"], c["cos"], c["sin"], EPS, "norm")
        good = em_qk_fwd(Em(), c["qkv"], c["w"], c["cos"], c["sin"], EPS, "norm")
        _rejected(lambda: check_qk_fwd(c, [q, good[1]]))
        _rejected(lambda: check_qk_fwd(c, [good[0], k]))
        slots, dw = run_qk_bwd(c, E)
        gs, gw = run_qk_bwd(c, Em())
        _rejected(lambda: check_qk_bwd(c, [slots[0], gs[1]], gw))
        _rejected(lambda: check_qk_bwd(c, gs, torch.stack([dw[0], gw[1]])))
    g = _gen(10)
    cos, sin = rc.tables(6, 64, g)
    t = torch.randn(2, 6, 64, generator=g)
    ref, fn = rc.rope_ref(t.double(), cos, sin)
    _rejected(lambda: rc.check("rope", em_rope(E, t, cos, sin), ref, fn))


# ----------------------------------------------------------------------------- planted faults
def _fault_fwd(fault, **kw):
    c = norm_fwd_case(**kw)
    check_norm_fwd(c, run_norm_fwd(c, Em()))                     # without the defect: inside
    _rejected(lambda: check_norm_fwd(c, run_norm_fwd(c, Em(fault=fault))))


def _fault_bwd(fault, only=None, **kw):
    c = norm_bwd_case(**kw)
    check_norm_bwd(c, run_norm_bwd(c, Em()))
    _rejected(lambda: check_norm_bwd(c, run_norm_bwd(c, Em(fault=fault)), only=only))


def test_planted_faults_norm_forward():
    for Tout in (F32, BF16):
        _fault_fwd("eps_omitted", D=192, Tout=Tout, fam="tiny")               # mean(x^2) = 1e-6 = eps
        _fault_fwd("rstd_neighbour", D=192, Tout=Tout, fam="hot")
        _fault_fwd("scale_no_one", D=192, Tout=Tout)
        _fault_fwd("mod_next_sample", D=192, Tout=Tout)
        _fault_fwd("mod_next_sample", D=192, Tout=Tout, shift=False)
        _fault_fwd("last_chunk_unnormalised", D=260, Tout=Tout)
        _fault_fwd("last_chunk_unwritten", D=1156, Tout=Tout)
        _fault_fwd("div_256nch", D=260, Tout=Tout)
        _fault_fwd("center_var_e2", D=192, Tout=Tout, center=True, fam="ln")   # |mean| = 30 std


def test_planted_faults_norm_backward():
    for Tg in (F32, BF16):
        _fault_bwd("no_msum", only=("dx",), D=192, Tg=Tg, center=True)
        _fault_bwd("beta_as_overwrite", only=("dx",), D=192, Tg=Tg, bx=1)
        _fault_bwd("beta_as_accumulate", only=("dx",), D=192, Tg=Tg, bx=0)
        _fault_bwd("drop_last_partial", only=("dshift",), D=192, Tg=Tg)
        _fault_bwd("drop_last_partial", only=("dscale",), D=260, Tg=Tg, rpb=5)
        _fault_bwd("drop_last_partial", only=("dgate",), D=192, Tg=Tg, gate=True)
        _fault_bwd("partials_next_sample", only=("dshift",), D=192, Tg=Tg)
        _fault_bwd("partials_next_sample", only=("dgate",), D=192, Tg=Tg, gate=True, center=True)
        _fault_bwd("dgate_pre_accumulate", only=("dgate",), D=192, Tg=Tg, gate=True, bx=1)


def test_planted_faults_rope():
    for Tq in (F32, BF16):
        for hd in (8, 72):
            c = qk_case(hd, Tq)
            run = lambda E: em_qk_fwd(E, c["qkv"], c["w"], c["cos"], c["sin"], EPS, "norm")      # noqa: E731
            check_qk_fwd(c, run(Em()))
            for fault in ("sin_sign", "pair_swapped", "table_row_next", "adjoint_as_forward", "wk_on_q", "k_at_v_offset", "rowsum_neighbour"):
                _rejected(lambda: check_qk_fwd(c, run(Em(fault=fault))))
            check_qk_bwd(c, *run_qk_bwd(c, Em()))
            for fault in ("sin_sign", "pair_swapped", "table_row_next", "adjoint_as_forward"):
                _rejected(lambda: check_qk_bwd(c, *run_qk_bwd(c, Em(fault=fault))))
        g = _gen(11)
        cos, sin = rc.tables(6, 64, g)
        t = torch.randn(2, 6, 64, generator=g).to(Tq)
        for tr in (False, True):
            ref, fn = rc.rope_ref(t.double(), cos, sin, tr)
            rc.check("rope", em_rope(Em(), t.float(), cos, sin, tr).to(Tq), ref, rc.stored(ref, fn, Tq))
            for fault in ("sin_sign", "pair_swapped", "table_row_next", "adjoint_as_forward"):
                _rejected(lambda: rc.check("rope", em_rope(Em(fault=fault), t.float(), cos, sin, tr).to(Tq), ref, rc.stored(ref, fn, Tq)))


# ----------------------------------------------------------------------------- the case tables reach every predicate
def test_case_table_covers_every_predicate():
    """Every dispatch predicate restated in the docstring of test_gpu_row_paths.py is both taken and not taken, from the tables' shapes alone."""
    seen = {}

    def note(name, v):
        seen.setdefault(name, set()).add(bool(v))

    for c in T.NORM_FWD:
        D, M, rpb = c["D"], c["M"], c["rpb"]
        note("fwd FULL", T.norm_fwd_full(c))
        if c["dtype"] == BF16 and D % 256 == 0 and not c["center"]:
            note("fwd FULL refused by M % 16", M % 16 != 0)
            note("fwd FULL refused by rows_per_batch % 16", rpb % 16 != 0)
        for n in ("shift", "scale", "rstd", "center"):
            note(f"fwd {n}", c[n])
        note("fwd bf16", c["dtype"] == BF16)
        note("fwd mod_ld == D", c["ld"] == 1)
        note("fwd partly filled last chunk", (D // 4) % 64 != 0)
        note("fwd last workgroup has rows past M", M % 16 != 0)
    assert {rc.nch(c["D"]) for c in T.NORM_FWD} >= {1, 2, 3, 5, 7, 8}
    assert {c["D"] for c in T.NORM_FWD} >= {4, 192, 256, 260, 768, 1152, 1156, 1792, 2048}
    for c in T.NORM_BWD:
        D, rpb = c["D"], c["rpb"]
        rw = T.rows_per_wg(rpb)
        gps = rpb // rw
        note("bwd FULL", T.norm_bwd_full(c))
        note("bwd GATE", c["gate"])
        note("bwd center", c["form"] == "ln")
        note("bwd bf16", c["dtype"] == BF16)
        note("bwd beta_x", c["bx"])
        if c["form"] == "rms":
            note("bwd beta_w", c["bw"])
        note("bwd dshift / dscale given", c["ds"])
        note("bwd mod_ld == D", c["ld"] == 1)
        if c["gate"]:
            note("bwd gate_ld == D", c["gld"] == 1)
        note("bwd waves without a row (rows_per_wg < 4)", rw < 4)
        note("bwd group_reduce<32> (B >= 256)", c["B"] >= 256)
        note("bwd gps >= 8 (unrolled body)", gps >= 8)
        note("bwd gps % 8 != 0 (tail)", gps % 8 != 0)
        note("bwd unrolled body and tail together", gps > 8 and gps % 8 != 0)
        note("bwd dynamic LDS above 64 KiB", 48 * D > 65536)
        note("bwd partly filled last chunk", (D // 4) % 64 != 0)
    assert {T.rows_per_wg(c["rpb"]) for c in T.NORM_BWD} >= {1, 2, 4, 16, 64}
    assert {rc.nch(c["D"]) for c in T.NORM_BWD} == {1, 2, 3, 5, 6, 7, 8}
    for form in ("rms", "ln"):
        for gate in (False, True):
            for dt in (F32, BF16):
                assert any(c["form"] == form and c["gate"] == gate and c["dtype"] == dt for c in T.NORM_BWD), (form, gate, dt)
    for c in T.GATE_BWD:
        note("gate_bwd dgate", c["dgate"])
        note("gate_bwd dbias", c["dbias"])
        note("gate_bwd dgate and dbias (mod_partials route)", c["dgate"] and c["dbias"])
        note("gate_bwd gate", c["gate"])
        note("gate_bwd bf16", c["dtype"] == BF16)
    kernels = {}
    for c in T.QK_FWD:
        kern, passes = T.qk_fwd_path(c)
        kernels.setdefault((kern, c["dtype"]), set()).add(passes)
        note("qk_fwd v given", c["v"])
        for m in ("norm", "rope", "plain"):
            note(f"qk_fwd mode {m}", c["mode"] == m)
        if c["dtype"] == BF16 and not c["v"] and c["hd"] in (64, 128) and c["mode"] != "plain":
            note(f"qk_fwd8 refused by the item count (hd {c['hd']})", kern != "fwd8")
        if c["mode"] == "norm" and c["hd"] > 64 and (c["hd"] // 4) & (c["hd"] // 4 - 1):
            note("qk_fwd dense refused by N % 8", c["N"] % 8 != 0)
        if kern.startswith("dense"):
            note("qk_fwd dense: part of one workgroup", c["B"] * c["N"] * c["H"] <= 8)
            note("qk_fwd dense: H == 1", c["H"] == 1)
    assert kernels[("fwd8", BF16)] >= {1, 2, 3}, kernels
    for k in (("generic16", F32), ("generic32", BF16), ("dense", F32), ("dense8", BF16)):
        assert kernels[k] >= {1, 2}, (k, kernels)
    assert {k for k, _ in kernels} == {"fwd8", "generic16", "generic32", "dense", "dense8"}
    assert {c["hd"] for c in T.QK_FWD if T.qk_fwd_path(c)[0] == "generic16"} >= {8, 16, 24, 64}
    assert {c["hd"] for c in T.QK_FWD if T.qk_fwd_path(c)[0] == "generic32"} >= {72, 96, 128}
    assert {c["hd"] for c in T.QK_FWD if T.qk_fwd_path(c)[0].startswith("dense")} >= {72, 88, 120}
    branches = set()
    for c in T.QK_BWD:
        lpr = 16 if c["hd"] <= 64 else 32
        items = c["B"] * c["N"] * c["H"]
        grid, m, g = T.qk_bwd_grid(items, lpr, c["H"])
        branches.add((lpr, "m == 1" if m == 1 else ("g >= m" if g >= m else "g < m")))
        note("qk_bwd 32 lanes per item", lpr == 32)
        note("qk_bwd grid rounded down", m > 1 and g >= m and g % m != 0)
        note("qk_bwd capped grid with a second pass", g == 2048 and items * lpr > grid * 256)
        note("qk_bwd group_reduce<32> (grid >= 256)", grid >= 256)
        note("qk_bwd dbias", c["dbias"])
        note("qk_bwd dv given", c["dv"])
        note("qk_bwd dv NULL with dbias", not c["dv"] and c["dbias"])
        note("qk_bwd beta_w", c["bw"])
        note("qk_bwd bf16", c["dtype"] == BF16)
        for md in ("norm", "rope", "plain"):
            note(f"qk_bwd mode {md}", c["mode"] == md)
        assert (grid * (256 // lpr)) % c["H"] == 0
    assert branches == {(lpr, b) for lpr in (16, 32) for b in ("m == 1", "g >= m", "g < m")}, branches
    assert {c["H"] for c in T.QK_BWD} >= {1, 3, 5, 12, 16}
    assert {c["hd"] for c in T.QK_BWD} >= {8, 16, 24, 64, 72, 88, 96, 120, 128}
    for c in T.ROPE:
        note("rope bf16", c["dtype"] == BF16)
        note("rope transposed", c["transposed"])
        note("rope second pass", T.rope_passes(c) > 1)
        note("rope hd 4", c["hd"] == 4)
        assert c["rows"] % c["N"] == 0
    for name, vals in seen.items():
        assert vals == {True, False}, f"predicate {name!r} is only ever {vals}"


def test_stated_backward_grids():
    """The grid, m and g written behind each case of the QK backward table."""
    import inspect
    import re
    src = inspect.getsource(T)
    for c in T.QK_BWD:
        line = next(ln for ln in src.splitlines() if f'"{c["name"]}"' in ln)
        mt = re.search(r"#\s*(\d+)\s*\((\d+), (\d+)\)", line)
        assert mt, line
        lpr = 16 if c["hd"] <= 64 else 32
        assert tuple(int(v) for v in mt.groups()) == T.qk_bwd_grid(c["B"] * c["N"] * c["H"], lpr, c["H"]), line
