"""Every dispatch path of the row kernels (csrc/elementwise.hip: norm + modulate, gate_bwd; csrc/qk_rope.hip: QK-norm / RoPE), element by
element, with the bounds of tests/row_check.py.

Seeded case tables drive the C ABI directly, so each case controls pointers, leading dimensions and NULLs.  Each case
  - places every input in a NaN-padded buffer and every output (rstd, dx with beta_x = 0, dy, the unused column blocks of a [B, 6 D]
    modulation buffer included) inside a buffer pre-filled with the NaN payload of its type: an unwritten element, a write outside the
    tensor or into a neighbouring column block, and a read of a buffer the entry point says it does not read all fail;
  - gives workspaces exactly the size the *_workspace_bytes function reports, plus a canary tail;
  - checks every element of every output against the f64 reference with the per-element bound (zero excluded elements), asserts that
    reference and bound are finite, and checks every canary;
  - runs a second time on fresh outputs and requires bitwise-equal results;
  - records the worst err / bound per path and output (printed at module teardown).
The norm backward is fed rstd made by the f64 reference (rounded to f32), never the forward kernel's output.

Dispatch predicates (host code of csrc/elementwise.hip and csrc/qk_rope.hip), each taken and not taken by some case
(tests/test_row_check_cpu.py::test_case_table_covers_every_predicate, computed from the tables alone):
  norm forward: FULL = bf16 && D % 256 == 0 && M % 16 == 0 && rows_per_batch % 16 == 0 && !center; NCH = ceil(D / 256) in 1 .. 8; a partly
    filled last chunk; shift / scale / rstd NULL; center.
  norm backward: FULL = bf16 && D % 256 == 0 && !center; GATE; center; rows_per_wg = largest of 64 .. 1 dividing rows_per_batch (1 and 2:
    whole waves without a row); gps = rows_per_batch / rows_per_wg below 8, a multiple of 8, neither; group_reduce<32> iff B >= 256; beta_x,
    beta_w; dshift / dscale NULL; dynamic LDS 48 D bytes above 64 KiB (D >= 1536).
  gate_bwd: dgate / dbias each given or not (both: the mod_partials route; one: group_reduce or colsum); gate NULL.
  qknorm_rope_fwd: dense (wq && hd > 64 && hd / 4 not a power of two && N % 8 == 0; bf16 -> dense8), fwd8 (bf16 && cos && !v && hd in
    {64, 128} && items % (256 / (hd / 8)) == 0), else the generic kernel with 16 (hd <= 64) or 32 lanes per item; grid caps 2048 / 4096
    and the grid-stride passes they cause (fwd8: the two-in-flight loop and its tail); norm / RoPE-only / plain; v NULL.
  qknorm_rope_bwd: lanes per item; qk_bwd_grid: m = H / gcd(H, groups per workgroup) = 1, m > 1 with g >= m, g < m; the capped grid and
    its second pass; group_reduce<32> iff grid >= 256; dbias; dv NULL; beta_w; the three modes.
  rope: dtype, transposed, the 8192-workgroup cap.
  every entry point: one dtype code it has no kernel for (dtype_dispatch, csrc/common.h) is refused with -1 and writes nothing
    (test_refused_dtype_codes; buffers of the f32 size, so a fall-through to the float kernel would show as a write, not as a fault).

First device run (MI355X): all 231 cases inside their bounds with zero excluded elements, every rerun bitwise equal, no canary touched; the
module takes about 3 s.  The backward launches with more than 64 KiB of dynamic LDS (D = 1536, 1792, 2048: 72, 84, 96 KiB) were accepted
as they are and computed the right values, so the host code needs no hipFuncSetAttribute for them.  Worst err / bound per family:
  bf16 outputs (y, dy, q | k, the dqkv slots, rope)   0.99 .. 1.00   (the half ulp of the store is all but the whole bound)
  norm forward, f32:  y 0.11 .. 0.27, rstd 0.001 .. 0.28 (RMS), y 0.13 .. 0.15, rstd 0.003 (LayerNorm form)
  norm backward:      dx 0.21 .. 0.89 (RMS), 0.005 .. 0.26 (LayerNorm form); f32 dy 0.27 .. 0.79 / 0.01 .. 0.14;
                      dshift <= 0.19, dscale <= 0.29, dw <= 0.06, dgate <= 0.14, dbias <= 0.05
  gate_bwd alone:     f32 dy <= 1.00 (one rounding: the bound is that rounding), dgate <= 0.22, dbias <= 0.01
  QK forward, f32:    norm 0.05 .. 0.29, RoPE only 0.78 .. 0.86
  QK backward, f32:   slots 0.008 .. 0.09, dwq / dwk <= 0.02, dbias <= 0.18
  rope, f32:          0.53 .. 0.98
"""
import math

import pytest
import torch

import row_check as rc
from test_gpu_attention_paths import Guard, _bits

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-6
RATIOS: dict = {}


@pytest.fixture(scope="module")
def lib():
    import time
    from ldmae_amd import _lib
    assert _lib.load().ldmae_arch() == b"gfx950"
    t0 = time.time()
    yield _lib
    if RATIOS:
        print(f"\nmodule wall time {time.time() - t0:.1f} s; worst |got - ref| / bound per path and output:")
        for k in sorted(RATIOS):
            print(f"  {k:52s} {RATIOS[k]:.3f}")


def _dt(dtype):
    return {F32: 0, BF16: 1}[dtype]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _record(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)


def _tn(dtype):
    return str(dtype)[6:]


def _gen(name):
    return torch.Generator().manual_seed(4000 + sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003)


def _p(g):
    return None if g is None else g.ptr()


class ModBuf:
    """Per-sample [B, D] vectors as the kernels take them: ld = 1 -> one guarded [B, D] buffer each; ld = 6 -> column blocks of ONE guarded
    [B, 6 D] buffer whose other blocks keep the NaN payload (inputs: must not be read; outputs: must not be written)."""

    def __init__(self, B, D, ld, names, values=None):
        self.B, self.D, self.ld, self.names = B, D, ld * D, list(names)
        values = values or {}
        if ld == 1:
            self.g = {n: Guard((B, D), F32, values.get(n)) for n in self.names}
        else:
            self.big = Guard((B, ld * D), F32)
            for n in self.names:
                if n in values:
                    self.view(n).copy_(values[n])

    def _blk(self, n):
        return 1 + 2 * self.names.index(n)            # blocks 1, 3, 5: every used block has an unused neighbour on both sides

    def view(self, n):
        if self.ld == self.D:
            return self.g[n].t
        b = self._blk(n)
        return self.big.t[:, b * self.D:(b + 1) * self.D]

    def ptr(self, n):
        return self.g[n].ptr() if self.ld == self.D else self.big.ptr() + 4 * self.D * self._blk(n)

    def intact(self):
        if self.ld == self.D:
            return all(g.intact() for g in self.g.values())
        used = {self._blk(n) for n in self.names}
        rest = [self.big.t[:, b * self.D:(b + 1) * self.D] for b in range(self.ld // self.D) if b not in used]
        return self.big.intact() and all(self.big.untouched(r) for r in rest)


def _twice(run):
    """run() -> dict name -> tensor (clones of fresh guarded outputs); twice, bitwise equal."""
    a = run()
    b = run()
    for n in a:
        assert torch.equal(_bits(a[n]), _bits(b[n])), f"{n}: rerun not bitwise equal"
    return a


def _chk(path, name, out, got, ref, bound):
    assert rc.finite(ref, bound), f"{name} {out}: reference or bound not finite"
    _record(f"{path}:{out}", rc.check(f"{name} {out}", got, ref, bound))


# ============================================================================= norm + modulate forward
def NF(name, D, M, rpb, dtype, ld=1, center=False, shift=True, scale=True, rstd=True, fam="unit"):
    return dict(name=name, D=D, M=M, rpb=rpb, dtype=dtype, ld=ld, center=center, shift=shift, scale=scale, rstd=rstd, fam=fam)


def norm_fwd_full(c):
    return c["dtype"] == BF16 and c["D"] % 256 == 0 and c["M"] % 16 == 0 and c["rpb"] % 16 == 0 and not c["center"]


NORM_FWD = []
for _D in (256, 768, 2048):                                    # FULL for bf16; the same shapes in f32 take the guarded kernel
    for _T in (F32, BF16):
        for _ld in (1, 6):
            NORM_FWD.append(NF(f"full_{_D}_{_tn(_T)}_ld{_ld}", _D, 32, 16, _T, _ld, fam="hot" if _ld == 6 else "unit"))
for _M, _r in ((20, 4), (24, 8), (15, 5)):                     # FULL refused by M or rows_per_batch
    for _T in (F32, BF16):
        NORM_FWD.append(NF(f"refused_768_M{_M}_rpb{_r}_{_tn(_T)}", 768, _M, _r, _T, 6 if _M == 24 else 1))
for _i, _D in enumerate((4, 192, 260, 1152, 1156, 1792)):      # guarded widths; 4, 260, 1156: a partly filled last chunk
    for _T in (F32, BF16):
        NORM_FWD.append(NF(f"guarded_{_D}_{_tn(_T)}", _D, 18, 6, _T, 1 + 5 * (_i % 2), fam="hot" if _D >= 192 and _T == BF16 else "unit"))
NORM_FWD += [
    NF("null_shift_768_bf16", 768, 32, 16, BF16, shift=False),
    NF("null_scale_768_bf16", 768, 32, 16, BF16, 6, scale=False),
    NF("null_both_768_bf16", 768, 32, 16, BF16, shift=False, scale=False),
    NF("null_rstd_768_bf16", 768, 32, 16, BF16, rstd=False),
    NF("null_shift_260_f32", 260, 10, 5, F32, 6, shift=False),
    NF("null_scale_192_bf16", 192, 10, 5, BF16, scale=False),
    NF("null_both_192_f32", 192, 10, 5, F32, shift=False, scale=False),
    NF("null_rstd_1156_f32", 1156, 10, 5, F32, rstd=False),
    NF("ln_192_f32", 192, 18, 6, F32, center=True, fam="ln"),
    NF("ln_192_bf16_ld6", 192, 18, 6, BF16, 6, center=True, fam="ln"),
    NF("ln_768_f32_ld6", 768, 32, 16, F32, 6, center=True, fam="ln"),
    NF("ln_768_bf16", 768, 32, 16, BF16, center=True, fam="ln"),
    NF("ln_768_bf16_null_both", 768, 16, 16, BF16, center=True, shift=False, scale=False, fam="ln"),
    NF("tiny_rows_768_bf16", 768, 32, 16, BF16, fam="tiny"),
    NF("tiny_rows_192_f32", 192, 18, 6, F32, fam="tiny"),
]


def _row_input(M, D, fam, g):
    x = torch.randn(M, D, generator=g)
    if fam == "hot":
        rc.hot(x, g)
    elif fam == "ln":
        x = 30.0 + x
    elif fam == "tiny":
        x = 1e-3 * x
    return x


def _mod_values(B, D, g, **which):
    return {n: (0.3 * torch.randn(B, D, generator=g)).cuda() for n, on in which.items() if on}


@pytest.mark.parametrize("c", NORM_FWD, ids=[c["name"] for c in NORM_FWD])
def test_norm_fwd(lib, c):
    D, M, rpb, T, center = c["D"], c["M"], c["rpb"], c["dtype"], c["center"]
    B, g = M // rpb, _gen(c["name"])
    x = _row_input(M, D, c["fam"], g)
    zrow = M // 2
    x[zrow] = 0.0                                              # one all-zero row: eps keeps rstd finite, the output is exactly shift (or 0)
    w = None if center else (1 + 0.1 * torch.randn(D, generator=g))
    vals = _mod_values(B, D, g, shift=c["shift"], scale=c["scale"])
    Gx, Gw = Guard((M, D), F32, x.cuda()), (None if center else Guard((D,), F32, w.cuda()))
    mod = ModBuf(B, D, c["ld"], list(vals), vals)
    psh, psc = (mod.ptr("shift") if c["shift"] else None), (mod.ptr("scale") if c["scale"] else None)

    def run():
        out, rstd = Guard((M, D), T), (Guard((M,), F32) if c["rstd"] else None)
        if center:
            lib.call("ldmae_layernorm_modulate_fwd", _dt(T), Gx.ptr(), psh, psc, mod.ld, out.ptr(), _p(rstd), M, D, rpb, EPS, _stream())
        else:
            lib.call("ldmae_rmsnorm_modulate_fwd", _dt(T), Gx.ptr(), Gw.ptr(), psh, psc, mod.ld, out.ptr(), _p(rstd), M, D, rpb, EPS, _stream())
        torch.cuda.synchronize()
        assert out.intact() and (rstd is None or rstd.intact()) and Gx.intact() and mod.intact(), "a canary changed"
        r = dict(y=out.t.clone())
        if rstd is not None:
            r["rstd"] = rstd.t.clone()
        return r

    got = _twice(run)
    ref = rc.norm_fwd_ref(Gx.t, None if center else Gw.t, vals.get("shift"), vals.get("scale"), rpb, EPS, center, T)
    path = f"norm_fwd[{'ln' if center else 'rms'},{_tn(T)},{'full' if norm_fwd_full(c) else 'guarded'},NCH{rc.nch(D)}]"
    _chk(path, c["name"], "y", got["y"], ref["y"], ref["by"])
    if c["rstd"]:
        _chk(path, c["name"], "rstd", got["rstd"], ref["rstd"], ref["brstd"])
    want = vals["shift"][zrow // rpb].to(T) if c["shift"] else torch.zeros(D, dtype=T, device="cuda")
    assert torch.equal(got["y"][zrow].float(), want.float()), "the all-zero row is not exactly shift"


# ============================================================================= norm + modulate backward (plain and gate-fused)
def NB(name, D, B, rpb, dtype, form="rms", gate=False, bx=0, bw=0, ld=1, ds=True, gld=1, fam="unit"):
    return dict(name=name, D=D, B=B, rpb=rpb, dtype=dtype, form=form, gate=gate, bx=bx, bw=bw, ld=ld, ds=ds, gld=gld, fam=fam)


def rows_per_wg(rpb):
    return next(r for r in (64, 32, 16, 8, 4, 2, 1) if rpb % r == 0)


def norm_bwd_full(c):
    return c["dtype"] == BF16 and c["D"] % 256 == 0 and c["form"] == "rms"


NORM_BWD = []
_k = 0
for _rpb, _B in ((5, 3), (6, 3), (36, 2), (80, 2), (1024, 2)):     # rows_per_wg 1, 2, 4, 16, 64; gps 5, 3, 9, 5, 16
    for _T in (F32, BF16):
        for _form in ("rms", "ln"):
            for _gate in (False, True):
                _D = (192, 256, 260, 768)[_k % 4] if _rpb != 1024 else (192, 256)[_k % 2]
                NORM_BWD.append(NB(f"rpb{_rpb}_{_D}_{_tn(_T)}_{_form}{'_gate' if _gate else ''}", _D, _B, _rpb, _T, _form, _gate,
                                   bx=_k % 2, bw=(_k // 2) % 2, ld=1 + 5 * ((_k // 3) % 2), gld=1 + 5 * ((_k // 5) % 2),
                                   fam="hot" if _k % 3 == 0 else "unit"))
                _k += 1
for _T in (F32, BF16):                                             # B >= 256: group_reduce_kernel<32> sums the per-sample weight gradients
    NORM_BWD.append(NB(f"B256_192_{_tn(_T)}_rms", 192, 256, 4, _T, "rms", bx=1, bw=1))
    NORM_BWD.append(NB(f"B256_192_{_tn(_T)}_rms_gate", 192, 256, 4, _T, "rms", True, ld=6, gld=6))
for _i, _D in enumerate((256, 768, 1152, 1156, 1536, 1792, 2048)):  # every NCH up to 8; from 1536 on more than 64 KiB of dynamic LDS
    for _T in (F32, BF16):
        for _gate in (False, True):
            _form = "ln" if (_i + _gate + (_T == BF16)) % 3 == 0 else "rms"
            NORM_BWD.append(NB(f"wide_{_D}_{_tn(_T)}_{_form}{'_gate' if _gate else ''}", _D, 2, 12, _T, _form, _gate, bx=(_i + _gate) % 2,
                               bw=_i % 2, ld=1 + 5 * (_i % 2), gld=6 if _gate and _i % 2 == 0 else 1, fam="hot" if _i % 2 else "unit"))
NORM_BWD += [
    NB("null_dshift_dscale_768_bf16", 768, 2, 16, BF16, ds=False),
    NB("null_dshift_dscale_260_f32_gate", 260, 2, 8, F32, "rms", True, bx=1, ds=False),
    NB("null_dshift_dscale_192_bf16_ln", 192, 2, 8, BF16, "ln", ds=False),
]


@pytest.mark.parametrize("c", NORM_BWD, ids=[c["name"] for c in NORM_BWD])
def test_norm_bwd(lib, c):
    D, B, rpb, T, center, gate = c["D"], c["B"], c["rpb"], c["dtype"], c["form"] == "ln", c["gate"]
    M, g = B * rpb, _gen(c["name"])
    x = _row_input(M, D, "ln" if center else c["fam"], g)
    dout = torch.randn(M, D, generator=g)
    if c["fam"] == "hot":
        rc.hot(dout, g)
    w = None if center else (1 + 0.1 * torch.randn(D, generator=g))
    scale = (0.3 * torch.randn(B, D, generator=g)).cuda()
    Gx, Gd = Guard((M, D), F32, x.cuda()), Guard((M, D), T, dout.to(T).cuda())
    Gw = None if center else Guard((D,), F32, w.cuda())
    mod = ModBuf(B, D, c["ld"], ["scale"], dict(scale=scale))
    rstd = rc.row_stats(Gx.t, EPS, center)[2][:, 0].float().contiguous()          # made by the f64 reference, rounded to f32
    Gr = Guard((M,), F32, rstd)
    dx_old = torch.randn(M, D, generator=g).cuda() if c["bx"] else None
    dw_old = torch.randn(D, generator=g).cuda() if c["bw"] and not center else None
    if gate:
        y = torch.randn(M, D, generator=g).to(T).cuda()
        gvals = dict(gate=(1 + 0.1 * torch.randn(B, D, generator=g)).cuda())
        Gy, gbuf = Guard((M, D), T, y), ModBuf(B, D, c["gld"], ["gate"], gvals)
    lb = lib.load()
    nws = (lb.ldmae_rmsnorm_modulate_bwd_gate_workspace_bytes if gate else lb.ldmae_rmsnorm_modulate_bwd_workspace_bytes)(M, D, rpb)
    assert nws > 0 and nws % 4 == 0

    def run():
        ws = Guard((nws // 4,), F32)
        dx = Guard((M, D), F32, dx_old)
        dmod = ModBuf(B, D, c["ld"], ["dshift", "dscale"]) if c["ds"] else None
        dw = None if center else Guard((D,), F32, dw_old)
        pds, pdc, dld = (dmod.ptr("dshift"), dmod.ptr("dscale"), dmod.ld) if c["ds"] else (None, None, D)
        head = (_dt(T), Gd.ptr(), Gx.ptr()) + (() if center else (Gw.ptr(),)) + (mod.ptr("scale"), mod.ld, Gr.ptr(), dx.ptr(), float(c["bx"]),
                                                                                 pds, pdc, dld) + (() if center else (dw.ptr(), float(c["bw"])))
        outs = [ws, dx] + ([dw] if dw else [])
        if gate:
            dy, dgate, dbias = Guard((M, D), T), ModBuf(B, D, c["gld"], ["dgate"]), Guard((D,), F32)
            lib.call("ldmae_layernorm_modulate_bwd_gate" if center else "ldmae_rmsnorm_modulate_bwd_gate", *head, Gy.ptr(), gbuf.ptr("gate"), gbuf.ld,
                     dy.ptr(), dgate.ptr("dgate"), dgate.ld, dbias.ptr(), M, D, rpb, ws.ptr(), _stream())
            outs += [dy, dgate, dbias]
        else:
            lib.call("ldmae_layernorm_modulate_bwd" if center else "ldmae_rmsnorm_modulate_bwd", *head, M, D, rpb, ws.ptr(), _stream())
        torch.cuda.synchronize()
        assert all(o.intact() for o in outs) and (dmod is None or dmod.intact()), "a canary around an output or the workspace changed"
        assert Gx.intact() and Gd.intact() and Gr.intact() and mod.intact()
        r = dict(dx=dx.t.clone())
        if dmod:
            r["dshift"], r["dscale"] = dmod.view("dshift").clone(), dmod.view("dscale").clone()
        if dw:
            r["dw"] = dw.t.clone()
        if gate:
            r["dy"], r["dgate"], r["dbias"] = dy.t.clone(), dgate.view("dgate").clone(), dbias.t.clone()
        return r

    got = _twice(run)
    ref = rc.norm_bwd_ref(Gd.t, Gx.t, None if center else Gw.t, scale, rstd, rpb, center, dx_old, dw_old,
                          Gy.t if gate else None, gvals["gate"] if gate else None)
    rw = rows_per_wg(rpb)
    path = (f"norm_bwd[{c['form']},{_tn(T)},{'gate' if gate else 'plain'},{'full' if norm_bwd_full(c) else 'guarded'},NCH{rc.nch(D)},"
            f"rw{rw},gps{rpb // rw}{',B256' if B >= 256 else ''}]")
    for n in got:
        if n != "dbias":
            _chk(path, c["name"], n, got[n], *ref[n])
    if gate:
        _record(path + ":dbias", rc.stored_colsum(c["name"] + " dbias", got["dbias"], got["dy"]))


# ============================================================================= gate_bwd alone
def GB(name, D, B, rpb, dtype, dgate, dbias, gate=True, gld=1):
    return dict(name=name, D=D, B=B, rpb=rpb, dtype=dtype, dgate=dgate, dbias=dbias, gate=gate, gld=gld)


GATE_BWD = []
for _i, (_dg, _db) in enumerate(((True, False), (False, True), (True, True), (False, False))):
    for _T in (F32, BF16):
        _D, _rpb = ((260, 36), (768, 5), (192, 80), (1156, 6))[_i] if _T == BF16 else ((192, 5), (260, 80), (768, 36), (4, 6))[_i]
        GATE_BWD.append(GB(f"gate_bwd_{_D}_rpb{_rpb}_{_tn(_T)}{'_dgate' if _dg else ''}{'_dbias' if _db else ''}", _D, 3, _rpb, _T, _dg, _db,
                           gld=1 + 5 * (_i % 2)))
GATE_BWD += [
    GB("gate_bwd_nullgate_192_bf16_dbias", 192, 2, 36, BF16, False, True, gate=False),
    GB("gate_bwd_nullgate_260_f32", 260, 2, 6, F32, False, False, gate=False),
    GB("gate_bwd_2048_bf16_dgate_dbias", 2048, 2, 12, BF16, True, True),
    GB("gate_bwd_B256_192_f32_dgate_dbias", 192, 256, 4, F32, True, True, gld=6),
]


@pytest.mark.parametrize("c", GATE_BWD, ids=[c["name"] for c in GATE_BWD])
def test_gate_bwd(lib, c):
    D, B, rpb, T = c["D"], c["B"], c["rpb"], c["dtype"]
    M, g = B * rpb, _gen(c["name"])
    dx = rc.hot(torch.randn(M, D, generator=g), g).cuda()
    y = torch.randn(M, D, generator=g).to(T).cuda() if c["dgate"] else None
    gvals = dict(gate=(1 + 0.1 * torch.randn(B, D, generator=g)).cuda()) if c["gate"] else {}
    Gdx, Gy = Guard((M, D), F32, dx), (Guard((M, D), T, y) if c["dgate"] else None)
    gbuf = ModBuf(B, D, c["gld"], list(gvals), gvals)
    nws = lib.load().ldmae_gate_bwd_workspace_bytes(M, D, rpb)
    assert nws > 0 and nws % 4 == 0

    def run():
        ws = Guard((nws // 4,), F32) if (c["dgate"] or c["dbias"]) else None
        dy = Guard((M, D), T)
        dgate = ModBuf(B, D, c["gld"], ["dgate"]) if c["dgate"] else None
        dbias = Guard((D,), F32) if c["dbias"] else None
        lib.call("ldmae_gate_bwd", _dt(T), Gdx.ptr(), _p(Gy), gbuf.ptr("gate") if c["gate"] else None, gbuf.ld, dy.ptr(),
                 dgate.ptr("dgate") if dgate else None, dgate.ld if dgate else D, _p(dbias), M, D, rpb, _p(ws), _stream())
        torch.cuda.synchronize()
        assert dy.intact() and all(o is None or o.intact() for o in (ws, dgate, dbias)) and Gdx.intact() and gbuf.intact(), "a canary changed"
        r = dict(dy=dy.t.clone())
        if dgate:
            r["dgate"] = dgate.view("dgate").clone()
        if dbias:
            r["dbias"] = dbias.t.clone()
        return r

    got = _twice(run)
    ref = rc.gate_bwd_ref(dx.double(), torch.zeros_like(dx, dtype=torch.float64), y, gvals.get("gate"), rpb, T)
    rw = rows_per_wg(rpb)
    path = f"gate_bwd[{_tn(T)},NCH{rc.nch(D)},rw{rw},gps{rpb // rw}{',dgate' if c['dgate'] else ''}{',dbias' if c['dbias'] else ''}]"
    _chk(path, c["name"], "dy", got["dy"], *ref["dy"])
    if c["dgate"]:
        _chk(path, c["name"], "dgate", got["dgate"], *ref["dgate"])
    if c["dbias"]:
        _record(path + ":dbias", rc.stored_colsum(c["name"] + " dbias", got["dbias"], got["dy"]))


# ============================================================================= QK-norm + RoPE forward
def QF(name, dtype, hd, B, N, H, v=True, mode="norm"):
    return dict(name=name, dtype=dtype, hd=hd, B=B, N=N, H=H, v=v, mode=mode)


def qk_fwd_path(c):
    """-> (kernel, grid-stride passes of the busiest workgroup), as ldmae_qknorm_rope_fwd dispatches."""
    hd, items, T = c["hd"], c["B"] * c["N"] * c["H"], c["dtype"]
    cpi = hd // 4
    if c["mode"] == "norm" and hd > 64 and cpi & (cpi - 1) and c["N"] % 8 == 0:
        ipw = 256 // (hd // 8) if T == BF16 else 256 // cpi
        return ("dense8" if T == BF16 else "dense"), math.ceil(math.ceil(items / ipw) / 4096)
    if T == BF16 and c["mode"] != "plain" and not c["v"] and hd in (64, 128) and items % (256 // (hd // 8)) == 0:
        return "fwd8", math.ceil(items * (hd // 8) / 256 / 2048)
    lpr = 16 if hd <= 64 else 32
    return f"generic{lpr}", math.ceil(math.ceil(items * lpr / 256) / 2048)


QK_FWD = []
for _T in (F32, BF16):
    for _hd, _N in ((8, 10), (16, 10), (24, 10), (64, 10), (96, 12), (128, 10), (72, 12)):     # 16 lanes per item up to 64, then 32
        for _v in (True, False):
            QK_FWD.append(QF(f"generic_{_hd}_{_tn(_T)}{'' if _v else '_nov'}", _T, _hd, 2, _N, 3, _v))
    for _hd in (72, 88, 120):                                   # densely packed threads, H = 1 and 3, part of one workgroup (B N = 8)
        QK_FWD.append(QF(f"dense_{_hd}_{_tn(_T)}_H1", _T, _hd, 1, 8, 1, _hd != 88))
        QK_FWD.append(QF(f"dense_{_hd}_{_tn(_T)}_H3", _T, _hd, 2, 16, 3, _hd == 88))
    for _hd in (16, 72):
        QK_FWD.append(QF(f"ropeonly_{_hd}_{_tn(_T)}", _T, _hd, 2, 24, 3, _hd == 16, "rope"))
        QK_FWD.append(QF(f"plain_{_hd}_{_tn(_T)}", _T, _hd, 2, 24, 3, True, "plain"))
QK_FWD += [
    # fwd8 (bf16, v NULL): a pass is 2048 workgroups x 256 / (hd / 8) items = 65536 at hd 64, 32768 at hd 128
    QF("fwd8_64_tail_only", BF16, 64, 1, 32, 2, False),                 # 64 items: below the cap, the tail alone
    QF("fwd8_64_two_passes", BF16, 64, 64, 1024, 2, False),             # 131072 items: one trip of the two-in-flight loop, no tail
    QF("fwd8_64_three_passes", BF16, 64, 64, 1024, 3, False),           # 196608 items: one trip plus the tail (75 MB of qkv)
    QF("fwd8_64_two_and_a_half_passes", BF16, 64, 64, 1280, 2, False),  # 163840 items: half of the lane groups take the tail, half do not
    QF("fwd8_64_odd_items_generic", BF16, 64, 1, 11, 3, False),         # 33 items, not a multiple of 32: the generic kernel
    QF("fwd8_64_ropeonly", BF16, 64, 2, 16, 4, False, "rope"),
    QF("fwd8_128_tail_only", BF16, 128, 1, 16, 2, False),
    QF("fwd8_128_two_passes", BF16, 128, 32, 1024, 2, False),           # 65536 items
    QF("fwd8_128_three_passes", BF16, 128, 32, 1024, 3, False),         # 98304 items
    QF("fwd8_128_odd_items_generic", BF16, 128, 1, 5, 3, False),
    # generic kernel past its 2048-workgroup cap (16 items per workgroup at 16 lanes per item): second grid-stride pass
    QF("generic_16_f32_second_pass", F32, 16, 2, 1200, 16, True),       # 38400 items > 32768
    QF("generic_128_bf16_second_pass", BF16, 128, 2, 1100, 8, True),    # 17600 items > 16384 (8 items per workgroup)
    # dense kernels past the 4096-workgroup cap: 14 items per workgroup at hd 72 in f32 (57344 per pass), 28 in bf16 (114688)
    QF("dense_72_f32_second_pass", F32, 72, 8, 2400, 3, True),          # 57600 items
    QF("dense8_72_bf16_second_pass", BF16, 72, 8, 4784, 3, False),      # 114816 items
]


def _qk_common(c, g):
    B, N, H, hd, T = c["B"], c["N"], c["H"], c["hd"], c["dtype"]
    cos, sin = rc.tables(N, hd, g)
    w = 1 + 0.1 * torch.randn(2, hd, generator=g)
    Gc, Gs, Gw = Guard((N, hd), F32, cos.cuda()), Guard((N, hd), F32, sin.cuda()), Guard((2, hd), F32, w.cuda())
    return B, N, H, hd, T, Gc, Gs, Gw


@pytest.mark.parametrize("c", QK_FWD, ids=[c["name"] for c in QK_FWD])
def test_qknorm_rope_fwd(lib, c):
    g = _gen(c["name"])
    B, N, H, hd, T, Gc, Gs, Gw = _qk_common(c, g)
    norm, plain = c["mode"] == "norm", c["mode"] == "plain"
    qkv = Guard((B, N, 3, H, hd), T)                         # v == NULL: the v slot keeps the NaN payload and must not be read
    for s in range(3 if c["v"] else 2):
        qkv.t[:, :, s] = rc.hot(torch.randn(B, N, H, hd, generator=g), g, 1, 8.0).to(T).cuda()
    qkv.t[0, N // 2, :2, H - 1] = 0                          # all-zero q and k rows
    pw = (Gw.ptr(), Gw.ptr() + 4 * hd) if norm else (None, None)
    pt = (None, None) if plain else (Gc.ptr(), Gs.ptr())

    def run():
        outs = {n: Guard((B, H, N, hd), T) for n in (("q", "k", "v") if c["v"] else ("q", "k"))}
        lib.call("ldmae_qknorm_rope_fwd", _dt(T), qkv.ptr(), *pw, *pt, outs["q"].ptr(), outs["k"].ptr(), _p(outs.get("v")), B, N, H, hd, EPS, _stream())
        torch.cuda.synchronize()
        assert all(o.intact() for o in outs.values()) and qkv.intact() and Gc.intact() and Gs.intact() and Gw.intact(), "a canary changed"
        return {n: o.t.clone() for n, o in outs.items()}

    got = _twice(run)
    kern, passes = qk_fwd_path(c)
    path = f"qk_fwd[{kern},{_tn(T)},{hd},{c['mode']}{',multi-pass' if passes > 1 else ''}]"
    for s, n in enumerate(("q", "k")):
        x = qkv.t[:, :, s].permute(0, 2, 1, 3)
        if plain:
            assert torch.equal(_bits(got[n]), _bits(x)), f"{n}: the plain relayout is not bit exact"
        else:
            _chk(path, c["name"], n, got[n], *rc.qk_fwd_ref(x, Gw.t[s] if norm else None, Gc.t, Gs.t, EPS, T))
    if c["v"]:
        assert torch.equal(_bits(got["v"]), _bits(qkv.t[:, :, 2].permute(0, 2, 1, 3))), "v is not a bit-exact copy"


# ============================================================================= QK-norm + RoPE backward
def QB(name, dtype, hd, B, N, H, mode="norm", dbias=True, dv=True, bw=0):
    return dict(name=name, dtype=dtype, hd=hd, B=B, N=N, H=H, mode=mode, dbias=dbias, dv=dv, bw=bw)


def qk_bwd_grid(items, lpr, H):
    """-> (grid, m, g) of qk_bwd_grid."""
    wg = (items * lpr + 255) // 256
    g = min(max(wg, 1), 2048)
    m = H // math.gcd(H, 256 // lpr)
    return (g // m * m if g >= m else m), m, g


QK_BWD = [
    # 16 lanes per item (16 groups per workgroup)                          grid  (m, g)
    QB("bwd_8_f32_H1", F32, 8, 2, 10, 1),                                   # 2   (1, 2)
    QB("bwd_8_bf16_H3", BF16, 8, 2, 10, 3, dbias=False),                    # 3   (3, 4)
    QB("bwd_16_bf16_H5", BF16, 16, 2, 10, 5),                               # 5   (5, 7)
    QB("bwd_16_f32_H3_small", F32, 16, 1, 8, 3, bw=1),                      # 3   (3, 2): g < m
    QB("bwd_24_f32_H12", F32, 24, 2, 10, 12, dv=False),                     # 15  (3, 15)
    QB("bwd_24_bf16_H16", BF16, 24, 1, 10, 16, bw=1),                       # 10  (1, 10)
    QB("bwd_64_bf16_H12", BF16, 64, 2, 16, 12, dv=False),                   # 24  (3, 24)
    QB("bwd_64_f32_H5", F32, 64, 2, 10, 5, dbias=False, bw=1),              # 5   (5, 7)
    QB("bwd_64_bf16_H5_small", BF16, 64, 1, 8, 5),                          # 5   (5, 3): g < m
    # 32 lanes per item (8 groups per workgroup)
    QB("bwd_72_bf16_H16", BF16, 72, 2, 12, 16, dv=False),                   # 48  (2, 48)
    QB("bwd_72_f32_H3", F32, 72, 2, 12, 3),                                 # 9   (3, 9)
    QB("bwd_88_f32_H1", F32, 88, 2, 12, 1, dbias=False),                    # 3   (1, 3)
    QB("bwd_96_bf16_H12", BF16, 96, 1, 12, 12, bw=1),                       # 18  (3, 18)
    QB("bwd_120_bf16_H5", BF16, 120, 1, 8, 5),                              # 5   (5, 5)
    QB("bwd_128_f32_H5_small", F32, 128, 1, 4, 5, dv=False),                # 5   (5, 3): g < m
    QB("bwd_128_bf16_H3", BF16, 128, 2, 16, 3),                             # 12  (3, 12)
    # more than 32768 items at hd 16: the capped grid, a second pass, and grid >= 256 for the 32-row-lane reduce
    QB("bwd_16_bf16_capped", BF16, 16, 2, 1200, 16, dv=False),              # 2048 (1, 2048), 38400 items
    QB("bwd_16_f32_capped_H3", F32, 16, 4, 2800, 3, bw=1),                  # 2046 (3, 2048), 33600 items
    QB("bwd_128_bf16_reduce32", BF16, 128, 2, 128, 12, dbias=False),        # 384 (3, 384)
    # RoPE adjoint only and the plain relayout
    QB("bwd_16_bf16_ropeonly", BF16, 16, 2, 10, 3, "rope"),                 # 3   (3, 4)
    QB("bwd_72_f32_ropeonly_nodv", F32, 72, 2, 12, 3, "rope", dv=False),    # 9   (3, 9)
    QB("bwd_64_bf16_ropeonly_nodbias", BF16, 64, 2, 10, 12, "rope", dbias=False),   # 15 (3, 15)
    QB("bwd_16_f32_plain", F32, 16, 2, 10, 3, "plain"),                     # 3   (3, 4)
    QB("bwd_72_bf16_plain_nodbias", BF16, 72, 2, 12, 5, "plain", dbias=False),      # 15 (5, 15)
]


@pytest.mark.parametrize("c", QK_BWD, ids=[c["name"] for c in QK_BWD])
def test_qknorm_rope_bwd(lib, c):
    g = _gen(c["name"])
    B, N, H, hd, T, Gc, Gs, Gw = _qk_common(c, g)
    norm, plain = c["mode"] == "norm", c["mode"] == "plain"
    qkv = Guard((B, N, 3, H, hd), T)                         # the v slot is never read; RoPE only: neither are the pre-norm rows
    if norm:
        for s in range(2):
            qkv.t[:, :, s] = rc.hot(torch.randn(B, N, H, hd, generator=g), g, 1, 8.0).to(T).cuda()
    grads = [Guard((B, H, N, hd), T, torch.randn(B, H, N, hd, generator=g).to(T).cuda()) for _ in range(3)]
    Gdq, Gdk, Gdv = grads[0], grads[1], (grads[2] if c["dv"] else None)
    vslot = grads[2].t.permute(0, 2, 1, 3)                   # dv == NULL: already in the v slot of dqkv (pre-filled by the test)
    dw_old = torch.randn(2, hd, generator=g).cuda() if c["bw"] else None
    pw = (Gw.ptr(), Gw.ptr() + 4 * hd) if norm else (None, None)
    pt = (None, None) if plain else (Gc.ptr(), Gs.ptr())
    nws = lib.load().ldmae_qknorm_rope_bwd_workspace_bytes(B, N, H, hd)
    assert nws > 0 and nws % 4 == 0

    def run():
        ws = Guard((nws // 4,), F32) if (not plain or c["dbias"]) else None
        dqkv = Guard((B, N, 3, H, hd), T)
        if not c["dv"]:
            dqkv.t[:, :, 2] = vslot
        dw = Guard((2, hd), F32, dw_old) if norm else None
        db = Guard((H, 3, hd), F32) if c["dbias"] else None
        lib.call("ldmae_qknorm_rope_bwd", _dt(T), Gdq.ptr(), Gdk.ptr(), _p(Gdv), None if plain else qkv.ptr(), *pw, *pt, dqkv.ptr(),
                 dw.ptr() if norm else None, dw.ptr() + 4 * hd if norm else None, float(c["bw"]), _p(db), B, N, H, hd, EPS, _p(ws), _stream())
        torch.cuda.synchronize()
        assert dqkv.intact() and all(o is None or o.intact() for o in (ws, dw, db)) and all(x.intact() for x in grads), "a canary changed"
        r = dict(dqkv=dqkv.t.clone())
        if norm:
            r["dw"] = dw.t.clone()
        if db:
            r["dbias"] = db.t.clone()
        return r

    got = _twice(run)
    lpr = 16 if hd <= 64 else 32
    grid, m, g0 = qk_bwd_grid(B * N * H, lpr, H)
    path = f"qk_bwd[lpr{lpr},{_tn(T)},{hd},{c['mode']}{',capped' if g0 == 2048 else ''}{',reduce32' if grid >= 256 else ''}]"
    dqkv = got["dqkv"]
    assert torch.equal(_bits(dqkv[:, :, 2]), _bits(vslot)), "the v slot is not a bit-exact copy of dv"
    for s, (n, G) in enumerate((("dq", Gdq), ("dk", Gdk))):
        slot = dqkv[:, :, s].permute(0, 2, 1, 3)
        if plain:
            assert torch.equal(_bits(slot), _bits(G.t)), f"{n}: the plain relayout is not bit exact"
            continue
        x = qkv.t[:, :, s].permute(0, 2, 1, 3) if norm else None
        wi = Gw.t[s] if norm else None
        _chk(path, c["name"], n + "-slot", slot, *rc.qk_bwd_ref(G.t, x, wi, Gc.t, Gs.t, EPS, T))
        if norm:
            _chk(path, c["name"], "dw" + n[1], got["dw"][s], *rc.qk_dw_ref(G.t, x, wi, Gc.t, Gs.t, EPS, dw_old[s] if c["bw"] else None))
    if c["dbias"]:
        rows = dqkv.permute(0, 1, 3, 2, 4).reshape(B * N, 3 * H * hd)            # (head, q | k | v, d) order of dbias
        _record(path + ":dbias", rc.stored_colsum(c["name"] + " dbias", got["dbias"].reshape(-1), rows))


# ============================================================================= stand-alone RoPE
def RP(name, dtype, hd, rows, N, transposed):
    return dict(name=name, dtype=dtype, hd=hd, rows=rows, N=N, transposed=transposed)


ROPE = []
for _T in (F32, BF16):
    for _tr in (0, 1):
        ROPE.append(RP(f"rope_4_{_tn(_T)}_t{_tr}", _T, 4, 30, 10, _tr))
        ROPE.append(RP(f"rope_64_{_tn(_T)}_t{_tr}", _T, 64, 36, 12, _tr))
ROPE += [
    # rows above 8192 * 256 / (hd / 4): the stride loop runs twice
    RP("rope_64_bf16_two_passes", BF16, 64, 131072 + 1024, 1024, 0),
    RP("rope_64_f32_two_passes_t1", F32, 64, 131072 + 512, 512, 1),
    RP("rope_4_f32_two_passes", F32, 4, 2097152 + 4096, 4096, 0),
    RP("rope_4_bf16_two_passes_t1", BF16, 4, 2098000, 1000, 1),
]


def rope_passes(c):
    return math.ceil(math.ceil(c["rows"] * (c["hd"] // 4) / 256) / 8192)


@pytest.mark.parametrize("c", ROPE, ids=[c["name"] for c in ROPE])
def test_rope(lib, c):
    g = _gen(c["name"])
    T, hd, rows, N = c["dtype"], c["hd"], c["rows"], c["N"]
    cos, sin = rc.tables(N, hd, g)
    Gc, Gs = Guard((N, hd), F32, cos.cuda()), Guard((N, hd), F32, sin.cuda())
    Gt = Guard((rows, hd), T, torch.randn(rows, hd, generator=g).to(T).cuda())

    def run():
        out = Guard((rows, hd), T)
        lib.call("ldmae_rope", _dt(T), Gt.ptr(), Gc.ptr(), Gs.ptr(), out.ptr(), rows, N, hd, c["transposed"], _stream())
        torch.cuda.synchronize()
        assert out.intact() and Gt.intact() and Gc.intact() and Gs.intact(), "a canary changed"
        return dict(out=out.t.clone())

    got = _twice(run)
    ref, fn = rc.rope_ref(Gt.t.double().view(rows // N, N, hd), Gc.t, Gs.t, bool(c["transposed"]))
    path = f"rope[{_tn(T)},{hd},{'adjoint' if c['transposed'] else 'forward'}{',two-pass' if rope_passes(c) > 1 else ''}]"
    _chk(path, c["name"], "out", got["out"].view(rows // N, N, hd), ref, rc.stored(ref, fn, T))


# ----------------------------------------------------------------------------- refused dtype codes
def test_refused_dtype_codes(lib):
    """One dtype code per entry point that it has no kernel for -- 2 (f16), or 0 (f32) for the residual + norm pass, which takes the 16-bit
    types only: the call returns -1 with a message that names the entry, launches nothing and leaves every output with its NaN payload.
    Every buffer has the f32 size whatever the code claims, so a fall-through to the float kernel would stay in bounds and show up as a
    write, never as a fault."""
    L, st = lib.load(), _stream()
    M, D, rpb, B, N, H, hd = 16, 256, 16, 1, 8, 1, 64
    f = lambda *s: Guard(s, F32, torch.zeros(s).cuda())        # noqa: E731  finite input
    o = lambda *s: Guard(s, F32)                               # noqa: E731  NaN-filled output
    x, w, mod, g, rstd, y, gate = f(M, D), f(D), f(1, D), f(M, D), f(M), f(M, D), f(1, D)
    out, rs, xout, dx, dsh, dsc, dw, dy, dgate, dbias = o(M, D), o(M), o(M, D), o(M, D), o(1, D), o(1, D), o(D), o(M, D), o(1, D), o(D)
    need = max(L.ldmae_rmsnorm_modulate_bwd_gate_workspace_bytes(M, D, rpb), L.ldmae_gate_bwd_workspace_bytes(M, D, rpb),
               L.ldmae_qknorm_rope_bwd_workspace_bytes(B, N, H, hd))
    ws = o(need // 4)
    bwd = (g.ptr(), x.ptr(), w.ptr(), mod.ptr(), D, rstd.ptr(), dx.ptr(), 0.0, dsh.ptr(), dsc.ptr(), D, dw.ptr(), 0.0)
    lbwd = (g.ptr(), x.ptr(), mod.ptr(), D, rstd.ptr(), dx.ptr(), 0.0, dsh.ptr(), dsc.ptr(), D)
    gt = (y.ptr(), gate.ptr(), D, dy.ptr(), dgate.ptr(), D, dbias.ptr())
    tail = (M, D, rpb, ws.ptr(), st)
    qkv, wq, cs, gq = f(B, N, 3 * H * hd), f(hd), f(N, hd), f(B, H, N, hd)
    q, k, v, dqkv, dwq, dwk, dbq = o(B, H, N, hd), o(B, H, N, hd), o(B, H, N, hd), o(B, N, 3 * H * hd), o(hd), o(hd), o(3 * H * hd)
    R = {
        "rmsnorm_modulate_fwd": (lambda: L.ldmae_rmsnorm_modulate_fwd(2, x.ptr(), w.ptr(), mod.ptr(), mod.ptr(), D, out.ptr(), rs.ptr(), M, D, rpb, EPS, st), 2),
        "layernorm_modulate_fwd": (lambda: L.ldmae_layernorm_modulate_fwd(2, x.ptr(), mod.ptr(), mod.ptr(), D, out.ptr(), rs.ptr(), M, D, rpb, EPS, st), 2),
        "res_rmsnorm_modulate_fwd": (lambda: L.ldmae_res_rmsnorm_modulate_fwd(0, x.ptr(), y.ptr(), gate.ptr(), D, None, None, 0, xout.ptr(), w.ptr(), mod.ptr(),
                                                                             mod.ptr(), D, out.ptr(), rs.ptr(), M, D, rpb, EPS, st), 0),
        "rmsnorm_modulate_bwd": (lambda: L.ldmae_rmsnorm_modulate_bwd(2, *bwd, *tail), 2),
        "rmsnorm_modulate_bwd_gate": (lambda: L.ldmae_rmsnorm_modulate_bwd_gate(2, *bwd, *gt, *tail), 2),
        "rmsnorm_modulate_bwd_gate_recompute": (lambda: L.ldmae_rmsnorm_modulate_bwd_gate_recompute(2, *bwd, *gt, *tail), None),     # its message has no code
        "layernorm_modulate_bwd": (lambda: L.ldmae_layernorm_modulate_bwd(2, *lbwd, *tail), 2),
        "layernorm_modulate_bwd_gate": (lambda: L.ldmae_layernorm_modulate_bwd_gate(2, *lbwd, *gt, *tail), 2),
        "gate_bwd": (lambda: L.ldmae_gate_bwd(2, g.ptr(), *gt, *tail), 2),
        "qknorm_rope_fwd": (lambda: L.ldmae_qknorm_rope_fwd(2, qkv.ptr(), wq.ptr(), wq.ptr(), cs.ptr(), cs.ptr(), q.ptr(), k.ptr(), v.ptr(), B, N, H, hd, EPS, st), 2),
        "qknorm_rope_bwd": (lambda: L.ldmae_qknorm_rope_bwd(2, gq.ptr(), gq.ptr(), gq.ptr(), qkv.ptr(), wq.ptr(), wq.ptr(), cs.ptr(), cs.ptr(), dqkv.ptr(), dwq.ptr(),
                                                           dwk.ptr(), 0.0, dbq.ptr(), B, N, H, hd, EPS, ws.ptr(), st), 2),
        "rope": (lambda: L.ldmae_rope(2, gq.ptr(), cs.ptr(), cs.ptr(), q.ptr(), B * H * N, N, hd, 0, st), 2),
    }
    for name, (fn, code) in R.items():
        status = fn()
        msg = lib.last_error()
        assert status == -1 and msg.startswith(name + ":"), f"{name}: not refused as an invalid argument (status {status}: {msg!r})"
        assert code is None or f"dtype {code}" in msg, msg
    torch.cuda.synchronize()
    for q_ in (out, rs, xout, dx, dsh, dsc, dw, dy, dgate, dbias, ws, q, k, v, dqkv, dwq, dwk, dbq):
        assert q_.intact() and q_.untouched(q_.t), "a refused call wrote to a buffer"
    for q_ in (x, w, mod, g, rstd, y, gate, qkv, wq, cs, gq):
        assert q_.intact(), "a canary changed"


def test_case_names_are_unique():
    names = [c["name"] for t in (NORM_FWD, NORM_BWD, GATE_BWD, QK_FWD, QK_BWD, ROPE) for c in t]
    assert len(names) == len(set(names))
