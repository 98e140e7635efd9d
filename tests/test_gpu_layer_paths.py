"""Every dispatch path of the VMAE layer kernels (csrc/vmae.hip) and of csrc/pointwise.hip (colsum, casts, thin GEMMs,
activations, multi_add, embedders, AdamW / EMA), element by element, with the bounds of tests/layer_check.py.

Seeded case tables drive the C ABI directly, so each case controls pointers, leading dimensions, NULLs, alignment and workspace sizes.  Each case
  - places every input in a NaN-padded buffer and every output in a buffer pre-filled with the NaN payload of its type (accumulating outputs:
    dx_accum, dtable, beta = 1 targets, multi_add destinations, the AdamW state get finite seeded contents): an unwritten element, a write
    outside the tensor and a read of a buffer the entry point says it does not read all fail;
  - gives workspaces exactly the size the *_workspace_bytes function reports (ldmae_mae_loss_groups rows for the loss partials), inside a
    canary;
  - checks every element of every output against the f64 reference with the per-element bound (zero excluded elements) -- or for equality of
    bits where layer_check.py says "bit exact" --, asserts that reference and bound are finite, and checks every canary;
  - runs a second time on fresh outputs and requires bitwise-equal results;
  - records the worst err / bound per path and output (printed at module teardown).
The LayerNorm backward is fed mean / rstd made by the f64 reference (rounded to f32), never the forward kernel's output.

Dispatch predicates (host code), each taken and not taken by some case (tests/test_layer_check_cpu.py::
test_case_table_covers_every_predicate, computed from the tables alone):
  layernorm_fwd: NV class of D (3, 6, 12, 16, 20; lowest and highest D of each, full and partly filled last chunk); out f32 / bf16 / f16;
    mean, rstd NULL; M = 1, M % 16 != 0; the 4096-workgroup cap and its second pass; rows with a large common offset.
  layernorm_bwd / _cast: NV class; T; M < 128, M % 128 != 0, M % 16 != 0; G = ceil(M / 128) below / above 64, not a multiple of 64; beta_w;
    dx_cast; the 160-KiB launch of D = 1280.
  colsum: dtype; nsub > 1 (ncol4 dividing 256 or not); a one-float4 last column block; ldx > N; every rung of colsum_rows; G = 1, < 256,
    >= 256; beta.
  restore_tokens / _bwd: NV class (3, 6, 8), full and partial; keep = 1, keep = L; dmask_token NULL with a NULL workspace; the 2048 cap.
  thin_nt: K, out type, pos, bias NULL, M below / at / above 128, rows_per_batch not dividing 128, a second column block.
  thin_tn: K, chunks 1, > 1, > 64, a second column block, dbias NULL, beta.
  conv3x3 / _bwd: the rgb kernel or the generic one for each reason (C, W % 4, input / output offset by 4 B); b NULL; dx NULL; the
    CONV_BWD_G cap.
  mae_loss: p, H != W, C, all-masked / all-visible, the 2048-workgroup cap.
  cast / cast_stack / cast_weight / multi_add / label_embed / adamw_ema / ema_only / random_masking / gather / scatter / patch_gather /
    latent_prologue: the shapes, NULLs and caps listed with each table below.

  gelu / gelu_tanh / swiglu / silu: every dtype the entry point takes; n = 1, n % 256 != 0, one case past the 8192-workgroup cap; arguments
    with 0, +-0, +-1e-30 and |x| up to 12 (GELU) or 90 (SwiGLU, SiLU), where the exponentials overflow and the formulas must return the limit.
  timestep_embedding: dim 2, 3, 256, 257; t in {0, 0.25, 1, 1000}; two values of max_period; B * half not a multiple of 256.
  latent_prologue with sample = 1: logvar below -30, above 20 and at both clamp points.
  refused arguments: besides the shape / alignment / workspace refusals, one dtype code per dtype-taking entry point that it has no kernel
    for (dtype_dispatch, csrc/common.h), on buffers of the f32 size: refused with -1, nothing launched, nothing written.
The error constants of the device math functions are measured with csrc/probe/intrinsic_probe and listed in layer_check.py.

Fixed with this suite: random_masking_kernel ordered -0.0 before +0.0 where the stable argsort it restates treats them as equal (found by
case masking "signed_zero"): both now map to one key; and erf_act<bf16 / f16> (csrc/common.h) used an erf whose f32 evaluation is
3.6 times less accurate than documented (found by case gelu_float16_n2097229, below): it now calls erff.

First device run (MI355X): 269 parametrised cases plus the 24 refused calls; the module takes about 4 s (3.9 s; the slowest case 0.8 s, the
first one, which loads the library).  All cases inside their bounds with zero excluded elements, every rerun bitwise equal, no canary touched, every refused call left its
buffers intact -- after one more fix the first run asked for:
  test_gelu[gelu_float16_n2097229], dx, missed its bound in 1 of 2097229 elements (x = -0.03029, g = 0.26147: got 0.12438965, ref 0.12442021,
  |diff| 3.05619e-05 against 3.05611e-05 = half an f16 ulp plus 4.35e-08 of f32 error, of which 1.96e-08 is 0.5 |g| x the 1.5e-7 allowed
  for erf).  Cause: erf_as, which served the 16-bit types, measures 9.0 u = 5.4e-7 absolute near x = -0.05 (csrc/probe/intrinsic_probe),
  not the 1.5e-7 its comment stated -- that is the error of the Abramowitz-Stegun formula in exact arithmetic.  Fixed in csrc/common.h:
  erf_act calls erff (1.4 u measured) for every type; the bound keeps the 1.5e-7.  Run again with it: 269 passed, the module in 3.0 s.
Worst err / bound per family and output:
  16-bit outputs (ln y, dx_cast, thin_nt, gelu, gelu_tanh, swiglu, silu y)   0.99 .. 1.00   (the half ulp of the store is all but the whole bound)
  ln_fwd, f32:    y 0.12 .. 0.32, mean 0.004 .. 0.21, rstd 0.02 .. 0.20        ln_bwd: dx 0.08 .. 0.34, dw <= 0.10, db <= 0.06
  colsum <= 0.06, restore dmask <= 0.04, thin_nt f32 0.08 .. 0.26, thin_tn dW <= 0.17, dbias <= 0.14, label dtable 0.12 .. 0.47
  conv3x3 out 0.08 .. 0.15, dx 0.07 .. 0.18, dw <= 0.07, db <= 0.02; mae_loss sums <= 0.04, dpred 0.41 .. 0.43
  gelu f32 y 0.43 .. 0.53, dx 0.46 .. 0.58; gelu_tanh f32 y 0.48 .. 0.69, dx 0.41 .. 0.62; swiglu f32 0.54; silu f32 y 0.79 .. 0.96, dx 0.40 .. 0.63
  timestep 0.22; latent_prologue 0.77 .. 0.91; adamw p <= 0.50, m <= 0.995, v <= 0.88, ema 0.50; ema_only 0.87 .. 0.99
  f32 ratios above 0.9 (adamw m, ema_only, silu y, latent_prologue): each is a chain of two or three roundings and nothing else, so the
  bound IS those roundings, and among millions of elements some take all of them in the same direction; no rule can be tightened there.
"""
import ctypes

import pytest
import torch

import layer_check as lc
from test_gpu_attention_paths import Guard, _bits

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
I64 = torch.int64
EPS = 1e-6
RATIOS: dict = {}
NCASES = [0]
DT = {F32: 0, BF16: 1, F16: 2}
TYPES = (F32, BF16, F16)


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


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _record(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)


def _tn(dtype):
    return str(dtype)[6:]


def _gen(name):
    return torch.Generator().manual_seed(7000 + sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003)


def _p(g):
    return None if g is None else g.ptr()


def _ids(cases):
    return [c["name"] for c in cases]


def _twice(run):
    """run() -> dict name -> tensor (clones of fresh guarded outputs); twice, bitwise equal."""
    a = run()
    b = run()
    for n in a:
        assert torch.equal(_bits(a[n]) if a[n].is_floating_point() else a[n], _bits(b[n]) if b[n].is_floating_point() else b[n]), \
            f"{n}: rerun not bitwise equal"
    return a


def _chk(path, name, out, got, ref, bound):
    ref, bound = ref.to(got.device), bound.to(got.device)
    assert lc.finite(ref, bound), f"{name} {out}: reference or bound not finite"
    _record(f"{path}:{out}", lc.check(f"{name} {out}", got, ref, bound))


def _same(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, f"{name}: shape / dtype"
    eq = _bits(got) == _bits(want) if got.is_floating_point() else got == want
    assert bool(eq.all()), f"{name}: {int((~eq).sum())} of {eq.numel()} elements differ in their bits"


def _ws(nbytes):
    """A workspace of exactly `nbytes` inside a canary."""
    assert nbytes > 0 and nbytes % 4 == 0
    return Guard((nbytes // 4,), F32)


class IGuard:
    """Guard for int64 outputs: the tensor sits between sentinel runs and is pre-filled with the sentinel."""
    S = -0x0DEAD0DEAD0DEAD

    def __init__(self, shape, front=32, back=256):
        n = 1
        for s in shape:
            n *= s
        self.n, self.front = n, front
        self.buf = torch.full((front + n + back,), self.S, dtype=I64, device="cuda")
        self.t = self.buf[front:front + n].view(shape)

    def intact(self):
        return bool((self.buf[:self.front] == self.S).all() and (self.buf[self.front + self.n:] == self.S).all())

    def ptr(self):
        return self.t.data_ptr()


class Off:
    """A tensor that starts `off` elements into a Guard (a pointer that is not 16-B aligned); the skipped elements keep the payload."""

    def __init__(self, shape, dtype, init=None, off=0):
        n = 1
        for s in shape:
            n *= s
        self.g, self.off = Guard((n + off,), dtype), off
        self.t = self.g.t[off:].view(shape)
        if init is not None:
            self.t.copy_(init)

    def intact(self):
        return self.g.intact() and self.g.untouched(self.g.t[:self.off])

    def ptr(self):
        return self.t.data_ptr()


def _payload_like(n, dtype):
    """A NaN buffer to pass where the entry point says an argument is unused."""
    return Guard((n,), dtype)


# ============================================================================= LayerNorm
LN_D = (4, 192, 196, 384, 388, 768, 772, 1024, 1028, 1280)


def ln_nv_class(D):
    n = (D + 63) // 64
    return 3 if n <= 3 else 6 if n <= 6 else 12 if n <= 12 else 16 if n <= 16 else 20


def ln_partial_chunk(D):
    return D % 64 != 0


def ln_fwd_capped(M):
    return (M + 15) // 16 > 4096


def LF(name, M, D, T, mean=True, rstd=True, fam="unit"):
    return dict(name=name, M=M, D=D, T=T, mean=mean, rstd=rstd, fam=fam)


LN_FWD = []
for _i, _D in enumerate(LN_D):
    for _T in TYPES:
        LN_FWD.append(LF(f"D{_D}_{_tn(_T)}", (18, 37, 5)[_i % 3], _D, _T, fam="offset" if _D in (192, 1028) and _T == F32 else "unit"))
LN_FWD += [
    LF("M1_D4_f32", 1, 4, F32), LF("M1_D1280_bf16", 1, 1280, BF16),
    LF("null_mean_D196_f32", 18, 196, F32, mean=False), LF("null_rstd_D772_bf16", 18, 772, BF16, rstd=False),
    LF("null_both_D388_f16", 18, 388, F16, mean=False, rstd=False),
    LF("offset_D1280_f32", 18, 1280, F32, fam="offset"), LF("offset_D4_f32", 18, 4, F32, fam="offset"),
    LF("cap_D4_f32", 65536 + 21, 4, F32), LF("cap_D4_bf16", 65536 + 21, 4, BF16),
]


def _ln_x(M, D, fam, g):
    x = torch.randn(M, D, generator=g)
    return 100.0 + x if fam == "offset" else x


@pytest.mark.parametrize("c", LN_FWD, ids=_ids(LN_FWD))
def test_layernorm_fwd(lib, c):
    M, D, T, g = c["M"], c["D"], c["T"], _gen("lnf" + c["name"])
    Gx = Guard((M, D), F32, _ln_x(M, D, c["fam"], g).cuda())
    Gw, Gb = Guard((D,), F32, (1 + 0.3 * torch.randn(D, generator=g)).cuda()), Guard((D,), F32, (0.3 * torch.randn(D, generator=g)).cuda())

    def run():
        out = Guard((M, D), T)
        mean, rstd = (Guard((M,), F32) if c["mean"] else None), (Guard((M,), F32) if c["rstd"] else None)
        lib.call("ldmae_layernorm_fwd", DT[T], Gx.ptr(), Gw.ptr(), Gb.ptr(), out.ptr(), _p(mean), _p(rstd), M, D, EPS, _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (out, mean, rstd, Gx, Gw, Gb) if q is not None), "a canary changed"
        r = dict(y=out.t.clone())
        if mean is not None:
            r["mean"] = mean.t.clone()
        if rstd is not None:
            r["rstd"] = rstd.t.clone()
        return r

    got = _twice(run)
    ref = lc.ln_fwd_ref(Gx.t, Gw.t, Gb.t, EPS, T)
    path = f"ln_fwd[{_tn(T)},NV{ln_nv_class(D)}]"
    for k in got:
        _chk(path, c["name"], k, got[k], *ref[k])
    NCASES[0] += 1


def LB(name, M, D, T, beta_w=0.0, cast=False, fam="unit"):
    return dict(name=name, M=M, D=D, T=T, beta_w=beta_w, cast=cast, fam=fam)


LN_BWD = []
for _i, _D in enumerate(LN_D):
    for _j, _T in enumerate(TYPES):
        LN_BWD.append(LB(f"D{_D}_{_tn(_T)}", (130, 37, 5)[(_i + _j) % 3], _D, _T, beta_w=float((_i + _j) % 2), cast=_T != F32 and _i % 2 == 0))
LN_BWD += [
    LB("G71_D4_f32", 128 * 70 + 5, 4, F32, beta_w=1.0), LB("G71_D4_bf16_cast", 128 * 70 + 5, 4, BF16, cast=True),
    LB("M256_D192_f16_cast", 256, 192, F16, beta_w=1.0, cast=True), LB("offset_D1280_f32", 130, 1280, F32, fam="offset"),
    LB("M1_D1280_bf16_cast", 1, 1280, BF16, cast=True),
]


def ln_bwd_groups(M):
    return (M + 127) // 128


@pytest.mark.parametrize("c", LN_BWD, ids=_ids(LN_BWD))
def test_layernorm_bwd(lib, c):
    M, D, T, beta, g = c["M"], c["D"], c["T"], c["beta_w"], _gen("lnb" + c["name"])
    x = _ln_x(M, D, c["fam"], g)
    xd = x.double()
    mean = xd.mean(-1)
    rstd = (((xd - mean[:, None]) ** 2).mean(-1) + EPS).rsqrt()
    Gx, Gg = Guard((M, D), F32, x.cuda()), Guard((M, D), T, torch.randn(M, D, generator=g).cuda())
    Gw = Guard((D,), F32, (1 + 0.3 * torch.randn(D, generator=g)).cuda())
    Gm, Gr = Guard((M,), F32, mean.float().cuda()), Guard((M,), F32, rstd.float().cuda())
    dx0, dw0, db0 = torch.randn(M, D, generator=g).cuda(), torch.randn(D, generator=g).cuda(), torch.randn(D, generator=g).cuda()
    nbytes = lib.load().ldmae_layernorm_bwd_workspace_bytes(M, D)

    def run():
        dx = Guard((M, D), F32, dx0)
        dxc = Guard((M, D), T) if c["cast"] else None
        dw, db = (Guard((D,), F32, dw0), Guard((D,), F32, db0)) if beta else (Guard((D,), F32), Guard((D,), F32))
        ws = _ws(nbytes)
        if c["cast"]:
            lib.call("ldmae_layernorm_bwd_cast", DT[T], Gg.ptr(), Gx.ptr(), Gw.ptr(), Gm.ptr(), Gr.ptr(), dx.ptr(), dxc.ptr(), dw.ptr(), db.ptr(),
                     beta, M, D, ws.ptr(), _stream())
        else:
            lib.call("ldmae_layernorm_bwd", DT[T], Gg.ptr(), Gx.ptr(), Gw.ptr(), Gm.ptr(), Gr.ptr(), dx.ptr(), dw.ptr(), db.ptr(), beta, M, D,
                     ws.ptr(), _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (dx, dxc, dw, db, ws, Gx, Gg, Gw, Gm, Gr) if q is not None), "a canary changed"
        r = dict(dx=dx.t.clone(), dw=dw.t.clone(), db=db.t.clone())
        if dxc is not None:
            r["dx_cast"] = dxc.t.clone()
        return r

    got = _twice(run)
    ref = lc.ln_bwd_ref(Gg.t, Gx.t, Gw.t, Gm.t, Gr.t, dx0, dw0, db0, beta)
    path = f"ln_bwd[{_tn(T)},NV{ln_nv_class(D)}]"
    for k in got:
        _chk(path, c["name"], k, got[k], *ref[k])
    NCASES[0] += 1


# ============================================================================= colsum
colsum_rows = lc.colsum_rows


def colsum_groups(M, N):
    return -(-M // colsum_rows(M, N))


def colsum_last_ncol4(N):
    return N // 4 - (((N + 1023) // 1024) - 1) * 256


def CS(name, M, N, T, gap=0, beta=0.0):
    return dict(name=name, M=M, N=N, T=T, gap=gap, beta=beta)


COLSUM = [
    CS("r8_G1_N4_f32", 5, 4, F32), CS("r8_N12_bf16_gap", 300, 12, BF16, gap=4), CS("r8_G257_N200_f16", 2053, 200, F16, beta=1.0),
    CS("r16_N4_f32_gap", 4100, 4, F32, gap=8, beta=1.0), CS("r32_N12_f32", 8200, 12, F32), CS("r64_N4_bf16", 16390, 4, BF16),
    CS("r128_N4_f16_gap", 32800, 4, F16, gap=4), CS("r256_N4_f32", 65540, 4, F32, beta=1.0),
    CS("N1024_f32", 37, 1024, F32), CS("N1028_bf16", 37, 1028, BF16, beta=1.0), CS("N1028_f32_gap", 300, 1028, F32, gap=12),
    CS("N2304_f16_gap", 37, 2304, F16, gap=4), CS("N2304_f32", 1400, 2304, F32, beta=1.0), CS("N200_f32_gap", 37, 200, F32, gap=56),
]


@pytest.mark.parametrize("c", COLSUM, ids=_ids(COLSUM))
def test_colsum(lib, c):
    M, N, T, beta, g = c["M"], c["N"], c["T"], c["beta"], _gen("cs" + c["name"])
    ldx = N + c["gap"]
    GX = Guard((M, ldx), T)                                   # the gap columns keep the NaN payload: they must not be read
    GX.t[:, :N] = torch.randn(M, N, generator=g).cuda()
    old = torch.randn(N, generator=g).cuda()
    nbytes = lib.load().ldmae_colsum_workspace_bytes(M, N)
    assert nbytes == colsum_groups(M, N) * N * 4

    def run():
        out, ws = (Guard((N,), F32, old) if beta else Guard((N,), F32)), _ws(nbytes)
        lib.call("ldmae_colsum", DT[T], GX.ptr(), ldx, M, N, out.ptr(), beta, ws.ptr(), _stream())
        torch.cuda.synchronize()
        assert out.intact() and ws.intact() and GX.intact(), "a canary changed"
        return dict(out=out.t.clone())

    got = _twice(run)
    ref, bound = lc.colsum_ref(GX.t[:, :N], old if beta else None)
    _chk(f"colsum[{_tn(T)},rows{colsum_rows(M, N)}]", c["name"], "out", got["out"], ref, bound)
    NCASES[0] += 1


# ============================================================================= restore_tokens
def rt_nv_class(D):
    n = (D + 63) // 64
    return 3 if n <= 3 else 6 if n <= 6 else 8


def rt_capped(B, L):
    return (B * L + 15) // 16 > 2048


def RT(name, B, L, keep, D, dmask=True):
    return dict(name=name, B=B, L=L, keep=keep, D=D, dmask=dmask)


RESTORE = [RT(f"D{_D}", 2, 21, 6, _D, dmask=_D != 196) for _D in (4, 68, 192, 196, 384, 388, 512)] + [
    RT("keep1_D68", 3, 17, 1, 68), RT("keepL_D192", 2, 19, 19, 192), RT("keepL_D4_null", 2, 5, 5, 4, dmask=False),
    RT("cap_D4", 3, 10929, 2732, 4), RT("cap_D4_null", 3, 10929, 2732, 4, dmask=False),
]


def _perm_ids(B, L, g):
    return torch.stack([torch.randperm(L, generator=g) for _ in range(B)]).cuda()


@pytest.mark.parametrize("c", RESTORE, ids=_ids(RESTORE))
def test_restore_tokens(lib, c):
    B, L, keep, D, g = c["B"], c["L"], c["keep"], c["D"], _gen("rt" + c["name"])
    ids = _perm_ids(B, L, g)
    Gx, Gm, Gp = Guard((B, keep, D), F32, torch.randn(B, keep, D, generator=g).cuda()), Guard((D,), F32, torch.randn(D, generator=g).cuda()), \
        Guard((L, D), F32, torch.randn(L, D, generator=g).cuda())
    Gd = Guard((B, L, D), F32, torch.randn(B, L, D, generator=g).cuda())
    nbytes = lib.load().ldmae_restore_tokens_bwd_workspace_bytes(B, L, D)

    def run():
        out, dx = Guard((B, L, D), F32), Guard((B, keep, D), F32)
        dm, ws = (Guard((D,), F32), _ws(nbytes)) if c["dmask"] else (None, None)
        lib.call("ldmae_restore_tokens", Gx.ptr(), Gm.ptr(), Gp.ptr(), ids.data_ptr(), out.ptr(), B, L, keep, D, _stream())
        lib.call("ldmae_restore_tokens_bwd", Gd.ptr(), ids.data_ptr(), dx.ptr(), _p(dm), B, L, keep, D, _p(ws), _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (out, dx, dm, ws, Gx, Gm, Gp, Gd) if q is not None), "a canary changed"
        r = dict(out=out.t.clone(), dx=dx.t.clone())
        if dm is not None:
            r["dmask"] = dm.t.clone()
        return r

    got = _twice(run)
    _same(c["name"] + " out", got["out"], lc.restore_ref(Gx.t, Gm.t, Gp.t, ids, keep))
    dx, (rm, bm) = lc.restore_bwd_ref(Gd.t, ids, keep)
    _same(c["name"] + " dx", got["dx"], dx)
    if c["dmask"]:
        _chk(f"restore_bwd[NV{rt_nv_class(D)}]", c["name"], "dmask", got["dmask"], rm, bm)
        if keep == L:
            assert not bool(got["dmask"].any()), "keep = L: the mask-token gradient is exactly zero"
    NCASES[0] += 1


# ============================================================================= thin GEMMs
def NT(name, M, N, K, T, pos=True, bias=True, rpb=52):
    return dict(name=name, M=M, N=N, K=K, T=T, pos=pos, bias=bias, rpb=rpb)


THIN_NT = [
    NT("M5_N4_K16_f32", 5, 4, 16, F32, rpb=3), NT("M128_N772_K32_bf16", 128, 772, 32, BF16), NT("M392_N1028_K16_f32", 392, 1028, 16, F32),
    NT("M392_N4_K32_f32_nopos", 392, 4, 32, F32, pos=False), NT("M128_N1028_K32_bf16_nobias", 128, 1028, 32, BF16, bias=False),
    NT("M5_N772_K16_bf16_nopos_nobias", 5, 772, 16, BF16, pos=False, bias=False), NT("M392_N772_K16_bf16_rpb196", 392, 772, 16, BF16, rpb=196),
    NT("M130_N260_K32_f32_nobias", 130, 260, 32, F32, bias=False, rpb=65), NT("M128_N4_K32_bf16_nopos", 128, 4, 32, BF16, pos=False),
    NT("M5_N1028_K16_f32_nopos", 5, 1028, 16, F32, pos=False),
]


@pytest.mark.parametrize("c", THIN_NT, ids=_ids(THIN_NT))
def test_thin_nt(lib, c):
    M, N, K, T, rpb, g = c["M"], c["N"], c["K"], c["T"], c["rpb"], _gen("nt" + c["name"])
    Gt, Gw = Guard((M, K), F32, torch.randn(M, K, generator=g).cuda()), Guard((N, K), F32, torch.randn(N, K, generator=g).cuda())
    Gb = Guard((N,), F32, torch.randn(N, generator=g).cuda()) if c["bias"] else None
    Gp = Guard((rpb, N), F32, torch.randn(rpb, N, generator=g).cuda()) if c["pos"] else None

    def run():
        out = Guard((M, N), T)
        lib.call("ldmae_thin_nt", DT[T], Gt.ptr(), Gw.ptr(), _p(Gb), _p(Gp), out.ptr(), M, N, K, rpb if c["pos"] else 0, _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (out, Gt, Gw, Gb, Gp) if q is not None), "a canary changed"
        return dict(out=out.t.clone())

    got = _twice(run)
    ref, bound = lc.thin_nt_ref(Gt.t, Gw.t, Gb.t if Gb else None, Gp.t if Gp else None, rpb, T)
    _chk(f"thin_nt[K{K},{_tn(T)},{'pos' if c['pos'] else 'nopos'}]", c["name"], "out", got["out"], ref, bound)
    NCASES[0] += 1


def TT(name, M, N, K, dbias=True, beta=0.0):
    return dict(name=name, M=M, N=N, K=K, dbias=dbias, beta=beta)


THIN_TN = [
    TT("M5_N4_K16", 5, 4, 16), TT("M512_N260_K32", 512, 260, 32, beta=1.0), TT("M1032_N772_K16", 1032, 772, 16),
    TT("M33283_N4_K32", 512 * 65 + 3, 4, 32, beta=1.0), TT("M33283_N4_K16_nodb", 512 * 65 + 3, 4, 16, dbias=False),
    TT("M1032_N260_K32_nodb", 1032, 260, 32, dbias=False, beta=1.0), TT("M5_N772_K32", 5, 772, 32),
]


def thin_chunks(M):
    return (M + 511) // 512


@pytest.mark.parametrize("c", THIN_TN, ids=_ids(THIN_TN))
def test_thin_tn(lib, c):
    M, N, K, beta, g = c["M"], c["N"], c["K"], c["beta"], _gen("tn" + c["name"])
    Gg, Gt = Guard((M, N), F32, torch.randn(M, N, generator=g).cuda()), Guard((M, K), F32, torch.randn(M, K, generator=g).cuda())
    w0, b0 = torch.randn(N, K, generator=g).cuda(), torch.randn(N, generator=g).cuda()
    nbytes = lib.load().ldmae_thin_tn_workspace_bytes(M, N, K)
    assert nbytes == thin_chunks(M) * (N * K + N) * 4

    def run():
        dW = Guard((N, K), F32, w0) if beta else Guard((N, K), F32)
        db = (Guard((N,), F32, b0) if beta else Guard((N,), F32)) if c["dbias"] else None
        ws = _ws(nbytes)
        lib.call("ldmae_thin_tn", Gg.ptr(), Gt.ptr(), dW.ptr(), _p(db), M, N, K, beta, ws.ptr(), nbytes, _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (dW, db, ws, Gg, Gt) if q is not None), "a canary changed"
        if not c["dbias"]:                                   # the bias partials' part of the workspace must stay unwritten
            assert ws.untouched(ws.t[thin_chunks(M) * N * K:]), "dbias == NULL: the workspace tail was written"
        r = dict(dW=dW.t.clone())
        if db is not None:
            r["dbias"] = db.t.clone()
        return r

    got = _twice(run)
    (rw, bw), (rb, bb) = lc.thin_tn_ref(Gg.t, Gt.t, w0 if beta else None, b0 if beta else None)
    path = f"thin_tn[K{K},chunks{'>64' if thin_chunks(M) > 64 else thin_chunks(M)}]"
    _chk(path, c["name"], "dW", got["dW"], rw, bw)
    if c["dbias"]:
        _chk(path, c["name"], "dbias", got["dbias"], rb, bb)
    NCASES[0] += 1


# ============================================================================= conv3x3
def conv_rgb(C, W, off_a, off_b):
    """conv_rgb_shape: C == 3, W % 4 == 0, both pointers 16-B aligned (offsets in floats from an aligned base)."""
    return C == 3 and W % 4 == 0 and off_a % 4 == 0 and off_b % 4 == 0


def CV(name, B, C, H, W, xoff=0, ooff=0, bias=True, dx=True):
    return dict(name=name, B=B, C=C, H=H, W=W, xoff=xoff, ooff=ooff, bias=bias, dx=dx)


CONV_FWD = [
    CV("rgb_W4", 2, 3, 5, 4), CV("rgb_W8", 1, 3, 6, 8), CV("rgb_H1", 2, 3, 1, 8), CV("rgb_W8_nobias", 2, 3, 3, 8, bias=False),
    CV("gen_C1", 2, 1, 5, 8), CV("gen_C2", 1, 2, 5, 8), CV("gen_C4", 1, 4, 5, 8), CV("gen_W10", 2, 3, 5, 10),
    CV("gen_xoff", 1, 3, 5, 8, xoff=1), CV("gen_ooff", 1, 3, 5, 8, ooff=1), CV("gen_W10_nobias", 1, 3, 4, 10, bias=False),
]
CONV_BWD = [
    CV("rgb_W4", 2, 3, 5, 4), CV("rgb_W8", 1, 3, 6, 8), CV("rgb_H1", 2, 3, 1, 8), CV("gen_W10", 2, 3, 5, 10),
    CV("gen_xoff", 1, 3, 5, 8, xoff=1), CV("gen_ooff", 1, 3, 5, 8, ooff=1), CV("nodx_W8", 2, 3, 5, 8, dx=False),
    CV("cap_W223", 3, 3, 393, 223), CV("cap_nodx", 3, 3, 393, 223, dx=False),
]


def conv_bwd_capped(B, H, W):
    return (B * H * W + 255) // 256 > 1024


@pytest.mark.parametrize("c", CONV_FWD, ids=_ids(CONV_FWD))
def test_conv3x3_fwd(lib, c):
    B, C, H, W, g = c["B"], c["C"], c["H"], c["W"], _gen("cf" + c["name"])
    Gx = Off((B, C, H, W), F32, torch.randn(B, C, H, W, generator=g).cuda(), c["xoff"])
    Gw = Guard((C, C, 3, 3), F32, torch.randn(C, C, 3, 3, generator=g).cuda())
    Gb = Guard((C,), F32, torch.randn(C, generator=g).cuda()) if c["bias"] else None

    def run():
        out = Off((B, C, H, W), F32, None, c["ooff"])
        lib.call("ldmae_conv3x3", Gx.ptr(), Gw.ptr(), _p(Gb), out.ptr(), B, C, H, W, _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (out, Gx, Gw, Gb) if q is not None), "a canary changed"
        return dict(out=out.t.clone())

    got = _twice(run)
    ref, bound = lc.conv_ref(Gx.t, Gw.t, Gb.t if Gb else None)
    _chk(f"conv3x3[{'rgb' if conv_rgb(C, W, c['xoff'], c['ooff']) else 'generic'}]", c["name"], "out", got["out"], ref, bound)
    NCASES[0] += 1


@pytest.mark.parametrize("c", CONV_BWD, ids=_ids(CONV_BWD))
def test_conv3x3_bwd(lib, c):
    B, C, H, W, g = c["B"], c["C"], c["H"], c["W"], _gen("cb" + c["name"])
    Gg = Off((B, C, H, W), F32, torch.randn(B, C, H, W, generator=g).cuda(), c["xoff"])
    Gx = Guard((B, C, H, W), F32, torch.randn(B, C, H, W, generator=g).cuda())
    Gw = Guard((C, C, 3, 3), F32, torch.randn(C, C, 3, 3, generator=g).cuda())
    nbytes = lib.load().ldmae_conv3x3_bwd_workspace_bytes(C)

    def run():
        dx = Off((B, C, H, W), F32, None, c["ooff"]) if c["dx"] else None
        dw, db, ws = Guard((C, C, 3, 3), F32), Guard((C,), F32), _ws(nbytes)
        lib.call("ldmae_conv3x3_bwd", Gg.ptr(), Gx.ptr(), Gw.ptr(), _p(dx), dw.ptr(), db.ptr(), B, C, H, W, ws.ptr(), _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (dx, dw, db, ws, Gg, Gx, Gw) if q is not None), "a canary changed"
        r = dict(dw=dw.t.clone(), db=db.t.clone())
        if dx is not None:
            r["dx"] = dx.t.clone()
        return r

    got = _twice(run)
    ref = lc.conv_bwd_ref(Gg.t, Gx.t, Gw.t, c["dx"])
    path = f"conv3x3_bwd[{'rgb' if conv_rgb(C, W, c['xoff'], c['ooff']) else 'generic'}{',cap' if conv_bwd_capped(B, H, W) else ''}]"
    for k in got:
        _chk(path, c["name"], k, got[k], *ref[k])
    NCASES[0] += 1


# ============================================================================= MAE loss
def ML(name, B, C, H, W, p, mask="rand"):
    return dict(name=name, B=B, C=C, H=H, W=W, p=p, mask=mask)


MAE_LOSS = [
    ML("p4_16x48_C3", 2, 3, 16, 48, 4), ML("p8_16x16_C1", 1, 1, 16, 16, 8), ML("p16_32x16_C3_all1", 1, 3, 32, 16, 16, "all1"),
    ML("p4_8x24_C1_all0", 2, 1, 8, 24, 4, "all0"), ML("p8_48x16_C3", 2, 3, 48, 16, 8), ML("cap_p16_512", 3, 3, 512, 512, 16),
]


def mae_groups(n):
    return min(max((n // 4 + 255) // 256, 1), 2048)


@pytest.mark.parametrize("c", MAE_LOSS, ids=_ids(MAE_LOSS))
def test_mae_loss(lib, c):
    B, C, H, W, p, g = c["B"], c["C"], c["H"], c["W"], c["p"], _gen("ml" + c["name"])
    n, Lp = B * C * H * W, (H // p) * (W // p)
    mask = {"rand": (torch.rand(B, Lp, generator=g) < 0.75).float(), "all1": torch.ones(B, Lp), "all0": torch.zeros(B, Lp)}[c["mask"]]
    Gx, Gt = Guard((B, C, H, W), F32, torch.randn(B, C, H, W, generator=g).cuda()), Guard((B, C, H, W), F32, torch.randn(B, C, H, W, generator=g).cuda())
    Gm, Gc = Guard((B, Lp), F32, mask.cuda()), Guard((2,), F32, torch.tensor([0.37, -1.3]).cuda())
    groups = lib.load().ldmae_mae_loss_groups(n)
    assert groups == mae_groups(n)

    def run():
        P, dx = Guard((groups, 2), F32), Guard((B, C, H, W), F32)
        lib.call("ldmae_mae_loss_fwd", Gx.ptr(), Gt.ptr(), Gm.ptr(), P.ptr(), B, C, H, W, p, _stream())
        lib.call("ldmae_mae_loss_bwd", Gx.ptr(), Gt.ptr(), Gm.ptr(), Gc.ptr(), dx.ptr(), B, C, H, W, p, _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (P, dx, Gx, Gt, Gm, Gc)), "a canary changed"
        return dict(P=P.t.clone(), dx=dx.t.clone())

    got = _twice(run)
    assert bool(torch.isfinite(got["P"]).all()) and bool((got["P"] >= 0).all()), "a partial is not a finite non-negative sum"
    ref, bound = lc.mae_loss_fwd_ref(Gx.t, Gt.t, Gm.t, p, lc.mae_loss_depth(n // 4, groups))   # the partial rows are added in f64 here: no further rounding
    path = f"mae_loss[p{p}{',cap' if n // 4 > 524288 else ''}]"
    _chk(path, c["name"], "sums", got["P"].double().sum(0), ref, bound)
    _chk(path, c["name"], "dpred", got["dx"], *lc.mae_loss_bwd_ref(Gx.t, Gt.t, Gm.t, Gc.t, p))
    if c["mask"] != "rand":
        assert float(got["P"][:, 0 if c["mask"] == "all0" else 1].abs().max()) == 0.0, "the empty side of the mask has a non-zero sum"
    NCASES[0] += 1


# ============================================================================= latent prologue (sample = 0)
def LP(name, B, C, HW, norm=True):
    return dict(name=name, B=B, C=C, HW=HW, norm=norm)


LATENT = [LP("C1_HW4", 2, 1, 4), LP("C16_HW1024", 2, 16, 1024), LP("C16_HW1028", 1, 16, 1028), LP("C1_HW1028_plain", 3, 1, 1028, norm=False),
          LP("C16_HW4_plain", 2, 16, 4, norm=False)]


@pytest.mark.parametrize("c", LATENT, ids=_ids(LATENT))
def test_latent_prologue_plain(lib, c):
    B, C, HW, g = c["B"], c["C"], c["HW"], _gen("lp" + c["name"])
    Gl = Guard((B, C, HW), F32, (3 * torch.randn(B, C, HW, generator=g)).cuda())
    Gm, Gs = (Guard((C,), F32, torch.randn(C, generator=g).cuda()), Guard((C,), F32, (0.5 + torch.rand(C, generator=g)).cuda())) if c["norm"] else (None, None)
    noise = _payload_like(B * C * HW, F32)                    # sample = 0: the noise must not be read

    def run():
        out = Guard((B, C, HW), F32)
        lib.call("ldmae_latent_prologue", Gl.ptr(), noise.ptr(), _p(Gm), _p(Gs), 0.7, out.ptr(), B, C, HW, 0, _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (out, Gl, Gm, Gs) if q is not None), "a canary changed"
        return dict(out=out.t.clone())

    got = _twice(run)
    ref, bound = lc.latent_ref(Gl.t, Gm.t if Gm else None, Gs.t if Gs else None, 0.7)
    _chk(f"latent_prologue[{'norm' if c['norm'] else 'plain'}]", c["name"], "out", got["out"], ref, bound)
    NCASES[0] += 1



# ============================================================================= activations (measured constants: layer_check.py)
def _act_args(n, lim, g, dtype=F32):
    """0, +-0, +-tiny, +-lim and uniform values in [-lim, lim]; half of them within +-4 where the functions bend."""
    x = (torch.rand(n, generator=g) * 2 - 1) * lim
    x[1::2] = (torch.rand(x[1::2].numel(), generator=g) * 2 - 1) * 4
    edge = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-6, -1e-6, lim, -lim, 0.5 * lim, -0.5 * lim, 88.8, -88.8])
    edge = edge[edge.abs() <= lim]
    k = min(n, edge.numel())
    x[:k] = edge[:k]
    return x.to(dtype)


def AC(name, kind, T, n):
    return dict(name=name, kind=kind, T=T, n=n)


ACT_N = (1, 1003, 8192 * 256 + 77)
ACT = [AC(f"gelu_{_tn(_T)}_n{_n}", "gelu", _T, _n) for _T in TYPES for _n in ACT_N] + \
      [AC(f"gelu_tanh_{_tn(_T)}_n{_n}", "gelu_tanh", _T, _n) for _T in (F32, BF16) for _n in ACT_N]


@pytest.mark.parametrize("c", ACT, ids=_ids(ACT))
def test_gelu(lib, c):
    T, n, g = c["T"], c["n"], _gen("ac" + c["name"])
    Gx, Gg = Guard((n,), T, _act_args(n, 12.0, g, T).cuda()), Guard((n,), T, torch.randn(n, generator=g).to(T).cuda())
    fwd, bwd = ("ldmae_gelu_fwd", "ldmae_gelu_bwd") if c["kind"] == "gelu" else ("ldmae_gelu_tanh_fwd", "ldmae_gelu_tanh_bwd")

    def run():
        y, dx = Guard((n,), T), Guard((n,), T)
        lib.call(fwd, DT[T], Gx.ptr(), y.ptr(), n, _stream())
        lib.call(bwd, DT[T], Gg.ptr(), Gx.ptr(), dx.ptr(), n, _stream())
        torch.cuda.synchronize()
        assert y.intact() and dx.intact() and Gx.intact() and Gg.intact(), "a canary changed"
        return dict(y=y.t.clone(), dx=dx.t.clone())

    got = _twice(run)
    rf, rb = (lc.gelu_fwd_ref, lc.gelu_bwd_ref) if c["kind"] == "gelu" else (lc.gelu_tanh_fwd_ref, lc.gelu_tanh_bwd_ref)
    path = f"{c['kind']}[{_tn(T)}{',cap' if ew_capped(n) else ''}]"
    _chk(path, c["name"], "y", got["y"], *rf(Gx.t))
    _chk(path, c["name"], "dx", got["dx"], *rb(Gg.t, Gx.t))
    NCASES[0] += 1


def SW(name, M, Hs, T):
    return dict(name=name, M=M, Hs=Hs, T=T)


SWIGLU = [SW("M1_Hs8_f32", 1, 8, F32), SW("M1_Hs8_bf16", 1, 8, BF16), SW("M3_Hs24_f32", 3, 24, F32), SW("M37_Hs264_bf16", 37, 264, BF16),
          SW("cap_bf16", 2049, 8192, BF16)]


@pytest.mark.parametrize("c", SWIGLU, ids=_ids(SWIGLU))
def test_swiglu(lib, c):
    M, Hs, T, g = c["M"], c["Hs"], c["T"], _gen("sw" + c["name"])
    Gh = Guard((M, 2 * Hs), T, _act_args(M * 2 * Hs, 90.0, g, T).view(M, 2 * Hs).cuda())
    Gg = Guard((M, Hs), T, torch.randn(M, Hs, generator=g).to(T).cuda())

    def run():
        hid, dh = Guard((M, Hs), T), Guard((M, 2 * Hs), T)
        lib.call("ldmae_swiglu_fwd", DT[T], Gh.ptr(), hid.ptr(), M, Hs, _stream())
        lib.call("ldmae_swiglu_bwd", DT[T], Gg.ptr(), Gh.ptr(), dh.ptr(), M, Hs, _stream())
        torch.cuda.synchronize()
        assert hid.intact() and dh.intact() and Gh.intact() and Gg.intact(), "a canary changed"
        return dict(hid=hid.t.clone(), dh12=dh.t.clone())

    got = _twice(run)
    path = f"swiglu[{_tn(T)}{',cap' if ew_capped(M * Hs // 8) else ''}]"
    _chk(path, c["name"], "hid", got["hid"], *lc.swiglu_fwd_ref(Gh.t))
    _chk(path, c["name"], "dh12", got["dh12"], *lc.swiglu_bwd_ref(Gg.t, Gh.t))
    NCASES[0] += 1


SILU = [dict(name=f"{_tn(_T)}_n{_n}", T=_T, n=_n) for _T in (F32, BF16) for _n in ACT_N]


@pytest.mark.parametrize("c", SILU, ids=_ids(SILU))
def test_silu(lib, c):
    T, n, g = c["T"], c["n"], _gen("si" + c["name"])
    Gx, Gg = Guard((n,), F32, _act_args(n, 90.0, g).cuda()), Guard((n,), F32, torch.randn(n, generator=g).cuda())

    def run():
        y, dx = Guard((n,), T), Guard((n,), F32)
        lib.call("ldmae_silu_fwd", DT[T], Gx.ptr(), y.ptr(), n, _stream())
        lib.call("ldmae_silu_bwd", Gg.ptr(), Gx.ptr(), dx.ptr(), n, _stream())
        torch.cuda.synchronize()
        assert y.intact() and dx.intact() and Gx.intact() and Gg.intact(), "a canary changed"
        return dict(y=y.t.clone(), dx=dx.t.clone())

    got = _twice(run)
    path = f"silu[{_tn(T)}{',cap' if ew_capped(n) else ''}]"
    _chk(path, c["name"], "y", got["y"], *lc.silu_fwd_ref(Gx.t, T))
    _chk(path, c["name"], "dx", got["dx"], *lc.silu_bwd_ref(Gg.t, Gx.t))
    NCASES[0] += 1


LATENT_S = [LP("C1_HW4", 2, 1, 4), LP("C16_HW1024", 2, 16, 1024), LP("C16_HW1028_plain", 1, 16, 1028, norm=False), LP("C1_HW1028", 3, 1, 1028)]


@pytest.mark.parametrize("c", LATENT_S, ids=_ids(LATENT_S))
def test_latent_prologue_sample(lib, c):
    B, C, HW, g = c["B"], c["C"], c["HW"], _gen("ls" + c["name"])
    mom = 3 * torch.randn(B, 2 * C, HW, generator=g)
    mom[:, C:] = 12 * torch.randn(B, C, HW, generator=g)                  # logvar: most inside (-30, 20), some beyond either clamp point
    mom[:, C:, 0], mom[:, C:, 1], mom[:, C:, 2], mom[:, C:, 3] = -30.0, 20.0, -45.0, 33.0
    Gm, Gn = Guard((B, 2 * C, HW), F32, mom.cuda()), Guard((B, C, HW), F32, torch.randn(B, C, HW, generator=g).cuda())
    Gmu, Gs = (Guard((C,), F32, torch.randn(C, generator=g).cuda()), Guard((C,), F32, (0.5 + torch.rand(C, generator=g)).cuda())) if c["norm"] else (None, None)

    def run():
        out = Guard((B, C, HW), F32)
        lib.call("ldmae_latent_prologue", Gm.ptr(), Gn.ptr(), _p(Gmu), _p(Gs), 0.7, out.ptr(), B, C, HW, 1, _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (out, Gm, Gn, Gmu, Gs) if q is not None), "a canary changed"
        return dict(out=out.t.clone())

    got = _twice(run)
    ref, bound = lc.latent_sample_ref(Gm.t, Gn.t, Gmu.t if Gmu else None, Gs.t if Gs else None, 0.7)
    _chk(f"latent_prologue[sample,{'norm' if c['norm'] else 'plain'}]", c["name"], "out", got["out"], ref, bound)
    NCASES[0] += 1


# ============================================================================= AdamW + EMA
HYP = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, ema_decay=0.9999)


def AD(name, n, steps, gs=1.0, wd=0.0, ema=True):
    return dict(name=name, n=n, steps=steps, gs=gs, wd=wd, ema=ema)


ADAMW = [
    AD("n4_step1", 4, (1,)), AD("n4160_step2_wd_gs", 4160, (2,), gs=2.0 ** -7, wd=0.05), AD("n4160_step10000_noema", 4160, (10000,), wd=0.05, ema=False),
    AD("n4160_chain_1_2_3", 4160, (1, 2, 3), gs=2.0 ** -7, wd=0.05), AD("n4_step1_noema_gs", 4, (1,), gs=2.0 ** -7, ema=False),
    AD("cap_step2", 4 * (8192 * 256 + 3), (2,), wd=0.05),
]


def ew_capped(work_items):
    return (work_items + 255) // 256 > 8192


@pytest.mark.parametrize("c", ADAMW, ids=_ids(ADAMW))
def test_adamw_ema(lib, c):
    n, g = c["n"], _gen("ad" + c["name"])
    first = c["steps"][0] == 1
    p0, g0 = torch.randn(n, generator=g).cuda(), (torch.randn(n, generator=g) / c["gs"]).cuda()
    g0[::7] = 0.0
    m0 = torch.zeros(n).cuda() if first else (0.1 * torch.randn(n, generator=g)).cuda()
    v0 = torch.zeros(n).cuda() if first else (0.01 * torch.rand(n, generator=g)).cuda()
    e0 = torch.randn(n, generator=g).cuda()
    Gg = Guard((n,), F32, g0)

    def run():
        P, M_, V = Guard((n,), F32, p0), Guard((n,), F32, m0), Guard((n,), F32, v0)
        E = Guard((n,), F32, e0) if c["ema"] else None
        r = {}
        for s in c["steps"]:
            lib.call("ldmae_adamw_ema", P.ptr(), Gg.ptr(), M_.ptr(), V.ptr(), _p(E), n, s, HYP["lr"], HYP["beta1"], HYP["beta2"], HYP["eps"],
                     c["wd"], HYP["ema_decay"], c["gs"], _stream())
            torch.cuda.synchronize()
            r.update({f"p@{s}": P.t.clone(), f"m@{s}": M_.t.clone(), f"v@{s}": V.t.clone()})
            if E is not None:
                r[f"ema@{s}"] = E.t.clone()
        assert all(q.intact() for q in (P, M_, V, E, Gg) if q is not None), "a canary changed"
        return r

    got = _twice(run)
    state = None
    for s in c["steps"]:
        a = lc.adam_scalars(s, HYP["lr"], HYP["beta1"], HYP["beta2"], HYP["eps"], c["wd"], HYP["ema_decay"], c["gs"])
        out = lc.adamw_ref(p0, g0, m0, v0, e0 if c["ema"] else None, a, state)
        state = (out["p"], out["m"], out["v"], out.get("ema"))
        for k, fl in out.items():
            _chk(f"adamw[{'ema' if c['ema'] else 'noema'},gs{'1' if c['gs'] == 1.0 else '2^-7'}]", c["name"], k, got[f"{k}@{s}"], fl.v, fl.e)
    NCASES[0] += 1


EMA_ONLY = [dict(name=f"n{_n}", n=_n) for _n in (1, 1003, 8192 * 256 + 77)]


@pytest.mark.parametrize("c", EMA_ONLY, ids=_ids(EMA_ONLY))
def test_ema_only(lib, c):
    n, g = c["n"], _gen("eo" + c["name"])
    e0, Gp = torch.randn(n, generator=g).cuda(), Guard((n,), F32, torch.randn(n, generator=g).cuda())

    def run():
        E = Guard((n,), F32, e0)
        lib.call("ldmae_ema_only", E.ptr(), Gp.ptr(), n, 0.9999, _stream())
        torch.cuda.synchronize()
        assert E.intact() and Gp.intact(), "a canary changed"
        return dict(ema=E.t.clone())

    got = _twice(run)
    _chk(f"ema_only[{'cap' if ew_capped(n) else 'plain'}]", c["name"], "ema", got["ema"], *lc.ema_ref(e0, Gp.t, 0.9999))
    NCASES[0] += 1


# ============================================================================= label embedding
NUM_CLASSES = 12          # labels are drawn from 0 .. 7: rows 8 .. 11 are never hit, row 12 only by dropped samples


def LE(name, B, D, drop):
    return dict(name=name, B=B, D=D, drop=drop)


LABEL = [LE("B1_D4_null", 1, 4, "null"), LE("B70_D192_mixed", 70, 192, "mixed"), LE("B256_D300_all", 256, 300, "all"),
         LE("B300_D192_mixed", 300, 192, "mixed"), LE("B300_D4_null", 300, 4, "null"), LE("B300_D300_all", 300, 300, "all")]


def label_passes(B):
    return (B + 255) // 256


@pytest.mark.parametrize("c", LABEL, ids=_ids(LABEL))
def test_label_embed(lib, c):
    B, D, g = c["B"], c["D"], _gen("le" + c["name"])
    R = NUM_CLASSES + 1
    y = torch.randint(0, 8, (B,), generator=g).cuda()
    drop = {"null": None, "mixed": (torch.rand(B, generator=g) < 0.3).to(torch.uint8).cuda(), "all": torch.ones(B, dtype=torch.uint8).cuda()}[c["drop"]]
    Gt, Gd = Guard((R, D), F32, torch.randn(R, D, generator=g).cuda()), Guard((B, D), F32, torch.randn(B, D, generator=g).cuda())
    t0 = torch.randn(R, D, generator=g).cuda()
    dp = None if drop is None else drop.data_ptr()

    def run():
        out, dt = Guard((B, D), F32), Guard((R, D), F32, t0)
        lib.call("ldmae_label_embed_fwd", Gt.ptr(), y.data_ptr(), dp, out.ptr(), B, D, NUM_CLASSES, _stream())
        lib.call("ldmae_label_embed_bwd", Gd.ptr(), y.data_ptr(), dp, dt.ptr(), B, D, NUM_CLASSES, R, _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (out, dt, Gt, Gd)), "a canary changed"
        return dict(out=out.t.clone(), dtable=dt.t.clone())

    got = _twice(run)
    rows = lc.label_rows(y, drop, NUM_CLASSES)
    _same(c["name"] + " out", got["out"], Gt.t[rows])
    ref, bound = lc.label_bwd_ref(Gd.t, y, drop, t0, NUM_CLASSES)
    _chk(f"label_embed_bwd[passes{label_passes(B)}]", c["name"], "dtable", got["dtable"], ref, bound)
    nohit = torch.ones(R, dtype=torch.bool, device="cuda")
    nohit[rows] = False
    assert nohit.any()
    _same(c["name"] + " rows nobody hits", got["dtable"][nohit], t0[nohit])
    NCASES[0] += 1


# ============================================================================= bit-exact kernels
def MK(name, L, keep):
    return dict(name=name, L=L, keep=keep)


MASKING = [MK("L1_keep0", 1, 0), MK("L1_keep1", 1, 1), MK("L2_keep1", 2, 1), MK("L3_keepL", 3, 3), MK("L200_keep50", 200, 50),
           MK("L255_keep1", 255, 1), MK("L256_keep64", 256, 64), MK("L257_keep0", 257, 0), MK("L4096_keep1024", 4096, 1024),
           MK("L4096_keepL", 4096, 4096)]
MASK_ROWS = ("random", "ties", "all_equal", "negative", "signed_zero")


def masking_noise(L, g):
    """One row per entry of MASK_ROWS."""
    r = torch.rand(5, L, generator=g)
    r[1] = (r[1] * 8).floor() / 8
    r[2] = 0.25
    r[3] = r[3] - 0.5
    r[3, ::3] = -((r[3, ::3] * 4).floor() / 4).abs()
    r[4] = torch.where(r[4] < 0.4, torch.tensor(-0.0), torch.where(r[4] < 0.8, torch.tensor(0.0), r[4] - 0.9))
    return r


@pytest.mark.parametrize("c", MASKING, ids=_ids(MASKING))
def test_random_masking(lib, c):
    L, keep, N = c["L"], c["keep"], len(MASK_ROWS)
    Gn = Guard((N, L), F32, masking_noise(L, _gen("mk" + c["name"])).cuda())

    def run():
        restore, mask, idk = IGuard((N, L)), Guard((N, L), F32), IGuard((N, max(keep, 1)))
        lib.call("ldmae_random_masking", Gn.ptr(), restore.ptr(), mask.ptr(), idk.ptr(), N, L, keep, _stream())
        torch.cuda.synchronize()
        assert restore.intact() and mask.intact() and idk.intact() and Gn.intact(), "a canary changed"
        if keep == 0:
            assert bool((idk.t == IGuard.S).all()), "keep = 0: ids_keep was written"
        return dict(restore=restore.t.clone(), mask=mask.t.clone(), ids_keep=idk.t[:, :keep].clone() if keep else idk.t[:, :0].clone())

    got = _twice(run)
    r, m, k = lc.masking_ref(Gn.t, keep)
    _same(c["name"] + " ids_restore", got["restore"], r.cuda())
    _same(c["name"] + " mask", got["mask"], m.cuda())
    _same(c["name"] + " ids_keep", got["ids_keep"].reshape(N, keep), k.cuda().reshape(N, keep))
    NCASES[0] += 1


@pytest.mark.parametrize("D", (4, 260))
def test_gather_scatter_rows(lib, D):
    N, L, keep, g = 3, 23, 7, _gen(f"gs{D}")
    ids = _perm_ids(N, L, g)[:, :keep].contiguous()
    Gx, Gd = Guard((N, L, D), F32, torch.randn(N, L, D, generator=g).cuda()), Guard((N, keep, D), F32, torch.randn(N, keep, D, generator=g).cuda())

    def run():
        out, dx = Guard((N, keep, D), F32), Guard((N, L, D), F32, torch.zeros(N, L, D).cuda())
        lib.call("ldmae_gather_rows", Gx.ptr(), ids.data_ptr(), out.ptr(), N, L, keep, D, _stream())
        lib.call("ldmae_scatter_rows", Gd.ptr(), ids.data_ptr(), dx.ptr(), N, L, keep, D, _stream())
        torch.cuda.synchronize()
        assert out.intact() and dx.intact() and Gx.intact() and Gd.intact(), "a canary changed"
        return dict(out=out.t.clone(), dx=dx.t.clone())

    got = _twice(run)
    idx = ids[:, :, None].expand(N, keep, D)
    _same("gather", got["out"], torch.gather(Gx.t, 1, idx))
    _same("scatter", got["dx"], torch.zeros(N, L, D, device="cuda").scatter_(1, idx, Gd.t))      # unvisited rows stay zero
    NCASES[0] += 1


def PG(name, p, C, keep, D, T):
    return dict(name=name, p=p, C=C, keep=keep, D=D, T=T)


PATCH = [PG("p1_C3_f32", 1, 3, 4, 4, F32), PG("p2_C4_bf16", 2, 4, 1, 192, BF16), PG("p8_C3_bf16", 8, 3, 5, 516, BF16), PG("p16_C4_f32", 16, 4, 9, 192, F32),
         PG("p16_C3_bf16", 16, 3, 3, 4, BF16), PG("p1_C4_bf16", 1, 4, 9, 516, BF16), PG("p2_C3_f32", 2, 3, 1, 4, F32), PG("p8_C4_f32", 8, 4, 2, 516, F32)]


@pytest.mark.parametrize("c", PATCH, ids=_ids(PATCH))
def test_patch_gather(lib, c):
    p, C, keep, D, T, N, grid, g = c["p"], c["C"], c["keep"], c["D"], c["T"], 2, 3, _gen("pg" + c["name"])
    S, K = grid * p, C * p * p
    ids = _perm_ids(N, grid * grid, g)[:, :keep].contiguous()          # out of order by construction
    Gi, Gp = Guard((N, C, S, S), F32, torch.randn(N, C, S, S, generator=g).cuda()), Guard((grid * grid, D), F32, torch.randn(grid * grid, D, generator=g).cuda())

    def run():
        tok, posg = Guard((N * keep, K), T), Guard((N * keep, D), F32)
        lib.call("ldmae_patch_gather", DT[T], Gi.ptr(), ids.data_ptr(), Gp.ptr(), tok.ptr(), posg.ptr(), N, keep, C, S, p, D, _stream())
        torch.cuda.synchronize()
        assert tok.intact() and posg.intact() and Gi.intact() and Gp.intact(), "a canary changed"
        return dict(tok=tok.t.clone(), posg=posg.t.clone())

    got = _twice(run)
    tok, posg = lc.patch_gather_ref(Gi.t, ids, Gp.t, p)
    _same(c["name"] + " tok", got["tok"], tok.to(T))                   # bf16: one rounding of the source
    _same(c["name"] + " posg", got["posg"], posg)
    NCASES[0] += 1


CAST_PAIRS = ((F32, BF16), (BF16, F32), (F32, F16), (F16, F32), (F32, F32))
CAST = [dict(name=f"{_tn(_s)}_{_tn(_d)}_n{_n}", src=_s, dst=_d, n=_n) for _s, _d in CAST_PAIRS for _n in (1, 7, 8, 9, 1003)] + [
    dict(name="cap_f32_bf16", src=F32, dst=BF16, n=8 * 8192 * 256 + 13)]


def _wide(n, g, dtype):
    """Values across the whole exponent range of the 16-bit types, ties to even and subnormal results included."""
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-30, 16, (n,), generator=g).float())
    x[::5] = (torch.randint(0, 2 ** 16, (x[::5].numel(),), generator=g).float() + 0.5) * 2.0 ** -8        # exact ties of bf16 at [1, 2^8) scale
    return x.to(dtype)


@pytest.mark.parametrize("c", CAST, ids=_ids(CAST))
def test_cast(lib, c):
    n, S, Dt = c["n"], c["src"], c["dst"]
    Gs = Guard((n,), S, _wide(n, _gen("ca" + c["name"]), S).cuda())

    def run():
        out = Guard((n,), Dt)
        lib.call("ldmae_cast", DT[S], DT[Dt], Gs.ptr(), out.ptr(), n, _stream())
        torch.cuda.synchronize()
        assert out.intact() and Gs.intact(), "a canary changed"
        return dict(out=out.t.clone())

    _same(c["name"], _twice(run)["out"], Gs.t.to(Dt))
    NCASES[0] += 1


CAST_STACK = [dict(name=f"count{_c}_n{_n}_{_tn(_T)}", count=_c, n=_n, T=_T) for _c, _n, _T in
              ((1, 8, BF16), (3, 8, F32), (64, 8, BF16), (3, 1000, BF16), (1, 8 * (1024 * 256 + 5), BF16), (2, 8 * (1024 * 256 + 5), F32))]


@pytest.mark.parametrize("c", CAST_STACK, ids=_ids(CAST_STACK))
def test_cast_stack(lib, c):
    count, n, T, g = c["count"], c["n"], c["T"], _gen("cs" + c["name"])
    srcs = [Guard((n,), F32, _wide(n, g, F32).cuda()) for _ in range(count)]
    arr = (ctypes.c_void_p * count)(*[s.ptr() for s in srcs])

    def run():
        out = Guard((count, n), T)
        lib.call("ldmae_cast_stack", DT[T], arr, count, n, out.ptr(), _stream())
        torch.cuda.synchronize()
        assert out.intact() and all(s.intact() for s in srcs), "a canary changed"
        return dict(out=out.t.clone())

    _same(c["name"], _twice(run)["out"], torch.stack([s.t for s in srcs]).to(T))
    NCASES[0] += 1


def cw64(R, C, doff_bytes):
    return R % 64 == 0 and C % 64 == 0 and doff_bytes % 16 == 0


def CW(name, R, C, T, doff=0, dst=True, dstT=True):
    return dict(name=name, R=R, C=C, T=T, doff=doff, dst=dst, dstT=dstT)


CAST_WEIGHT = [
    CW("64_128x64_bf16", 128, 64, BF16), CW("64_64x128_f16", 64, 128, F16), CW("64_64x64_f32", 64, 64, F32),
    CW("64_nodst_bf16", 64, 128, BF16, dst=False), CW("64_nodstT_f32", 128, 64, F32, dstT=False),
    CW("32_R96_bf16", 96, 64, BF16), CW("32_C96_f16", 64, 96, F16), CW("32_off8_bf16", 64, 64, BF16, doff=8), CW("32_off8_f32", 64, 64, F32, doff=8),
    CW("32_R1_f32", 1, 5, F32), CW("32_C1_bf16", 7, 1, BF16), CW("32_small_f16", 20, 31, F16), CW("32_R33_C70_bf16", 33, 70, BF16),
    CW("32_nodst_f16", 20, 31, F16, dst=False), CW("32_nodstT_bf16", 33, 70, BF16, dstT=False),
]


@pytest.mark.parametrize("c", CAST_WEIGHT, ids=_ids(CAST_WEIGHT))
def test_cast_weight(lib, c):
    R, C, T, g = c["R"], c["C"], c["T"], _gen("cw" + c["name"])
    off = c["doff"] // torch.empty(0, dtype=T).element_size()
    Gs = Guard((R, C), F32, _wide(R * C, g, F32).view(R, C).cuda())

    def run():
        d, dT = (Off((R, C), T, None, off) if c["dst"] else None), (Off((C, R), T, None, off) if c["dstT"] else None)
        lib.call("ldmae_cast_weight", DT[T], Gs.ptr(), _p(d), _p(dT), R, C, _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (d, dT, Gs) if q is not None), "a canary changed"
        r = {}
        if d is not None:
            r["dst"] = d.t.clone()
        if dT is not None:
            r["dstT"] = dT.t.clone()
        return r

    got = _twice(run)
    if c["dst"]:
        _same(c["name"] + " dst", got["dst"], Gs.t.to(T))
    if c["dstT"]:
        _same(c["name"] + " dstT", got["dstT"], Gs.t.to(T).T.contiguous())
    NCASES[0] += 1


MULTI_ADD = [dict(name="count1_n1", lens=(1,)), dict(name="count32_mixed", lens=tuple((1, 255, 256, 65537)[i % 4] for i in range(32))),
             dict(name="count3_long_first", lens=(65537, 1, 255))]


@pytest.mark.parametrize("c", MULTI_ADD, ids=_ids(MULTI_ADD))
def test_multi_add(lib, c):
    g, k = _gen("ma" + c["name"]), len(c["lens"])
    d0 = [torch.randn(n, generator=g).cuda() for n in c["lens"]]
    srcs = [Guard((n,), F32, torch.randn(n, generator=g).cuda()) for n in c["lens"]]

    def run():
        dsts = [Guard((n,), F32, d) for n, d in zip(c["lens"], d0)]
        da, sa = (ctypes.c_void_p * k)(*[d.ptr() for d in dsts]), (ctypes.c_void_p * k)(*[s.ptr() for s in srcs])
        lib.call("ldmae_multi_add", k, da, sa, (ctypes.c_long * k)(*c["lens"]), _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in dsts + srcs), "a canary changed"
        return {f"dst{i}": d.t.clone() for i, d in enumerate(dsts)}

    got = _twice(run)
    for i in range(k):
        _same(f"{c['name']} dst{i}", got[f"dst{i}"], d0[i] + srcs[i].t)       # one correctly rounded f32 add
    NCASES[0] += 1


TIMESTEP = [dict(name=f"dim{_d}_B{_B}_mp{_mp}", dim=_d, B=_B, mp=_mp) for _d, _B, _mp in ((2, 4, 10000.0), (3, 4, 10000.0), (256, 3, 10000.0), (257, 4, 100.0),
                                                                                     (257, 5, 10000.0))]


@pytest.mark.parametrize("c", TIMESTEP, ids=_ids(TIMESTEP))
def test_timestep_embedding(lib, c):
    """Every element inside its bound; the padding column of an odd dim exactly +0.0; t = 0 -> cos = 1 and sin = 0 exactly."""
    dim, B, half = c["dim"], c["B"], c["dim"] // 2
    Gt = Guard((B,), F32, torch.tensor([0.0, 0.25, 1.0, 1000.0, 0.5])[:B].cuda())

    def run():
        out = Guard((B, dim), F32)
        lib.call("ldmae_timestep_embedding", Gt.ptr(), out.ptr(), B, dim, c["mp"], _stream())
        torch.cuda.synchronize()
        assert out.intact() and Gt.intact(), "a canary changed"
        return dict(out=out.t.clone())

    out = _twice(run)["out"]
    _chk(f"timestep[{'odd' if dim & 1 else 'even'}]", c["name"], "out", out, *lc.timestep_ref(Gt.t, dim, c["mp"]))
    if dim & 1:
        _same(c["name"] + " zero column", out[:, -1], torch.zeros(B, device="cuda"))
    _same(c["name"] + " t = 0", out[0, :2 * half], torch.cat([torch.ones(half), torch.zeros(half)]).cuda())
    NCASES[0] += 1


# ============================================================================= refused arguments
def _refusals(L):
    """name -> (callable returning the status, the guards that must stay intact)."""
    f = lambda *s, T=F32: Guard(s, T, torch.zeros(s, dtype=T).cuda())       # noqa: E731  finite input
    o = lambda *s, T=F32: Guard(s, T)                                        # noqa: E731  NaN-filled output
    st = _stream()
    ids = torch.zeros(2, 4, dtype=I64).cuda()
    R = {}

    def add(name, fn, *guards):
        R[name] = (fn, guards)

    x, w, b, y, mu, rs = f(4, 1284), f(1284), f(1284), o(4, 1284), o(4), o(4)
    add("layernorm_fwd D % 4", lambda: L.ldmae_layernorm_fwd(0, x.ptr(), w.ptr(), b.ptr(), y.ptr(), mu.ptr(), rs.ptr(), 4, 6, EPS, st), y, mu, rs)
    add("layernorm_fwd D > 1280", lambda: L.ldmae_layernorm_fwd(0, x.ptr(), w.ptr(), b.ptr(), y.ptr(), mu.ptr(), rs.ptr(), 4, 1284, EPS, st), y, mu, rs)
    g16, dx, dxc, dw, db, ws = f(4, 1284, T=BF16), o(4, 1284), o(4, 1284), o(1284), o(1284), o(4096)
    m_, r_ = f(4), f(4)
    for nm, D in (("D % 4", 6), ("D > 1280", 1284)):
        add(f"layernorm_bwd {nm}", lambda D=D: L.ldmae_layernorm_bwd(1, g16.ptr(), x.ptr(), w.ptr(), m_.ptr(), r_.ptr(), dx.ptr(), dw.ptr(), db.ptr(), 0.0,
                                                                    4, D, ws.ptr(), st), dx, dw, db, ws)
    add("layernorm_bwd_cast f32 dx_cast", lambda: L.ldmae_layernorm_bwd_cast(0, x.ptr(), x.ptr(), w.ptr(), m_.ptr(), r_.ptr(), dx.ptr(), dxc.ptr(), dw.ptr(),
                                                                             db.ptr(), 0.0, 4, 64, ws.ptr(), st), dx, dxc, dw, db, ws)
    do, rdx, dm, rws = f(2, 4, 516), o(2, 2, 516), o(516), o(8192)
    add("restore_tokens_bwd D > 512", lambda: L.ldmae_restore_tokens_bwd(do.ptr(), ids.data_ptr(), rdx.ptr(), dm.ptr(), 2, 4, 2, 516, rws.ptr(), st), rdx, dm, rws)
    add("restore_tokens_bwd dmask without workspace", lambda: L.ldmae_restore_tokens_bwd(do.ptr(), ids.data_ptr(), rdx.ptr(), dm.ptr(), 2, 4, 2, 64, None, st),
        rdx, dm)
    lat, noise, lm, lo = f(2, 2, 8), f(2, 1, 8), f(1), o(2, 1, 8)
    add("latent_prologue mean only", lambda: L.ldmae_latent_prologue(lat.ptr(), None, lm.ptr(), None, 1.0, lo.ptr(), 2, 1, 8, 0, st), lo)
    add("latent_prologue std only", lambda: L.ldmae_latent_prologue(lat.ptr(), None, None, lm.ptr(), 1.0, lo.ptr(), 2, 1, 8, 0, st), lo)
    add("latent_prologue sample without noise", lambda: L.ldmae_latent_prologue(lat.ptr(), None, None, None, 1.0, lo.ptr(), 2, 1, 8, 1, st), lo)
    tg, tt, tdw, tdb = f(8, 4), f(8, 16), o(4, 16), o(4)
    need = L.ldmae_thin_tn_workspace_bytes(8, 4, 16)
    tws = _ws(need)
    add("thin_tn beta 0.5", lambda: L.ldmae_thin_tn(tg.ptr(), tt.ptr(), tdw.ptr(), tdb.ptr(), 8, 4, 16, 0.5, tws.ptr(), need, st), tdw, tdb, tws)
    add("thin_tn short workspace", lambda: L.ldmae_thin_tn(tg.ptr(), tt.ptr(), tdw.ptr(), tdb.ptr(), 8, 4, 16, 0.0, tws.ptr(), need - 4, st), tdw, tdb, tws)
    cs, cd = f(64), o(64, T=BF16)
    add("cast misaligned src", lambda: L.ldmae_cast(0, 1, cs.ptr() + 4, cd.ptr(), 8, st), cd)
    add("cast misaligned dst", lambda: L.ldmae_cast(0, 1, cs.ptr(), cd.ptr() + 2, 8, st), cd)
    add("cast bf16 -> f16", lambda: L.ldmae_cast(1, 2, cs.ptr(), cd.ptr(), 8, st), cd)
    add("cast bf16 -> bf16", lambda: L.ldmae_cast(1, 1, cs.ptr(), cd.ptr(), 8, st), cd)
    ap, ag, am, av, ae = o(8), f(8), o(8), o(8), o(8)
    hyp = (HYP["lr"], HYP["beta1"], HYP["beta2"], HYP["eps"], 0.0, HYP["ema_decay"], 1.0)
    add("adamw_ema n % 4", lambda: L.ldmae_adamw_ema(ap.ptr(), ag.ptr(), am.ptr(), av.ptr(), ae.ptr(), 6, 1, *hyp, st), ap, am, av, ae)
    add("adamw_ema step 0", lambda: L.ldmae_adamw_ema(ap.ptr(), ag.ptr(), am.ptr(), av.ptr(), ae.ptr(), 8, 0, *hyp, st), ap, am, av, ae)
    cg, cx, cw_, cdx, cdw, cdb = f(1, 4, 4, 4), f(1, 4, 4, 4), f(4, 4, 3, 3), o(1, 4, 4, 4), o(4, 4, 3, 3), o(4)
    cws = _ws(L.ldmae_conv3x3_bwd_workspace_bytes(4))
    add("conv3x3_bwd C = 4", lambda: L.ldmae_conv3x3_bwd(cg.ptr(), cx.ptr(), cw_.ptr(), cdx.ptr(), cdw.ptr(), cdb.ptr(), 1, 4, 4, 4, cws.ptr(), st), cdx, cdw, cdb, cws)
    add("conv3x3_bwd C = 1", lambda: L.ldmae_conv3x3_bwd(cg.ptr(), cx.ptr(), cw_.ptr(), cdx.ptr(), cdw.ptr(), cdb.ptr(), 1, 1, 4, 4, cws.ptr(), st), cdx, cdw, cdb, cws)
    lp, li, lmk, lP, ldx, lc_ = f(1, 1, 12, 12), f(1, 1, 12, 12), f(1, 36), o(4, 2), o(1, 1, 12, 12), f(2)
    for nm, p in (("p % 4", 6), ("p not dividing H", 8)):
        add(f"mae_loss_fwd {nm}", lambda p=p: L.ldmae_mae_loss_fwd(lp.ptr(), li.ptr(), lmk.ptr(), lP.ptr(), 1, 1, 12, 12, p, st), lP)
        add(f"mae_loss_bwd {nm}", lambda p=p: L.ldmae_mae_loss_bwd(lp.ptr(), li.ptr(), lmk.ptr(), lc_.ptr(), ldx.ptr(), 1, 1, 12, 12, p, st), ldx)
    # A dtype code the entry point has no kernel for: 2 (f16) where only f32 / bf16 exist, 7 where all three do.  Every buffer has the f32
    # size whatever the code claims, so a fall-through to the float kernel would stay in bounds and show up below as a write.
    h12, hid, dh12, dhid = f(16, 256), o(16, 128), o(16, 256), f(16, 128)
    add("swiglu_fwd dtype 2", lambda: L.ldmae_swiglu_fwd(2, h12.ptr(), hid.ptr(), 16, 128, st), hid)
    add("swiglu_bwd dtype 2", lambda: L.ldmae_swiglu_bwd(2, dhid.ptr(), h12.ptr(), dh12.ptr(), 16, 128, st), dh12)
    ex, eg, ey = f(64), f(64), o(64)
    add("silu_fwd dtype 2", lambda: L.ldmae_silu_fwd(2, ex.ptr(), ey.ptr(), 64, st), ey)
    add("gelu_tanh_fwd dtype 2", lambda: L.ldmae_gelu_tanh_fwd(2, ex.ptr(), ey.ptr(), 64, st), ey)
    add("gelu_tanh_bwd dtype 2", lambda: L.ldmae_gelu_tanh_bwd(2, eg.ptr(), ex.ptr(), ey.ptr(), 64, st), ey)
    add("gelu_fwd dtype 7", lambda: L.ldmae_gelu_fwd(7, ex.ptr(), ey.ptr(), 64, st), ey)
    add("gelu_bwd dtype 7", lambda: L.ldmae_gelu_bwd(7, eg.ptr(), ex.ptr(), ey.ptr(), 64, st), ey)
    nT, nW, nb, nout = f(16, 16), f(256, 16), f(256), o(16, 256)
    add("thin_nt dtype 2", lambda: L.ldmae_thin_nt(2, nT.ptr(), nW.ptr(), nb.ptr(), None, nout.ptr(), 16, 256, 16, 16, st), nout)
    img, ppos, ptok, pposg = f(1, 3, 16, 16), f(16, 256), o(4, 48), o(4, 256)
    add("patch_gather dtype 2", lambda: L.ldmae_patch_gather(2, img.ptr(), ids.data_ptr(), ppos.ptr(), ptok.ptr(), pposg.ptr(), 1, 4, 3, 16, 4, 256, st), ptok, pposg)
    sX, sout, sws = f(16, 256), o(256), o(4096)
    add("colsum dtype 7", lambda: L.ldmae_colsum(7, sX.ptr(), 256, 16, 256, sout.ptr(), 0.0, sws.ptr(), st), sout, sws)
    wd, wdT = o(16, 256), o(256, 16)
    add("cast_weight dtype 7", lambda: L.ldmae_cast_weight(7, sX.ptr(), wd.ptr(), wdT.ptr(), 16, 256, st), wd, wdT)
    srcs = (ctypes.c_void_p * 1)(cs.ptr())
    add("cast_stack dtype 2", lambda: L.ldmae_cast_stack(2, srcs, 1, 8, ey.ptr(), st), ey)
    add("layernorm_fwd dtype 7", lambda: L.ldmae_layernorm_fwd(7, x.ptr(), w.ptr(), b.ptr(), y.ptr(), mu.ptr(), rs.ptr(), 4, 64, EPS, st), y, mu, rs)
    add("layernorm_bwd dtype 7", lambda: L.ldmae_layernorm_bwd(7, x.ptr(), x.ptr(), w.ptr(), m_.ptr(), r_.ptr(), dx.ptr(), dw.ptr(), db.ptr(), 0.0, 4, 64,
                                                              ws.ptr(), st), dx, dw, db, ws)
    add("layernorm_bwd_cast dtype 7", lambda: L.ldmae_layernorm_bwd_cast(7, x.ptr(), x.ptr(), w.ptr(), m_.ptr(), r_.ptr(), dx.ptr(), dxc.ptr(), dw.ptr(),
                                                                        db.ptr(), 0.0, 4, 64, ws.ptr(), st), dx, dxc, dw, db, ws)
    mq, msc = o(16, 64), o(32)
    add("mx8_quantize dtype 2", lambda: L.ldmae_mx8_quantize(2, sX.ptr(), 256, mq.ptr(), msc.ptr(), 16, 256, st), mq, msc)
    return R


REFUSED = ["layernorm_fwd D % 4", "layernorm_fwd D > 1280", "layernorm_bwd D % 4", "layernorm_bwd D > 1280", "layernorm_bwd_cast f32 dx_cast",
           "restore_tokens_bwd D > 512", "restore_tokens_bwd dmask without workspace", "latent_prologue mean only", "latent_prologue std only",
           "latent_prologue sample without noise", "thin_tn beta 0.5", "thin_tn short workspace", "cast misaligned src", "cast misaligned dst",
           "cast bf16 -> f16", "cast bf16 -> bf16", "adamw_ema n % 4", "adamw_ema step 0", "conv3x3_bwd C = 4", "conv3x3_bwd C = 1",
           "mae_loss_fwd p % 4", "mae_loss_bwd p % 4", "mae_loss_fwd p not dividing H", "mae_loss_bwd p not dividing H",
           "swiglu_fwd dtype 2", "swiglu_bwd dtype 2", "silu_fwd dtype 2", "gelu_tanh_fwd dtype 2", "gelu_tanh_bwd dtype 2", "gelu_fwd dtype 7",
           "gelu_bwd dtype 7", "thin_nt dtype 2", "patch_gather dtype 2", "colsum dtype 7", "cast_weight dtype 7", "cast_stack dtype 2",
           "layernorm_fwd dtype 7", "layernorm_bwd dtype 7", "layernorm_bwd_cast dtype 7", "mx8_quantize dtype 2"]


def test_refused_arguments(lib):
    """Each call returns a negative status with a message, launches nothing and leaves every output buffer with its NaN payload."""
    R = _refusals(lib.load())
    assert sorted(R) == sorted(REFUSED)
    for name in REFUSED:
        fn, guards = R[name]
        rc = fn()
        assert rc == -1 and lib.last_error(), f"{name}: not refused as an invalid argument (status {rc})"
    torch.cuda.synchronize()
    for name in REFUSED:
        for q in R[name][1]:
            assert q.intact() and q.untouched(q.t), f"{name}: a refused call wrote to a buffer"
    NCASES[0] += len(REFUSED)
