"""Every dispatch path of the evaluation kernels, element by element, with the bounds of tests/eval_check.py: csrc/inception.hip (convolution,
pools, global average, FID pre-processing, feature statistics), csrc/adm_eval.hip (ADM pre-processing, spatial tap, row norms, pairwise
logits, k-NN radii, precision / recall flags, softmax + Inception Score sums) and csrc/tokenizer_eval.hip (LPIPS pre-processing and head in
f32 and f16, SSIM, the PNG quantiser and both SSE paths).

Seeded case tables drive the C ABI directly (ldmae_amd._lib), so each case controls pointers, leading dimensions, NULLs and alignment.  Each case
  - places every input in a NaN-padded buffer (sentinel-padded for integer types), channel slices inside rows whose other channels hold the
    payload, and every output in a buffer pre-filled with the payload (accumulating outputs -- fid_stats' sum / cross, lpips_layer's out --
    get seeded finite contents; the flags of pr_flags are zeroed by the caller, as the entry point asks);
  - gives workspaces exactly the size *_workspace_bytes / ldmae_knn_partials_bytes report, inside a canary;
  - checks every element of every output against the reference with its per-element bound, or for equal bits where eval_check.py says
    "exact", and checks every canary; the only excluded elements are the undecided flags of pr_flags (at most 1 % per case);
  - runs a second time on fresh outputs and requires bitwise-equal results;
  - records the worst err / bound per path and output (printed at module teardown).
k-NN radii and the flags are fed norms (and radii) made by the f64 reference rounded to f32, never a kernel's output.

Host predicates, each taken and not taken by some case (tests/test_eval_check_cpu.py::test_case_table_covers_every_predicate, from the
tables alone): the convolution's `vec` by each of its five reasons, relu, bias NULL; pool mode; launch_pairwise's `vec` by each of its three
reasons; nsplit below / at / above the column-tile count for knn_radii and pr_flags; the lpips_chunks and qz_blocks caps; each C of
lpips_layer for each T.

Fixed with this suite: png_quantize (csrc/tokenizer_eval.hip) promised `127.5 x + 128` with product and sum rounded separately, as torch
evaluates the expression, and spelled that __fadd_rn(__fmul_rn(..)); the HIP headers define both as plain operators, so the compiler
contracted them into one v_fma (v_fmamk_f32 in the kernel's assembly).  Found by test_quantize_and_sse[hw255]: 132 of 1530 bytes one level
low, all of them at inputs (k - 128) / 127.5, where the product is an integer but for its rounding.  The function now states the two
operations under `#pragma clang fp contract(off)`.  Effect on reported numbers: none on the bytes of 2e7 uniform random inputs, none on any
of the 256 values k / 127.5 - 1 or (k / 255 - 0.5) / 0.5 an 8-bit image decodes to (there 127.5 x + 128 = k + 1/2, far from an integer);
63 of the 256 values (k - 128) / 127.5 move up one level, to what torch gives.  PSNR and rFID of real reconstructions do not move.
First device run (MI355X), before the fix: 104 of the then 113 cases ran, 103 inside their bounds with every rerun bitwise equal and no canary
touched, and test_quantize_and_sse[hw255] failed as described above.  With the fix and the LPIPS head, SSIM and refused-call cases added: 132
parametrised cases plus the 38 refused calls, all passing with zero excluded elements other than the undecided flags (0.05 % of u_in in case
g257x193_D20_nk8, none in any other case), every refused call inert; the module takes 2.0 s (2.7 s with
collection; the slowest cases are the two chunk-cap cases at 0.55 s, then the first one, which loads the library).
Worst err / bound per family and output:
  conv vec 0.079, scalar 0.065; avg pool 0.47; global_avgpool 0.05; fid_preprocess 0.16; fid_stats sum 0.33, cross 0.33
  row_sqnorms 0.99; logits vec 0.24, scalar 0.30; knn radii 1.00; pr_flags: no decided flag wrong, <= 0.05 % undecided
  softmax_is p 0.38, h 0.08, S 0.33; lpips_prep f32 0.92, f16 1.00; lpips_layer 0.007 .. 0.052; ssim 0.046
  bit exact, no ratio: max pool, adm_preprocess, adm_spatial_tap, quantiser, both SSE paths, the zero channels of lpips_prep, equal halves
  of lpips_layer, the constant image of ssim, ReLU zeros.
Ratios near 1, from the code: row_sqnorms and lpips_prep[f16] are one correctly rounded conversion of a (nearly) exact value, so half an ulp of
the output IS the bound and some element among hundreds takes all of it; lpips_prep[f32] is two roundings and nothing else (0.92 of 2 u
relative).  knn radii: index 0 is the self-distance, reference exactly 0, interval [0, e]; the kernel's clamped 0 sits on the interval's lower
end, which counts as ratio 1 of the half width.
Ratios far below 1: lpips_layer and ssim propagate worst-case roundings through chains of 64 .. 512 (22) terms and, for ssim, through the
cancellation m2 - m0^2; real roundings average out.  The bounds (2e-6 .. 9e-6 absolute for lpips_layer, 2e-5 .. 5e-5 for ssim) are still
per image, derived, and tight enough that the planted faults of test_eval_check_cpu.py fail them.
"""
import math

import numpy as np
import pytest
import torch

import eval_check as ec
from test_gpu_attention_paths import Guard, _bits

pytestmark = pytest.mark.gpu

F32, F16, F64 = torch.float32, torch.float16, torch.float64
U8, I32, I64 = torch.uint8, torch.int32, torch.int64
RATIOS: dict = {}
NCASES = [0]


@pytest.fixture(scope="module")
def lib():
    import time
    from ldmae_amd import _lib
    assert _lib.load().ldmae_arch() == b"gfx950"
    t0 = time.time()
    yield _lib
    if RATIOS:
        print(f"\n{NCASES[0]} cases; module wall time {time.time() - t0:.1f} s; worst |got - ref| / bound per path and output:")
        for k in sorted(RATIOS):
            print(f"  {k:44s} {RATIOS[k]:.3f}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _record(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)


def _gen(name):
    return torch.Generator().manual_seed(9000 + sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003)


def _ids(cases):
    return [c["name"] for c in cases]


def _p(g):
    return None if g is None else g.ptr()


# payload per type: (integer view, bits)
_SENT = {F32: (torch.int32, 0x7FC0DEAD), F16: (torch.int16, 0x7E5A), F64: (I64, 0x7FF8DEAD0DEAD0DE), U8: (U8, 0xA5), I32: (I32, -0x0DEAD0DE),
         I64: (I64, -0x0DEAD0DEAD0DEAD)}


class SGuard:
    """Guard for any element type, with an optional offset of `off` elements from the 256-B aligned start of the tensor's slot: the tensor
    sits between payload runs (NaN payload for floating types, a sentinel for integers) and is pre-filled with the payload."""

    def __init__(self, shape, dtype, init=None, off=0, front=128, back=2048):
        it, bits = _SENT[dtype]
        n = math.prod(shape)
        self.it, self.bits, self.n, self.front = it, bits, n, front + off
        self.buf = torch.empty(front + off + n + back, dtype=dtype, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.buf.view(it).fill_(bits)
        self.t = self.buf[self.front:self.front + n].view(shape)
        if init is not None:
            self.t.copy_(init)

    def intact(self):
        b = self.buf.view(self.it)
        return bool((b[:self.front] == self.bits).all() and (b[self.front + self.n:] == self.bits).all())

    def untouched(self, view):
        return bool((view.contiguous().view(self.it) == self.bits).all())

    def ptr(self):
        return self.t.data_ptr()


def _ws(nbytes):
    """A workspace of exactly `nbytes` inside a canary (256-B aligned start)."""
    assert nbytes > 0 and nbytes % 4 == 0
    return SGuard((nbytes // 4,), F32, front=128)


def _raw(t):
    return _bits(t) if t.dtype in (F32, F16) else t.contiguous().view(_SENT[t.dtype][0]) if t.is_floating_point() else t


def _twice(run):
    a = run()
    b = run()
    for n in a:
        assert torch.equal(_raw(a[n]), _raw(b[n])), f"{n}: rerun not bitwise equal"
    return a


def _chk(path, name, out, got, ref, bound):
    assert ec.finite(ref, bound), f"{name} {out}: reference or bound not finite"
    _record(f"{path}:{out}", ec.check(f"{name} {out}", got.cpu(), ref, bound))


def _same(name, got, want):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f"{name}: shape / dtype {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    eq = _raw(got) == _raw(want)
    assert bool(eq.all()), f"{name}: {int((~eq).sum())} of {eq.numel()} elements differ in their bits"


def _sliced(shape_full, off, C, data, dtype=F32, shift=0):
    """A [..., ld] guarded tensor whose channels [off, off + C) hold `data` and whose other channels keep the payload."""
    g = SGuard(shape_full, dtype, off=shift)
    g.t[..., off:off + C] = data.cuda()
    return g


def _rest_untouched(g, off, C):
    ld = g.t.shape[-1]
    return g.untouched(g.t[..., :off]) and g.untouched(g.t[..., off + C:]) if ld > C else True


# ============================================================================= convolution
def CV(name, B, H, W, Cin, Cout, kh, kw, sh=1, sw=1, ph=0, pw=0, relu=0, bias=1, ldx=None, xoff=0, ldo=None, ooff=0, xshift=0, wshift=0):
    return dict(name=name, B=B, H=H, W=W, Cin=Cin, Cout=Cout, kh=kh, kw=kw, sh=sh, sw=sw, ph=ph, pw=pw, relu=relu, bias=bias,
                ldx=ldx or Cin + xoff, xoff=xoff, ldo=ldo or Cout + ooff, ooff=ooff, xshift=xshift, wshift=wshift)


CONV = [
    CV("M1_cin4_cout1", 1, 3, 3, 4, 1, 3, 3),
    CV("M126_two_images_cin8_cout63", 2, 9, 7, 8, 63, 3, 3, ph=1, pw=1, relu=1),
    CV("M128_1x1_cin16_cout64", 2, 8, 8, 16, 64, 1, 1, bias=0),
    CV("M330_cin12_cout65", 3, 10, 11, 12, 65, 3, 3, ph=1, pw=1, relu=1, bias=0),
    CV("1x7_cin20_cout96", 2, 5, 9, 20, 96, 1, 7, pw=3, relu=1),
    CV("7x1_cin32_cout64", 2, 9, 5, 32, 64, 7, 1, ph=3),
    CV("5x5_cin4_cout65", 2, 7, 6, 4, 65, 5, 5, ph=2, pw=2, relu=1),
    CV("stem_cin3_s2_odd", 2, 10, 9, 3, 63, 3, 3, sh=2, sw=2, relu=1),
    CV("cin5_3x3", 1, 6, 7, 5, 8, 3, 3, ph=1, pw=1, ldx=8),
    CV("xoff2_cin8", 1, 6, 6, 8, 16, 3, 3, ph=1, pw=1, ldx=16, xoff=2, relu=1),
    CV("ldx7_cin4", 1, 6, 5, 4, 16, 3, 3, ph=1, pw=1, ldx=7),
    CV("x_plus4B_cin8", 1, 6, 6, 8, 16, 3, 3, ph=1, pw=1, xshift=1, relu=1),
    CV("w_plus4B_cin8", 1, 6, 6, 8, 16, 3, 3, ph=1, pw=1, wshift=1, bias=0),
    CV("s2_odd_cin16", 2, 8, 10, 16, 64, 3, 3, sh=2, sw=2, ph=1, pw=1, relu=1),
    CV("sh1_sw2_cin8", 2, 7, 9, 8, 32, 3, 3, sh=1, sw=2, ph=1, pw=1),
    CV("sh2_sw1_cin4", 1, 9, 6, 4, 8, 3, 3, sh=2, sw=1, ph=1, pw=1, relu=1),
    CV("ph0_pw1_cin4", 2, 6, 6, 4, 8, 3, 3, ph=0, pw=1),
    CV("ph2_pw0_5x1_cin8", 1, 5, 4, 8, 8, 5, 1, ph=2, pw=0, relu=1),
    CV("kernel_over_image_cin12", 2, 2, 5, 12, 24, 3, 3, ph=1, pw=1),
    CV("slices_cin8_cout63", 2, 6, 7, 8, 63, 3, 3, ph=1, pw=1, ldx=24, xoff=8, ldo=80, ooff=7, relu=1),
    CV("slices_cin3_cout65", 1, 12, 12, 3, 65, 3, 3, ldx=5, xoff=1, ldo=70, ooff=5, bias=0, relu=1),
    CV("s2_slices_cin16", 2, 9, 9, 16, 96, 3, 3, sh=2, sw=2, ldx=32, xoff=16, ldo=96, ooff=0),
]


def conv_vec_reasons(c):
    """The five conjuncts of `vec` in ldmae_conv2d_nhwc_f32, as the case makes them (the buffers start 256-B aligned)."""
    return dict(cin=c["Cin"] % 4 == 0, xoff=c["xoff"] % 4 == 0, ldx=c["ldx"] % 4 == 0, x_al=c["xshift"] % 4 == 0, w_al=c["wshift"] % 4 == 0)


def conv_M(c):
    Ho, Wo = ec.conv_out(c["H"], c["W"], c["kh"], c["kw"], c["sh"], c["sw"], c["ph"], c["pw"])
    return c["B"] * Ho * Wo


def conv_inputs(c):
    g = _gen("conv" + c["name"])
    x = torch.randn(c["B"], c["H"], c["W"], c["Cin"], generator=g)
    w = torch.randn(c["Cout"], c["kh"], c["kw"], c["Cin"], generator=g) / math.sqrt(c["kh"] * c["kw"] * c["Cin"])
    b = 0.5 * torch.randn(c["Cout"], generator=g) if c["bias"] else None
    return x, w, b


def conv_reference(c):
    x, w, b = conv_inputs(c)
    return ec.conv_ref(x, w, b, c["sh"], c["sw"], c["ph"], c["pw"], c["relu"])


@pytest.mark.parametrize("c", CONV, ids=_ids(CONV))
def test_conv2d(lib, c):
    x, w, b = conv_inputs(c)
    B, H, W, Cin, Cout = c["B"], c["H"], c["W"], c["Cin"], c["Cout"]
    Ho, Wo = ec.conv_out(H, W, c["kh"], c["kw"], c["sh"], c["sw"], c["ph"], c["pw"])
    Gx = _sliced((B, H, W, c["ldx"]), c["xoff"], Cin, x, shift=c["xshift"])
    Gw = SGuard((Cout, c["kh"] * c["kw"] * Cin), F32, w.reshape(Cout, -1).cuda(), off=c["wshift"])
    Gb = Guard((Cout,), F32, b.cuda()) if b is not None else None
    assert (Gx.ptr() % 16 == 0) == (c["xshift"] % 4 == 0) and (Gw.ptr() % 16 == 0) == (c["wshift"] % 4 == 0)

    def run():
        out = SGuard((B, Ho, Wo, c["ldo"]), F32)
        lib.call("ldmae_conv2d_nhwc_f32", Gx.ptr(), c["ldx"], c["xoff"], Gw.ptr(), _p(Gb), out.ptr(), c["ldo"], c["ooff"], B, H, W, Cin, Cout,
                 c["kh"], c["kw"], c["sh"], c["sw"], c["ph"], c["pw"], c["relu"], _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (out, Gx, Gw, Gb) if q is not None), "a canary changed"
        assert _rest_untouched(out, c["ooff"], Cout), "channels outside the output slice were written"
        return dict(out=out.t[..., c["ooff"]:c["ooff"] + Cout].clone())

    got = _twice(run)
    ref, bound, pre = conv_reference(c)
    path = "conv[vec]" if all(conv_vec_reasons(c).values()) else "conv[scalar]"
    _chk(path, c["name"], "out", got["out"], ref, bound)
    if c["relu"]:                                                   # ReLU zeros are exact zeros
        assert bool((_bits(got["out"].cpu())[pre + bound < 0] == 0).all()) and bool((got["out"] >= 0).all()), "ReLU left a non-zero"
    NCASES[0] += 1


# ============================================================================= pools
def PL(name, mode, B, H, W, C, k, s, p, ldx=None, xoff=0, ldo=None, ooff=0, neg=False):
    return dict(name=name, mode=mode, B=B, H=H, W=W, C=C, k=k, s=s, p=p, ldx=ldx or C + xoff, xoff=xoff, ldo=ldo or C + ooff, ooff=ooff, neg=neg)


POOL = []
for _m in (0, 1):
    _t = "max" if _m == 0 else "avg"
    POOL += [
        PL(f"{_t}_k3s1p1_c65", _m, 2, 5, 7, 65, 3, 1, 1),
        PL(f"{_t}_k3s2p0_c1", _m, 2, 8, 6, 1, 3, 2, 0),
        PL(f"{_t}_k1s1p0_slices", _m, 1, 3, 4, 7, 1, 1, 0, ldx=12, xoff=3, ldo=9, ooff=2),
        PL(f"{_t}_k2s2p0_c5", _m, 3, 7, 5, 5, 2, 2, 0),
        PL(f"{_t}_k5s1p2_slices", _m, 1, 4, 6, 9, 5, 1, 2, ldx=16, xoff=4, ldo=20, ooff=11),
    ]
POOL.append(PL("max_all_negative_k3s1p1", 0, 1, 4, 5, 3, 3, 1, 1, neg=True))


def pool_inputs(c):
    x = torch.randn(c["B"], c["H"], c["W"], c["C"], generator=_gen("pool" + c["name"]))
    return -1.0 - x.abs() if c["neg"] else x


def pool_total(c):
    Ho, Wo = (c["H"] + 2 * c["p"] - c["k"]) // c["s"] + 1, (c["W"] + 2 * c["p"] - c["k"]) // c["s"] + 1
    return c["B"] * Ho * Wo * c["C"]


@pytest.mark.parametrize("c", POOL, ids=_ids(POOL))
def test_pool2d(lib, c):
    x = pool_inputs(c)
    B, H, W, C, k, s, p = c["B"], c["H"], c["W"], c["C"], c["k"], c["s"], c["p"]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    Gx = _sliced((B, H, W, c["ldx"]), c["xoff"], C, x)

    def run():
        out = SGuard((B, Ho, Wo, c["ldo"]), F32)
        lib.call("ldmae_pool2d_nhwc_f32", c["mode"], Gx.ptr(), c["ldx"], c["xoff"], out.ptr(), c["ldo"], c["ooff"], B, H, W, C, k, s, p, _stream())
        torch.cuda.synchronize()
        assert out.intact() and Gx.intact(), "a canary changed"
        assert _rest_untouched(out, c["ooff"], C), "channels outside the output slice were written"
        return dict(out=out.t[..., c["ooff"]:c["ooff"] + C].clone())

    got = _twice(run)
    if c["mode"] == 0:
        _same(c["name"], got["out"], ec.maxpool_exact(x, k, s, p))
    else:
        _chk("pool[avg]", c["name"], "out", got["out"], *ec.avgpool_ref(x, k, s, p))
    NCASES[0] += 1


GAP = [dict(name="hw1", B=2, HW=1, C=5, ldx=5, xoff=0), dict(name="hw64_slice", B=3, HW=64, C=65, ldx=70, xoff=3),
       dict(name="hw289_slice", B=2, HW=289, C=7, ldx=8, xoff=1)]


@pytest.mark.parametrize("c", GAP, ids=_ids(GAP))
def test_global_avgpool(lib, c):
    B, HW, C = c["B"], c["HW"], c["C"]
    x = 0.5 + torch.randn(B, HW, C, generator=_gen("gap" + c["name"]))
    Gx = _sliced((B, HW, c["ldx"]), c["xoff"], C, x)

    def run():
        out = Guard((B, C), F32)
        lib.call("ldmae_global_avgpool_nhwc_f32", Gx.ptr(), c["ldx"], c["xoff"], out.ptr(), B, HW, C, _stream())
        torch.cuda.synchronize()
        assert out.intact() and Gx.intact(), "a canary changed"
        return dict(out=out.t.clone())

    _chk("global_avgpool", c["name"], "out", _twice(run)["out"], *ec.global_avgpool_ref(x))
    NCASES[0] += 1


# ============================================================================= pre-processing
FIDPRE = [dict(name="up", B=2, H=5, W=7, Ho=13, Wo=11), dict(name="down_over2", B=1, H=30, W=26, Ho=13, Wo=11),
          dict(name="identity", B=2, H=13, W=11, Ho=13, Wo=11), dict(name="one_pixel", B=1, H=1, W=1, Ho=4, Wo=3),
          dict(name="down_up_mixed", B=1, H=20, W=9, Ho=13, Wo=11), dict(name="up_over2", B=1, H=4, W=3, Ho=11, Wo=13)]
ADMPRE = FIDPRE[:4] + [dict(name="one_row", B=1, H=1, W=9, Ho=5, Wo=12), dict(name="clamp_last", B=2, H=3, W=3, Ho=7, Wo=7),
                       dict(name="down_up_mixed", B=1, H=20, W=9, Ho=13, Wo=11)]


def image_u8(c, tag):
    img = torch.randint(0, 256, (c["B"], c["H"], c["W"], 3), generator=_gen(tag + c["name"]), dtype=torch.int64).to(U8)
    img.view(-1)[0], img.view(-1)[-1] = 0, 255
    return img


def _preprocess(lib, entry, c, img):
    B, H, W, Ho, Wo = c["B"], c["H"], c["W"], c["Ho"], c["Wo"]
    Gi = SGuard((B, H, W, 3), U8, img.cuda())

    def run():
        out = Guard((B, Ho, Wo, 3), F32)
        lib.call(entry, Gi.ptr(), out.ptr(), B, H, W, Ho, Wo, _stream())
        torch.cuda.synchronize()
        assert out.intact() and Gi.intact(), "a canary changed"
        return dict(out=out.t.clone())

    return _twice(run)["out"]


@pytest.mark.parametrize("c", FIDPRE, ids=_ids(FIDPRE))
def test_fid_preprocess(lib, c):
    img = image_u8(c, "fidpre")
    _chk("fid_preprocess", c["name"], "out", _preprocess(lib, "ldmae_fid_preprocess", c, img), *ec.fid_preprocess_ref(img, c["Ho"], c["Wo"]))
    NCASES[0] += 1


@pytest.mark.parametrize("c", ADMPRE, ids=_ids(ADMPRE))
def test_adm_preprocess(lib, c):
    img = image_u8(c, "admpre")
    _same(c["name"], _preprocess(lib, "ldmae_adm_preprocess", c, img), torch.from_numpy(ec.adm_preprocess_f32(img.numpy(), c["Ho"], c["Wo"])))
    NCASES[0] += 1


def test_adm_spatial_tap(lib):
    B, HW, C, ldx, xoff = 2, 9, 7, 12, 3
    x = torch.randn(B, HW, C, generator=_gen("tap"))
    Gx = _sliced((B, HW, ldx), xoff, C, x)

    def run():
        out = Guard((B, HW * C), F32)
        lib.call("ldmae_adm_spatial_tap", Gx.ptr(), ldx, xoff, out.ptr(), B, HW, C, _stream())
        torch.cuda.synchronize()
        assert out.intact() and Gx.intact(), "a canary changed"
        return dict(out=out.t.clone())

    _same("spatial_tap", _twice(run)["out"], x.reshape(B, HW * C))
    NCASES[0] += 1


# ============================================================================= feature statistics
STATS = [dict(name=f"D{D}_n{n}", D=D, n=n, n2=n2) for D, n, n2 in ((1, 1, 16), (63, 15, 1), (64, 16, 17), (65, 17, 15), (200, 50, 17), (65, 50, 1))]


def stats_inputs(c):
    g = _gen("stats" + c["name"])
    D = c["D"]
    f1, f2 = 0.3 + torch.randn(c["n"], D, generator=g), 0.3 + torch.randn(c["n2"], D, generator=g)
    shift = 0.3 + 0.1 * torch.randn(D, generator=g)
    s0 = torch.randn(D, generator=g, dtype=F64)
    a = torch.randn(D, D, generator=g, dtype=F64)
    return f1, f2, shift, s0, a + a.T


@pytest.mark.parametrize("c", STATS, ids=_ids(STATS))
def test_fid_stats(lib, c):
    f1, f2, shift, s0, c0 = stats_inputs(c)
    D = c["D"]
    G1, G2, Gs = Guard(tuple(f1.shape), F32, f1.cuda()), Guard(tuple(f2.shape), F32, f2.cuda()), Guard((D,), F32, shift.cuda())

    def run():
        sm, cr = SGuard((D,), F64, s0.cuda()), SGuard((D, D), F64, c0.cuda())
        lib.call("ldmae_fid_stats_accumulate", G1.ptr(), c["n"], D, Gs.ptr(), sm.ptr(), cr.ptr(), _stream())
        torch.cuda.synchronize()
        one = dict(sum1=sm.t.clone(), cross1=cr.t.clone())
        lib.call("ldmae_fid_stats_accumulate", G2.ptr(), c["n2"], D, Gs.ptr(), sm.ptr(), cr.ptr(), _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (sm, cr, G1, G2, Gs)), "a canary changed"
        return dict(one, sum2=sm.t.clone(), cross2=cr.t.clone())

    got = {k: v.cpu().numpy() for k, v in _twice(run).items()}
    r1 = ec.fid_stats_ref(f1.numpy(), shift.numpy(), s0.numpy(), c0.numpy())
    # the second call accumulates into what the first one left: its reference starts from the first call's own output
    r2 = ec.fid_stats_ref(f2.numpy(), shift.numpy(), got["sum1"], got["cross1"])
    for tag, r in (("1", r1), ("2", r2)):
        _record("fid_stats:sum", ec.check64(f"{c['name']} sum{tag}", got["sum" + tag], *r["sum"]))
        _record("fid_stats:cross", ec.check64(f"{c['name']} cross{tag}", got["cross" + tag], *r["cross"]))
        cr = got["cross" + tag]
        assert (cr.view(np.int64) == cr.T.copy().view(np.int64)).all(), "cross is not bitwise symmetric"
    NCASES[0] += 1


# ============================================================================= row norms, pairwise logits
SQN = [dict(name=f"M{M}_D{D}", M=M, D=D) for M, D in ((1, 1), (4, 63), (5, 64), (4, 65), (5, 2023), (1, 2023))]


@pytest.mark.parametrize("c", SQN, ids=_ids(SQN))
def test_row_sqnorms(lib, c):
    M, D = c["M"], c["D"]
    x = torch.randn(M, D, generator=_gen("sqn" + c["name"]))
    Gx = Guard((M, D), F32, x.cuda())

    def run():
        out = Guard((M,), F32)
        lib.call("ldmae_row_sqnorms_f32", Gx.ptr(), M, D, out.ptr(), _stream())
        torch.cuda.synchronize()
        assert out.intact() and Gx.intact(), "a canary changed"
        return dict(out=out.t.clone())

    _chk("row_sqnorms", c["name"], "out", _twice(run)["out"], *ec.row_sqnorms_ref(x))
    NCASES[0] += 1


def PW(name, M, N, D, uoff=0, woff=0):
    return dict(name=name, M=M, N=N, D=D, uoff=uoff, woff=woff)


LOGITS = [PW("M1_N1_D1", 1, 1, 1), PW("M127_N63_D3", 127, 63, 3), PW("M128_N64_D4", 128, 64, 4), PW("M129_N65_D15", 129, 65, 15),
          PW("M300_N130_D16", 300, 130, 16), PW("M5_N3_D17", 5, 3, 17), PW("M129_N130_D20", 129, 130, 20), PW("M127_N65_D36", 127, 65, 36),
          PW("u_plus4B_D16", 128, 64, 16, uoff=1), PW("w_plus4B_D20", 5, 65, 20, woff=1)]


def pair_vec_reasons(D, uoff, voff):
    """The three conjuncts of `vec` in launch_pairwise."""
    return dict(d=D % 4 == 0, u_al=uoff % 4 == 0, v_al=voff % 4 == 0)


def logits_inputs(c):
    g = _gen("logits" + c["name"])
    return torch.randn(c["M"], c["D"], generator=g), torch.randn(c["N"], c["D"], generator=g)


@pytest.mark.parametrize("c", LOGITS, ids=_ids(LOGITS))
def test_pairwise_logits(lib, c):
    u, w = logits_inputs(c)
    M, N, D = c["M"], c["N"], c["D"]
    Gu, Gw = SGuard((M, D), F32, u.cuda(), off=c["uoff"]), SGuard((N, D), F32, w.cuda(), off=c["woff"])

    def run():
        out = Guard((M, N), F32)
        lib.call("ldmae_pairwise_logits", Gu.ptr(), M, D, Gw.ptr(), N, out.ptr(), _stream())
        torch.cuda.synchronize()
        assert out.intact() and Gu.intact() and Gw.intact(), "a canary changed"
        return dict(out=out.t.clone())

    path = "logits[vec]" if all(pair_vec_reasons(D, c["uoff"], c["woff"]).values()) else "logits[scalar]"
    _chk(path, c["name"], "out", _twice(run)["out"], *ec.logits_ref(u, w))
    NCASES[0] += 1


# ============================================================================= k-NN radii
def col_tiles(N):
    return (N + 63) // 64


def nsplit_set(N):
    """nsplit 1, 2, the column-tile count and a value above it."""
    return sorted({1, 2, col_tiles(N), col_tiles(N) + 3})


KNN = [dict(name="N8_D3_all", N=8, D=3, nhood=(0, 1, 2, 3, 4, 5, 6, 7), off=0), dict(name="N65_D7_all", N=65, D=7, nhood=(7, 0, 5, 2, 1, 3, 4, 6), off=0),
       dict(name="N129_D20_nk1", N=129, D=20, nhood=(3,), off=0), dict(name="N200_D36_all", N=200, D=36, nhood=(0, 1, 2, 3, 4, 5, 6, 7), off=0),
       dict(name="N6_D20_kmax5", N=6, D=20, nhood=(5,), off=0), dict(name="N129_D20_plus4B", N=129, D=20, nhood=(0, 4, 7), off=1)]


def norms_f32(x):
    """|x_i|^2 from the f64 reference, rounded to f32 once (not the kernel's output)."""
    return (x.double() ** 2).sum(-1).float()


def knn_inputs(c):
    x = torch.randn(c["N"], c["D"], generator=_gen("knn" + c["name"]))
    x[1] = x[0]                                                     # duplicated rows: distance 0 next to the self-distance
    if c["N"] > 70:
        x[70] = x[0]
        x[c["N"] - 1] = x[5]
    return x, norms_f32(x)


@pytest.mark.parametrize("c", KNN, ids=_ids(KNN))
def test_knn_radii(lib, c):
    x, nrm = knn_inputs(c)
    N, D, nh = c["N"], c["D"], c["nhood"]
    nk = len(nh)
    Gx, Gn = SGuard((N, D), F32, x.cuda(), off=c["off"]), Guard((N,), F32, nrm.cuda())
    nhood = (torch.ones(8, dtype=I32) * 99)
    nhood[:nk] = torch.tensor(nh, dtype=I32)
    d, e = ec.pair_dist(x, nrm, x, nrm)
    lo, hi = ec.knn_interval(d, e, nh)
    first = None
    for ns in nsplit_set(N):
        nbytes = lib.load().ldmae_knn_partials_bytes(N, ns)
        assert nbytes == N * ns * 2 * 8 * 4

        def run():
            part, rad = _ws(nbytes), Guard((N, nk), F32)
            lib.call("ldmae_knn_radii", Gx.ptr(), Gn.ptr(), N, D, nhood.numpy().ctypes.data, nk, ns, part.ptr(), rad.ptr(), _stream())
            torch.cuda.synchronize()
            assert all(q.intact() for q in (part, rad, Gx, Gn)), "a canary changed"
            return dict(radii=rad.t.clone())

        got = _twice(run)["radii"]
        if first is None:
            first = got
            path = "knn[vec]" if all(pair_vec_reasons(D, c["off"], c["off"]).values()) else "knn[scalar]"
            _record(f"{path}:radii", ec.check_interval(c["name"], got.cpu(), lo, hi))
        else:
            _same(f"{c['name']} nsplit {ns} against nsplit 1", got, first)
    NCASES[0] += 1


# ============================================================================= precision / recall flags
def PR(name, M, N, D, nhood, kind="gauss", off=0):
    return dict(name=name, M=M, N=N, D=D, nhood=nhood, kind=kind, off=off)


PRF = [PR("g131x70_D3_nk1", 131, 70, 3, (3,)), PR("g131x150_D7_nk2", 131, 150, 7, (1, 4)), PR("g257x193_D20_nk8", 257, 193, 20, (0, 1, 2, 3, 4, 5, 6, 7)),
       PR("g5x3_D3_nk2", 5, 3, 3, (1, 2)), PR("g300x129_D8_nk2", 300, 129, 8, (2, 5)), PR("g131x70_D20_plus4B", 131, 70, 20, (3,), off=1),
       PR("int131x70_D3_nk2", 131, 70, 3, (1, 3), kind="int"), PR("int5x3_D4_nk1", 5, 3, 4, (1,), kind="int"),
       PR("int257x193_D8_nk8", 257, 193, 8, (0, 1, 2, 3, 4, 5, 6, 7), kind="int"),
       PR("far131x70_D7_all0", 131, 70, 7, (1, 4), kind="far")]


def pr_inputs(c):
    """-> u, nu, ru, v, nv, rv: rows, f32 norms from the f64 reference, radii from the f64 k-NN of each set rounded to f32."""
    g = _gen("pr" + c["name"])
    M, N, D = c["M"], c["N"], c["D"]
    if c["kind"] == "int":                                          # small integers: every product, sum and distance is exact in f32 (e = 0)
        u = torch.randint(-3, 4, (M, D), generator=g).float()
        v = torch.randint(-3, 4, (N, D), generator=g).float()
    else:
        cen = torch.randn(6, D, generator=g)
        u = cen[torch.randint(0, 6, (M,), generator=g)] + 0.3 * torch.randn(M, D, generator=g)
        v = cen[torch.randint(0, 6, (N,), generator=g)] + 0.3 * torch.randn(N, D, generator=g)
        if c["kind"] == "far":
            v = v + 40.0
    if M < 10:                                                      # two outliers, so that even the smallest case has flags of both values
        u[0], v[0] = 100.0, -10.0
    def radii(x):
        X = x.double()
        dd = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1).sort(-1).values
        r = dd[:, torch.tensor(c["nhood"])].float()
        return r
    return u, norms_f32(u), radii(u), v, norms_f32(v), radii(v)


def pr_reference(c):
    """-> (u1, u0, v1, v0): flags that must be 1 / must be 0."""
    u, nu, ru, v, nv, rv = pr_inputs(c)
    if c["kind"] == "int":
        d = ((u.double()[:, None, :] - v.double()[None, :, :]) ** 2).sum(-1)
        return ec.pr_decide(d, torch.zeros_like(d), rv, ru)
    d, e = ec.pair_dist(u, nu, v, nv)
    return ec.pr_decide(d, e, rv, ru)


@pytest.mark.parametrize("c", PRF, ids=_ids(PRF))
def test_pr_flags(lib, c):
    u, nu, ru, v, nv, rv = pr_inputs(c)
    M, N, D, nk = c["M"], c["N"], c["D"], len(c["nhood"])
    Gu, Gv = SGuard((M, D), F32, u.cuda(), off=c["off"]), SGuard((N, D), F32, v.cuda(), off=c["off"])
    Gnu, Gnv, Gru, Grv = Guard((M,), F32, nu.cuda()), Guard((N,), F32, nv.cuda()), Guard((M, nk), F32, ru.cuda()), Guard((N, nk), F32, rv.cuda())
    u1, u0, v1, v0 = pr_reference(c)
    first = None
    for ns in nsplit_set(N):
        def run():
            fu, fv = SGuard((M, nk), I32), SGuard((N, nk), I32)
            fu.t.zero_()
            fv.t.zero_()
            lib.call("ldmae_pr_flags", Gu.ptr(), Gnu.ptr(), Gru.ptr(), M, Gv.ptr(), Gnv.ptr(), Grv.ptr(), N, D, nk, ns, fu.ptr(), fv.ptr(), _stream())
            torch.cuda.synchronize()
            assert all(q.intact() for q in (fu, fv, Gu, Gv, Gnu, Gnv, Gru, Grv)), "a canary changed"
            return dict(u_in=fu.t.clone(), v_in=fv.t.clone())

        got = _twice(run)
        path = "pr[vec]" if all(pair_vec_reasons(D, c["off"], c["off"]).values()) else "pr[scalar]"
        cap = 0.0 if c["kind"] == "int" else 0.01
        _record(f"{path}:undecided u_in", ec.check_flags(f"{c['name']} u_in nsplit {ns}", got["u_in"].cpu(), u1, u0, cap))
        _record(f"{path}:undecided v_in", ec.check_flags(f"{c['name']} v_in nsplit {ns}", got["v_in"].cpu(), v1, v0, cap))
        if c["kind"] == "far":
            assert not bool(got["u_in"].any()) and not bool(got["v_in"].any())
        if first is None:
            first = got
        else:
            _same(f"{c['name']} u_in nsplit {ns}", got["u_in"], first["u_in"])
            _same(f"{c['name']} v_in nsplit {ns}", got["v_in"], first["v_in"])
    NCASES[0] += 1


# ============================================================================= softmax + Inception Score sums
IS_CASES = [dict(name=f"M{M}_C{C}_split{s}", M=M, C=C, split=s) for M, C, s in
            ((1, 1, 1), (127, 255, 100), (128, 256, 128), (129, 257, 129), (300, 1008, 500), (300, 257, 129), (300, 255, 100), (5, 1008, 1))]


def is_inputs(c):
    M, C = c["M"], c["C"]
    x = 3.0 * torch.randn(M, C, generator=_gen("is" + c["name"]))
    if C > 1:
        x[0, C // 2] = x[0].max() - 200.0                           # p = 0 exactly: the 0 log 0 := 0 branch
        if M > 1:
            x[1] = 1.25                                             # an all-equal row
        if M > 2:
            x[2, C - 1] = x[2].max() + 30.0                         # one-hot dominant
    return x


@pytest.mark.parametrize("c", IS_CASES, ids=_ids(IS_CASES))
def test_adm_softmax_is(lib, c):
    M, C, split = c["M"], c["C"], c["split"]
    x = is_inputs(c)
    Gx = Guard((M, C), F32, x.cuda())
    ns = (M + split - 1) // split
    nbytes = lib.load().ldmae_adm_is_workspace_bytes(M, C, split)
    assert nbytes == (M * C * 4 + 255) // 256 * 256 + ns * ((split + 127) // 128) * C * 8

    def run():
        ws, h, S = _ws(nbytes), SGuard((M,), F64), SGuard((ns, C), F64)
        lib.call("ldmae_adm_softmax_is", Gx.ptr(), M, C, split, ws.ptr(), h.ptr(), S.ptr(), _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (ws, h, S, Gx)), "a canary changed"
        return dict(p=ws.t[:M * C].view(M, C).clone(), h=h.t.clone(), S=S.t.clone())

    got = _twice(run)
    ref = ec.softmax_is_ref(x, split)
    _chk("softmax_is", c["name"], "p", got["p"], *ref["p"])
    _record("softmax_is:h", ec.check64(f"{c['name']} h", got["h"].cpu().numpy(), *ref["h"]))
    _record("softmax_is:S", ec.check64(f"{c['name']} S", got["S"].cpu().numpy(), *ref["S"]))
    if C > 1:
        assert float(got["p"][0, C // 2]) == 0.0, "the case no longer reaches p == 0"
    NCASES[0] += 1


# ============================================================================= LPIPS pre-processing
LPREP = [dict(name="B1_5x7", B=1, H=5, W=7), dict(name="B2_9x13", B=2, H=9, W=13), dict(name="B3_16x16", B=3, H=16, W=16)]


def lprep_inputs(c):
    g = _gen("lprep" + c["name"])
    a, b = torch.randn(c["B"], 3, c["H"], c["W"], generator=g), torch.randn(c["B"], 3, c["H"], c["W"], generator=g)
    a.view(-1)[:4] = torch.tensor([4.0e4, -4.0e4, 29300.0, 0.0])    # beyond +-65504 after the division: the f16 form saturates
    return a, b


@pytest.mark.parametrize("c", LPREP, ids=_ids(LPREP))
@pytest.mark.parametrize("T", (F32, F16), ids=("f32", "f16"))
def test_lpips_prep(lib, c, T):
    a, b = lprep_inputs(c)
    B, H, W = c["B"], c["H"], c["W"]
    ch = 4 if T == F32 else 8
    Ga, Gb = Guard((B, 3, H, W), F32, a.cuda()), Guard((B, 3, H, W), F32, b.cuda())

    def run():
        out = Guard((2 * B, H, W, ch), T)
        lib.call("ldmae_lpips_prep" if T == F32 else "ldmae_lpips_prep_f16", Ga.ptr(), Gb.ptr(), out.ptr(), B, H, W, _stream())
        torch.cuda.synchronize()
        assert out.intact() and Ga.intact() and Gb.intact(), "a canary changed"
        return dict(out=out.t.clone())

    got = _twice(run)["out"]
    _chk(f"lpips_prep[{'f32' if T == F32 else 'f16'}]", c["name"], "out", got[..., :3], *ec.lpips_prep_ref(a, b, T))
    _same(c["name"] + " zero channels", got[..., 3:], torch.zeros(2 * B, H, W, ch - 3, dtype=T))
    if T == F16:
        assert float(got[0, 0, 0, 0]) == 65504.0 and float(got[0, 0, 1, 0]) == -65504.0, "the case no longer saturates"
    NCASES[0] += 1


# ============================================================================= quantiser + SSE
QZ = [dict(name="hw1", B=2, H=1, W=1, kind="rand"), dict(name="hw255", B=2, H=5, W=51, kind="rand"), dict(name="hw1025", B=3, H=25, W=41, kind="rand"),
      dict(name="hw513x513_cap", B=1, H=513, W=513, kind="rand"), dict(name="all255", B=2, H=5, W=51, kind="all255")]
QZ_EDGE = (-1.0, 1.0, -1.0039216, 0.9960785, 0.0, -2.0, 3.0, 127.0 / 127.5 - 1.0, 1.0 / 255.0, -0.5, 0.5, 1e-8)


def qz_blocks(n):
    return min(256, max(1, (n + 1023) // 1024))


def qz_capped(n):
    return (n + 1023) // 1024 > 256


def qz_inputs(c):
    g = _gen("qz" + c["name"])
    B, H, W = c["B"], c["H"], c["W"]
    if c["kind"] == "all255":
        return torch.full((B, 3, H, W), -2.0), torch.full((B, 3, H, W), 2.0)
    dec, ref = 1.1 * (2 * torch.rand(B, 3, H, W, generator=g) - 1), 1.1 * (2 * torch.rand(B, 3, H, W, generator=g) - 1)
    # exact half-way points of the quantiser and their f32 neighbours
    k = torch.randint(0, 256, (B, 3, H, W), generator=g).float()
    half = (k - 128.0) / 127.5
    dec = torch.where(torch.rand(B, 3, H, W, generator=g) < 0.3, half, dec)
    n = min(len(QZ_EDGE), dec.numel())
    dec.view(-1)[:n] = torch.tensor(QZ_EDGE)[:n]
    return dec, ref


@pytest.mark.parametrize("c", QZ, ids=_ids(QZ))
def test_quantize_and_sse(lib, c):
    dec, ref = qz_inputs(c)
    B, H, W = c["B"], c["H"], c["W"]
    HW = H * W
    Gd, Gr = Guard((B, 3, H, W), F32, dec.cuda()), Guard((B, 3, H, W), F32, ref.cuda())
    nbytes = lib.load().ldmae_sse_workspace_bytes(B, HW)
    assert nbytes == B * qz_blocks(HW) * 8
    want_d = np.ascontiguousarray(ec.quantize_f32(dec.numpy()).transpose(0, 2, 3, 1))
    want_r = np.ascontiguousarray(ec.quantize_f32(ref.numpy()).transpose(0, 2, 3, 1))
    want_sse = ec.sse_exact(want_d.reshape(B, -1), want_r.reshape(B, -1))

    def run():
        d8, r8, sse, ws = SGuard((B, H, W, 3), U8), SGuard((B, H, W, 3), U8), SGuard((B,), I64), _ws(nbytes)
        lib.call("ldmae_recon_quantize_psnr", Gd.ptr(), Gr.ptr(), d8.ptr(), r8.ptr(), sse.ptr(), B, H, W, ws.ptr(), _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (d8, r8, sse, ws, Gd, Gr)), "a canary changed"
        return dict(d8=d8.t.clone(), r8=r8.t.clone(), sse=sse.t.clone())

    got = _twice(run)
    _same(c["name"] + " dec8", got["d8"], torch.from_numpy(want_d))
    _same(c["name"] + " ref8", got["r8"], torch.from_numpy(want_r))
    _same(c["name"] + " sse", got["sse"], torch.from_numpy(want_sse))
    if c["kind"] == "all255":
        assert int(got["sse"][0]) == 255 * 255 * 3 * HW

    # the u8 path on the same bytes
    n = 3 * HW
    Ga, Gb = SGuard((B, n), U8, torch.from_numpy(want_d).reshape(B, n).cuda()), SGuard((B, n), U8, torch.from_numpy(want_r).reshape(B, n).cuda())
    nb2 = lib.load().ldmae_sse_workspace_bytes(B, n)
    assert nb2 == B * qz_blocks(n) * 8

    def run2():
        sse, ws = SGuard((B,), I64), _ws(nb2)
        lib.call("ldmae_sse_u8", Ga.ptr(), Gb.ptr(), sse.ptr(), B, n, ws.ptr(), _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (sse, ws, Ga, Gb)), "a canary changed"
        return dict(sse=sse.t.clone())

    _same(c["name"] + " sse_u8", _twice(run2)["sse"], torch.from_numpy(want_sse))
    NCASES[0] += 1


# ============================================================================= LPIPS head of one tap
def LL(name, T, C, h, w, B=2, equal=False):
    return dict(name=name, T=T, C=C, h=h, w=w, B=B, equal=equal)


LP_HW = ((1, 1), (1, 7), (17, 23), (19, 27))
LPL = []
for _j, _T in enumerate((F32, F16)):
    for _i, _C in enumerate((64, 128, 256, 512)):
        _h, _w = LP_HW[(_i + _j) % 4]
        LPL.append(LL(f"{'f32' if _T == F32 else 'f16'}_C{_C}_hw{_h * _w}", _T, _C, _h, _w))
    LPL.append(LL(f"{'f32' if _T == F32 else 'f16'}_C64_hw65792_cap", _T, 64, 257, 256, B=1))
LPL += [LL("f32_C128_equal_halves", F32, 128, 17, 23, equal=True), LL("f16_C512_equal_halves", F16, 512, 19, 27, equal=True),
        LL("f32_C64_hw513", F32, 64, 19, 27), LL("f16_C64_hw391", F16, 64, 17, 23), LL("f32_C512_hw1", F32, 512, 1, 1), LL("f16_C256_hw7", F16, 256, 1, 7)]


def lpips_capped(HW):
    return (HW + 511) // 512 > 128


def lpl_inputs(c):
    g = _gen("lpl" + c["name"])
    B, HW, C = c["B"], c["h"] * c["w"], c["C"]
    f = torch.randn(2 * B, HW, C, generator=g).to(c["T"])
    if HW >= 7:
        f[0, 1] = 0                                                 # an all-zero pixel in one half ...
        f[0, 2] = 0
        f[B, 2] = 0                                                 # ... and in both
        f[0, 3] = (1e-6 * torch.randn(C, generator=g)).to(c["T"])  # a pixel whose norm is near the 1e-10 of the denominator's scale
    if c["equal"]:
        f[B:] = f[:B]
    return f, torch.rand(C, generator=g), torch.randn(B, generator=g)


_LPL_REF: dict = {}


def lpl_reference(c):
    if c["name"] not in _LPL_REF:
        f, lw, old = lpl_inputs(c)
        _LPL_REF[c["name"]] = ec.lpips_layer_ref(f, lw, old, c["B"])
    return _LPL_REF[c["name"]]


@pytest.mark.parametrize("c", LPL, ids=_ids(LPL))
def test_lpips_layer(lib, c):
    f, lw, old = lpl_inputs(c)
    B, h, w, C, T = c["B"], c["h"], c["w"], c["C"], c["T"]
    Gf, Gw = Guard((2 * B, h * w, C), T, f.cuda()), Guard((C,), F32, lw.cuda())
    nbytes = lib.load().ldmae_lpips_workspace_bytes(B, h, w)
    assert nbytes == B * ec.lpips_chunks(h * w) * 4

    def run():
        out, ws = Guard((B,), F32, old.cuda()), _ws(nbytes)
        lib.call("ldmae_lpips_layer" if T == F32 else "ldmae_lpips_layer_f16", Gf.ptr(), Gw.ptr(), out.ptr(), B, h, w, C, ws.ptr(), _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (out, ws, Gf, Gw)), "a canary changed"
        return dict(out=out.t.clone())

    got = _twice(run)["out"]
    if c["equal"]:
        _same(c["name"] + ": equal halves add exactly 0", got, old)
    _chk(f"lpips_layer[{'f32' if T == F32 else 'f16'},C{C}]", c["name"], "out", got, *lpl_reference(c))
    NCASES[0] += 1


# ============================================================================= SSIM
def SS(name, B, C, H, W, lo=0.0, hi=1.0, dr=1.0, kind="rand", scale=1.0):
    return dict(name=name, B=B, C=C, H=H, W=W, lo=lo, hi=hi, dr=dr, kind=kind, scale=scale)


SSIM = [SS("11x12_c3", 2, 3, 11, 12), SS("12x11_c1", 1, 1, 12, 11), SS("42x43_c3", 1, 3, 42, 43), SS("43x42_c1_noclamp_dr2", 2, 1, 43, 42, lo=-10.0, hi=10.0, dr=2.0),
        SS("75x75_c1", 1, 1, 75, 75), SS("75x11_c3_b2", 2, 3, 75, 11), SS("11x75_c1_dr255", 1, 1, 11, 75, hi=255.0, dr=255.0, scale=255.0),
        SS("43x12_c3_constant", 1, 3, 43, 12, kind="const"), SS("12x75_c1_negated_constant", 1, 1, 12, 75, lo=-1.0, hi=1.0, dr=2.0, kind="negconst")]


def ssim_inputs(c):
    g = _gen("ssim" + c["name"])
    shape = (c["B"], c["C"], c["H"], c["W"])
    if c["kind"] == "const":
        X = torch.full(shape, 0.3)
        return X, X.clone()
    if c["kind"] == "negconst":
        X = torch.full(shape, 0.4)
        return X, -X
    X = (1.4 * torch.rand(shape, generator=g) - 0.2) * c["scale"]
    return X, X + 0.1 * c["scale"] * torch.randn(shape, generator=g)


def ssim_clamp_active(c):
    X, Y = ssim_inputs(c)
    return bool(((X < c["lo"]) | (X > c["hi"]) | (Y < c["lo"]) | (Y > c["hi"])).any())


_SSIM_REF: dict = {}


def ssim_reference(c):
    if c["name"] not in _SSIM_REF:
        X, Y = ssim_inputs(c)
        _SSIM_REF[c["name"]] = ec.ssim_ref(X, Y, c["lo"], c["hi"], c["dr"])
    return _SSIM_REF[c["name"]]


@pytest.mark.parametrize("c", SSIM, ids=_ids(SSIM))
def test_ssim(lib, c):
    X, Y = ssim_inputs(c)
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    Gx, Gy = Guard((B, C, H, W), F32, X.cuda()), Guard((B, C, H, W), F32, Y.cuda())
    nbytes = lib.load().ldmae_ssim_workspace_bytes(B, C, H, W)
    assert nbytes == B * C * ((H - 10 + 31) // 32) * ((W - 10 + 31) // 32) * 4

    def run():
        out, ws = Guard((B,), F32), _ws(nbytes)
        lib.call("ldmae_ssim", Gx.ptr(), Gy.ptr(), out.ptr(), B, C, H, W, c["lo"], c["hi"], c["dr"], ws.ptr(), _stream())
        torch.cuda.synchronize()
        assert all(q.intact() for q in (out, ws, Gx, Gy)), "a canary changed"
        return dict(out=out.t.clone())

    got = _twice(run)["out"]
    if c["kind"] == "const":
        _same(c["name"] + ": a constant image gives exactly 1", got, torch.ones(B))
    _chk("ssim", c["name"], "out", got, *ssim_reference(c))
    NCASES[0] += 1


# ============================================================================= refused calls
def test_refusals_are_loud_and_write_nothing(lib):
    """One call per LDMAE_REQUIRE of the three files (but `ssim: image too large`, which no H W below 2^31 reaches): an error code, a
    message, and every buffer as it was."""
    L = lib.load()
    A, Bf, Cf, D = Guard((4096,), F32), Guard((4096,), F32), Guard((4096,), F32), Guard((4096,), F32)
    a, b, o, w = A.ptr(), Bf.ptr(), Cf.ptr(), D.ptr()
    nh_ok, nh_bad = np.array([0, 3], dtype=np.int32), np.array([0, 8], dtype=np.int32)
    s = _stream()
    calls = [
        ("ldmae_conv2d_nhwc_f32", (a, 4, 0, b, None, o, 4, 0, 0, 4, 4, 4, 4, 3, 3, 1, 1, 1, 1, 0, s)),                 # B = 0
        ("ldmae_conv2d_nhwc_f32", (a, 4, 1, b, None, o, 4, 0, 1, 4, 4, 4, 4, 3, 3, 1, 1, 1, 1, 0, s)),                 # xoff + Cin > ldx
        ("ldmae_conv2d_nhwc_f32", (a, 4, 0, b, None, o, 4, 0, 1, 2, 4, 4, 4, 5, 3, 1, 1, 1, 1, 0, s)),                 # kernel over the padded image
        ("ldmae_conv2d_nhwc_f32", (a, 1, 0, b, None, o, 4, 0, 1, 4096, 4096, 1, 4, 4096, 4096, 1, 1, 0, 0, 0, s)),     # K = 2^24
        ("ldmae_pool2d_nhwc_f32", (0, a, 4, 0, o, 4, 0, 1, 4, 4, 4, 0, 1, 0, s)),                                       # k = 0
        ("ldmae_pool2d_nhwc_f32", (2, a, 4, 0, o, 4, 0, 1, 4, 4, 4, 3, 1, 1, s)),                                       # mode 2
        ("ldmae_pool2d_nhwc_f32", (0, a, 4, 0, o, 4, 1, 1, 4, 4, 4, 3, 1, 1, s)),                                       # ooff + C > ldo
        ("ldmae_pool2d_nhwc_f32", (1, a, 4, 0, o, 4, 0, 1, 2, 2, 4, 5, 1, 1, s)),                                       # window over the padded image
        ("ldmae_global_avgpool_nhwc_f32", (a, 4, 2, o, 1, 4, 4, s)),
        ("ldmae_fid_preprocess", (a, o, 0, 4, 4, 4, 4, s)),
        ("ldmae_fid_stats_accumulate", (a, 0, 4, b, o, w, s)),
        ("ldmae_adm_preprocess", (a, o, 1, 4, 4, 0, 4, s)),
        ("ldmae_adm_spatial_tap", (a, 4, 2, o, 1, 4, 4, s)),
        ("ldmae_row_sqnorms_f32", (a, 0, 4, o, s)),
        ("ldmae_pairwise_logits", (a, 4, 0, b, 4, o, s)),
        ("ldmae_knn_radii", (None, b, 8, 4, nh_ok.ctypes.data, 2, 1, o, w, s)),
        ("ldmae_knn_radii", (a, b, 8, 4, nh_ok.ctypes.data, 9, 1, o, w, s)),                                            # nk = 9
        ("ldmae_knn_radii", (a, b, 8, 4, nh_bad.ctypes.data, 2, 1, o, w, s)),                                           # index 8
        ("ldmae_knn_radii", (a, b, 3, 4, nh_ok.ctypes.data, 2, 1, o, w, s)),                                            # N <= kmax
        ("ldmae_pr_flags", (a, b, b, 4, a, b, b, 4, 4, 1, 1, None, w, s)),
        ("ldmae_pr_flags", (a, b, b, 4, a, b, b, 4, 4, 1, 0, o, w, s)),                                                 # nsplit = 0
        ("ldmae_adm_softmax_is", (a, 4, 4, 0, b, o, w, s)),                                                             # split = 0
        ("ldmae_adm_softmax_is", (a, 70000, 1, 1, b, o, w, s)),                                                         # 70000 chunks
        ("ldmae_lpips_prep", (a, b, o, 0, 4, 4, s)),
        ("ldmae_lpips_prep", (a, b, o + 4, 1, 4, 4, s)),                                                                # out not 16-B aligned
        ("ldmae_lpips_prep_f16", (a, b, o, 1, 0, 4, s)),
        ("ldmae_lpips_prep_f16", (a, b, o + 8, 1, 4, 4, s)),
        ("ldmae_lpips_layer", (a, b, o, 0, 2, 2, 64, w, s)),
        ("ldmae_lpips_layer", (a, b, o, 1, 2, 2, 96, w, s)),                                                            # C = 96
        ("ldmae_lpips_layer", (a + 4, b, o, 1, 2, 2, 64, w, s)),                                                        # features not 16-B aligned
        ("ldmae_lpips_layer_f16", (a, b + 4, o, 1, 2, 2, 64, w, s)),
        ("ldmae_ssim", (a, b, o, 0, 1, 11, 11, 0.0, 1.0, 1.0, w, s)),
        ("ldmae_ssim", (a, b, o, 1, 1, 10, 11, 0.0, 1.0, 1.0, w, s)),                                                   # below the 11 x 11 window
        ("ldmae_ssim", (a, b, o, 1, 1, 11, 11, 1.0, 0.0, 1.0, w, s)),                                                   # lo > hi
        ("ldmae_recon_quantize_psnr", (a, b, o, w, w + 2048, 0, 4, 4, w + 4096, s)),
        ("ldmae_recon_quantize_psnr", (a, b, o, w, w + 2052, 1, 4, 4, w + 4096, s)),                                    # sse not 8-B aligned
        ("ldmae_sse_u8", (a, b, o, 1, 0, w, s)),
        ("ldmae_sse_u8", (a, b, o, 1, 16, w + 4, s)),                                                                   # workspace not 8-B aligned
    ]
    for name, args in calls:
        rc = getattr(L, name)(*args)
        torch.cuda.synchronize()
        assert rc != 0, f"{name}{args[:-1]} was accepted"
        assert lib.last_error(), f"{name}: refused without a message"
        for q in (A, Bf, Cf, D):
            assert q.intact() and q.untouched(q.t), f"{name}: a refused call wrote to a buffer"
    assert L.ldmae_knn_partials_bytes(0, 1) == -1 and L.ldmae_knn_partials_bytes(4, 0) == -1 and L.ldmae_adm_is_workspace_bytes(4, 4, 0) == -1
    assert L.ldmae_ssim_workspace_bytes(1, 1, 10, 11) == 0
    NCASES[0] += len(calls)
