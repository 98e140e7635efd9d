"""Every dispatch path of the GEMM family, element by element, at ragged edges and strides.

A seeded table of cases drives the C ABI directly (ldmae_gemm_nt, ldmae_gemm_tn, ldmae_colsum, ldmae_thin_nt, ldmae_thin_tn), so each
case controls its leading dimensions, operand offsets and launch flags.  Each case
  - places every output inside a larger buffer filled with a NaN payload: columns [N, ld), rows past the last one and a tail; operands
    sit in NaN-padded buffers too, so a read past K, past the last row or past a slice's columns reaches a result as NaN;
  - checks every element against an f64 reference of the same rounded operands with the bound of tests/gemm_check.py, and every
    canary bit;
  - runs a second time and requires bitwise-equal results;
  - asserts which kernel family ran (ldmae_launch_counts) and, for TN, the split count it meant to reach.
test_case_table_covers_every_predicate keeps the table honest: every dispatch predicate (copied from the C dispatch) is both selected
and missed by some case.  The wrapper tests at the end pin the layout rules of ldmae_amd.ops."""
import pytest
import torch

import gemm_check as gc

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
EPI_BIAS, EPI_GATE_RES, EPI_BIAS_POS, EPI_BIAS_GELU, EPI_SWIGLU, EPI_SWIGLU_BWD, EPI_GELU_BWD = 0, 1, 2, 3, 4, 5, 6
TILE, HALF = 0x100, 0x200
_BITS = {F32: (torch.int32, 0x7FC0DEAD), BF16: (torch.int16, 0x7FDE), F16: (torch.int16, 0x7E5A)}
RATIOS: dict = {}


@pytest.fixture(scope="module")
def lib():
    from ldmae_amd import _lib
    assert _lib.load().ldmae_arch() == b"gfx950"
    yield _lib
    if RATIOS:
        print("\nworst |got - ref| / bound per path and output:")
        for k in sorted(RATIOS):
            print(f"  {k:40s} {RATIOS[k]:.3f}")


def _dt(dtype):
    return {F32: 0, BF16: 1, F16: 2}[dtype]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _record(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)


class Canvas:
    """A rows x cols tensor at row stride ld inside a buffer whose every other element holds the NaN payload of its dtype."""

    def __init__(self, rows, cols, ld, dtype, init=None, off=0):
        it, bits = _BITS[dtype]
        n = off + (rows + 3) * ld + 64
        self.dtype, self.bits, self.it = dtype, bits, it
        self.buf = torch.empty(n, dtype=dtype, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.buf.view(it).fill_(bits)
        self.t = self.buf[off:off + rows * ld].view(rows, ld)[:, :cols]
        self.mask = torch.ones(n, dtype=torch.bool, device="cuda")
        self.mask[off:off + rows * ld].view(rows, ld)[:, :cols] = False
        if init is not None:
            self.t.copy_(init)

    def intact(self):
        return bool((self.buf.view(self.it)[self.mask] == self.bits).all())


def _randn(rows, cols, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(rows, cols, device="cuda", generator=g) * scale


def operand(rows, cols, dtype, ld, seed, scale=1.0, off=0):
    """Operand in a NaN-padded buffer (row stride ld, first element `off` elements past a 256-B boundary)."""
    return Canvas(rows, cols, ld, dtype, _randn(rows, cols, seed, scale).to(dtype), off)


def lines_ok(epi, a, b, M, N, K, lda, ldb):
    """gemm_nt_lines.hip: lines_shape_ok."""
    if M < 8 or N < 8 or M % 8 or N % 8 or K % 64 or lda % 64 or ldb % 64:
        return False
    if a.data_ptr() % 128 or b.data_ptr() % 128:
        return False
    return not (epi == EPI_SWIGLU and N % 256)


def nfast(epi, N, ldc, rpb):
    """gemm_nt_common.h: the vector (fast) epilogue's condition."""
    return N % 8 == 0 and ldc % 8 == 0 and (epi != EPI_GATE_RES or rpb % 16 == 0)


# ----------------------------------------------------------------------------- the table
def _nt(name, dtype, M, N, K, out=None, epi=EPI_BIAS, **kw):
    return dict(kind="nt", name=name, dtype=dtype, out=out or dtype, M=M, N=N, K=K, epi=epi, **kw)


def _tn(name, dtype, M, N, K, **kw):
    return dict(kind="tn", name=name, dtype=dtype, M=M, N=N, K=K, **kw)


L10 = 256 * 41 + 8
CASES = [
    # NT f32 kernel (64x64x16 tiles): tiny / odd M and N, lda > K, ldc = N + 4, beta = 1, no bias, bf16 out
    _nt("f32_1x7x16", F32, 1, 7, 16),
    _nt("f32_7x1x48_lda", F32, 7, 1, 48, lda=52),
    _nt("f32_63x65x784_ldc", F32, 63, 65, 784, ldc=69, lda=800),
    _nt("f32_65x63x48_beta", F32, 65, 63, 48, beta=1.0, ldc=67),
    _nt("f32_200x200x784_nobias", F32, 200, 200, 784, bias=False),
    _nt("f32_200x200x16_beta_fast", F32, 200, 200, 16, beta=1.0),
    _nt("f32_200x7x16_bf16out", F32, 200, 7, 16, out=BF16, ldc=11),
    _nt("f32_1x200x48_bf16out", F32, 1, 200, 48, out=BF16),
    _nt("f32_65x200x48_bf16out_fast", F32, 65, 200, 48, out=BF16, lda=64),
    _nt("f32_gate_res", F32, 200, 65, 48, epi=EPI_GATE_RES, rpb=8, gate="ld", ldc=69),
    _nt("f32_gate_res_fast", F32, 192, 200, 48, epi=EPI_GATE_RES, rpb=16, gate="ld"),
    _nt("f32_pos", F32, 63, 200, 16, epi=EPI_BIAS_POS, rpb=21, ldc=204),
    _nt("f32_gelu", F32, 65, 63, 784, epi=EPI_BIAS_GELU, ldc=67),
    _nt("f32_gelu_bwd", F32, 200, 200, 48, epi=EPI_GELU_BWD),
    # NT bf16 whole-line kernel
    _nt("lines_8x24x64", BF16, 8, 24, 64),
    _nt("lines_24x8x192_f32out", BF16, 24, 8, 192, out=F32, lda=256),
    _nt("lines_264x264x1152", BF16, 264, 264, 1152, lda=1216, ldb=1216),
    _nt("lines_264x264x1152_tile_f32out", BF16, 264, 264, 1152, out=F32, flags=TILE),
    _nt("lines_L10x264x192_pers", BF16, L10, 264, 192, lda=256),
    _nt("lines_L10x264x192_tile", BF16, L10, 264, 192, flags=TILE),
    _nt("lines_264xL10x64_f32out_beta", BF16, 264, L10, 64, out=F32, beta=1.0),
    _nt("lines_L10xL10x64", BF16, L10, L10, 64),
    _nt("lines_ldc_guarded", BF16, 264, 264, 192, ldc=268),
    _nt("lines_gate_res_none_rpb_M", BF16, 264, 264, 192, epi=EPI_GATE_RES, rpb=264, gate="none"),
    _nt("lines_gate_res_ld_rpb16", BF16, L10 - 8, 264, 192, epi=EPI_GATE_RES, rpb=16, gate="ld"),
    _nt("lines_gate_res_rpb8_f32y", BF16, 264, 264, 192, epi=EPI_GATE_RES, rpb=8, gate="ld", ydt=F32),
    _nt("lines_gate_res_noy", BF16, 264, 264, 64, epi=EPI_GATE_RES, rpb=24, gate="ld", save_y=False, ydt=F32),
    _nt("lines_pos", BF16, 264, 264, 192, out=F32, epi=EPI_BIAS_POS, rpb=88),
    _nt("lines_gelu", BF16, 264, 264, 1152, epi=EPI_BIAS_GELU),
    _nt("lines_gelu_bwd", BF16, 264, 264, 192, epi=EPI_GELU_BWD),
    _nt("lines_swiglu", BF16, 264, 512, 192, epi=EPI_SWIGLU),
    _nt("lines_swiglu_L10", BF16, L10, 512, 64, epi=EPI_SWIGLU),
    _nt("lines_swiglu_bwd_ragged", BF16, 264, 264, 192, epi=EPI_SWIGLU_BWD),
    _nt("lines_swiglu_bwd_whole", BF16, 512, 256, 192, epi=EPI_SWIGLU_BWD),
    # NT bf16 persistent ring kernel (everything the whole-line kernel refuses, or on request)
    _nt("ring_M_ragged", BF16, 203, 264, 192),
    _nt("ring_N_ragged", BF16, 264, 203, 192, out=F32),
    _nt("ring_lda_K8", BF16, 264, 264, 192, lda=200),
    _nt("ring_A_off16", BF16, 264, 264, 192, lda=256, a_off=8),
    _nt("ring_half_lines", BF16, 264, 264, 1152, flags=HALF),
    _nt("ring_half_lines_L10_tile", BF16, L10, 264, 192, flags=HALF | TILE),
    _nt("ring_ldc_guarded_beta", BF16, 203, 264, 192, out=F32, beta=1.0, ldc=268),
    _nt("ring_gate_res", BF16, 264, 200, 192, epi=EPI_GATE_RES, rpb=8, gate="ld", ldc=204, flags=HALF),
    _nt("ring_gate_res_fast", BF16, 256, 264, 192, epi=EPI_GATE_RES, rpb=16, gate="ld", flags=HALF),
    _nt("ring_pos", BF16, 203, 264, 192, out=F32, epi=EPI_BIAS_POS, rpb=29),
    _nt("ring_gelu", BF16, 203, 264, 192, epi=EPI_BIAS_GELU),
    _nt("ring_gelu_bwd", BF16, 264, 203, 192, epi=EPI_GELU_BWD),
    _nt("ring_swiglu", BF16, 203, 512, 192, epi=EPI_SWIGLU),
    _nt("ring_swiglu_bwd_ragged", BF16, 203, 264, 192, epi=EPI_SWIGLU_BWD),
    # NT f16 whole-line kernel
    _nt("f16_8x24x64", F16, 8, 24, 64),
    _nt("f16_264x264x1152_f32out", F16, 264, 264, 1152, out=F32, lda=1216),
    _nt("f16_L10x264x192", F16, L10, 264, 192),
    _nt("f16_ldc_guarded", F16, 264, 264, 192, ldc=268),
    _nt("f16_gate_res", F16, 264, 264, 192, epi=EPI_GATE_RES, rpb=8, gate="ld"),
    _nt("f16_pos", F16, 264, 264, 192, out=F32, epi=EPI_BIAS_POS, rpb=88),
    _nt("f16_gelu", F16, 264, 264, 192, epi=EPI_BIAS_GELU),
    _nt("f16_gelu_bwd", F16, 264, 264, 192, epi=EPI_GELU_BWD),
    # TN: ring kernel (bf16 / f16, M % 32 == 0), 128x128 bf16 fallback, f32
    _tn("tn_ring_32", BF16, 32, 264, 200, splits="one"),
    _tn("tn_ring_96_lda", BF16, 96, 72, 264, lda=80, ldb=272),
    _tn("tn_ring_416", BF16, 416, 200, 8, bias=True),
    _tn("tn_ring_4096_beta", BF16, 4096, 264, 264, beta=1.0, bias=True, splits="many"),
    _tn("tn_ring_4096_8x72", BF16, 4096, 8, 72, bias=True),
    _tn("tn_ring_32_beta_direct_off", BF16, 32, 72, 72, beta=1.0, bias=True),
    _tn("tn_f16_ring_416", F16, 416, 264, 72, bias=True),
    _tn("tn_bf16_8", BF16, 8, 72, 200, splits="one"),
    _tn("tn_bf16_200_lda", BF16, 200, 264, 72, lda=272, bias=True),
    _tn("tn_bf16_408_beta", BF16, 408, 200, 264, beta=1.0, bias=True),
    _tn("tn_f16_200", F16, 200, 72, 8, bias=True),
    _tn("tn_f32_8", F32, 8, 72, 200),
    _tn("tn_f32_408_beta", F32, 408, 264, 72, beta=1.0, bias=True, ldb=76),
    _tn("tn_f32_4096", F32, 4096, 200, 264, bias=True, splits="many"),
    # column sums and the thin (K = 16 / 32) f32 products
    dict(kind="colsum", name="colsum_f32", dtype=F32, M=203, N=72, ld=76),
    dict(kind="colsum", name="colsum_bf16_beta", dtype=BF16, M=4099, N=264, ld=272, beta=1.0),
    dict(kind="colsum", name="colsum_f16", dtype=F16, M=9, N=1028, ld=1032, beta=1.0),
    dict(kind="thin_nt", name="thin_nt_16", M=203, N=200, K=16),
    dict(kind="thin_nt", name="thin_nt_32_pos_bf16", M=1029, N=72, K=32, pos=True, out=BF16),
    dict(kind="thin_tn", name="thin_tn_16", M=203, N=200, K=16),
    dict(kind="thin_tn", name="thin_tn_32_beta", M=1029, N=72, K=32, beta=1.0),
]


def test_case_names_are_unique():
    names = [c["name"] for c in CASES]
    assert len(names) == len(set(names))


# ----------------------------------------------------------------------------- NT
def _nt_call(lib, c, a, b, C, ldc, bias, beta, xin, xout, gate, gate_ld, rpb, out_dt):
    lib.call("ldmae_gemm_nt", _dt(c["dtype"]), _dt(out_dt), c["epi"] | c.get("flags", 0), a.data_ptr(), a.stride(0), b.data_ptr(),
             b.stride(0), C.data_ptr() if C is not None else None, ldc, c["M"], c["N"], c["K"], bias.data_ptr() if bias is not None else None,
             float(beta), xin.data_ptr() if xin is not None else None, xout.data_ptr() if xout is not None else None,
             gate.data_ptr() if gate is not None else None, gate_ld, rpb, _stream())


def _nt_path(c, a, b):
    if c["dtype"] == F32:
        return "nt_f32"
    if c["dtype"] == F16:
        return "nt_f16_lines"
    ok = lines_ok(c["epi"], a, b, c["M"], c["N"], c["K"], a.stride(0), b.stride(0)) and not c.get("flags", 0) & HALF
    return "nt_bf16_lines" if ok else "nt_bf16_ring"


def run_nt(lib, c, keep=None):
    """keep: a dict that receives the outputs of the first run (tests/test_gpu_gemm_diag.py compares them across tune keys)"""
    dtype, out_dt, M, N, K, epi = c["dtype"], c["out"], c["M"], c["N"], c["K"], c["epi"]
    lda, ldb = c.get("lda", K), c.get("ldb", K)
    ldc = c.get("ldc", N)
    beta = c.get("beta", 0.0)
    s = 1000 + sum(map(ord, c["name"]))
    A = operand(M, K, dtype, lda, s, off=c.get("a_off", 0))
    B = operand(N, K, dtype, ldb, s + 1, scale=K ** -0.5)
    a, b = A.t, B.t
    bias = _randn(1, N, s + 2)[0] if c.get("bias", True) and epi != EPI_GELU_BWD and epi != EPI_SWIGLU_BWD else None
    path = _nt_path(c, a, b)
    canv, outs = {}, {}
    xin = xout = gate = None
    gate_ld, rpb = 0, c.get("rpb", 0)
    C = None
    if epi == EPI_BIAS:
        old = _randn(M, N, s + 3).to(out_dt) if beta else None
        canv["C"] = Canvas(M, N, ldc, out_dt, old)
        C = canv["C"].t
    elif epi == EPI_GATE_RES:
        ydt = c.get("ydt", out_dt)
        out_dt = ydt
        if c.get("save_y", True):
            canv["y"] = Canvas(M, N, ldc, ydt)
            C = canv["y"].t
        xin = _randn(M, N, s + 4)
        canv["xout"] = Canvas(M, N, N, F32)
        xout = canv["xout"].t
        if c["gate"] == "ld":
            G = Canvas(M // rpb, N, N + 12, F32, _randn(M // rpb, N, s + 5))
            gate, gate_ld = G.t, G.t.stride(0)
    elif epi == EPI_BIAS_POS:
        canv["C"] = Canvas(M, N, ldc, out_dt)
        C = canv["C"].t
        xin = _randn(rpb, N, s + 6)
    elif epi == EPI_BIAS_GELU:
        canv["C"], canv["pre"] = Canvas(M, N, ldc, out_dt), Canvas(M, N, ldc, out_dt)
        C, xout = canv["C"].t, canv["pre"].t
    elif epi == EPI_GELU_BWD:
        canv["C"] = Canvas(M, N, ldc, out_dt)
        C = canv["C"].t
        P = operand(M, N, out_dt, ldc, s + 7, scale=2.0)          # the pre-activation, read with C's row stride
        xin = P.t
    elif epi == EPI_SWIGLU:
        canv["h12"], canv["hid"] = Canvas(M, N, N, BF16), Canvas(M, N // 2, N // 2, BF16)
        C, xout = canv["h12"].t, canv["hid"].t
    elif epi == EPI_SWIGLU_BWD:
        Hs = N
        canv["dh12"] = Canvas(M, 2 * Hs, 2 * Hs, BF16)
        C, ldc = canv["dh12"].t, 2 * Hs
        xin = _randn(M, 2 * Hs, s + 8, 2.0).to(BF16)
        whole = M % 128 == 0 and Hs % 64 == 0
        canv["part"] = Canvas((M + 127) // 128, 2 * Hs, 2 * Hs, F32, None if whole else torch.zeros((M + 127) // 128, 2 * Hs, device="cuda"))
        xout = canv["part"].t
    olds = {k: v.t.clone() for k, v in canv.items()}

    def go():
        for k, v in canv.items():
            v.t.copy_(olds[k])
        lib.launch_counts(reset=True)
        _nt_call(lib, c, a, b, C, ldc, bias, beta, xin, xout, gate, gate_ld, rpb, out_dt)
        counts = lib.launch_counts()
        torch.cuda.synchronize()
        return counts, {k: v.t.clone() for k, v in canv.items()}

    counts, first = go()
    fam = {F32: "nt_f32", BF16: "nt_bf16", F16: "nt_f16"}[dtype]
    assert counts == {k: (1 if k == fam else 0) for k in counts}, counts
    _, second = go()
    for k in first:
        assert torch.equal(first[k].view(_BITS[first[k].dtype][0]), second[k].view(_BITS[first[k].dtype][0])), f"{k}: rerun not bitwise equal"
        assert canv[k].intact(), f"{k}: a canary outside the output changed"

    ref_acc, S_acc = gc.nt_ref(a, b)
    bias_row = bias[None, :] if bias is not None else None
    key = f"{path}/{['bias', 'gate_res', 'pos', 'gelu', 'swiglu', 'swiglu_bwd', 'gelu_bwd'][epi]}->{str(out_dt)[6:]}"
    if epi == EPI_BIAS:
        ref, S = ref_acc, S_acc
        if bias is not None:
            ref, S = ref + bias_row.double(), S + bias_row.double().abs()
        if beta:
            ref, S = ref + olds["C"].double(), S + olds["C"].double().abs()
        _record(key, gc.check_sum(c["name"], first["C"], ref, S, K, out_dt))
    elif epi == EPI_GATE_RES:
        ref, S = ref_acc + bias_row.double(), S_acc + bias_row.double().abs()
        if "y" in first:
            _record(key + ":y", gc.check_sum(c["name"] + " y", first["y"], ref, S, K, out_dt))
        g = gate.repeat_interleave(rpb, 0) if gate is not None else torch.ones(M, N, device="cuda")
        _record(key + ":xout", gc.check_gate_res(c["name"] + " xout", first["xout"], xin, g, ref, S, K, out_dt))
    elif epi == EPI_BIAS_POS:
        p = xin.repeat(M // rpb + 1, 1)[:M].double()
        ref, S = ref_acc + bias_row.double() + p, S_acc + bias_row.double().abs() + p.abs()
        _record(key, gc.check_sum(c["name"], first["C"], ref, S, K, out_dt))
    elif epi == EPI_BIAS_GELU:
        ref, S = ref_acc + bias_row.double(), S_acc + bias_row.double().abs()
        _record(key + ":pre", gc.check_sum(c["name"] + " pre", first["pre"], ref, S, K, out_dt))
        erf = gc.ERF_LIBM if out_dt == F32 else gc.ERF_AS
        _record(key + ":act", gc.check_gelu(c["name"] + " gelu", first["C"], first["pre"], out_dt == F32, out_dt, erf))
    elif epi == EPI_GELU_BWD:
        erf = gc.ERF_LIBM if out_dt == F32 else gc.ERF_AS
        _record(key, gc.check_gelu_bwd(c["name"], first["C"], ref_acc, S_acc, K, xin, out_dt, out_dt, erf))
    elif epi == EPI_SWIGLU:
        ref, S = ref_acc + bias_row.double(), S_acc + bias_row.double().abs()
        _record(key + ":h12", gc.check_sum(c["name"] + " h12", first["h12"], ref, S, K, BF16))
        _record(key + ":hid", gc.check_swiglu(c["name"] + " hid", first["hid"], first["h12"]))
    else:
        _record(key + ":dh12", gc.check_swiglu_bwd(c["name"], first["dh12"], ref_acc, S_acc, K, xin))
        ref, S = gc.colsum_ref(first["dh12"])
        # per-128-row partials of dh12 AS STORED, summed here in f64 (the wrapper sums them with colsum)
        _record(key + ":dbias", gc.check_sum(c["name"] + " dbias", first["part"].double().sum(0), ref, S, M, F32))
    if keep is not None:
        keep.update(first)
    return path


# ----------------------------------------------------------------------------- TN, colsum, thin
def run_tn(lib, c, keep=None):
    """keep: as in run_nt"""
    dtype, M, N, K = c["dtype"], c["M"], c["N"], c["K"]
    lda, ldb, beta, with_bias = c.get("lda", N), c.get("ldb", K), c.get("beta", 0.0), c.get("bias", False)
    s = 2000 + sum(map(ord, c["name"]))
    a, b = operand(M, N, dtype, lda, s).t, operand(M, K, dtype, ldb, s + 1).t
    d = _dt(dtype)
    splits = lib.load().ldmae_gemm_tn_splits(d, M, N, K)
    if "splits" in c:
        assert (splits > 1) == (c["splits"] == "many"), (c["splits"], splits)
    ring = dtype != F32 and M % 32 == 0
    canv = {"out": Canvas(N, K, K, F32, _randn(N, K, s + 2) if beta else None)}
    if with_bias:
        canv["dbias"] = Canvas(1, N, N, F32, _randn(1, N, s + 3) if beta else None)
    olds = {k: v.t.clone() for k, v in canv.items()}
    nb = max(lib.load().ldmae_gemm_tn_workspace_bytes(d, M, N, K), lib.load().ldmae_colsum_workspace_bytes(M, N) if with_bias else 0)
    ws = torch.empty(nb // 4 + 64, dtype=F32, device="cuda")

    def go():
        for k, v in canv.items():
            v.t.copy_(olds[k])
        lib.launch_counts(reset=True)
        lib.call("ldmae_gemm_tn", d, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), canv["out"].t.data_ptr(),
                 canv["dbias"].t.data_ptr() if with_bias else None, M, N, K, float(beta), ws.data_ptr(), ws.numel() * 4, _stream())
        counts = lib.launch_counts()
        torch.cuda.synchronize()
        return counts, {k: v.t.clone() for k, v in canv.items()}

    counts, first = go()
    fam = {F32: "tn_f32", BF16: "tn_bf16", F16: "tn_f16"}[dtype]
    assert counts == {k: (1 if k == fam else 0) for k in counts}, counts
    _, second = go()
    for k in first:
        assert torch.equal(first[k], second[k]), f"{k}: rerun not bitwise equal"
        assert canv[k].intact(), f"{k}: a canary outside the output changed"
    path = "tn_ring" if ring else ("tn_bf16" if dtype != F32 else "tn_f32")
    path += "_direct" if splits == 1 and beta == 0 else "_split"
    ref, S = gc.tn_ref(a, b, olds["out"] if beta else None)
    _record(path + ":out", gc.check_sum(c["name"], first["out"], ref, S, M, F32))
    if with_bias:
        ref, S = gc.colsum_ref(a, olds["dbias"][0] if beta else None)
        _record(path + ":dbias", gc.check_sum(c["name"] + " dbias", first["dbias"][0], ref, S, M, F32))
    if keep is not None:
        keep.update(first)
    return path, splits


def run_colsum(lib, c):
    dtype, M, N, beta = c["dtype"], c["M"], c["N"], c.get("beta", 0.0)
    x = operand(M, N, dtype, c["ld"], 3000 + M).t
    out = Canvas(1, N, N, F32, _randn(1, N, 7) if beta else None)
    old = out.t.clone()
    ws = torch.empty(lib.load().ldmae_colsum_workspace_bytes(M, N) // 4 + 64, dtype=F32, device="cuda")
    res = []
    for _ in range(2):
        out.t.copy_(old)
        lib.call("ldmae_colsum", _dt(dtype), x.data_ptr(), x.stride(0), M, N, out.t.data_ptr(), float(beta), ws.data_ptr(), _stream())
        res.append(out.t.clone())
    assert torch.equal(res[0], res[1]) and out.intact()
    ref, S = gc.colsum_ref(x, old[0] if beta else None)
    _record("colsum", gc.check_sum(c["name"], res[0][0], ref, S, M, F32))


def run_thin_nt(lib, c):
    M, N, K, out_dt = c["M"], c["N"], c["K"], c.get("out", F32)
    t, w = operand(M, K, F32, K, 4000 + M).t, operand(N, K, F32, K, 4001 + M).t
    bias = _randn(1, N, 4002)[0]
    rpb = 7 if c.get("pos") else 0
    pos = _randn(rpb, N, 4003) if rpb else None
    out = Canvas(M, N, N, out_dt)
    res = []
    for _ in range(2):
        lib.call("ldmae_thin_nt", _dt(out_dt), t.data_ptr(), w.data_ptr(), bias.data_ptr(), pos.data_ptr() if rpb else None, out.t.data_ptr(),
                 M, N, K, rpb, _stream())
        res.append(out.t.clone())
    assert torch.equal(res[0], res[1]) and out.intact()
    adds = [bias[None, :]] + ([pos.repeat(M // rpb + 1, 1)[:M]] if rpb else [])
    ref, S = gc.nt_ref(t, w, *adds)
    _record(f"thin_nt->{str(out_dt)[6:]}", gc.check_sum(c["name"], res[0], ref, S, K, out_dt))


def run_thin_tn(lib, c):
    M, N, K, beta = c["M"], c["N"], c["K"], c.get("beta", 0.0)
    g, t = operand(M, N, F32, N, 5000 + M).t, operand(M, K, F32, K, 5001 + M).t
    dW = Canvas(N, K, K, F32, _randn(N, K, 5002) if beta else None)
    db = Canvas(1, N, N, F32, _randn(1, N, 5003) if beta else None)
    olds = dW.t.clone(), db.t.clone()
    ws = torch.empty(lib.load().ldmae_thin_tn_workspace_bytes(M, N, K) // 4 + 64, dtype=F32, device="cuda")
    res = []
    for _ in range(2):
        dW.t.copy_(olds[0])
        db.t.copy_(olds[1])
        lib.call("ldmae_thin_tn", g.data_ptr(), t.data_ptr(), dW.t.data_ptr(), db.t.data_ptr(), M, N, K, float(beta), ws.data_ptr(),
                 ws.numel() * 4, _stream())
        res.append((dW.t.clone(), db.t.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and dW.intact() and db.intact()
    ref, S = gc.tn_ref(g, t, olds[0] if beta else None)
    _record("thin_tn:dW", gc.check_sum(c["name"], res[0][0], ref, S, M, F32))
    ref, S = gc.colsum_ref(g, olds[1][0] if beta else None)
    _record("thin_tn:db", gc.check_sum(c["name"] + " db", res[0][1][0], ref, S, M, F32))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_gemm_path(lib, case):
    kind = case["kind"]
    if kind == "nt":
        path = run_nt(lib, case)
        if "expect" in case:
            assert path == case["expect"]
    elif kind == "tn":
        run_tn(lib, case)
    else:
        {"colsum": run_colsum, "thin_nt": run_thin_nt, "thin_tn": run_thin_tn}[kind](lib, case)


def test_case_table_covers_every_predicate(lib):
    """Every dispatch predicate is selected by at least one case and missed by another (a later edit of the table cannot drop a path)."""
    seen = {}

    def note(name, v):
        seen.setdefault(name, set()).add(bool(v))

    for c in CASES:
        if c["kind"] == "nt":
            K, lda, ldb = c["K"], c.get("lda", c["K"]), c.get("ldb", c["K"])
            if c["dtype"] != F32:
                aligned = c.get("a_off", 0) == 0       # operands start on 256-B boundaries unless offset
                M, N, epi = c["M"], c["N"], c["epi"]
                ok = not (M < 8 or N < 8 or M % 8 or N % 8 or K % 64 or lda % 64 or ldb % 64) and aligned and not (epi == EPI_SWIGLU and N % 256)
                note("lines_shape_ok", ok)
                if c["dtype"] == BF16:
                    note("bf16 whole-line kernel", ok and not c.get("flags", 0) & HALF)
                    note("half-lines flag", c.get("flags", 0) & HALF)
                    note("tile launch flag", c.get("flags", 0) & TILE)
            if c["epi"] not in (EPI_SWIGLU, EPI_SWIGLU_BWD):
                note(f"nfast[{c['dtype']}]", nfast(c["epi"], c["N"], c.get("ldc", c["N"]), c.get("rpb", 16)))
            if c["epi"] == EPI_GATE_RES:
                note("gate_res rows_per_batch % 16", c["rpb"] % 16 == 0)
                note("gate", c["gate"] != "none")
            if c["epi"] == EPI_BIAS and c["dtype"] != F16:        # fp16 GEMMs take beta = 0 only
                note(f"beta[{c['dtype']}]", c.get("beta", 0.0))
        elif c["kind"] == "tn":
            d = _dt(c["dtype"])
            splits = lib.load().ldmae_gemm_tn_splits(d, c["M"], c["N"], c["K"])
            note("tn ring (M % 32 == 0, 16-bit)", c["dtype"] != F32 and c["M"] % 32 == 0)
            note("tn direct (1 split, beta 0)", splits == 1 and c.get("beta", 0.0) == 0)
            note("tn splits > 1", splits > 1)
            note("tn dbias", c.get("bias", False))
            if c.get("bias", False):
                note("tn dbias accumulated (beta 1)", c.get("beta", 0.0))
                note("tn dbias fused on the ring", c["dtype"] != F32 and c["M"] % 32 == 0)
    epis = {c["epi"] for c in CASES if c["kind"] == "nt"}
    assert epis == set(range(7))
    for name, vals in seen.items():
        assert vals == {True, False}, f"predicate {name!r} is only ever {vals}"


def test_f16_refused_shape_names_the_kernel(lib):
    A, B = operand(203, 64, F16, 64, 1).t, operand(64, 64, F16, 64, 2).t          # M % 8 != 0: no bf16-style ring fallback for fp16
    C = torch.empty(203, 64, dtype=F16, device="cuda")
    with pytest.raises(RuntimeError, match=r"gemm_nt\(fp16\): shape outside the whole-line kernel \(M=203 N=64"):
        lib.call("ldmae_gemm_nt", 2, 2, EPI_BIAS, A.data_ptr(), 64, B.data_ptr(), 64, C.data_ptr(), 64, 203, 64, 64, None, 0.0, None, None,
                 None, 0, 0, _stream())


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("epi", [EPI_SWIGLU, EPI_SWIGLU_BWD], ids=["swiglu", "swiglu_bwd"])
def test_swiglu_with_f32_output_is_refused(lib, dtype, epi):
    """The SwiGLU epilogues write bf16 only: the library returns LDMAE_ERR_INVALID (-1) before any launch, whatever the operand type."""
    M, N, K = 256, 256, 64
    A, B = operand(M, K, dtype, K, 1).t, operand(N, K, dtype, K, 2).t
    C, x = Canvas(M, 2 * N, 2 * N, F32), Canvas(M, 2 * N, 2 * N, F32)
    lib.launch_counts(reset=True)
    rc = lib.load().ldmae_gemm_nt(_dt(dtype), _dt(F32), epi, A.data_ptr(), K, B.data_ptr(), K, C.t.data_ptr(), 2 * N if epi == EPI_SWIGLU_BWD else N,
                                  M, N, K, None, 0.0, x.t.data_ptr(), x.t.data_ptr(), None, 0, 0, _stream())
    assert rc == -1 and "epilogue is bf16 only" in lib.last_error()
    torch.cuda.synchronize()
    assert not any(lib.launch_counts().values()) and C.intact() and x.intact()
    assert bool((C.t.view(torch.int32) == _BITS[F32][1]).all()), "a refused call wrote its output"


# ----------------------------------------------------------------------------- wrapper layout rules (ldmae_amd.ops)
@pytest.fixture(scope="module")
def ops(lib):
    from ldmae_amd import ops
    return ops


def _ref_check(name, got, a, b, bias, K):
    ref, S = gc.nt_ref(a, b, bias[None, :] if bias is not None else None)
    return gc.check_sum(name, got, ref, S, K)


def test_column_strided_inputs_are_copied(ops):
    """A column-strided view passes every C-side check (lda >= K, lda % 8 == 0) but is not a row-major operand: the wrappers copy it."""
    M, N, K = 264, 200, 192
    wide = _randn(M, 2 * K, 11).to(BF16)
    a = wide[:, ::2]                                     # strides (2K, 2)
    w = _randn(N, K, 12, K ** -0.5).to(BF16)
    bias = _randn(1, N, 13)[0]
    _ref_check("gemm_nt", ops.gemm_nt(a, w, bias), a.contiguous(), w, bias, K)
    _ref_check("gemm_nt (b strided)", ops.gemm_nt(w, a, None), w, a.contiguous(), None, K)
    wt = _randn(K, N, 14, K ** -0.5).to(BF16)
    _ref_check("gemm_nt (b transposed view)", ops.gemm_nt(a, wt.T, bias), a.contiguous(), wt.T.contiguous(), bias, K)
    # gemm_tn / colsum
    g = _randn(M, 2 * N, 15).to(BF16)[:, ::2]
    out, db = ops.gemm_tn(g, a, with_bias=True)
    ref, S = gc.tn_ref(g.contiguous(), a.contiguous())
    gc.check_sum("gemm_tn", out, ref, S, M)
    ref, S = gc.colsum_ref(g.contiguous())
    gc.check_sum("gemm_tn dbias", db, ref, S, M)
    gc.check_sum("colsum", ops.colsum(g), ref, S, M)
    # gated residual: xin column-strided, gate column-strided; xout comes back contiguous
    T = 8
    xin = _randn(M, 2 * N, 16)[:, ::2]
    gate = _randn(M // T, 2 * N, 17)[:, ::2]
    xo, y = ops.gemm_nt_gate_res(a, w, bias, xin, gate, T)
    assert xo.is_contiguous() and xo.shape == (M, N)
    ref, S = gc.nt_ref(a.contiguous(), w, bias[None, :])
    gc.check_gate_res("gate_res", xo, xin.contiguous(), gate.contiguous().repeat_interleave(T, 0), ref, S, K, BF16)
    # row slices of a wider buffer stay zero-copy (the leading dimension is passed through)
    rows = _randn(M, K + 64, 18).to(BF16)[:, :K]
    assert ops._arg(rows, "x", rows=True) is rows


def test_pos_and_thin_inputs(ops):
    M, N, K, T = 64, 200, 16, 16
    t = _randn(M, 2 * K, 20)[:, ::2]
    w = _randn(N, K, 21)
    bias = _randn(1, 2 * N, 22)[0, ::2]                  # a strided bias vector is copied
    pos = _randn(T, 2 * N, 23)[:, ::2]
    ref, S = gc.nt_ref(t.contiguous(), w, bias.contiguous()[None, :], pos.contiguous().repeat(M // T, 1))
    gc.check_sum("gemm_nt_pos", ops.gemm_nt_pos(t, w, bias, pos, T), ref, S, K)
    gc.check_sum("thin_nt", ops.thin_nt(t, w, bias, pos, T), ref, S, K)
    dW, db = ops.thin_tn(_randn(M, 2 * N, 24)[:, ::2], t)
    g = _randn(M, 2 * N, 24)[:, ::2].contiguous()
    ref, S = gc.tn_ref(g, t.contiguous())
    gc.check_sum("thin_tn", dW, ref, S, M)


def test_bad_outputs_and_arguments_raise(ops):
    M, N, K = 64, 64, 64
    a, w = _randn(M, K, 30).to(BF16), _randn(N, K, 31).to(BF16)
    bias = _randn(1, N, 32)[0]
    with pytest.raises(RuntimeError, match="gemm_nt out: the kernel writes rows"):
        ops.gemm_nt(a, w, out=torch.empty(N, M, device="cuda").T)
    with pytest.raises(RuntimeError, match="gemm_nt out: dtype"):
        ops.gemm_nt(a, w, out=torch.empty(M, N, device="cuda"), out_dtype=BF16)
    with pytest.raises(RuntimeError, match="gemm_nt bias: dtype"):
        ops.gemm_nt(a, w, bias.to(BF16))
    with pytest.raises(RuntimeError, match="gemm_nt bias: shape"):
        ops.gemm_nt(a, w, _randn(1, N + 1, 33)[0])
    with pytest.raises(RuntimeError, match="must be \\[M,K\\] and \\[N,K\\] of one dtype"):
        ops.gemm_nt(a, w.float())
    with pytest.raises(RuntimeError, match="gemm_tn out: the kernel writes a contiguous"):
        ops.gemm_tn(a, w, out=torch.empty(N, K + 4, device="cuda")[:, :K], beta=1.0)
    with pytest.raises(RuntimeError, match="gemm_tn dbias_out: the kernel writes a contiguous"):
        ops.gemm_tn(a, w, with_bias=True, dbias_out=torch.empty(2 * N, device="cuda")[::2])
    with pytest.raises(RuntimeError, match="colsum out: the kernel writes a contiguous"):
        ops.colsum(a, out=torch.empty(2 * K, device="cuda")[::2], beta=1.0)
    with pytest.raises(RuntimeError, match="gemm_nt_gate_res xout: the kernel writes a contiguous"):
        ops.gemm_nt_gate_res(a, w, bias, _randn(M, N, 34), None, M, xout=torch.empty(M, 2 * N, device="cuda")[:, ::2])
    with pytest.raises(RuntimeError, match="gemm_nt_gate_res xin: dtype"):
        ops.gemm_nt_gate_res(a, w, bias, _randn(M, N, 34).to(BF16), None, M)
    with pytest.raises(RuntimeError, match="gemm_nt_gate_res xin: .* elements"):
        ops.gemm_nt_gate_res(a, w, bias, _randn(M, N + 8, 34), None, M)
    with pytest.raises(RuntimeError, match="gemm_nt_gate_res gate: shape"):
        ops.gemm_nt_gate_res(a, w, bias, _randn(M, N, 34), _randn(2, N, 35), 16)
    with pytest.raises(RuntimeError, match="gemm_nt_pos pos: dtype"):
        ops.gemm_nt_pos(a, w, bias, _randn(8, N, 36).to(BF16), 8)
    with pytest.raises(RuntimeError, match="cast_weight w: dtype"):
        ops.cast_weight(a, BF16)
    with pytest.raises(RuntimeError, match="thin_nt t: dtype"):
        ops.thin_nt(_randn(M, 16, 37).to(BF16), _randn(N, 16, 38))
