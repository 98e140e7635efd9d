"""The per-element GEMM bound (tests/gemm_check.py) on CPU products: it accepts a correctly rounded result and rejects the small faults
a norm-wise 2e-2 check lets through -- truncation instead of round-to-nearest-even, one element 2 ulp off, one 64-deep K block
missing from one 256x256 tile, a wrong last row or column."""
import pytest
import torch

import gemm_check as gc


def _operands(M, N, K, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(dtype)
    b = (torch.randn(N, K, generator=g) * K ** -0.5).to(dtype)
    bias = torch.randn(N, generator=g)
    return a, b, bias


def _f32_product(a, b, bias):
    """What a kernel with f32 accumulation computes (an f32 sum of the exact products plus the bias)."""
    return a.float() @ b.float().T + bias


def _truncate_bf16(x):
    """Round toward zero to bf16 (drop the low 16 bits of the f32 pattern)."""
    return (x.float().view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
def test_accepts_correctly_rounded(out_dtype):
    a, b, bias = _operands(300, 264, 1152, 1)
    ref, S = gc.nt_ref(a, b, bias)
    got = _f32_product(a, b, bias).to(out_dtype)
    assert gc.check_sum("nt", got, ref, S, 1152) <= 1.0
    # the f64 result rounded once is the best any kernel can do: well inside the bound
    assert gc.check_sum("nt", ref.to(out_dtype), ref, S, 1152) <= 1.0


def test_accepts_tn_and_colsum():
    g = torch.Generator().manual_seed(2)
    a, b = torch.randn(416, 72, generator=g).to(torch.bfloat16), torch.randn(416, 200, generator=g).to(torch.bfloat16)
    old = torch.randn(72, 200, generator=g)
    ref, S = gc.tn_ref(a, b, old)
    assert gc.check_sum("tn", old + a.float().T @ b.float(), ref, S, 416) <= 1.0
    ref, S = gc.colsum_ref(a)
    assert gc.check_sum("colsum", a.float().sum(0), ref, S, 416) <= 1.0


def test_rejects_truncation():
    a, b, bias = _operands(256, 256, 256, 3)
    ref, S = gc.nt_ref(a, b, bias)
    got = _truncate_bf16(_f32_product(a, b, bias))
    with pytest.raises(gc.BoundError, match="out of bound"):
        gc.check_sum("nt", got, ref, S, 256)


def test_rejects_one_element_two_ulp_off():
    a, b, bias = _operands(264, 264, 1152, 4)
    ref, S = gc.nt_ref(a, b, bias)
    got = _f32_product(a, b, bias).to(torch.bfloat16)
    assert gc.check_sum("nt", got, ref, S, 1152) <= 1.0
    i, j = 137, 201
    x = got[i, j].float()
    got[i, j] = (x + 2 * gc.ulp(x.double(), torch.bfloat16).float()).to(torch.bfloat16)
    with pytest.raises(gc.BoundError, match=r"worst at \(137, 201\)"):
        gc.check_sum("nt", got, ref, S, 1152)


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
def test_rejects_a_missing_k_block_of_one_tile(out_dtype):
    M, N, K = 512, 512, 1152
    a, b, bias = _operands(M, N, K, 5)
    ref, S = gc.nt_ref(a, b, bias)
    acc = _f32_product(a, b, bias)
    # tile (1, 0) of the 256x256 grid drops K block 10 (k = 640..703)
    k0 = 640
    acc[256:512, 0:256] -= a[256:512, k0:k0 + 64].float() @ b[0:256, k0:k0 + 64].float().T
    with pytest.raises(gc.BoundError, match="out of bound"):
        gc.check_sum("nt", acc.to(out_dtype), ref, S, K)


@pytest.mark.parametrize("where", ["row", "col"])
def test_rejects_a_wrong_last_row_or_column(where):
    M, N, K = 200, 65, 48
    a, b, bias = _operands(M, N, K, 6, torch.float32)
    ref, S = gc.nt_ref(a, b, bias)
    got = _f32_product(a, b, bias)
    if where == "row":
        got[-1] = got[-2]                     # a stale row
    else:
        got[:, -1] -= bias[-1]                # the last column without its bias
    with pytest.raises(gc.BoundError):
        gc.check_sum("nt", got, ref, S, K)


def test_rejects_nan():
    a, b, bias = _operands(16, 16, 64, 7)
    ref, S = gc.nt_ref(a, b, bias)
    got = _f32_product(a, b, bias)
    got[3, 5] = float("nan")
    with pytest.raises(gc.BoundError, match=r"worst at \(3, 5\)"):
        gc.check_sum("nt", got, ref, S, 64)


def test_ulp():
    x = torch.tensor([1.0, 1.5, 2.0, 0.0, -3.0, 1e-40], dtype=torch.float64)
    assert gc.ulp(x, torch.bfloat16).tolist() == [2 ** -7, 2 ** -7, 2 ** -6, 2 ** -133, 2 ** -6, 2 ** -133]
    assert gc.ulp(x, torch.float16)[:3].tolist() == [2 ** -10, 2 ** -10, 2 ** -9] and float(gc.ulp(x, torch.float16)[3]) == 2 ** -24
    assert gc.ulp(x, torch.float32)[:3].tolist() == [2 ** -23, 2 ** -23, 2 ** -22]


def test_activation_checks_accept_the_f32_formulas():
    g = torch.Generator().manual_seed(8)
    pre = (torch.randn(64, 256, generator=g) * 3).to(torch.bfloat16)
    x = pre.float()
    out = (0.5 * x * (1 + torch.erf(x * 0.70710678118654752))).to(torch.bfloat16)
    assert gc.check_gelu("gelu", out, pre, False, torch.bfloat16, gc.ERF_AS) <= 1.0
    h12 = (torch.randn(64, 512, generator=g) * 2).to(torch.bfloat16)
    x1, x2 = h12[:, :256].float(), h12[:, 256:].float()
    assert gc.check_swiglu("swiglu", (x1 * torch.sigmoid(x1) * x2).to(torch.bfloat16), h12) <= 1.0
    bad = (x1 * torch.sigmoid(x1) * x2 * 1.02).to(torch.bfloat16)
    with pytest.raises(gc.BoundError):
        gc.check_swiglu("swiglu", bad, h12)
