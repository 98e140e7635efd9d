"""Every entry point that takes a dtype code refuses the codes it has no kernel for, before anything touches a device.

The row / pointwise / VMAE-layer / MX8 entry points choose their kernel with dtype_dispatch (csrc/common.h) over exactly the types they are
instantiated for.  A code outside that set used to fall through to the f32 kernel: with fp16 buffers (LDMAE_F16 is what _lib.dt() makes of
torch.float16) that kernel runs past the end of buffers half the size it assumes.  Here every entry is called with every code of
{0, 1, 2, 7, -1} it does not accept, on small valid shapes and dummy non-null 16-byte-aligned pointers: the call must return
LDMAE_ERR_INVALID (-1) and name itself and the code in ldmae_last_error().  An entry that missed the check would reach the HIP runtime, which
has no device on the machines this test runs on, and return LDMAE_ERR_HIP (-2).

With a GPU present the test skips itself: a missed check would launch a kernel on address 16.  tests/test_gpu_row_paths.py and
tests/test_gpu_layer_paths.py make the same calls there on real, guarded buffers.
"""
import ctypes

import pytest
import torch

from ldmae_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers: only where no kernel can be launched")

CODES = (0, 1, 2, 7, -1)
F32_BF16, ALL3, BF16_ONLY, BF16_F16 = (0, 1), (0, 1, 2), (1,), (1, 2)
P, P2 = ctypes.c_void_p(16), ctypes.c_void_p(32)
M, D, RPB, EPS = 16, 256, 16, 1e-6
B, N, H, HD = 1, 8, 1, 64
N8 = 8
_BWD = (P, P, P, P, D, P, P, 0.0, P, P, D, P, 0.0)                           # dout, x, w, scale, mod_ld, rstd, dx, beta_x, dshift, dscale, dmod_ld, dw, beta_w
_LBWD = (P, P, P, D, P, P, 0.0, P, P, D)                                     # the same without w / dw / beta_w
_GATE = (P, P, D, P, P, D, P)                                                # y, gate, gate_ld, dy, dgate, dgate_ld, dbias

# entry -> (name in the message, accepted codes, arguments after the dtype code)
ENTRIES = {
    "ldmae_rmsnorm_modulate_fwd": ("rmsnorm_modulate_fwd", F32_BF16, (P, P, P, P, D, P, P, M, D, RPB, EPS, None)),
    "ldmae_layernorm_modulate_fwd": ("layernorm_modulate_fwd", F32_BF16, (P, P, P, D, P, P, M, D, RPB, EPS, None)),
    "ldmae_rmsnorm_modulate_bwd": ("rmsnorm_modulate_bwd", F32_BF16, _BWD + (M, D, RPB, P, None)),
    "ldmae_rmsnorm_modulate_bwd_gate": ("rmsnorm_modulate_bwd_gate", F32_BF16, _BWD + _GATE + (M, D, RPB, P, None)),
    "ldmae_rmsnorm_modulate_bwd_gate_recompute": ("rmsnorm_modulate_bwd_gate_recompute", BF16_ONLY, _BWD + _GATE + (M, D, RPB, P, None)),
    "ldmae_layernorm_modulate_bwd": ("layernorm_modulate_bwd", F32_BF16, _LBWD + (M, D, RPB, P, None)),
    "ldmae_layernorm_modulate_bwd_gate": ("layernorm_modulate_bwd_gate", F32_BF16, _LBWD + _GATE + (M, D, RPB, P, None)),
    "ldmae_res_rmsnorm_modulate_fwd": ("res_rmsnorm_modulate_fwd", BF16_F16, (P, P, P, D, P, P, D, P2, P, P, P, D, P, P, M, D, RPB, EPS, None)),
    "ldmae_qknorm_rope_fwd": ("qknorm_rope_fwd", F32_BF16, (P, P, P, P, P, P, P, P, B, N, H, HD, EPS, None)),
    "ldmae_qknorm_rope_bwd": ("qknorm_rope_bwd", F32_BF16, (P, P, P, P, P, P, P, P, P, P, P, 0.0, P, B, N, H, HD, EPS, P, None)),
    "ldmae_rope": ("rope", F32_BF16, (P, P, P, P, B * N * H, N, HD, 0, None)),
    "ldmae_swiglu_fwd": ("swiglu_fwd", F32_BF16, (P, P, M, D, None)),
    "ldmae_swiglu_bwd": ("swiglu_bwd", F32_BF16, (P, P, P, M, D, None)),
    "ldmae_gate_bwd": ("gate_bwd", F32_BF16, (P, P, P, D, P, P, D, P, M, D, RPB, P, None)),
    "ldmae_silu_fwd": ("silu_fwd", F32_BF16, (P, P, N8, None)),
    "ldmae_thin_nt": ("thin_nt", F32_BF16, (P, P, P, P, P, M, D, 16, RPB, None)),
    "ldmae_patch_gather": ("patch_gather", F32_BF16, (P, P, P, P, P, 1, N8, 3, 16, 4, D, None)),
    "ldmae_gelu_tanh_fwd": ("gelu_tanh_fwd", F32_BF16, (P, P, N8, None)),
    "ldmae_gelu_tanh_bwd": ("gelu_tanh_bwd", F32_BF16, (P, P, P, N8, None)),
    "ldmae_mx8_quantize": ("mx8_quantize", F32_BF16, (P, D, P, P, M, D, None)),
    "ldmae_colsum": ("colsum", ALL3, (P, D, M, D, P, 0.0, P, None)),
    "ldmae_cast_weight": ("cast_weight", ALL3, (P, P, P, M, D, None)),
    "ldmae_layernorm_fwd": ("layernorm_fwd", ALL3, (P, P, P, P, P, P, M, D, EPS, None)),
    "ldmae_layernorm_bwd": ("layernorm_bwd", ALL3, (P, P, P, P, P, P, P, P, 0.0, M, D, P, None)),
    "ldmae_layernorm_bwd_cast": ("layernorm_bwd", ALL3, (P, P, P, P, P, P, None, P, P, 0.0, M, D, P, None)),      # reports under the shared name
    "ldmae_gelu_fwd": ("gelu_fwd", ALL3, (P, P, N8, None)),
    "ldmae_gelu_bwd": ("gelu_bwd", ALL3, (P, P, P, N8, None)),
}
# the one refusal whose (unchanged) message does not carry the code
NO_CODE_IN_MESSAGE = {"ldmae_rmsnorm_modulate_bwd_gate_recompute"}
CAST_PAIRS = {(0, 1), (1, 0), (0, 2), (2, 0), (0, 0)}

CASES = [(e, c) for e, (_, ok, _a) in ENTRIES.items() for c in CODES if c not in ok]


def test_table_matches_the_header():
    """Every entry of the table is declared with a leading int dtype code and as many arguments as the table passes; the table has every
    accepted set of the contract (include/ldmae_hip.h states the rule at the dtype codes)."""
    for entry, (_name, ok, args) in ENTRIES.items():
        res, argt = _lib.SIGNATURES[entry]
        assert res is ctypes.c_int and argt[0] is ctypes.c_int and len(argt) == 1 + len(args), entry
        assert set(ok) < set(CODES)
    assert len(ENTRIES) == 27 and len(CASES) == 18 * 3 + 4 + 3 + 7 * 2      # f32 | bf16, bf16 alone, bf16 | f16, all three


@pytest.mark.parametrize("entry,code", CASES, ids=[f"{e[6:]}-{c}" for e, c in CASES])
def test_unaccepted_code_is_refused(entry, code):
    name, _ok, args = ENTRIES[entry]
    rc = getattr(_lib.load(), entry)(code, *args)
    msg = _lib.last_error()
    assert rc == -1, f"{entry}(dtype {code}) returned {rc}: {msg!r}"
    assert msg.startswith(name + ":"), msg
    assert entry in NO_CODE_IN_MESSAGE or f"dtype {code}" in msg, msg


@pytest.mark.parametrize("src,dst", [(s, d) for s in CODES for d in CODES if (s, d) not in CAST_PAIRS])
def test_cast_refuses_every_other_pair(src, dst):
    rc = _lib.load().ldmae_cast(src, dst, P, P2, N8, None)
    msg = _lib.last_error()
    assert rc == -1 and msg.startswith("cast:") and f"{src} -> {dst}" in msg, (rc, msg)


@pytest.mark.parametrize("code", [c for c in CODES if c not in F32_BF16])
def test_cast_stack_refuses(code):
    srcs = (ctypes.c_void_p * 1)(16)                       # a host array of device pointers: read on the host, never dereferenced
    rc = _lib.load().ldmae_cast_stack(code, srcs, 1, N8, P, None)
    msg = _lib.last_error()
    assert rc == -1 and msg.startswith("cast_stack:") and f"dtype {code}" in msg, (rc, msg)
