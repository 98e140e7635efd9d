"""Thin tensor-level wrappers over the C ABI (one python function per entry point).

Every function allocates its outputs with torch (caching allocator) and enqueues
the kernel on torch's current stream.  No function here computes anything in
PyTorch: if the library is missing, or a tensor is on the CPU, they raise.
"""
from __future__ import annotations

import ctypes
import functools
import os
import weakref

import torch

from . import _lib as L
from ._lib import (BF16, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_POS, EPI_F16_INF, EPI_GATE_RES, EPI_GELU_BWD, EPI_HALF_LINES, EPI_SWIGLU, EPI_SWIGLU_BWD, EPI_TILE_LAUNCH, F32, call, dt,
                   ptr)

mx8_launch_counts = L.mx8_launch_counts      # the MXFP8 sampling mode's own counters (quantise, norm + quantise, GEMM)
launch_counts = L.launch_counts      # launch counts by kernel family (which arithmetic type, which GEMM form the calls were dispatched to)

_ws = {}


def stream(device=None):
    """The handle of torch's current stream on `device` (default: the current device) -- torch.cuda.current_stream(device).cuda_stream, as
    _lib.stream() returns it, without the torch.cuda.Stream object that call builds for every wrapper call.  It and _ws_bytes below pay for the
    argument checks: with the checks alone every wrapper of the train steps costs about 2 to 7 us of host time more than before it had them, far out
    of the run-to-run spread; this saves 2.2 to 2.5 us per call, _ws_bytes about 2 us per backward wrapper (profiles/ops_args_host.txt)."""
    if device is not None and not isinstance(device, torch.device):
        device = torch.device(device)
    idx = None if device is None else device.index
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device() if idx is None else idx)


@functools.lru_cache(maxsize=1024)
def _ws_bytes(entry, *dims):
    """The scratch size an entry point asks for (every ldmae_*_workspace_bytes query of this file): a pure function of the extents, asked of
    the library once per shape instead of once per call."""
    return getattr(L.load(), entry)(*dims)


def workspace(nbytes: int, device, slot: str = "main") -> torch.Tensor:
    """Grow-only f32 scratch buffer per (device, slot, STREAM): the library's entry points take their scratch from the caller and use it only inside
    the launches they enqueue, so two calls may share a buffer exactly when they are ordered on one stream -- work enqueued on different streams
    (the weight-gradient side stream, a data-parallel reducer, two modules driven from two host threads) gets buffers of its own."""
    key = (device, slot, stream(device))
    n = max(1, (int(nbytes) + 3) // 4)
    t = _ws.get(key)
    if t is None or t.numel() < n:
        t = torch.empty(int(n * 1.25) + 1024, dtype=torch.float32, device=device)
        _ws[key] = t
    return t


_F32_BF16 = (torch.float32, torch.bfloat16)                       # the dtype sets the entry points dispatch on (include/ldmae_hip.h: the dtype codes)
_B16 = (torch.bfloat16, torch.float16)
_FLOATS = (torch.float32, torch.bfloat16, torch.float16)
_FLAGS = (torch.uint8, torch.bool)                                # one byte per element


def _arg(t, what, dtype=None, shape=None, rows=False, out=False, numel=None, like=None, align=0, at_least=0, copy=True):
    """THE check of one tensor argument of a wrapper (attributes only: no synchronisation, no device work); `what` = "<op> <argument>".
    None passes (an optional argument).  dtype: one torch dtype, or a tuple of accepted ones.  shape: the exact shape; entries that are no
    integers are wildcards and name the dimension in the message ((B, "Ho", "Wo", 3), or "NHWC" for four of them), so a shape fixes the rank.
    numel= / at_least=: the element count (at least that many) of an operand the kernel addresses flat, whatever its torch shape.  like=: an
    anchor tensor whose device t must share.  align=: the address must be a multiple of that many bytes.
    LAYOUT.  rows=True: the kernel reads it row by row with a leading dimension (t.stride(0)): elements of a row must be adjacent, rows may be
    further apart (a row slice of a wider buffer stays zero-copy).  rows=False: the kernel reads it densely.  An input of another layout is
    copied, unless copy=False (the kernel must see this very tensor); an output (out=True) must already have the layout.
    Everything that does not hold raises RuntimeError: the op and argument, what was found against what was expected, then the whole contract."""
    if t is None:
        return None
    if (dtype is not None and t.dtype != dtype and (type(dtype) is not tuple or t.dtype not in dtype)
            or shape is not None and t.shape != shape and not _shape_fits(t.shape, shape)
            or numel is not None and t.numel() != numel
            or at_least and t.numel() < at_least or like is not None and t.device != like.device or align and t.data_ptr() % align):
        raise _refusal(t, what, dtype, shape, rows, out, numel, like, align, at_least, copy)
    if rows:
        st, sh = t.stride(), t.shape
        ok = len(st) == 2 and (st[1] == 1 or sh[1] <= 1) and (st[0] >= sh[1] or sh[0] <= 1)
    else:
        ok = t.is_contiguous()
    if ok:
        return t
    if out or not copy:
        raise _refusal(t, what, dtype, shape, rows, out, numel, like, align, at_least, copy)
    return t.contiguous()


def _refusal(t, what, dtype, shape, rows, out, numel, like, align, at_least, copy):
    """The error of _arg, off its fast path: the first thing that does not hold (in _arg's order; none of them: the layout), then the contract."""
    if dtype is not None and t.dtype != dtype and (type(dtype) is not tuple or t.dtype not in dtype):
        why = f"dtype {t.dtype}, expected {' or '.join(map(str, dtype)) if type(dtype) is tuple else dtype}"
    elif shape is not None and not _shape_fits(t.shape, shape):
        why = f"shape {tuple(t.shape)}, expected {_shape_text(shape)}"
    elif numel is not None and t.numel() != numel:
        why = f"{t.numel()} elements (shape {tuple(t.shape)}), expected {numel}"
    elif at_least and t.numel() < at_least:
        why = f"{t.numel()} elements (shape {tuple(t.shape)}), expected at least {at_least}"
    elif like is not None and t.device != like.device:
        why = f"device {t.device}, expected {like.device}"
    elif align and t.data_ptr() % align:
        why = f"the tensor's storage must be {align}-byte aligned"
    else:
        form = "rows with adjacent elements (stride(1) == 1, stride(0) >= columns)" if rows else "a contiguous tensor"
        why = f"the kernel {'writes' if out else 'reads'} {form}; got strides {tuple(t.stride())} for shape {tuple(t.shape)}"
    need = ["a" if copy and not out else "a row-strided" if rows else "a contiguous"]
    if dtype is not None:
        need.append(" or ".join(str(d)[6:] for d in (dtype if type(dtype) is tuple else (dtype,))))
    if shape is not None:
        need.append(_shape_text(shape))
    need.append("tensor")
    if numel is not None or at_least:
        need.append(f"of {numel} elements" if numel is not None else f"of at least {at_least} element(s)")
    if like is not None:
        need.append(f"on {like.device}")
    if align:
        need.append(f"in {align}-byte aligned storage")
    return RuntimeError(f"{what}: {why} (need {' '.join(need)})")


def _shape_fits(got, want):
    """Slow path of _arg's shape check: `want` has wildcard entries (anything that is no int), or is no tuple."""
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):                      # (a plain loop: the anchors of the training path come here on every call)
        if w != g and isinstance(w, int):
            return False
    return True


def _shape_text(shape):
    return shape if isinstance(shape, str) else "[" + ", ".join(map(str, shape)) + "]"


def _ld(t):
    """Leading dimension of a 2-D tensor that passed _arg(rows=True) (a single row: its length)."""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _mod_ld(a, b=None):
    """Row stride of a modulation pair, (shift, scale) or (dshift, dscale) -- [B, D] views of one tensor: the first one given, 0 with neither."""
    return a.stride(0) if a is not None else (b.stride(0) if b is not None else 0)


def _mod_views(a, b, what_a, what_b, B, D, like, out=False):
    """A modulation pair -- (shift, scale) or (dshift, dscale); either may be None -- as the row kernels address it: two [B, D] f32 views read
    in place (copy=False) at ONE row stride, which is returned (_mod_ld)."""
    a = _arg(a, what_a, torch.float32, (B, D), rows=True, out=out, like=like, copy=False)
    b = _arg(b, what_b, torch.float32, (B, D), rows=True, out=out, like=like, copy=False)
    if a is not None and b is not None and B > 1 and a.stride(0) != b.stride(0):
        raise RuntimeError(f"{what_b}: row stride {b.stride(0)} against {a.stride(0)} of its partner (need two views at one row stride)")
    return _mod_ld(a, b)


def _batches(op, M, rows_per_batch):
    """B of M = B * rows_per_batch token rows (the rows of the modulation and gate views)."""
    if rows_per_batch <= 0 or M % rows_per_batch:
        raise RuntimeError(f"{op}: M={M} is not a multiple of rows_per_batch={rows_per_batch}")
    return M // rows_per_batch


def _pair(a, b, what):
    """The two operands of an NT product: same dtype, same K; both read as rows."""
    if b.dtype != a.dtype or a.dim() != 2 or b.dim() != 2 or b.shape[1] != a.shape[1]:
        raise RuntimeError(f"{what}: operands {tuple(a.shape)} {a.dtype} and {tuple(b.shape)} {b.dtype} must be [M,K] and [N,K] of one dtype")
    return _arg(a, what + " a", rows=True), _arg(b, what + " b", rows=True)


# ----------------------------------------------------------------------------- side stream for weight gradients
_side = {}


def side_stream(device):
    """One extra HIP stream per device for work that is off the backward critical path (the dW = dY^T X GEMMs: their results are
    only needed by the optimizer).  OPT-IN (LDMAE_TN_STREAM=1): measured 3-5 % SLOWER on MI355X -- the 160-KiB-LDS GEMM workgroups
    cannot share a CU with the persistent NT GEMM or the attention workgroups, so the streams mostly take turns and lose L2 locality."""
    st = _side.get(device)
    if st is None:
        st = torch.cuda.Stream(device=device)
        _side[device] = st
    return st


class SideGemms:
    """dW GEMMs of one backward on the side stream: `tn(a, b)` is ordered after everything enqueued so far on the current stream;
    `join()` makes the current stream wait for all of them (call before handing the results to autograd)."""

    def __init__(self, device, enabled=True):
        self.enabled = enabled and os.environ.get("LDMAE_TN_STREAM", "0") == "1"
        self.main = torch.cuda.current_stream(device)
        self.side = side_stream(device) if self.enabled else None

    def tn(self, a, b, out=None, beta=0.0):
        if not self.enabled:
            return gemm_tn(a, b, out=out, beta=beta)
        self.side.wait_stream(self.main)
        with torch.cuda.stream(self.side):
            return gemm_tn(a, b, out=out, beta=beta, ws_slot="tn_side")

    def join(self):
        if self.enabled:
            self.main.wait_stream(self.side)


# ----------------------------------------------------------------------------- GEMMs
# Launch mode of the bf16 GEMMs, owned by the CALLER (a train driver that knows it shares the chip with RCCL's collective kernels sets
# "tile"; everything else keeps "persistent") and handed to the library PER CALL as a flag in `epi` -- the C ABI keeps no mode.
# Until a driver says otherwise ("auto"): persistent, except in a process that belongs to a torch.distributed world of more than one rank
# (the reference's own train_accum.py under accelerate / DDP through the drop-in: nobody there calls set_gemm_launch_mode) -> tile.
_GEMM_MODE = "auto"
_AUTO_FLAG = None          # resolved once torch.distributed is initialised (the world does not change afterwards)


def set_gemm_launch_mode(mode: str) -> None:
    """"persistent" (one workgroup per CU walks the tiles), "tile" (one 256x256 tile per workgroup; bitwise-equal results) or "auto"."""
    global _GEMM_MODE
    if mode not in ("persistent", "tile", "auto"):
        raise ValueError(f"gemm launch mode {mode!r}: 'persistent', 'tile' or 'auto'")
    _GEMM_MODE = mode


_HALF_LINES = 0            # EPI_HALF_LINES while a test / tool asks for the half-line NT kernel (set_gemm_half_lines)


def set_gemm_half_lines(on: bool) -> None:
    """A/B switch of tests and tools: bf16 NT GEMMs keep the half-line kernel (gemm_nt_persist_kernel) where the whole-line kernel
    (gemm_nt_lines.hip, the default) would run.  Bitwise-equal results; a per-call flag of the C ABI like the launch mode."""
    global _HALF_LINES
    _HALF_LINES = EPI_HALF_LINES if on else 0


def _launch_flag() -> int:
    global _AUTO_FLAG
    if _GEMM_MODE != "auto":
        return (EPI_TILE_LAUNCH if _GEMM_MODE == "tile" else 0) | _HALF_LINES
    if _AUTO_FLAG is not None:
        return _AUTO_FLAG | _HALF_LINES
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return _HALF_LINES
    _AUTO_FLAG = EPI_TILE_LAUNCH if dist.get_world_size() > 1 else 0
    return _AUTO_FLAG | _HALF_LINES


def gemm_launch_mode() -> str:
    return "tile" if (_launch_flag() & EPI_TILE_LAUNCH) else "persistent"


def _grad_flag(dtype, grad) -> int:
    """fp16 GRADIENT outputs overflow to infinity (torch's fp16 autocast semantics: the loss scaler then skips the step); forward fp16 outputs
    saturate at +-65504.  A per-call flag of the C ABI (LDMAE_EPI_F16_INF)."""
    return EPI_F16_INF if (grad and dtype == torch.float16) else 0


def gemm_nt(a, b, bias=None, out_dtype=None, out=None, beta=0.0, grad=False):
    """out[M,N] = a[M,K] @ b[N,K]^T + bias (+ beta*out)."""
    a, b = _pair(a, b, "gemm_nt")
    M, K = a.shape
    N = b.shape[0]
    bias = _arg(bias, "gemm_nt bias", torch.float32, (N,))
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype or a.dtype, device=a.device)
    else:
        _arg(out, "gemm_nt out", out_dtype or (a.dtype, torch.float32), (M, N), rows=True, out=True)
    call("ldmae_gemm_nt", dt(a.dtype), dt(out.dtype), EPI_BIAS | _launch_flag() | _grad_flag(out.dtype, grad), ptr(a), _ld(a), ptr(b), _ld(b), ptr(out), _ld(out),
         M, N, K, ptr(bias), float(beta), None, None, None, 0, 0, stream())
    return out


def gemm_nt_gate_res(a, b, bias, xin, gate, rows_per_batch, save_y=True, xout=None, y_dtype=None):
    """y = a @ b^T + bias ; xout = xin + gate[batch] * y.  Returns (xout, y or None).  gate: [B, D] view (any row stride).
    The residual adds y ROUNDED to `y_dtype` (default: the activation type -- what the reference's autocast Linear hands to
    `x + gate * branch`, lightningdit.py:248-249); y_dtype=float32 with save_y=False adds the unrounded product."""
    a, b = _pair(a, b, "gemm_nt_gate_res")
    M, K = a.shape
    N = b.shape[0]
    nb = _batches("gemm_nt_gate_res", M, rows_per_batch)
    bias = _arg(bias, "gemm_nt_gate_res bias", torch.float32, (N,))
    xin = _arg(xin, "gemm_nt_gate_res xin", torch.float32, numel=M * N)
    gate = _arg(gate, "gemm_nt_gate_res gate", torch.float32, (nb, N), rows=True)
    y_dtype = y_dtype or a.dtype
    y = torch.empty(M, N, dtype=y_dtype, device=a.device) if save_y else None
    if xout is None:
        xout = torch.empty(M, N, dtype=torch.float32, device=a.device)
    else:
        _arg(xout, "gemm_nt_gate_res xout", torch.float32, out=True, numel=M * N)
    call("ldmae_gemm_nt", dt(a.dtype), dt(y_dtype), EPI_GATE_RES | _launch_flag(), ptr(a), _ld(a), ptr(b), _ld(b), ptr(y), N,
         M, N, K, ptr(bias), 0.0, ptr(xin), ptr(xout), ptr(gate), _ld(gate) if gate is not None else 0, rows_per_batch, stream())
    return xout, y


def gemm_nt_pos(a, b, bias, pos, rows_per_batch):
    """out = a @ b^T + bias + pos[row % rows_per_batch]   (f32 out; patch embed)."""
    a, b = _pair(a, b, "gemm_nt_pos")
    M, K = a.shape
    N = b.shape[0]
    bias = _arg(bias, "gemm_nt_pos bias", torch.float32, (N,))
    pos = _arg(pos, "gemm_nt_pos pos", torch.float32, numel=rows_per_batch * N)
    out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    call("ldmae_gemm_nt", dt(a.dtype), F32, EPI_BIAS_POS | _launch_flag(), ptr(a), _ld(a), ptr(b), _ld(b), ptr(out), N,
         M, N, K, ptr(bias), 0.0, ptr(pos), None, None, 0, rows_per_batch, stream())
    return out


def gemm_nt_gelu(a, b, bias, save_pre=True):
    """(gelu(a @ b^T + bias), pre-activation or None)."""
    a, b = _pair(a, b, "gemm_nt_gelu")
    M, K = a.shape
    N = b.shape[0]
    bias = _arg(bias, "gemm_nt_gelu bias", torch.float32, (N,))
    out = torch.empty(M, N, dtype=a.dtype, device=a.device)
    pre = torch.empty_like(out) if save_pre else None
    call("ldmae_gemm_nt", dt(a.dtype), dt(a.dtype), EPI_BIAS_GELU | _launch_flag(), ptr(a), _ld(a), ptr(b), _ld(b), ptr(out), N,
         M, N, K, ptr(bias), 0.0, None, ptr(pre), None, 0, 0, stream())
    return out, pre


def gemm_nt_gelu_bwd(dy, w2t, pre):
    """dpre = gelu_bwd(dy @ w2t^T, pre): the input gradient of fc2 with the GELU backward in the GEMM's epilogue (w2t = [hidden, D] transposed
    copy of fc2's weight; pre = fc1's pre-activation as gemm_nt_gelu saved it).  Same bits as gelu_bwd(gemm_nt(dy, w2t), pre)."""
    dy, w2t = _pair(dy, w2t, "gemm_nt_gelu_bwd")
    M, K = dy.shape
    N = w2t.shape[0]
    pre = _arg(pre, "gemm_nt_gelu_bwd pre", dy.dtype, numel=M * N)          # read with C's row stride N
    out = torch.empty(M, N, dtype=dy.dtype, device=dy.device)
    call("ldmae_gemm_nt", dt(dy.dtype), dt(dy.dtype), EPI_GELU_BWD | _launch_flag() | _grad_flag(dy.dtype, True), ptr(dy), _ld(dy), ptr(w2t), _ld(w2t), ptr(out), N,
         M, N, K, None, 0.0, ptr(pre), None, None, 0, 0, stream())
    return out


def gemm_nt_swiglu(a, w12, b12, save_h12=True):
    """(h12, hid): h12 = a @ w12^T + b12 ([x1 | x2]), hid = silu(x1) * x2.  bf16: one GEMM with the SwiGLU epilogue;
    otherwise the GEMM followed by ldmae_swiglu_fwd (same numbers: the epilogue rounds to bf16 before the activation).
    save_h12=False (forward-only; bf16 path): h12, which only the backward pass reads, is not stored and None is returned for it."""
    a, w12 = _pair(a, w12, "gemm_nt_swiglu")
    M, K = a.shape
    N = w12.shape[0]
    b12 = _arg(b12, "gemm_nt_swiglu bias", torch.float32, (N,))
    if a.dtype == torch.bfloat16 and N % 256 == 0 and K % 64 == 0:
        h12 = torch.empty(M, N, dtype=a.dtype, device=a.device) if save_h12 else None
        hid = torch.empty(M, N // 2, dtype=a.dtype, device=a.device)
        call("ldmae_gemm_nt", BF16, BF16, EPI_SWIGLU | _launch_flag(), ptr(a), _ld(a), ptr(w12), _ld(w12), ptr(h12), N, M, N, K, ptr(b12), 0.0,
             None, ptr(hid), None, 0, 0, stream())
        return h12, hid
    h12 = gemm_nt(a, w12, b12)
    return h12, swiglu_fwd(h12)


FUSED_QKV = os.environ.get("LDMAE_FUSED_QKV", "1") != "0"      # module switch for A/B runs (tools/bench_qkv_rope.py)
# A/B switch, read at call time: 1 = the training block forms its gated residuals in the norm's row pass (res_rmsnorm_modulate_fwd) and never
# stores the mid-block residual stream; 0 = the EPI_GATE_RES epilogue + rmsnorm_modulate_fwd pair.  Bitwise the same step either way.
FUSED_RESNORM = os.environ.get("LDMAE_FUSED_RESNORM", "1") != "0"


def gemm_nt_qkv_rope_ok(a, w, B, N, H, hd):
    """Does the fused qkv GEMM (QK-norm / RoPE in the epilogue) cover this call?  bf16, head dim 64, B*N % 256 == 0, N % 128 == 0, rows on 128-B lines.
    LDMAE_FUSED_QKV=0 keeps the GEMM + ldmae_qknorm_rope_fwd pair (A/B runs; bitwise the same q2 / k2)."""
    if a.dtype != torch.bfloat16 or not FUSED_QKV or _HALF_LINES:
        return False
    if a.data_ptr() % 128 or w.data_ptr() % 128 or w.shape[0] != 3 * H * hd or a.stride(1) != 1 or w.stride(1) != 1:
        return False
    return bool(L.load().ldmae_gemm_nt_qkv_rope_ok(B, N, H, hd, a.shape[1], a.stride(0), w.stride(0)))


def gemm_nt_qkv_rope(a, w, bias, wq, wk, cos, sin, B, N, H, hd, eps=1e-6, store_raw_qk=True):
    """(qkv, q2, k2): the qkv Linear with q_norm / k_norm / RoPE applied in its epilogue (lightningdit.py:68-74 in one kernel).  qkv [B*N, 3*H*hd] as
    gemm_nt writes it (store_raw_qk=False -- forward-only: only the v third is written, the q / k thirds stay uninitialised), q2 / k2 [B, H, N, hd] bitwise
    what qknorm_rope_fwd makes of the stored q / k.  wq = wk = None: RoPE only.  Call gemm_nt_qkv_rope_ok first."""
    a, w = _pair(a, w, "gemm_nt_qkv_rope")
    M, K = a.shape
    if M != B * N or w.shape[0] != 3 * H * hd:
        raise RuntimeError(f"gemm_nt_qkv_rope: operands {tuple(a.shape)} and {tuple(w.shape)} must be [B*N, K] and [3*H*hd, K] = [{B * N}, K] and [{3 * H * hd}, K]")
    bias = _arg(bias, "gemm_nt_qkv_rope bias", torch.float32, (3 * H * hd,), like=a)
    wq, wk = _arg(wq, "gemm_nt_qkv_rope wq", torch.float32, (hd,), like=a), _arg(wk, "gemm_nt_qkv_rope wk", torch.float32, (hd,), like=a)
    cos, sin = _arg(cos, "gemm_nt_qkv_rope cos", torch.float32, (N, hd), like=a), _arg(sin, "gemm_nt_qkv_rope sin", torch.float32, (N, hd), like=a)
    qkv = torch.empty(M, 3 * H * hd, dtype=a.dtype, device=a.device)
    q2 = torch.empty(B, H, N, hd, dtype=a.dtype, device=a.device)
    k2 = torch.empty_like(q2)
    call("ldmae_gemm_nt_qkv_rope", ptr(a), _ld(a), ptr(w), _ld(w), ptr(bias), ptr(qkv), ptr(q2), ptr(k2), ptr(wq), ptr(wk), ptr(cos), ptr(sin),
         B, N, H, hd, K, eps, 1 if store_raw_qk else 0, 1 if (_launch_flag() & EPI_TILE_LAUNCH) else 0, stream())
    return qkv, q2, k2


# ----------------------------------------------------------------------------- MXFP8 sampling mode (include/ldmae_hip.h: the contract)
def mx8_quantize(x):
    """(q [M,K] uint8 e4m3fn bytes, scales [M,K/32] uint8 E8M0 bytes) of the rows of x (f32 or bf16; K % 128 == 0; rows may be strided)."""
    if x.dtype not in (torch.float32, torch.bfloat16) or x.dim() != 2:
        raise RuntimeError(f"mx8_quantize: a 2-D float32 or bfloat16 tensor, got {tuple(x.shape)} {x.dtype}")
    x = _arg(x, "mx8_quantize x", rows=True)
    M, K = x.shape
    if K % 128:
        raise RuntimeError(f"mx8_quantize: K={K} is not a multiple of 128")
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    sc = torch.empty(M, K // 32, dtype=torch.uint8, device=x.device)
    call("ldmae_mx8_quantize", dt(x.dtype), ptr(x), _ld(x), ptr(q), ptr(sc), M, K, stream())
    return q, sc


def rmsnorm_modulate_fwd_mx8(x, w, shift, scale, rows_per_batch, eps=1e-6):
    """(q, scales, rstd): rmsnorm_modulate_fwd(..., torch.bfloat16) and mx8_quantize of its output in one kernel, bitwise the pair."""
    x = _arg(x, "rmsnorm_modulate_fwd_mx8 x", torch.float32, ("M", "D"))
    M, D = x.shape
    if w is None:
        raise RuntimeError("rmsnorm_modulate_fwd_mx8: needs the RMSNorm weight (the LayerNorm form is not built in this mode)")
    if D % 128:
        raise RuntimeError(f"rmsnorm_modulate_fwd_mx8: D={D} is not a multiple of 128")
    B = _batches("rmsnorm_modulate_fwd_mx8", M, rows_per_batch)
    w = _arg(w, "rmsnorm_modulate_fwd_mx8 w", torch.float32, (D,), like=x)
    ld = _mod_views(shift, scale, "rmsnorm_modulate_fwd_mx8 shift", "rmsnorm_modulate_fwd_mx8 scale", B, D, x)
    q = torch.empty(M, D, dtype=torch.uint8, device=x.device)
    sc = torch.empty(M, D // 32, dtype=torch.uint8, device=x.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    call("ldmae_rmsnorm_modulate_fwd_mx8", ptr(x), ptr(w), ptr(shift), ptr(scale), ld, ptr(q), ptr(sc), ptr(rstd), M, D, rows_per_batch, eps, stream())
    return q, sc, rstd


def _mx8_pair(aq, asc, wq, wsc, what):
    """The operands of a block-scaled NT product: uint8 elements [M,K] / [N,K] read as rows, dense uint8 scales [M,K/32] / [N,K/32]."""
    for t, name in ((aq, "aq"), (asc, "a scales"), (wq, "wq"), (wsc, "w scales")):
        if t.dtype != torch.uint8 or t.dim() != 2:
            raise RuntimeError(f"{what} {name}: a 2-D uint8 tensor, got {tuple(t.shape)} {t.dtype}")
    if wq.shape[1] != aq.shape[1] or aq.shape[1] % 128:
        raise RuntimeError(f"{what}: operands {tuple(aq.shape)} and {tuple(wq.shape)} must be [M,K] and [N,K] with K % 128 == 0")
    K = aq.shape[1]
    aq, wq = _arg(aq, what + " aq", rows=True), _arg(wq, what + " wq", rows=True)
    asc = _arg(asc, what + " a scales", torch.uint8, (aq.shape[0], K // 32))
    wsc = _arg(wsc, what + " w scales", torch.uint8, (wq.shape[0], K // 32))
    return aq, asc, wq, wsc


def gemm_nt_mx8(aq, asc, wq, wsc, bias=None, out_dtype=torch.bfloat16, out=None):
    """out[M,N] = dequant(aq, asc) @ dequant(wq, wsc)^T + bias on the block-scaled fp8 MFMA; out bf16 or f32."""
    aq, asc, wq, wsc = _mx8_pair(aq, asc, wq, wsc, "gemm_nt_mx8")
    M, K = aq.shape
    N = wq.shape[0]
    bias = _arg(bias, "gemm_nt_mx8 bias", torch.float32, (N,))
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=aq.device)
    else:
        _arg(out, "gemm_nt_mx8 out", out_dtype, (M, N), rows=True, out=True)
    call("ldmae_gemm_nt_mx8", dt(out.dtype), EPI_BIAS | (_launch_flag() & EPI_TILE_LAUNCH), ptr(aq), ptr(asc), _ld(aq), ptr(wq), ptr(wsc), _ld(wq), ptr(out), _ld(out),
         M, N, K, ptr(bias), None, None, None, 0, 0, stream())
    return out


def gemm_nt_gate_res_mx8(aq, asc, wq, wsc, bias, xin, gate, rows_per_batch, save_y=False, xout=None, y_dtype=torch.bfloat16):
    """gemm_nt_gate_res on block-scaled fp8 operands: y = dequant(a) @ dequant(w)^T + bias ; xout = xin + gate[batch] * y (y rounded to y_dtype)."""
    aq, asc, wq, wsc = _mx8_pair(aq, asc, wq, wsc, "gemm_nt_gate_res_mx8")
    M, K = aq.shape
    N = wq.shape[0]
    nb = _batches("gemm_nt_gate_res_mx8", M, rows_per_batch)
    bias = _arg(bias, "gemm_nt_gate_res_mx8 bias", torch.float32, (N,))
    xin = _arg(xin, "gemm_nt_gate_res_mx8 xin", torch.float32, numel=M * N)
    gate = _arg(gate, "gemm_nt_gate_res_mx8 gate", torch.float32, (nb, N), rows=True)
    y = torch.empty(M, N, dtype=y_dtype, device=aq.device) if save_y else None
    if xout is None:
        xout = torch.empty(M, N, dtype=torch.float32, device=aq.device)
    else:
        _arg(xout, "gemm_nt_gate_res_mx8 xout", torch.float32, out=True, numel=M * N)
    call("ldmae_gemm_nt_mx8", dt(y_dtype), EPI_GATE_RES | (_launch_flag() & EPI_TILE_LAUNCH), ptr(aq), ptr(asc), _ld(aq), ptr(wq), ptr(wsc), _ld(wq), ptr(y), N,
         M, N, K, ptr(bias), ptr(xin), ptr(xout), ptr(gate), _ld(gate) if gate is not None else 0, rows_per_batch, stream())
    return xout, y


def gemm_nt_swiglu_mx8(aq, asc, w12q, w12sc, b12, save_h12=False):
    """(h12 or None, hid) of gemm_nt_swiglu on block-scaled fp8 operands (bf16 outputs; N = 2 Hs a multiple of 256)."""
    aq, asc, w12q, w12sc = _mx8_pair(aq, asc, w12q, w12sc, "gemm_nt_swiglu_mx8")
    M, K = aq.shape
    N = w12q.shape[0]
    if N % 256:
        raise RuntimeError(f"gemm_nt_swiglu_mx8: N={N} (2 * hidden) is not a multiple of 256")
    b12 = _arg(b12, "gemm_nt_swiglu_mx8 bias", torch.float32, (N,))
    h12 = torch.empty(M, N, dtype=torch.bfloat16, device=aq.device) if save_h12 else None
    hid = torch.empty(M, N // 2, dtype=torch.bfloat16, device=aq.device)
    call("ldmae_gemm_nt_mx8", BF16, EPI_SWIGLU | (_launch_flag() & EPI_TILE_LAUNCH), ptr(aq), ptr(asc), _ld(aq), ptr(w12q), ptr(w12sc), _ld(w12q), ptr(h12), N,
         M, N, K, ptr(b12), None, ptr(hid), None, 0, 0, stream())
    return h12, hid


def gemm_nt_qkv_rope_mx8_ok(aq, wq, B, N, H, hd):
    """Does the block-scaled qkv GEMM with the QK-norm / RoPE epilogue cover this call?  (head dim 64, B*N % 256 == 0, N % 128 == 0)"""
    if aq.dtype != torch.uint8 or wq.dtype != torch.uint8 or aq.dim() != 2 or wq.dim() != 2:
        return False
    if aq.data_ptr() % 128 or wq.data_ptr() % 128 or wq.shape[0] != 3 * H * hd or aq.stride(1) != 1 or wq.stride(1) != 1:
        return False
    return bool(L.load().ldmae_gemm_nt_qkv_rope_mx8_ok(B, N, H, hd, aq.shape[1], aq.stride(0), wq.stride(0)))


def gemm_nt_qkv_rope_mx8(aq, asc, wq, wsc, bias, nwq, nwk, cos, sin, B, N, H, hd, eps=1e-6, store_raw_qk=False):
    """(qkv, q2, k2) of gemm_nt_qkv_rope on block-scaled fp8 operands (nwq / nwk: the QK-norm weights, None: RoPE only).  Call
    gemm_nt_qkv_rope_mx8_ok first."""
    aq, asc, wq, wsc = _mx8_pair(aq, asc, wq, wsc, "gemm_nt_qkv_rope_mx8")
    M, K = aq.shape
    if M != B * N or wq.shape[0] != 3 * H * hd:
        raise RuntimeError(f"gemm_nt_qkv_rope_mx8: operands {tuple(aq.shape)} and {tuple(wq.shape)} must be [B*N, K] and [3*H*hd, K] = [{B * N}, K] and [{3 * H * hd}, K]")
    bias = _arg(bias, "gemm_nt_qkv_rope_mx8 bias", torch.float32, (3 * H * hd,), like=aq)
    nwq, nwk = _arg(nwq, "gemm_nt_qkv_rope_mx8 nwq", torch.float32, (hd,), like=aq), _arg(nwk, "gemm_nt_qkv_rope_mx8 nwk", torch.float32, (hd,), like=aq)
    cos, sin = _arg(cos, "gemm_nt_qkv_rope_mx8 cos", torch.float32, (N, hd), like=aq), _arg(sin, "gemm_nt_qkv_rope_mx8 sin", torch.float32, (N, hd), like=aq)
    qkv = torch.empty(M, 3 * H * hd, dtype=torch.bfloat16, device=aq.device)
    q2 = torch.empty(B, H, N, hd, dtype=torch.bfloat16, device=aq.device)
    k2 = torch.empty_like(q2)
    call("ldmae_gemm_nt_qkv_rope_mx8", ptr(aq), ptr(asc), _ld(aq), ptr(wq), ptr(wsc), _ld(wq), ptr(bias), ptr(qkv), ptr(q2), ptr(k2), ptr(nwq), ptr(nwk),
         ptr(cos), ptr(sin), B, N, H, hd, K, eps, 1 if store_raw_qk else 0, 1 if (_launch_flag() & EPI_TILE_LAUNCH) else 0, stream())
    return qkv, q2, k2


def gemm_nt_swiglu_bwd(dy, w3t, h12, with_bias=False):
    """dh12 = swiglu_bwd(dy @ w3t^T, h12)   (w3t = [Hs, D] transposed copy of w3).  with_bias: also the column sums of dh12 (the
    bias gradient of w12), formed in the GEMM epilogue as per-128-row partials and summed here."""
    dy, w3t = _pair(dy, w3t, "gemm_nt_swiglu_bwd")
    M, K = dy.shape
    Hs = w3t.shape[0]
    h12 = _arg(h12, "gemm_nt_swiglu_bwd h12", dy.dtype, numel=M * 2 * Hs)
    if dy.dtype == torch.bfloat16 and Hs % 8 == 0 and K % 64 == 0:
        dh12 = torch.empty(h12.shape, dtype=dy.dtype, device=dy.device)
        # every (128-row group, column) of the partial-sum matrix is written by exactly one wave when the tile grid is whole: no 33 MB fill
        whole = M % 128 == 0 and Hs % 64 == 0
        part = (torch.empty if whole else torch.zeros)((M + 127) // 128, 2 * Hs, dtype=torch.float32, device=dy.device) if with_bias else None
        call("ldmae_gemm_nt", BF16, BF16, EPI_SWIGLU_BWD | _launch_flag(), ptr(dy), _ld(dy), ptr(w3t), _ld(w3t), ptr(dh12), 2 * Hs, M, Hs, K, None, 0.0,
             ptr(h12), ptr(part), None, 0, 0, stream())
        return (dh12, colsum(part)) if with_bias else dh12
    dh12 = swiglu_bwd(gemm_nt(dy, w3t), h12)
    return (dh12, colsum(dh12)) if with_bias else dh12


def gemm_tn(a, b, out=None, beta=0.0, with_bias=False, ws_slot="tn", dbias_out=None):
    """out[N,K] (f32) = beta*out + a[M,N]^T @ b[M,K]   (weight gradient).  with_bias: also return the column sums of `a`
    (the bias gradient of the same Linear), fused into the same kernel on the bf16 path.  dbias_out (f32 [N], contiguous): the bias gradient
    is accumulated THERE under the same beta as `out` (a .grad slab view: no fresh zero-filled buffer, no add afterwards)."""
    if b.dtype != a.dtype or a.dim() != 2 or b.dim() != 2 or b.shape[0] != a.shape[0]:
        raise RuntimeError(f"gemm_tn: operands {tuple(a.shape)} {a.dtype} and {tuple(b.shape)} {b.dtype} must be [M,N] and [M,K] of one dtype")
    a, b = _arg(a, "gemm_tn a", rows=True), _arg(b, "gemm_tn b", rows=True)
    M, N = a.shape
    K = b.shape[1]
    if out is None:
        out = torch.empty(N, K, dtype=torch.float32, device=a.device)
        beta = 0.0
    else:
        _arg(out, "gemm_tn out", torch.float32, (N, K), out=True)
    if dbias_out is not None:
        if not with_bias:
            raise RuntimeError("gemm_tn: dbias_out must be a contiguous f32 [N] buffer and needs with_bias=True")
        dbias = _arg(dbias_out, "gemm_tn dbias_out", torch.float32, (N,), out=True)
    else:
        # the C entry applies ONE beta to C and to dbias: a fresh bias-gradient buffer must be zero when the caller accumulates into `out`
        dbias = (torch.zeros if beta != 0.0 else torch.empty)(N, dtype=torch.float32, device=a.device) if with_bias else None
    d = dt(a.dtype)
    nb = max(_ws_bytes("ldmae_gemm_tn_workspace_bytes", d, M, N, K), _ws_bytes("ldmae_colsum_workspace_bytes", M, N) if with_bias else 0)
    ws = workspace(nb, a.device, ws_slot)
    call("ldmae_gemm_tn", d, ptr(a), _ld(a), ptr(b), _ld(b), ptr(out), ptr(dbias), M, N, K, float(beta), ptr(ws), ws.numel() * 4,
         stream())
    return (out, dbias) if with_bias else out


def colsum(x, out=None, beta=0.0):
    x = _arg(x, "colsum x", _FLOATS, ("M", "N"), rows=True)
    M, N = x.shape
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=x.device)
        beta = 0.0
    else:
        _arg(out, "colsum out", torch.float32, (N,), out=True)
    ws = workspace(_ws_bytes("ldmae_colsum_workspace_bytes", M, N), x.device, "colsum")
    call("ldmae_colsum", dt(x.dtype), ptr(x), _ld(x), M, N, ptr(out), float(beta), ptr(ws), stream())
    return out


def cast_weight(w, dtype, transposed=True, straight=True):
    """f32 master weight [R,C] -> (copy in `dtype` or None, [C,R] transposed copy or None)."""
    w = _arg(w, "cast_weight w", torch.float32, ("R", "C"))
    R, C = w.shape
    dst = torch.empty(R, C, dtype=dtype, device=w.device) if straight else None
    dstT = torch.empty(C, R, dtype=dtype, device=w.device) if transposed else None
    call("ldmae_cast_weight", dt(dtype), ptr(w), ptr(dst), ptr(dstT), R, C, stream())
    return dst, dstT


def cast(x, dtype):
    if x.dtype == dtype:
        return x
    x = _arg(x, "cast x", _FLOATS)
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    call("ldmae_cast", dt(x.dtype), dt(dtype), ptr(x), ptr(out), x.numel(), stream())
    return out


_THIN = os.environ.get("LDMAE_THIN_GEMM", "1") != "0"       # 0: the generic f32 MFMA GEMMs for these shapes too (A/B)


def thin_ok(N, K):
    """Shapes the thin (K = 16 / 32) f32 products take: see ldmae_thin_nt / ldmae_thin_tn."""
    return _THIN and K in (16, 32) and N % 4 == 0


def thin_nt(t, w, bias=None, pos=None, rows_per_batch=0, out_dtype=torch.float32):
    """out[M,N] = t[M,K] @ w[N,K]^T + bias (+ pos[row % rows_per_batch]) for K = 16 / 32, f32 inputs; one streaming pass."""
    t = _arg(t, "thin_nt t", torch.float32, ("M", "K"))
    M, K = t.shape
    w = _arg(w, "thin_nt w", torch.float32, ("N", K), like=t)
    N = w.shape[0]
    bias = _arg(bias, "thin_nt bias", torch.float32, (N,), like=t)
    pos = _arg(pos, "thin_nt pos", torch.float32, numel=rows_per_batch * N, like=t)
    out = torch.empty(M, N, dtype=out_dtype, device=t.device)
    call("ldmae_thin_nt", dt(out_dtype), ptr(t), ptr(w), ptr(bias), ptr(pos), ptr(out), M, N, K,
         int(rows_per_batch), stream())
    return out


def thin_tn(g, t, with_bias=True):
    """(dW[N,K] = g[M,N]^T @ t[M,K], column sums of g or None) for K = 16 / 32, f32; one pass over g."""
    g = _arg(g, "thin_tn g", torch.float32, ("M", "N"))
    M, N = g.shape
    t = _arg(t, "thin_tn t", torch.float32, (M, "K"), like=g)
    K = t.shape[1]
    dW = torch.empty(N, K, dtype=torch.float32, device=g.device)
    db = torch.empty(N, dtype=torch.float32, device=g.device) if with_bias else None
    ws = workspace(_ws_bytes("ldmae_thin_tn_workspace_bytes", M, N, K), g.device)
    call("ldmae_thin_tn", ptr(g), ptr(t), ptr(dW), ptr(db), M, N, K, 0.0, ptr(ws), ws.numel() * 4, stream())
    return dW, db


def multi_add_(dsts, srcs):
    """dsts[i] += srcs[i] (contiguous f32 tensors of equal sizes pairwise), one launch."""
    k = len(dsts)
    if len(srcs) != k:
        raise RuntimeError(f"multi_add_: {k} destinations with {len(srcs)} sources")
    for d_ in dsts:
        _arg(d_, "multi_add_ dst (contiguous f32 pairs of equal size)", torch.float32, out=True, like=dsts[0])
    srcs = [_arg(s_, "multi_add_ src (contiguous f32 pairs of equal size)", torch.float32, numel=d_.numel(), like=d_) for d_, s_ in zip(dsts, srcs)]
    da = (ctypes.c_void_p * k)(*[d_.data_ptr() for d_ in dsts])
    sa = (ctypes.c_void_p * k)(*[s_.data_ptr() for s_ in srcs])
    na = (ctypes.c_long * k)(*[d_.numel() for d_ in dsts])
    call("ldmae_multi_add", k, da, sa, na, stream())


def cast_stack(tensors, dtype):
    """Equally shaped contiguous f32 tensors -> one stacked [len * rows, cols] tensor in `dtype`, one launch."""
    t0 = tensors[0]
    n_each = t0.numel()
    srcs = [_arg(t, "cast_stack source (f32 tensors of one size)", torch.float32, numel=n_each, like=t0) for t in tensors]
    if t0.dim() < 1:
        raise RuntimeError("cast_stack source (f32 tensors of one size): at least one dimension expected")
    out = torch.empty((len(tensors) * t0.shape[0],) + tuple(t0.shape[1:]), dtype=dtype, device=t0.device)
    arr = (ctypes.c_void_p * len(srcs))(*[t.data_ptr() for t in srcs])
    call("ldmae_cast_stack", dt(dtype), arr, len(srcs), n_each, ptr(out), stream())
    return out


# ----------------------------------------------------------------------------- norms / elementwise
def rmsnorm_modulate_fwd(x, w, shift, scale, rows_per_batch, out_dtype, eps=1e-6):
    """modulate(norm(x), shift, scale) (lightningdit.py:26-30,248-249).  w: the RMSNorm weight; w=None: nn.LayerNorm(elementwise_affine=False)
    -- the blocks built with use_rmsnorm=False (:200-201) -- on the same kernels (the norm of the centred row)."""
    x = _arg(x, "rmsnorm_modulate_fwd x", torch.float32, ("M", "D"))
    M, D = x.shape
    B = _batches("rmsnorm_modulate_fwd", M, rows_per_batch)
    w = _arg(w, "rmsnorm_modulate_fwd w", torch.float32, (D,), like=x)
    ld = _mod_views(shift, scale, "rmsnorm_modulate_fwd shift", "rmsnorm_modulate_fwd scale", B, D, x)
    out = torch.empty(M, D, dtype=out_dtype, device=x.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    if w is None:
        call("ldmae_layernorm_modulate_fwd", dt(out_dtype), ptr(x), ptr(shift), ptr(scale), ld, ptr(out), ptr(rstd), M, D, rows_per_batch, eps, stream())
        return out, rstd
    call("ldmae_rmsnorm_modulate_fwd", dt(out_dtype), ptr(x), ptr(w), ptr(shift), ptr(scale), ld, ptr(out), ptr(rstd), M, D,
         rows_per_batch, eps, stream())
    return out, rstd


def res_rmsnorm_modulate_fwd(x, ya, gate_a, yb=None, gate_b=None, w=None, shift=None, scale=None, rows_per_batch=0, eps=1e-6,
                             want_xout=False, want_norm=True):
    """The gated residual(s) of a block and the norm behind them in one pass over the rows: r = x + gate_a[b] * ya (+ gate_b[b] * yb);
    -> (xout or None, xm or None, rstd or None) with xout = r (f32) and (xm, rstd) = rmsnorm_modulate_fwd(r, w, shift, scale) in ya's
    type.  ya / yb: the Linear outputs as stored (bf16 / fp16); gates [B, D] f32 views (any row stride).  Bitwise gemm_nt_gate_res's
    residual followed by rmsnorm_modulate_fwd."""
    x = _arg(x, "res_rmsnorm_modulate_fwd x", torch.float32, ("M", "D"))
    M, D = x.shape
    if not (want_xout or want_norm):
        raise RuntimeError("res_rmsnorm_modulate_fwd: nothing requested (want_xout / want_norm)")
    B = _batches("res_rmsnorm_modulate_fwd", M, rows_per_batch)
    ya = _arg(ya, "res_rmsnorm_modulate_fwd ya (bfloat16 or float16 branch outputs of one type)", _B16, (M, D), like=x)
    yb = _arg(yb, "res_rmsnorm_modulate_fwd yb (bfloat16 or float16 branch outputs of one type)", ya.dtype, (M, D), like=x)
    gate_a = _arg(gate_a, "res_rmsnorm_modulate_fwd gate_a", torch.float32, (B, D), rows=True, like=x)
    gate_b = _arg(gate_b, "res_rmsnorm_modulate_fwd gate_b", torch.float32, (B, D), rows=True, like=x)
    xout = torch.empty(M, D, dtype=torch.float32, device=x.device) if want_xout else None
    out = rstd = None
    ld = 0
    if want_norm:
        w = _arg(w, "res_rmsnorm_modulate_fwd w", torch.float32, (D,), like=x)
        ld = _mod_views(shift, scale, "res_rmsnorm_modulate_fwd shift", "res_rmsnorm_modulate_fwd scale", B, D, x)
        out = torch.empty(M, D, dtype=ya.dtype, device=x.device)
        rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    else:
        w = shift = scale = None
    call("ldmae_res_rmsnorm_modulate_fwd", dt(ya.dtype), ptr(x), ptr(ya), ptr(gate_a), _ld(gate_a), ptr(yb), ptr(gate_b),
         _ld(gate_b) if gate_b is not None else 0, ptr(xout), ptr(w), ptr(shift), ptr(scale), ld, ptr(out), ptr(rstd), M, D, rows_per_batch, eps,
         stream())
    return xout, out, rstd


def _norm_bwd_checked(dout, x, w, scale, rstd, dx_accum, dshift, dscale, rows_per_batch, y=None, gate=None, dgate=None):
    """The checks of the five norm + modulate backward forms, once (RMSNorm / LayerNorm, alone or with the gate backward and its recompute
    form: y, gate, dgate) -> (M, D, and what the kernel reads densely, copied where it must be: dout, x, w, rstd, y)."""
    x = _arg(x, "rmsnorm_modulate_bwd x", torch.float32, ("M", "D"))
    M, D = x.shape
    B = _batches("rmsnorm_modulate_bwd", M, rows_per_batch)
    dout = _arg(dout, "rmsnorm_modulate_bwd dout", _F32_BF16, (M, D), like=x)
    w = _arg(w, "rmsnorm_modulate_bwd w", torch.float32, (D,), like=x)
    _mod_views(scale, None, "rmsnorm_modulate_bwd scale", None, B, D, x)
    rstd = _arg(rstd, "rmsnorm_modulate_bwd rstd", torch.float32, (M,), like=x)
    _arg(dx_accum, "rmsnorm_modulate_bwd dx_accum", torch.float32, (M, D), out=True, like=x)
    _mod_views(dshift, dscale, "rmsnorm_modulate_bwd dshift", "rmsnorm_modulate_bwd dscale", B, D, x, out=True)
    y = _arg(y, "rmsnorm_modulate_bwd y", dout.dtype, (M, D), like=x)
    _arg(gate, "rmsnorm_modulate_bwd gate", torch.float32, (B, D), rows=True, like=x, copy=False)
    _arg(dgate, "rmsnorm_modulate_bwd dgate", torch.float32, (B, D), rows=True, out=True, like=x)
    return M, D, dout, x, w, rstd, y


def _norm_bwd_args(dout, x, w, scale, rstd, dx_accum, dshift, dscale, accumulate, dw):
    """The leading arguments of the four ldmae_*norm_modulate_bwd* entries; the LayerNorm forms (w is None) take neither w nor dw / beta_w."""
    head = [dt(dout.dtype), ptr(dout), ptr(x)] + ([] if w is None else [ptr(w)])
    return head + [ptr(scale), _mod_ld(scale), ptr(rstd), ptr(dx_accum), 1.0 if accumulate else 0.0, ptr(dshift), ptr(dscale),
                   _mod_ld(dshift, dscale)] + ([] if w is None else [ptr(dw), 0.0])


def rmsnorm_modulate_bwd(dout, x, w, scale, rstd, dx_accum, dshift, dscale, rows_per_batch, accumulate=True):
    """dx_accum += dx (in place; accumulate=False: dx_accum = dx, the buffer may be uninitialised); writes dshift/dscale views ([B,D], any
    row stride); returns dw [D] (None for w=None: LayerNorm without affine parameters, use_rmsnorm=False, has no weight gradient)."""
    M, D, dout, x, w, rstd, _ = _norm_bwd_checked(dout, x, w, scale, rstd, dx_accum, dshift, dscale, rows_per_batch)
    ws = workspace(_ws_bytes("ldmae_rmsnorm_modulate_bwd_workspace_bytes", M, D, rows_per_batch), x.device)
    dw = None if w is None else torch.empty(D, dtype=torch.float32, device=x.device)
    call("ldmae_layernorm_modulate_bwd" if w is None else "ldmae_rmsnorm_modulate_bwd",
         *_norm_bwd_args(dout, x, w, scale, rstd, dx_accum, dshift, dscale, accumulate, dw), M, D, rows_per_batch, ptr(ws), stream())
    return dw


def rmsnorm_modulate_bwd_gate(dout, x, w, scale, rstd, dx_accum, dshift, dscale, y, gate, dgate, rows_per_batch, act_dtype, accumulate=True,
                              recompute=False):
    """rmsnorm_modulate_bwd followed by gate_bwd(dx_accum, y, gate, dgate, with_bias=True) in one pass over the rows.
    Returns (dw [D] or None as above, dy [M,D] act dtype, dbias [D]).  recompute: `x` is the residual stream BEFORE the gated residual under
    the norm (the forward ran res_rmsnorm_modulate_fwd and never stored the normalised row); the kernel rebuilds that row as x + gate * y.
    Bitwise the plain form handed the row materialised; bf16, RMSNorm form."""
    if recompute and (w is None or dout.dtype != torch.bfloat16):
        raise RuntimeError("rmsnorm_modulate_bwd_gate(recompute=True): the RMSNorm form with bfloat16 activations only")
    if y is None or gate is None or dgate is None or act_dtype != dout.dtype:
        raise RuntimeError(f"rmsnorm_modulate_bwd_gate: needs y, gate and dgate, and act_dtype {act_dtype} = dout's {dout.dtype} (y is read, dy written in it)")
    M, D, dout, x, w, rstd, y = _norm_bwd_checked(dout, x, w, scale, rstd, dx_accum, dshift, dscale, rows_per_batch, y, gate, dgate)
    dy = torch.empty(M, D, dtype=act_dtype, device=x.device)
    dbias = torch.empty(D, dtype=torch.float32, device=x.device)
    ws = workspace(_ws_bytes("ldmae_rmsnorm_modulate_bwd_gate_workspace_bytes", M, D, rows_per_batch), x.device)
    dw = None if w is None else torch.empty(D, dtype=torch.float32, device=x.device)
    entry = "ldmae_layernorm_modulate_bwd_gate" if w is None else "ldmae_rmsnorm_modulate_bwd_gate" + ("_recompute" if recompute else "")
    call(entry, *_norm_bwd_args(dout, x, w, scale, rstd, dx_accum, dshift, dscale, accumulate, dw), ptr(y), ptr(gate), gate.stride(0),
         ptr(dy), ptr(dgate), dgate.stride(0), ptr(dbias), M, D, rows_per_batch, ptr(ws), stream())
    return dw, dy, dbias


def qknorm_rope_fwd(qkv, wq, wk, cos, sin, B, N, H, hd, eps=1e-6, copy_v=True):
    """copy_v=False: v gets no head-major copy (returned as None); attention then reads it from the packed qkv (attention_fwd_pv).
    wq = wk = None: RoPE only (the block built with use_qknorm=False: q_norm = k_norm = nn.Identity, lightningdit.py:60-61)."""
    qkv = _arg(qkv, "qknorm_rope_fwd qkv", _F32_BF16, numel=B * N * 3 * H * hd)
    wq, wk = _arg(wq, "qknorm_rope_fwd wq", torch.float32, (hd,), like=qkv), _arg(wk, "qknorm_rope_fwd wk", torch.float32, (hd,), like=qkv)
    cos, sin = _arg(cos, "qknorm_rope_fwd cos", torch.float32, (N, hd), like=qkv), _arg(sin, "qknorm_rope_fwd sin", torch.float32, (N, hd), like=qkv)
    q = torch.empty(B, H, N, hd, dtype=qkv.dtype, device=qkv.device)
    k = torch.empty_like(q)
    v = torch.empty_like(q) if copy_v else None
    call("ldmae_qknorm_rope_fwd", dt(qkv.dtype), ptr(qkv), ptr(wq), ptr(wk), ptr(cos), ptr(sin), ptr(q), ptr(k), ptr(v), B, N, H, hd, eps, stream())
    return q, k, v


def qknorm_rope_bwd(dq, dk, dv, qkv, wq, wk, cos, sin, B, N, H, hd, eps=1e-6, with_bias=False, dqkv=None):
    """Backward of qknorm_rope_fwd: (dqkv [B,N,3,H,hd], dwq, dwk[, dbias [3*H*hd]]).  with_bias: the bias gradient of the qkv Linear
    (column sums of dqkv as stored), formed in the same pass.  dv=None with dqkv given: dv already sits in the v slot of dqkv
    (attention_bwd_pv) and is left there."""
    qkv = _arg(qkv, "qknorm_rope_bwd qkv", _F32_BF16, numel=B * N * 3 * H * hd)
    dq, dk = _arg(dq, "qknorm_rope_bwd dq", qkv.dtype, (B, H, N, hd), like=qkv), _arg(dk, "qknorm_rope_bwd dk", qkv.dtype, (B, H, N, hd), like=qkv)
    dv = _arg(dv, "qknorm_rope_bwd dv", qkv.dtype, (B, H, N, hd), like=qkv)
    wq, wk = _arg(wq, "qknorm_rope_bwd wq", torch.float32, (hd,), like=qkv), _arg(wk, "qknorm_rope_bwd wk", torch.float32, (hd,), like=qkv)
    cos, sin = _arg(cos, "qknorm_rope_bwd cos", torch.float32, (N, hd), like=qkv), _arg(sin, "qknorm_rope_bwd sin", torch.float32, (N, hd), like=qkv)
    if dqkv is None:
        dqkv = torch.empty(qkv.shape, dtype=qkv.dtype, device=qkv.device)
    else:
        _arg(dqkv, "qknorm_rope_bwd dqkv", qkv.dtype, numel=qkv.numel(), out=True, like=qkv)
    dwq = torch.empty(hd, dtype=torch.float32, device=qkv.device) if wq is not None else None      # wq = wk = None: RoPE adjoint only
    dwk = torch.empty_like(dwq) if wq is not None else None
    db = torch.empty(H, 3, hd, dtype=torch.float32, device=qkv.device) if with_bias else None
    ws = workspace(_ws_bytes("ldmae_qknorm_rope_bwd_workspace_bytes", B, N, H, hd), qkv.device)
    call("ldmae_qknorm_rope_bwd", dt(qkv.dtype), ptr(dq), ptr(dk), ptr(dv), ptr(qkv), ptr(wq), ptr(wk), ptr(cos), ptr(sin), ptr(dqkv),
         ptr(dwq), ptr(dwk), 0.0, ptr(db), B, N, H, hd, eps, ptr(ws), stream())
    if with_bias:
        return dqkv, dwq, dwk, db.permute(1, 0, 2).reshape(-1)          # (head, q|k|v, d) -> the Linear's (q|k|v, head, d) order
    return dqkv, dwq, dwk


def rope(t, cos, sin, transposed=False):
    """t [..., N, hd] (f32 or bf16, contiguous) -> t*cos + rotate_half(t)*sin with cos/sin [N, hd] f32 (VisionRotaryEmbeddingFast.forward);
    transposed: the adjoint (backward)."""
    cos = _arg(cos, "rope cos", torch.float32, ("N", "hd"))
    N, hd = cos.shape
    sin = _arg(sin, "rope sin", torch.float32, (N, hd), like=cos)
    t = _arg(t, "rope t", _F32_BF16, (*t.shape[:-2], N, hd), like=cos)
    out = torch.empty(t.shape, dtype=t.dtype, device=t.device)
    call("ldmae_rope", dt(t.dtype), ptr(t), ptr(cos), ptr(sin), ptr(out), t.numel() // hd, N, hd, 1 if transposed else 0, stream())
    return out


_ATTN_HDS = (16, 32, 64, 72, 128)            # head dims the attention kernels are instantiated for (csrc/attention.hip: attn_hd_dispatch)
_ATTN_HDS_F32 = (16, 32, 64, 72, 80, 96, 128)      # ... and the f32 kernels (attn_hd_dispatch_f32): their backward's LDS tiles end at head_dim 96


def _attn_hds(dtype):
    return _ATTN_HDS_F32 if dtype == torch.float32 else _ATTN_HDS


def _attn_pad(hd: int, dtype=None) -> int:
    for h in _attn_hds(dtype):
        if h >= hd:
            return h
    raise RuntimeError(f"ldmae_amd attention: head_dim {hd} is above the largest instantiated kernel (128)")


def _attn_out(B, H, N, hd, like):
    """(o [B, N, H*hd] of like's type, lse [B, H, N] f32) as every attention forward writes them."""
    return torch.empty(B, N, H * hd, dtype=like.dtype, device=like.device), torch.empty(B, H, N, dtype=torch.float32, device=like.device)


def _attn_delta(B, H, N, like):
    """The [2][B, H, NP] f32 scratch of the attention backwards: rows padded to whole 64-row tiles."""
    return torch.empty(2, B, H, (N + 63) // 64 * 64, dtype=torch.float32, device=like.device)


def attention_fwd(q, k, v, scale):
    """softmax(q k^T * scale) v.  q, k, v: [B,H,N,hd]; returns (o [B,N,H*hd], lse [B,H,N] f32).
    bf16 head dims that are not a multiple of 32 (LightningDiT-XL: 72, VMAE: 16) are zero-padded to the next multiple of 32
    INSIDE the kernels (LDS images and register fragments); HBM tensors keep the true head dim."""
    q = _arg(q, "attention_fwd q", _FLOATS, ("B", "H", "N", "hd"))
    k, v = _arg(k, "attention_fwd k", q.dtype, q.shape, like=q), _arg(v, "attention_fwd v", q.dtype, q.shape, like=q)
    B, H, N, hd = q.shape
    if hd not in _attn_hds(q.dtype):
        # Head dims outside the instantiated set (16, 32, 64, 72, 128) -- e.g. 24 (mae_for_ldmae_f8d16_prev_large), 80 (mae_vit_huge), 8: zero
        # columns add nothing to q . k and produce zero output columns, so the next larger kernel on zero-padded copies is exact (`scale` is
        # the caller's, from the true head dim).  Costs the copies; the shipped archs never come here.
        P = _attn_pad(hd, q.dtype)
        pad = lambda t: torch.nn.functional.pad(t, (0, P - hd))      # noqa: E731
        o, lse = attention_fwd(pad(q), pad(k), pad(v), scale)
        return o.view(B, N, H, P)[..., :hd].reshape(B, N, H * hd), lse
    o, lse = _attn_out(B, H, N, hd, q)
    call("ldmae_attention_fwd", dt(q.dtype), ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), B, H, N, hd, float(scale), stream())
    return o, lse


def attention_bwd(q, k, v, o, do, lse, scale):
    q = _arg(q, "attention_bwd q", _FLOATS, ("B", "H", "N", "hd"))
    k, v = _arg(k, "attention_bwd k", q.dtype, q.shape, like=q), _arg(v, "attention_bwd v", q.dtype, q.shape, like=q)
    B, H, N, hd = q.shape
    o, do = _arg(o, "attention_bwd o", q.dtype, numel=q.numel(), like=q), _arg(do, "attention_bwd do", q.dtype, numel=q.numel(), like=q)
    lse = _arg(lse, "attention_bwd lse", torch.float32, (B, H, N), like=q)
    if hd not in _attn_hds(q.dtype):                          # head dims the kernels are not instantiated for: zero-padded (see attention_fwd)
        P = _attn_pad(hd, q.dtype)
        pad, padt = (lambda t: torch.nn.functional.pad(t, (0, P - hd))), (lambda t: torch.nn.functional.pad(t.reshape(B, N, H, hd), (0, P - hd)).reshape(B, N, H * P))
        dq, dk, dv = attention_bwd(pad(q), pad(k), pad(v), padt(o), padt(do), lse, scale)
        return dq[..., :hd].contiguous(), dk[..., :hd].contiguous(), dv[..., :hd].contiguous()
    dq, dk, dv = (torch.empty(q.shape, dtype=q.dtype, device=q.device) for _ in range(3))
    delta = _attn_delta(B, H, N, q)
    call("ldmae_attention_bwd", dt(q.dtype), ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), ptr(lse), ptr(dq), ptr(dk), ptr(dv), ptr(delta),
         B, H, N, hd, float(scale), stream())
    return dq, dk, dv


def qk_score_bound(wq, wk, hd, scale):
    """One float on the device: hd * max|wq| * max|wk| * scale * log2(e) * 1.02, an upper bound of every attention score (in the kernels'
    log2 units) of heads that went through QK-RMSNorm with these weights and RoPE -- for attention_fwd_pv(bound=...)."""
    wq = _arg(wq, "qk_score_bound wq", torch.float32, (hd,))
    wk = _arg(wk, "qk_score_bound wk", torch.float32, (hd,), like=wq)
    out = torch.empty(1, dtype=torch.float32, device=wq.device)
    call("ldmae_qk_score_bound", ptr(wq), ptr(wk), hd, float(scale), ptr(out), stream())
    return out


def attention_fwd_pv(q, k, qkv, scale, bound=None):
    """q, k head-major [B,H,N,hd]; v read from the packed qkv [B*N, 3*H*hd] (bf16).  bound: a proven upper bound of the scores
    (qk_score_bound): the softmax then runs with a static shift instead of a running maximum (same result, fewer vector instructions)."""
    q = _arg(q, "attention_fwd_pv q", torch.bfloat16, ("B", "H", "N", "hd"))
    k = _arg(k, "attention_fwd_pv k", torch.bfloat16, q.shape, like=q)
    qkv = _arg(qkv, "attention_fwd_pv qkv", torch.bfloat16, numel=3 * q.numel(), like=q)
    bound = _arg(bound, "attention_fwd_pv bound", torch.float32, numel=1, like=q)
    B, H, N, hd = q.shape
    o, lse = _attn_out(B, H, N, hd, q)
    if bound is not None:
        call("ldmae_attention_fwd_pv_bounded", dt(q.dtype), ptr(q), ptr(k), ptr(qkv), ptr(o), ptr(lse), ptr(bound), B, H, N, hd, float(scale), stream())
    else:
        call("ldmae_attention_fwd_pv", dt(q.dtype), ptr(q), ptr(k), ptr(qkv), ptr(o), ptr(lse), B, H, N, hd, float(scale), stream())
    return o, lse


def attention_bwd_pv(q, k, qkv, o, do, lse, scale):
    """-> (dq, dk head-major, dqkv with ONLY its v slot written: dv in the packed layout)."""
    q = _arg(q, "attention_bwd_pv q", torch.bfloat16, ("B", "H", "N", "hd"))
    k = _arg(k, "attention_bwd_pv k", torch.bfloat16, q.shape, like=q)
    qkv = _arg(qkv, "attention_bwd_pv qkv", torch.bfloat16, numel=3 * q.numel(), like=q)
    o, do = _arg(o, "attention_bwd_pv o", torch.bfloat16, numel=q.numel(), like=q), _arg(do, "attention_bwd_pv do", torch.bfloat16, numel=q.numel(), like=q)
    B, H, N, hd = q.shape
    lse = _arg(lse, "attention_bwd_pv lse", torch.float32, (B, H, N), like=q)
    dq, dk = torch.empty(q.shape, dtype=q.dtype, device=q.device), torch.empty(q.shape, dtype=q.dtype, device=q.device)
    dqkv = torch.empty(qkv.shape, dtype=q.dtype, device=q.device)
    delta = _attn_delta(B, H, N, q)
    call("ldmae_attention_bwd_pv", dt(q.dtype), ptr(q), ptr(k), ptr(qkv), ptr(o), ptr(do), ptr(lse), ptr(dq), ptr(dk), ptr(dqkv), ptr(delta),
         B, H, N, hd, float(scale), stream())
    return dq, dk, dqkv


def attention_bwd_pv_qknorm(q, k, qkv, o, do, lse, scale, wq, wk, cos, sin, eps=1e-6):
    """attention_bwd_pv + qknorm_rope_bwd(with_bias=True) in one (bf16, head_dim 64 / 128): -> (dqkv [B,N,3,H,hd] complete, dwq, dwk,
    dbias [3*H*hd])."""
    q = _arg(q, "attention_bwd_pv_qknorm q", torch.bfloat16, ("B", "H", "N", "hd"))
    k = _arg(k, "attention_bwd_pv_qknorm k", torch.bfloat16, q.shape, like=q)
    qkv = _arg(qkv, "attention_bwd_pv_qknorm qkv", torch.bfloat16, numel=3 * q.numel(), like=q)
    o = _arg(o, "attention_bwd_pv_qknorm o", torch.bfloat16, numel=q.numel(), like=q)
    do = _arg(do, "attention_bwd_pv_qknorm do", torch.bfloat16, numel=q.numel(), like=q)
    B, H, N, hd = q.shape
    lse = _arg(lse, "attention_bwd_pv_qknorm lse", torch.float32, (B, H, N), like=q)
    wq, wk = _arg(wq, "attention_bwd_pv_qknorm wq", torch.float32, (hd,), like=q), _arg(wk, "attention_bwd_pv_qknorm wk", torch.float32, (hd,), like=q)
    cos = _arg(cos, "attention_bwd_pv_qknorm cos", torch.float32, (N, hd), like=q)
    sin = _arg(sin, "attention_bwd_pv_qknorm sin", torch.float32, (N, hd), like=q)
    dqkv = torch.empty(qkv.shape, dtype=q.dtype, device=q.device)
    if wq is not None:
        dw2 = torch.empty(2 * hd, dtype=torch.float32, device=q.device)      # dwq | dwk adjacent: the library reduces straight into them
        dwq, dwk = dw2[:hd], dw2[hd:]
    else:
        dwq = dwk = None                                                      # RoPE adjoint only (use_qknorm=False)
    db = torch.empty(3 * H * hd, dtype=torch.float32, device=q.device)
    ws = workspace(_ws_bytes("ldmae_attention_bwd_pv_qknorm_workspace_bytes", B, H, N, hd), q.device)
    call("ldmae_attention_bwd_pv_qknorm", dt(q.dtype), ptr(q), ptr(k), ptr(qkv), ptr(o), ptr(do), ptr(lse), ptr(wq), ptr(wk), ptr(cos),
         ptr(sin), float(eps), ptr(dqkv), ptr(dwq), ptr(dwk), ptr(db), ptr(ws), B, H, N, hd, float(scale), stream())
    return dqkv, dwq, dwk, db


# attention_fwd_qkv: B*H*N*N from which the extra pass over the k slots pays (256 images x 24 heads x 1024^2: -7 %); LDMAE_BOUNDED_ATTN_MIN overrides
BOUNDED_ATTENTION_MIN_SCORES = int(os.environ.get("LDMAE_BOUNDED_ATTN_MIN", 1 << 31))


def attention_fwd_qkv(qkv, B, N, H, hd, scale):
    """Attention straight on the packed token-major qkv [B*N, 3*H*hd] (bf16; f32 at head_dim 16): no head-major relayout.  -> (o [B,N,H*hd], lse).
    Long sequences of small heads (the 1024-token VMAE decoder: the kernel is bound by vector issue) first take one pass over the k slots
    for max |k|^2 per (image, head): with each query's own norm it bounds the scores, and the softmax runs with that static shift instead of
    a running maximum (same result; ldmae_k_norm_max + ldmae_attention_fwd_qkv_bounded)."""
    qkv = _arg(qkv, "attention_fwd_qkv qkv", _FLOATS, numel=B * N * 3 * H * hd)
    if hd not in _attn_hds(qkv.dtype):                        # (see attention_fwd: head-major zero-padded copies)
        return attention_fwd(*heads_split(qkv, B, N, H, hd), scale)
    o, lse = _attn_out(B, H, N, hd, qkv)
    if qkv.dtype == torch.bfloat16 and hd <= 32 and N >= 512 and B * H * N * N >= BOUNDED_ATTENTION_MIN_SCORES:
        kmax = torch.empty(B * H, 2, dtype=torch.float32, device=qkv.device)
        call("ldmae_k_norm_max", ptr(qkv), ptr(kmax), B, N, H, hd, stream())
        call("ldmae_attention_fwd_qkv_bounded", dt(qkv.dtype), ptr(qkv), ptr(o), ptr(lse), ptr(kmax), B, H, N, hd, float(scale), stream())
    else:
        call("ldmae_attention_fwd_qkv", dt(qkv.dtype), ptr(qkv), ptr(o), ptr(lse), B, H, N, hd, float(scale), stream())
    return o, lse


def attention_bwd_qkv(qkv, o, do, lse, B, N, H, hd, scale):
    """-> dqkv [B*N, 3*H*hd] (dq / dk / dv written in the packed layout)."""
    qkv = _arg(qkv, "attention_bwd_qkv qkv", _FLOATS, numel=B * N * 3 * H * hd)
    o = _arg(o, "attention_bwd_qkv o", qkv.dtype, numel=B * N * H * hd, like=qkv)
    do = _arg(do, "attention_bwd_qkv do", qkv.dtype, numel=B * N * H * hd, like=qkv)
    lse = _arg(lse, "attention_bwd_qkv lse", torch.float32, (B, H, N), like=qkv)
    if hd not in _attn_hds(qkv.dtype):                        # (see attention_fwd: head-major zero-padded copies)
        q, k, v = heads_split(qkv, B, N, H, hd)
        return heads_merge(*attention_bwd(q, k, v, o, do, lse, scale), B, N, H, hd)
    dqkv = torch.empty(qkv.shape, dtype=qkv.dtype, device=qkv.device)
    delta = _attn_delta(B, H, N, qkv)
    call("ldmae_attention_bwd_qkv", dt(qkv.dtype), ptr(qkv), ptr(o), ptr(do), ptr(lse), ptr(dqkv), ptr(delta), B, H, N, hd, float(scale), stream())
    return dqkv


def swiglu_fwd(h12):
    h12 = _arg(h12, "swiglu_fwd h12", _F32_BF16, ("M", "2*Hs"))
    M, H2 = h12.shape
    hid = torch.empty(M, H2 // 2, dtype=h12.dtype, device=h12.device)
    call("ldmae_swiglu_fwd", dt(h12.dtype), ptr(h12), ptr(hid), M, H2 // 2, stream())
    return hid


def swiglu_bwd(dhid, h12):
    h12 = _arg(h12, "swiglu_bwd h12", _F32_BF16, ("M", "2*Hs"))
    M, H2 = h12.shape
    dhid = _arg(dhid, "swiglu_bwd dhid", h12.dtype, (M, H2 // 2), like=h12)
    dh12 = torch.empty(M, H2, dtype=h12.dtype, device=h12.device)
    call("ldmae_swiglu_bwd", dt(h12.dtype), ptr(dhid), ptr(h12), ptr(dh12), M, H2 // 2, stream())
    return dh12


def gate_bwd(dxout, y, gate, dgate, rows_per_batch, act_dtype, with_bias=False):
    """dy = dxout * gate[b] (act dtype);  dgate view [B,D] <- sum_n dxout*y (skipped when dgate is None).
    with_bias: also return the column sums of dy (the bias gradient of the Linear that produced the branch)."""
    dxout = _arg(dxout, "gate_bwd dxout", torch.float32, ("M", "D"))
    M, D = dxout.shape
    B = _batches("gate_bwd", M, rows_per_batch)
    y = _arg(y, "gate_bwd y", act_dtype, (M, D), like=dxout)
    _arg(gate, "gate_bwd gate", torch.float32, (B, D), rows=True, like=dxout, copy=False)
    _arg(dgate, "gate_bwd dgate", torch.float32, (B, D), rows=True, out=True, like=dxout)
    dy = torch.empty(M, D, dtype=act_dtype, device=dxout.device)
    dbias = torch.empty(D, dtype=torch.float32, device=dxout.device) if with_bias else None
    need_ws = dgate is not None or with_bias
    ws = workspace(_ws_bytes("ldmae_gate_bwd_workspace_bytes", M, D, rows_per_batch), dxout.device) if need_ws else None
    call("ldmae_gate_bwd", dt(act_dtype), ptr(dxout), ptr(y), ptr(gate), gate.stride(0) if gate is not None else 0, ptr(dy), ptr(dgate),
         dgate.stride(0) if dgate is not None else 0, ptr(dbias), M, D, rows_per_batch, ptr(ws), stream())
    return (dy, dbias) if with_bias else dy


def timestep_embedding(t, dim=256, max_period=10000.0):
    """t [B] of any real type (converted to f32, as the reference's t.float()) -> the [B, dim] sinusoidal embedding."""
    t = _arg(t.float(), "timestep_embedding t", torch.float32, ("B",))
    out = torch.empty(t.shape[0], dim, dtype=torch.float32, device=t.device)
    call("ldmae_timestep_embedding", ptr(t), ptr(out), t.shape[0], dim, float(max_period), stream())
    return out


def silu_fwd(x, out_dtype=torch.float32):
    x = _arg(x, "silu_fwd x", torch.float32)
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    call("ldmae_silu_fwd", dt(out_dtype), ptr(x), ptr(out), x.numel(), stream())
    return out


def silu_bwd(dy, x):
    x = _arg(x, "silu_bwd x", torch.float32)
    dy = _arg(dy, "silu_bwd dy", torch.float32, x.shape, like=x)
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    call("ldmae_silu_bwd", ptr(dy), ptr(x), ptr(dx), x.numel(), stream())
    return dx


def label_embed_fwd(table, y, drop, num_classes):
    table = _arg(table, "label_embed_fwd table", torch.float32, ("rows", "D"))
    y = _arg(y, "label_embed_fwd y", torch.int64, ("B",), like=table)
    B, D = y.shape[0], table.shape[1]
    drop = _arg(drop, "label_embed_fwd drop", _FLAGS, (B,), like=table)
    out = torch.empty(B, D, dtype=torch.float32, device=table.device)
    call("ldmae_label_embed_fwd", ptr(table), ptr(y), ptr(drop), ptr(out), B, D, num_classes, stream())
    return out


def label_embed_bwd(dout, y, drop, num_classes, rows):
    dout = _arg(dout, "label_embed_bwd dout", torch.float32, ("B", "D"))
    B, D = dout.shape
    y = _arg(y, "label_embed_bwd y", torch.int64, (B,), like=dout)
    drop = _arg(drop, "label_embed_bwd drop", _FLAGS, (B,), like=dout)
    dtable = torch.zeros(rows, D, dtype=torch.float32, device=dout.device)
    call("ldmae_label_embed_bwd", ptr(dout), ptr(y), ptr(drop), ptr(dtable), B, D, num_classes, rows, stream())
    return dtable


# Bumped by every op that rewrites parameter storage through the C ABI (torch's own version counters do not see those writes): part of the
# key of the forward-only weight-copy cache below.
WEIGHT_EPOCH = 0
_WCACHE: dict = {}


def invalidate_weight_cache() -> None:
    """Call after writing parameter STORAGE behind torch's back -- through the flat slab the parameters are views of (dist.broadcast(
    flat.params), flat.params.copy_(ema), a checkpoint restored into the slab): those writes bump neither the parameters' version
    counters nor WEIGHT_EPOCH, and a cached bf16 copy would silently go stale."""
    global WEIGHT_EPOCH
    WEIGHT_EPOCH += 1


def _cached(key, anchor, stamp, make):
    """The one lookup of the forward-only weight caches: the value under `key` while `stamp` is unchanged and `anchor` (the tensor whose id() is
    in the key) is still that object -- the weak reference guards against a recycled id(); otherwise make() is stored and returned."""
    hit = _WCACHE.get(key)
    if hit is not None and hit[0]() is anchor and hit[1] == stamp:
        return hit[2]
    if len(_WCACHE) > 4096:
        _WCACHE.clear()
    c = make()
    _WCACHE[key] = (weakref.ref(anchor), stamp, c)
    return c


def cached_weight_copy(w, dtype):
    """`dtype` copy of the f32 master weight `w` for FORWARD-ONLY use (sampling / encoding under no_grad runs the same weights hundreds of
    times: 112 cast launches per XL/1 forward).  Valid while the storage pointer, torch's version counter of `w` and WEIGHT_EPOCH are
    unchanged; training never comes here (its weights change every step)."""
    return _cached((id(w), dtype), w, (w.data_ptr(), w._version, WEIGHT_EPOCH), lambda: cast_weight(w, dtype, transposed=False, straight=True)[0])


def cached_weight_mx8(w):
    """(q, scales) of the f32 master weight `w` [N, K], MX-quantised along K, for FORWARD-ONLY use: cached under the rule of
    cached_weight_copy."""
    return _cached((id(w), "mx8"), w, (w.data_ptr(), w._version, WEIGHT_EPOCH), lambda: mx8_quantize(w))


def cached_stack_copy(tensors, dtype):
    """cast_stack for FORWARD-ONLY use (sampling re-runs the same weights hundreds of times): valid while every source's storage pointer and
    version counter and WEIGHT_EPOCH are unchanged.  Keyed by the first tensor, like cached_weight_copy."""
    w = tensors[0]
    return _cached((id(w), dtype, "stack", len(tensors)), w, (tuple((t.data_ptr(), t._version) for t in tensors), WEIGHT_EPOCH),
                   lambda: cast_stack(tensors, dtype))


def adamw_ema(p, g, m, v, ema, step, lr, beta1, beta2, eps, weight_decay, ema_decay, grad_scale=1.0):
    global WEIGHT_EPOCH
    _arg(p, "adamw_ema p", torch.float32, out=True)
    _arg(g, "adamw_ema g", torch.float32, numel=p.numel(), like=p, out=True)
    _arg(m, "adamw_ema m", torch.float32, numel=p.numel(), like=p, out=True)
    _arg(v, "adamw_ema v", torch.float32, numel=p.numel(), like=p, out=True)
    _arg(ema, "adamw_ema ema", torch.float32, numel=p.numel(), like=p, out=True)
    WEIGHT_EPOCH += 1
    call("ldmae_adamw_ema", ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), p.numel(), int(step), float(lr), float(beta1), float(beta2),
         float(eps), float(weight_decay), float(ema_decay), float(grad_scale), stream())


def ema_only(ema, p, ema_decay):
    global WEIGHT_EPOCH
    _arg(p, "ema_only p", torch.float32, copy=False)
    _arg(ema, "ema_only ema", torch.float32, numel=p.numel(), like=p, out=True)
    WEIGHT_EPOCH += 1
    call("ldmae_ema_only", ptr(ema), ptr(p), p.numel(), float(ema_decay), stream())


def _track_args(op, tracks, coefs, p):
    """The (count, 4 slab pointers, 4 coefficients) tail of the two track entries: 1..4 f32 slabs of p's length on p's device, written in
    place (out=True: never copied), one c_k = 1 - beta_k(t) each."""
    tracks, coefs = list(tracks), [float(c) for c in coefs]
    if not 1 <= len(tracks) <= 4 or len(coefs) != len(tracks):
        raise RuntimeError(f"{op}: {len(tracks)} track slabs with {len(coefs)} coefficients (need 1..4 of each, one coefficient per slab)")
    for k, t in enumerate(tracks):
        _arg(t, f"{op} track {k}", dtype=torch.float32, numel=p.numel(), like=p, out=True)
    pad = 4 - len(tracks)
    return (len(tracks), *[ptr(t) for t in tracks], *([None] * pad), *coefs, *([0.0] * pad))


def adamw_ema_tracks(p, g, m, v, ema, tracks, coefs, step, lr, beta1, beta2, eps, weight_decay, ema_decay, grad_scale=1.0):
    """`adamw_ema` plus the power-function EMA tracks of the post-hoc EMA in the same pass: p, m, v, ema come out bit for bit as `adamw_ema`
    writes them; tracks[k] <- tracks[k] + coefs[k] (p_new - tracks[k]) (coefs[k] == 1: p_new is stored, the slab is not read)."""
    global WEIGHT_EPOCH
    op = "adamw_ema_tracks"
    _arg(p, op + " p", dtype=torch.float32, out=True)
    for name, t in (("g", g), ("m", m), ("v", v), ("ema", ema)):
        _arg(t, f"{op} {name}", dtype=torch.float32, numel=p.numel(), like=p, out=True)
    tail = _track_args(op, tracks, coefs, p)
    WEIGHT_EPOCH += 1
    call("ldmae_adamw_ema_tracks", ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), p.numel(), int(step), float(lr), float(beta1), float(beta2),
         float(eps), float(weight_decay), float(ema_decay), float(grad_scale), *tail, stream())


def ema_tracks_only(p, tracks, coefs):
    """The track update alone, for parameters the optimizer does not touch (the frozen tail)."""
    op = "ema_tracks_only"
    _arg(p, op + " p", dtype=torch.float32, copy=False)
    tail = _track_args(op, tracks, coefs, p)
    call("ldmae_ema_tracks_only", ptr(p), p.numel(), *tail, stream())


def snapshot_accumulate(acc, x, coef):
    """acc (f64) += coef * x (f32), element by element; coef is a python float (f64)."""
    _arg(acc, "snapshot_accumulate acc", dtype=torch.float64, out=True)
    _arg(x, "snapshot_accumulate x", dtype=torch.float32, numel=acc.numel(), like=acc, copy=False)
    call("ldmae_snapshot_accumulate", ptr(acc), ptr(x), acc.numel(), float(coef), stream())


def snapshot_finish(acc, out=None):
    """The f64 accumulator rounded to f32 (into `out`, or a new tensor of acc's shape)."""
    _arg(acc, "snapshot_finish acc", dtype=torch.float64, copy=False)
    out = torch.empty(acc.shape, dtype=torch.float32, device=acc.device) if out is None else out
    _arg(out, "snapshot_finish out", dtype=torch.float32, numel=acc.numel(), like=acc, out=True)
    call("ldmae_snapshot_finish", ptr(out), ptr(acc), acc.numel(), stream())
    return out


# ----------------------------------------------------------------------------- VMAE
def random_masking(noise, keep):
    noise = _arg(noise, "random_masking noise", torch.float32, ("N", "L"))
    N, Lq = noise.shape
    ids_restore = torch.empty(N, Lq, dtype=torch.int64, device=noise.device)
    mask = torch.empty(N, Lq, dtype=torch.float32, device=noise.device)
    ids_keep = torch.empty(N, keep, dtype=torch.int64, device=noise.device)
    call("ldmae_random_masking", ptr(noise), ptr(ids_restore), ptr(mask), ptr(ids_keep), N, Lq, keep, stream())
    return ids_keep, mask, ids_restore


def patch_embed_kept(img, ids_keep, pos, w2d, bias, patch, dtype):
    """Patch embedding of the kept tokens only: img [N,C,S,S] f32, ids_keep [N,keep] i64, pos [L,D] f32, w2d [D, C*p*p] f32 master weight
    -> [N, keep, D] f32 = conv(img)[kept] + bias + pos[kept].  Same bits as embedding all patches (gemm_nt_pos) and gathering."""
    img = _arg(img.float(), "patch_embed_kept img", torch.float32, ("N", "C", "S", "S"))
    N, C, S, S2 = img.shape
    if S2 != S or patch <= 0 or S % patch:
        raise RuntimeError(f"patch_embed_kept img: shape {tuple(img.shape)}, expected square images of whole {patch}-pixel patches")
    ids_keep = _arg(ids_keep, "patch_embed_kept ids_keep", torch.int64, (N, "keep"), like=img)
    w2d = _arg(w2d, "patch_embed_kept w2d", torch.float32, ("D", C * patch * patch), like=img)
    keep, D = ids_keep.shape[1], w2d.shape[0]
    pos = _arg(pos, "patch_embed_kept pos", torch.float32, ("L", D), like=img, at_least=(S // patch) ** 2 * D)
    bias = _arg(bias, "patch_embed_kept bias", torch.float32, (D,), like=img)
    tok = torch.empty(N * keep, C * patch * patch, dtype=dtype, device=img.device)
    posg = torch.empty(N * keep, D, dtype=torch.float32, device=img.device)
    call("ldmae_patch_gather", dt(dtype), ptr(img), ptr(ids_keep), ptr(pos), ptr(tok), ptr(posg), N, keep, C, S, patch, D, stream())
    wb = cast(w2d, dtype)         # 192 x 192: one tiny launch (w2d is a fresh view per call, so the id-keyed weight cache does not apply)
    out, _ = gemm_nt_gate_res(tok, wb, bias, posg, None, keep, save_y=False, xout=posg, y_dtype=torch.float32)   # unrounded, as gemm_nt_pos
    return out.view(N, keep, D)


def latent_prologue(moments, noise=None, lat_mean=None, lat_std=None, multiplier=1.0, sample=True):
    """Device-side counterpart of ImgLatentDataset.__getitem__ after the shard read: moments [B, 2C, H, W] f32 (sample) or latents
    [B, C, H, W] -> normalised model input [B, C, H, W] f32.  noise [B, C, H, W] (drawn by the caller); lat_mean / lat_std [C]-sized."""
    mom = _arg(moments.float(), "latent_prologue moments", torch.float32, ("B", "2C" if sample else "C", "H", "W"))
    B, C2, H, W = mom.shape
    if sample and C2 % 2:
        raise RuntimeError(f"latent_prologue moments: shape {tuple(mom.shape)}, expected [B, 2C, H, W] (mean | logvar)")
    C = C2 // 2 if sample else C2
    nz = _arg(noise.float() if noise is not None and sample else None, "latent_prologue noise", torch.float32, (B, C, H, W), like=mom)
    mu = _arg(lat_mean.float().reshape(-1) if lat_mean is not None else None, "latent_prologue lat_mean", torch.float32, (C,), like=mom)
    sd = _arg(lat_std.float().reshape(-1) if lat_std is not None else None, "latent_prologue lat_std", torch.float32, (C,), like=mom)
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=mom.device)
    call("ldmae_latent_prologue", ptr(mom), ptr(nz), ptr(mu), ptr(sd), float(multiplier), ptr(out), B, C, H * W, 1 if sample else 0, stream())
    return out


# ----------------------------------------------------------------------------- held-out validation (csrc/fm_valid.hip), f32
def fm_valid_plan(stored, idx, t, lat_mean=None, lat_std=None, multiplier=1.0, sample=True, seed=0):
    """Model input and regression target of a validation batch in one launch: stored [B, 2C, H, W] f32 (mean | logvar, sample) or [B, C, H, W];
    idx [B] int64, the GLOBAL index of each sample; t [B] f32.  With z = normal(seed, 2 idx[b]) and x0 = normal(seed, 2 idx[b] + 1) (the named
    draws of `normal`, C H W values each, never stored): x1 = latent_prologue(stored, z, ...), xt = t x1 + (1 - t) x0 and ut = x1 - x0 with the
    roundings of ICPlan.plan.  Returns (xt, ut) [B, C, H, W] f32: the rows of sample i depend on (stored[i], seed, i, t[i]) alone."""
    if stored.dim() != 4 or (sample and stored.shape[1] % 2):
        raise RuntimeError(f"fm_valid_plan stored: shape {tuple(stored.shape)}, expected [B, {'2C' if sample else 'C'}, H, W]")
    B, C2, H, W = stored.shape
    C = C2 // 2 if sample else C2
    stored = _arg(stored, "fm_valid_plan stored", torch.float32, align=16)
    idx = _arg(idx, "fm_valid_plan idx", torch.int64, (B,), like=stored)
    t = _arg(t, "fm_valid_plan t", torch.float32, (B,), like=stored)
    if (lat_mean is None) != (lat_std is None):
        raise RuntimeError("fm_valid_plan: give both lat_mean and lat_std, or neither")
    mu, sd = (_arg(s.reshape(-1) if s is not None else None, f"fm_valid_plan {w}", torch.float32, (C,), like=stored)
              for s, w in ((lat_mean, "lat_mean"), (lat_std, "lat_std")))
    xt = torch.empty(B, C, H, W, dtype=torch.float32, device=stored.device)
    ut = torch.empty_like(xt)
    call("ldmae_fm_valid_plan_f32", ptr(stored), ptr(idx), ptr(t), ptr(mu), ptr(sd), float(multiplier), 1 if sample else 0,
         int(seed) & (2 ** 64 - 1), ptr(xt), ptr(ut), B, C, H * W, stream())
    return xt, ut


def _row_reduce_out(op, partials, a, out):
    """What rowdot and row_mse share once their two operands [B, ...] are checked: B and the row length m, the result out [B] (checked, or made
    here) and the workspace of partial sums that `partials` (the entry's own ldmae_*_partials) sizes -> (B, m, out, partial).  No string is
    built unless something is wrong: the two run once per model evaluation."""
    if a.dim() < 1 or a.numel() == 0:
        raise RuntimeError(f"{op}: two non-empty tensors of at least one dimension expected, got {tuple(a.shape)}")
    B, m = a.shape[0], a.numel() // a.shape[0]
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=a.device)
    else:
        _arg(out, op + " out", torch.float32, numel=B, out=True, like=a)
    return B, m, out, torch.empty(int(partials(B, m)), dtype=torch.float32, device=a.device)


def row_mse(a, u, out=None):
    """out[b] = mean over everything but dim 0 of (float(a[b]) - u[b])^2: mean_flat((a - u) ** 2) with a f32 or bf16 and u f32, in f32, as a
    two-stage fixed-order sum (bitwise reproducible).  A tensor of another layout is copied first (the DiT returns a permuted view)."""
    a = _arg(a, "row_mse a", (torch.float32, torch.bfloat16))
    u = _arg(u, "row_mse u", torch.float32, a.shape, like=a)
    B, m, out, partial = _row_reduce_out("row_mse", L.load().ldmae_row_mse_partials, a, out)
    call("ldmae_row_mse", dt(a.dtype), ptr(a), ptr(u), ptr(out), B, m, ptr(partial), stream())
    return out


# ----------------------------------------------------------------------------- guidance rules of the sampler (csrc/guidance.hip)
GUIDANCE_RULES = {"cfg": 0, "rescale": 1, "apg": 2}


def guidance_combine(rule, pos, neg, scale, k=None, x=None, t=None, phi=0.7, eta=0.0, norm_threshold=0.0, momentum=0.0, mom=None, out=None):
    """The guided velocity of `rule` ('cfg' / 'rescale' / 'apg': the contract of ldmae_guidance_combine) in one launch.  pos (main / conditional
    output), neg (null-class / guide output) [B, C, H, W] f32 or bf16, same type; the first k channels (default: all C) are guided, the rest of
    out is pos.  apg also takes the state x [B, C, H, W] f32, the times t [B] f32 and optionally the momentum buffer mom [B, k H W] f32, updated
    in place (momentum != 0 needs it).  out: f32 [B, C, H, W], may be pos itself when pos is f32.  A tensor of another layout is copied first (the
    DiT returns a permuted view)."""
    if rule not in GUIDANCE_RULES:
        raise RuntimeError(f"guidance_combine rule: {rule!r}, expected one of {sorted(GUIDANCE_RULES)}")
    if pos.dim() != 4 or pos.numel() == 0:
        raise RuntimeError(f"guidance_combine pos: shape {tuple(pos.shape)}, expected a non-empty [B, C, H, W]")
    B, C, H, W = pos.shape
    if neg.dim() == 4 and neg.shape[0] == B and neg.shape[2:] == pos.shape[2:] and neg.shape[1] != C:
        raise RuntimeError(f"guidance_combine neg: {neg.shape[1]} channels against the {C} of pos: learn_sigma outputs (out_channels != in_channels) are not "
                           "guided here; pass the velocity channels only")
    k = C if k is None else k
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= C:
        raise RuntimeError(f"guidance_combine k: {k!r} guided channels, expected an integer in 1 .. C = {C}")
    aliased = out is pos
    pos = _arg(pos, "guidance_combine pos", (torch.float32, torch.bfloat16), copy=not aliased)
    neg = _arg(neg, "guidance_combine neg", pos.dtype, pos.shape, like=pos)
    if rule == "rescale" and not 0.0 <= float(phi) <= 1.0:
        raise RuntimeError(f"guidance_combine phi: {phi!r}, expected a value in [0, 1]")
    if rule == "apg":
        if float(norm_threshold) < 0.0:
            raise RuntimeError(f"guidance_combine norm_threshold: {norm_threshold!r} must not be negative (0 = off)")
        if x is None or t is None:
            raise RuntimeError("guidance_combine: rule 'apg' needs the state x and the times t")
        if x.dim() == 4 and x.shape[0] == B and x.shape[2:] == pos.shape[2:] and x.shape[1] != C:
            raise RuntimeError(f"guidance_combine x: {x.shape[1]} channels against the {C} of pos: learn_sigma shapes (out_channels != in_channels) are "
                               "not guided here")
        x = _arg(x, "guidance_combine x", torch.float32, pos.shape, like=pos)
        t = _arg(t, "guidance_combine t", torch.float32, (B,), like=pos)
        if mom is None and float(momentum) != 0.0:
            raise RuntimeError(f"guidance_combine mom: momentum = {momentum!r} needs the momentum buffer [B, k*H*W] = [{B}, {k * H * W}]")
        _arg(mom, "guidance_combine mom", torch.float32, (B, k * H * W), out=True, like=pos)
    else:
        x = t = mom = None
    if out is None:
        out = torch.empty(B, C, H, W, dtype=torch.float32, device=pos.device)
    else:
        _arg(out, "guidance_combine out", torch.float32, pos.shape, out=True, like=pos)
    call("ldmae_guidance_combine", GUIDANCE_RULES[rule], dt(pos.dtype), ptr(pos), ptr(neg), ptr(x), ptr(t), ptr(mom), ptr(out), B, C, H * W, k,
         float(scale), float(phi), float(eta), float(norm_threshold), float(momentum), stream())
    return out


def check_crop_table(offsets, geom, blob_bytes):
    """The range checks ldmae_crop_resize_flip_u8 leaves to its caller, on the HOST copy of the tables: offsets [B] i64, geom [B, 8] i32 =
    (h, w, top, left, ch, cw, flip, 0).  Raises ValueError naming the first bad sample."""
    if geom.dim() != 2 or geom.shape[1] != 8:
        raise ValueError(f"crop_resize_flip: geom must be [B, 8] (h, w, top, left, ch, cw, flip, 0), got {tuple(geom.shape)}")
    if offsets.dim() != 1 or offsets.shape[0] != geom.shape[0] or geom.shape[0] < 1:
        raise ValueError(f"crop_resize_flip: offsets {tuple(offsets.shape)} does not go with geom {tuple(geom.shape)}")
    g, off = geom.to(torch.int64), offsets.to(torch.int64)
    h, w, top, left, ch, cw = (g[:, i] for i in range(6))
    checks = (((h < 1) | (w < 1), "an empty image"), ((ch < 1) | (cw < 1), "an empty crop box (ch, cw >= 1)"),
              ((top < 0) | (left < 0) | (top + ch > h) | (left + cw > w), "a crop box that leaves the image"),
              ((ch > 16384) | (cw > 16384), "a crop side above 16384"),
              ((off < 0) | (off + 3 * h * w > int(blob_bytes)), f"an image that ends past the blob ({int(blob_bytes)} bytes)"))
    for bad, what in checks:
        if bool(bad.any()):
            b = int(bad.nonzero()[0])
            raise ValueError(f"crop_resize_flip: sample {b} has {what}: offset {int(off[b])}, geom {geom[b].tolist()}")


def crop_resize_flip(blob, offsets, geom, S, mean=0.5, std=0.5, out_dtype=torch.float32, out=None):
    """RandomResizedCrop's resample + flip + ToTensor + Normalize of a batch of packed uint8 images in one launch (ldmae_crop_resize_flip_u8):
    blob uint8 [n] on the device; offsets [B] i64 and geom [B, 8] i32 -> [B, 3, S, S] f32 or bf16.  HOST tables are checked (check_crop_table) and
    uploaded here; DEVICE tables are used as they are -- the kernel trusts them, so their host copy must have gone through check_crop_table
    (datasets/packed_images.py does that before its own upload)."""
    if blob.dtype != torch.uint8 or blob.dim() != 1 or not blob.is_contiguous():
        raise ValueError("crop_resize_flip: blob must be a contiguous 1-D uint8 tensor")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"crop_resize_flip: out_dtype {out_dtype} (float32 or bfloat16)")
    if int(S) < 1 or float(std) == 0.0:
        raise ValueError(f"crop_resize_flip: S={S} must be positive and std={std} non-zero")
    if not offsets.is_cuda or not geom.is_cuda:
        if offsets.is_cuda or geom.is_cuda:
            raise ValueError("crop_resize_flip: offsets and geom must both be host tensors or both device tensors")
        check_crop_table(offsets, geom, blob.numel())
        offsets, geom = offsets.to(blob.device, torch.int64), geom.to(blob.device, torch.int32)
    elif geom.dim() != 2 or geom.shape[1] != 8 or offsets.shape != geom.shape[:1]:
        raise ValueError(f"crop_resize_flip: geom must be [B, 8] and offsets [B], got {tuple(geom.shape)} and {tuple(offsets.shape)}")
    if offsets.dtype != torch.int64 or geom.dtype != torch.int32 or not offsets.is_contiguous() or not geom.is_contiguous():
        raise ValueError("crop_resize_flip: device tables must be contiguous int64 offsets and int32 geom")
    B = geom.shape[0]
    if out is None:
        out = torch.empty(B, 3, S, S, dtype=out_dtype, device=blob.device)
    elif out.shape != (B, 3, S, S) or out.dtype != out_dtype or not out.is_contiguous() or out.device != blob.device:
        raise ValueError(f"crop_resize_flip: out must be a contiguous {out_dtype} [{B}, 3, {S}, {S}] tensor on {blob.device}")
    call("ldmae_crop_resize_flip_u8", ptr(blob), blob.numel(), ptr(offsets), ptr(geom), ptr(out), 1 if out_dtype == torch.bfloat16 else 0,
         B, int(S), float(mean), float(std), stream())
    return out


def gather_rows(x, ids):
    x = _arg(x, "gather_rows x", torch.float32, ("N", "L", "D"))
    N, Lq, D = x.shape
    ids = _arg(ids, "gather_rows ids", torch.int64, (N, "keep"), like=x)
    keep = ids.shape[1]
    out = torch.empty(N, keep, D, dtype=torch.float32, device=x.device)
    call("ldmae_gather_rows", ptr(x), ptr(ids), ptr(out), N, Lq, keep, D, stream())
    return out


def scatter_rows(dout, ids, Lq):
    dout = _arg(dout, "scatter_rows dout", torch.float32, ("N", "keep", "D"))
    N, keep, D = dout.shape
    ids = _arg(ids, "scatter_rows ids", torch.int64, (N, keep), like=dout)
    dx = torch.zeros(N, Lq, D, dtype=torch.float32, device=dout.device)
    call("ldmae_scatter_rows", ptr(dout), ptr(ids), ptr(dx), N, Lq, keep, D, stream())
    return dx


def restore_tokens(x, mask_token, pos, ids_restore):
    """Decoder input of the pre-training step (models_mae.py:536-541) in one pass: x [B, keep, D] f32, mask_token [D], pos [L, D], ids_restore
    [B, L] i64 -> [B, L, D] = (kept row or mask token) + pos."""
    x = _arg(x, "restore_tokens x", torch.float32, ("B", "keep", "D"))
    B, keep, D = x.shape
    ids_restore = _arg(ids_restore, "restore_tokens ids_restore", torch.int64, (B, "L"), like=x)
    Lq = ids_restore.shape[1]
    mask_token = _arg(mask_token, "restore_tokens mask_token", torch.float32, (D,), like=x)
    pos = _arg(pos, "restore_tokens pos", torch.float32, ("L", D), like=x, at_least=Lq * D)
    out = torch.empty(B, Lq, D, dtype=torch.float32, device=x.device)
    call("ldmae_restore_tokens", ptr(x), ptr(mask_token), ptr(pos), ptr(ids_restore), ptr(out), B, Lq, keep, D, stream())
    return out


def restore_tokens_bwd(dout, ids_restore, keep, need_mask_grad=True):
    """-> (dx [B, keep, D], dmask_token [D] or None)."""
    dout = _arg(dout, "restore_tokens_bwd dout", torch.float32, ("B", "L", "D"))
    B, Lq, D = dout.shape
    ids_restore = _arg(ids_restore, "restore_tokens_bwd ids_restore", torch.int64, (B, Lq), like=dout)
    dx = torch.empty(B, keep, D, dtype=torch.float32, device=dout.device)
    dm = torch.empty(D, dtype=torch.float32, device=dout.device) if need_mask_grad else None
    ws = workspace(_ws_bytes("ldmae_restore_tokens_bwd_workspace_bytes", B, Lq, D), dout.device) if need_mask_grad else None
    call("ldmae_restore_tokens_bwd", ptr(dout), ptr(ids_restore), ptr(dx), ptr(dm), B, Lq, keep, D, ptr(ws), stream())
    return dx, dm


def _vmae_encoder_args(x, blob, nblocks, dim):
    """What the two forms of the fused VMAE encoder share: x [B, tokens, dim] (any float type: converted to f32) and the weight blob of the
    size the kernels expect, read in place -> (x, out, B, tokens)."""
    x = _arg(x.float(), "vmae_encoder_fwd x", torch.float32, ("B", "tokens", dim))
    _arg(blob, "vmae_encoder_fwd blob", like=x, copy=False)
    need = L.load().ldmae_vmae_encoder_blob_bytes(nblocks)
    if blob.numel() * blob.element_size() != need:
        raise RuntimeError(f"vmae_encoder_fwd: weight blob has {blob.numel() * blob.element_size()} bytes, the kernels expect {need}")
    return x, torch.empty(x.shape, dtype=torch.float32, device=x.device), x.shape[0], x.shape[1]


def vmae_encoder_fwd(x, blob, nblocks, dim, heads, hidden, eps=1e-6):
    """The whole VMAE encoder stack (blocks + closing LayerNorm) in one launch: x [B, tokens, dim] f32 -> same shape (inference, bf16 MFMA,
    f32 residual stream in registers).  `blob`: weights packed by tokenizer/fused_encoder.py."""
    x, out, B, T = _vmae_encoder_args(x, blob, nblocks, dim)
    call("ldmae_vmae_encoder_fwd", ptr(x), ptr(out), ptr(blob), B, T, dim, heads, hidden, nblocks, float(eps), stream())
    return out


def vmae_encoder_fwd_tiled(x, blob, nblocks, dim, heads, hidden, eps=1e-6, f16=False):
    """The same stack on sequences of several whole 256-token tiles per image (the docking encoder on all 1024 patches): three launches per
    block -- q|k|v of a tile, flash attention on the packed qkv, proj + MLP of a tile -- from the same weight blob.  f16: the TF32-class form
    (the blob packed in fp16)."""
    x, out, B, T = _vmae_encoder_args(x, blob, nblocks, dim)
    D = dim
    ws = workspace(_ws_bytes("ldmae_vmae_encoder_fwd_tiled_workspace_bytes", B, T), x.device)
    call("ldmae_vmae_encoder_fwd_tiled_f16" if f16 else "ldmae_vmae_encoder_fwd_tiled", ptr(x), ptr(out), ptr(blob), ptr(ws), B, T, D, heads, hidden,
         nblocks, float(eps), stream())
    return out


def heads_split(qkv, B, N, H, hd):
    """[B,N,3,H,hd] -> q,k,v [B,H,N,hd] (no norm / rope)."""
    qkv = _arg(qkv, "heads_split qkv", _F32_BF16, numel=B * N * 3 * H * hd)
    if hd % 8 != 0:
        # head dims off the kernels' 8-element grid (12: the pre-training tree's mae_for_ldmae_f8d16_small, VMAE/models_mae.py:1036-1041): a pure
        # re-layout, done by torch's copy; the attention wrappers then zero-pad the heads to the next instantiated head dim
        t = qkv.view(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
        return t[0].contiguous(), t[1].contiguous(), t[2].contiguous()
    q = torch.empty(B, H, N, hd, dtype=qkv.dtype, device=qkv.device)
    k, v = torch.empty_like(q), torch.empty_like(q)
    call("ldmae_qknorm_rope_fwd", dt(qkv.dtype), ptr(qkv), None, None, None, None, ptr(q), ptr(k), ptr(v), B, N, H, hd, 0.0, stream())
    return q, k, v


def heads_merge(dq, dk, dv, B, N, H, hd):
    """inverse of heads_split for the gradients: -> [B*N, 3*H*hd]."""
    dq = _arg(dq, "heads_merge dq", _F32_BF16, (B, H, N, hd))
    dk, dv = _arg(dk, "heads_merge dk", dq.dtype, (B, H, N, hd), like=dq), _arg(dv, "heads_merge dv", dq.dtype, (B, H, N, hd), like=dq)
    if hd % 8 != 0:                                   # (see heads_split)
        return torch.stack((dq, dk, dv), 0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * hd)
    dqkv = torch.empty(B * N, 3 * H * hd, dtype=dq.dtype, device=dq.device)
    call("ldmae_qknorm_rope_bwd", dt(dq.dtype), ptr(dq), ptr(dk), ptr(dv), None, None, None, None, None, ptr(dqkv), None, None, 0.0,
         None, B, N, H, hd, 0.0, None, stream())
    return dqkv


def conv3x3(x, w, b):
    x = _arg(x, "conv3x3 x", torch.float32, ("B", "C", "H", "W"))
    B, C, Hh, Ww = x.shape
    w, b = _arg(w, "conv3x3 w", torch.float32, (C, C, 3, 3), like=x), _arg(b, "conv3x3 b", torch.float32, (C,), like=x)
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    call("ldmae_conv3x3", ptr(x), ptr(w), ptr(b), ptr(out), B, C, Hh, Ww, stream())
    return out


def conv3x3_bwd(dout, x, w, need_dx=True):
    x = _arg(x, "conv3x3_bwd x", torch.float32, ("B", "C", "H", "W"))
    B, C, Hh, Ww = x.shape
    dout, w = _arg(dout, "conv3x3_bwd dout", torch.float32, x.shape, like=x), _arg(w, "conv3x3_bwd w", torch.float32, (C, C, 3, 3), like=x)
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device) if need_dx else None
    dw = torch.empty(C, C, 3, 3, dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = workspace(_ws_bytes("ldmae_conv3x3_bwd_workspace_bytes", C), x.device, "conv")
    call("ldmae_conv3x3_bwd", ptr(dout), ptr(x), ptr(w), ptr(dx), ptr(dw), ptr(db), B, C, Hh, Ww, ptr(ws), stream())
    return dx, dw, db


def _mae_loss_args(pred_img, imgs, mask, p):
    """What the two passes of the MAE loss share: imgs and pred_img [B, C, H, W] f32, mask [B, (H/p)*(W/p)] f32 (1 = masked)."""
    imgs = _arg(imgs, "mae_loss imgs", torch.float32, ("B", "C", "H", "W"))
    B, C, Hh, Ww = imgs.shape
    if int(p) <= 0 or Hh % int(p) or Ww % int(p):
        raise RuntimeError(f"mae_loss imgs: shape {tuple(imgs.shape)}, expected whole {p}-pixel patches")
    pred_img = _arg(pred_img, "mae_loss pred_img", torch.float32, imgs.shape, like=imgs)
    mask = _arg(mask, "mae_loss mask", torch.float32, (B, (Hh // int(p)) * (Ww // int(p))), like=imgs)
    return pred_img, imgs, mask, B, C, Hh, Ww


def mae_loss_fwd(pred_img, imgs, mask, p):
    """-> [2] f32 on the device: (sum over masked patches' pixels of (pred - img)^2, the same over visible patches)."""
    pred_img, imgs, mask, B, C, Hh, Ww = _mae_loss_args(pred_img, imgs, mask, p)
    G = L.load().ldmae_mae_loss_groups(imgs.numel())
    part = torch.empty(G, 2, dtype=torch.float32, device=imgs.device)
    call("ldmae_mae_loss_fwd", ptr(pred_img), ptr(imgs), ptr(mask), ptr(part), B, C, Hh, Ww, int(p), stream())
    return part.sum(0)


def mae_loss_bwd(pred_img, imgs, mask, coef, p):
    pred_img, imgs, mask, B, C, Hh, Ww = _mae_loss_args(pred_img, imgs, mask, p)
    coef = _arg(coef, "mae_loss_bwd coef", torch.float32, (2,), like=imgs)
    d = torch.empty(imgs.shape, dtype=torch.float32, device=imgs.device)
    call("ldmae_mae_loss_bwd", ptr(pred_img), ptr(imgs), ptr(mask), ptr(coef), ptr(d), B, C, Hh, Ww, int(p), stream())
    return d


def layernorm_fwd(x, w, b, out_dtype, eps=1e-6):
    x = _arg(x, "layernorm_fwd x", torch.float32, ("M", "D"))
    M, D = x.shape
    w, b = _arg(w, "layernorm_fwd w", torch.float32, (D,), like=x), _arg(b, "layernorm_fwd b", torch.float32, (D,), like=x)
    out = torch.empty(M, D, dtype=out_dtype, device=x.device)
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    call("ldmae_layernorm_fwd", dt(out_dtype), ptr(x), ptr(w), ptr(b), ptr(out), ptr(mean), ptr(rstd), M, D, eps, stream())
    return out, mean, rstd


def layernorm_bwd(dout, x, w, mean, rstd, dx_accum, cast=False):
    """dx_accum += dLN/dx; -> (dw, db), with cast=True (16-bit dout) also the updated dx_accum rounded to dout's type."""
    x = _arg(x, "layernorm_bwd x", torch.float32, ("M", "D"))
    M, D = x.shape
    dout = _arg(dout, "layernorm_bwd dout", _FLOATS, (M, D), like=x)
    w = _arg(w, "layernorm_bwd w", torch.float32, (D,), like=x)
    mean, rstd = _arg(mean, "layernorm_bwd mean", torch.float32, (M,), like=x), _arg(rstd, "layernorm_bwd rstd", torch.float32, (M,), like=x)
    _arg(dx_accum, "layernorm_bwd dx_accum", torch.float32, (M, D), out=True, like=x)
    dw = torch.empty(D, dtype=torch.float32, device=x.device)
    db = torch.empty_like(dw)
    ws = workspace(_ws_bytes("ldmae_layernorm_bwd_workspace_bytes", M, D), x.device)
    dxc = torch.empty(M, D, dtype=dout.dtype, device=x.device) if cast else None
    call("ldmae_layernorm_bwd_cast", dt(dout.dtype), ptr(dout), ptr(x), ptr(w), ptr(mean), ptr(rstd), ptr(dx_accum), ptr(dxc), ptr(dw), ptr(db), 0.0,
         M, D, ptr(ws), stream())
    return (dw, db, dxc) if cast else (dw, db)


def gelu_bwd(dout, pre):
    pre = _arg(pre, "gelu_bwd pre", _FLOATS)
    dout = _arg(dout, "gelu_bwd dout", pre.dtype, pre.shape, like=pre)
    dx = torch.empty(pre.shape, dtype=pre.dtype, device=pre.device)
    call("ldmae_gelu_bwd", dt(pre.dtype), ptr(dout), ptr(pre), ptr(dx), pre.numel(), stream())
    return dx


def gelu_tanh_fwd(x):
    """nn.GELU(approximate="tanh") (the timm Mlp of a use_swiglu=False LightningDiT block, lightningdit.py:208,219-224)."""
    x = _arg(x, "gelu_tanh_fwd x", _F32_BF16)
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    call("ldmae_gelu_tanh_fwd", dt(x.dtype), ptr(x), ptr(out), x.numel(), stream())
    return out


def gelu_tanh_bwd(dout, pre):
    pre = _arg(pre, "gelu_tanh_bwd pre", _F32_BF16)
    dout = _arg(dout, "gelu_tanh_bwd dout", pre.dtype, pre.shape, like=pre)
    dx = torch.empty(pre.shape, dtype=pre.dtype, device=pre.device)
    call("ldmae_gelu_tanh_bwd", dt(pre.dtype), ptr(dout), ptr(pre), ptr(dx), pre.numel(), stream())
    return dx


# ----------------------------------------------------------------------------- KID and density / coverage (csrc/adm_eval.hip: PW_KID, PW_COUNT)
# Two more passes of the ADM evaluator's pairwise core (row_sqnorms, default_col_splits and _pair_tiles are with its other wrappers below).
# The kernels work on the caller's tensors as they are (copy=False); the KID index tables are HOST tables, checked and uploaded here.

def ball_counts(u, ru, v, nu=None, nv=None, nsplit=None):
    """u [M, D] with ONE radius per row ru [M] (squared distances, a column of knn_radii) and v [N, D] -> int32 [M]:
    counts[i] = #{ j : d(i, j) < ru[i] }, strictly less, d the squared distance of knn_radii / pr_flags (density and coverage, Naeem et
    al. 2020).  Integer sums: the same for every nsplit."""
    _arg(u, "ball_counts u", torch.float32, ("M", "D"), copy=False)
    M, D = u.shape
    _arg(v, "ball_counts v", torch.float32, ("N", D), copy=False, like=u)
    N = v.shape[0]
    _arg(ru, "ball_counts ru", torch.float32, (M,), copy=False, like=u)
    nu = row_sqnorms(u) if nu is None else nu
    nv = row_sqnorms(v) if nv is None else nv
    _arg(nu, "ball_counts nu", torch.float32, (M,), copy=False, like=u)
    _arg(nv, "ball_counts nv", torch.float32, (N,), copy=False, like=u)
    nsplit = default_col_splits(M, N) if nsplit is None else int(nsplit)
    if nsplit < 1:
        raise RuntimeError(f"ball_counts: nsplit {nsplit} (>= 1)")
    nbytes = L.load().ldmae_ball_counts_partials_bytes(M, nsplit)
    part = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=u.device)
    counts = torch.empty(M, dtype=torch.int32, device=u.device)
    call("ldmae_ball_counts", ptr(u), ptr(nu), ptr(ru), M, ptr(v), ptr(nv), N, D, nsplit, ptr(part), ptr(counts), stream())
    return counts


def check_kid_index_table(idx, n_rows, what):
    """The range check ldmae_kid_sums leaves to its caller, on the HOST copy of one index table: [S, m] integers, every entry in [0, n_rows).
    Returns the table as a contiguous int32 host tensor.  Raises ValueError naming the first bad subset and position."""
    idx = torch.as_tensor(idx)
    if idx.is_cuda:
        raise ValueError(f"kid_sums: {what} is checked on its host copy; got a tensor on {idx.device}")
    if idx.dim() != 2 or idx.shape[0] < 1 or idx.shape[1] < 2 or idx.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"kid_sums: {what} must be an [S, m] int32 / int64 table with S >= 1 and m >= 2, got {tuple(idx.shape)} {idx.dtype}")
    bad = (idx < 0) | (idx >= int(n_rows))
    if bool(bad.any()):
        s, i = (int(t) for t in bad.nonzero()[0])
        raise ValueError(f"kid_sums: {what}[{s}, {i}] = {int(idx[s, i])} (subset {s}, position {i}) is outside [0, {int(n_rows)})")
    return idx.to(torch.int32).contiguous()


def kid_sums(a, b, idx_a, idx_b, gamma, coef0=1.0, nsplit=None):
    """The sums of KID's unbiased MMD^2 over S subsets in one launch (ldmae_kid_sums): a [Na, D], b [Nb, D] f32 on the device; idx_a / idx_b
    [S, m] HOST index tables (numpy or torch, checked here against [0, Na) / [0, Nb) and uploaded; rows are read through them, not gathered)
    -> f64 [S, 3] = (sum_{i != j} k(a_i, a_j), sum_{i != j} k(b_i, b_j), sum_{i, j} k(a_i, b_j)), k(x, y) = (gamma x.y + coef0)^3 with the dot
    product, the fma and the two multiplies in f32 and the sums in f64.  Bitwise the same for every nsplit."""
    _arg(a, "kid_sums a", torch.float32, ("Na", "D"), copy=False)
    Na, D = a.shape
    _arg(b, "kid_sums b", torch.float32, ("Nb", D), copy=False, like=a)
    Nb = b.shape[0]
    ia, ib = check_kid_index_table(idx_a, Na, "idx_a"), check_kid_index_table(idx_b, Nb, "idx_b")
    if ia.shape != ib.shape:
        raise ValueError(f"kid_sums: idx_a {tuple(ia.shape)} and idx_b {tuple(ib.shape)} must have one shape [S, m]")
    S, m = ia.shape
    if m > min(Na, Nb):
        raise ValueError(f"kid_sums: subsets of {m} rows from {Na} / {Nb} feature rows")
    if nsplit is None:                       # as default_col_splits, with the 3 S (subset, pair) planes of the grid counted in
        row_tiles, col_tiles = _pair_tiles(m)[0], _pair_tiles(m)[1]
        nsplit = max(1, min(col_tiles, -(-2048 // (row_tiles * 3 * S))))
    nsplit = int(nsplit)
    if nsplit < 1:
        raise RuntimeError(f"kid_sums: nsplit {nsplit} (>= 1)")
    ia, ib = ia.to(a.device), ib.to(a.device)
    _arg(ia, "kid_sums idx_a", torch.int32, (S, m), copy=False, like=a)
    _arg(ib, "kid_sums idx_b", torch.int32, (S, m), copy=False, like=a)
    nbytes = _ws_bytes("ldmae_kid_workspace_bytes", S, m)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=a.device)
    out = torch.empty(S, 3, dtype=torch.float64, device=a.device)
    call("ldmae_kid_sums", ptr(a), Na, ptr(b), Nb, D, ptr(ia), ptr(ib), S, m, float(gamma), float(coef0), nsplit, ptr(ws), ptr(out), stream())
    return out


# ----------------------------------------------------------------------------- linear probe and k-NN (csrc/linprobe.hip), DESIGN.md section 23
# The kernels work on the caller's tensors as they are (copy=False, out=True).  Label tables are HOST tables: check_labels checks and uploads them.
TOPK_MAX_K = 256            # LDMAE_TOPK_MAX_K
KNN_VOTE_MAX_C = 12288      # LDMAE_KNN_VOTE_MAX_C


def check_labels(labels, num_classes, device, what="labels"):
    """The range check the kernels leave to their caller, on the HOST copy of a label vector: [B] integers, every entry in [0, num_classes).
    Returns the int64 device copy.  Raises ValueError naming the first bad entry."""
    labels = torch.as_tensor(labels)
    if labels.is_cuda:
        raise ValueError(f"{what} are checked on their host copy; got a tensor on {labels.device}")
    if labels.dim() != 1 or labels.numel() < 1 or labels.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what} must be a non-empty [B] int32 / int64 vector, got {tuple(labels.shape)} {labels.dtype}")
    bad = (labels < 0) | (labels >= int(num_classes))
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise ValueError(f"{what}[{i}] = {int(labels[i])} is outside [0, {int(num_classes)})")
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"ldmae_amd ops need tensors on a HIP device (no CPU fallback); got {device}")
    return labels.to(device, torch.int64).contiguous()


def _device_labels(labels, num_classes, like, n, what):
    """Host labels: checked and uploaded; a device int64 vector is taken as one check_labels has returned."""
    if not (torch.is_tensor(labels) and labels.is_cuda):
        labels = check_labels(labels, num_classes, like.device, what)
    return _arg(labels, what, torch.int64, (n,), copy=False, like=like)


def token_mean(x, col0=0, d=None):
    """x [B, N, W] f32 / bf16 / fp16, channels adjacent, token rows W' >= W apart (a channel slice of a wider buffer is read in place)
    -> f32 [B, d]: the mean over the N tokens of channels [col0, col0 + d) (d None: all from col0).  Fixed summation order."""
    if x.dim() != 3 or x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise RuntimeError(f"token_mean x: a [B, N, W] float32 / bfloat16 / float16 tensor expected, got {tuple(x.shape)} {x.dtype}")
    B, N, W = x.shape
    d = W - int(col0) if d is None else int(d)
    if B < 1 or N < 1 or col0 < 0 or d < 1 or col0 + d > W:
        raise RuntimeError(f"token_mean: channels [{col0}, {col0 + d}) of {tuple(x.shape)}")
    ldx = x.stride(1) if N > 1 else (x.stride(0) if B > 1 else W)
    if (W > 1 and x.stride(2) != 1) or ldx < W or (B > 1 and x.stride(0) != N * ldx):
        raise RuntimeError(f"token_mean x: the kernel reads token rows with adjacent channels at one row stride; got strides {tuple(x.stride())} "
                           f"for shape {tuple(x.shape)}")
    out = torch.empty(B, d, dtype=torch.float32, device=x.device)
    call("ldmae_token_mean", dt(x.dtype), ptr(x), ldx, int(col0), ptr(out), B, N, d, stream())
    return out


def bn1d_fwd(x, run_mean, run_var, training=True, eps=1e-6, momentum=0.1, out=None, save=False):
    """BatchNorm1d(affine=False) of x [B, D] f32 (rows may be strided) -> xhat [B, D].  training: batch statistics (two-pass biased variance),
    run_mean / run_var [D] updated IN PLACE (momentum, unbiased variance); B = 1 is refused.  Not training: normalises with the running
    statistics.  save=True (training): also returns (mean, rstd)."""
    _arg(x, "bn1d_fwd x", torch.float32, ("B", "D"), rows=True, copy=False)
    B, D = x.shape
    if training and B < 2:
        raise ValueError(f"bn1d_fwd: Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    _arg(run_mean, "bn1d_fwd run_mean", torch.float32, (D,), out=True, like=x)
    _arg(run_var, "bn1d_fwd run_var", torch.float32, (D,), out=True, like=x)
    if out is None:
        out = torch.empty(B, D, dtype=torch.float32, device=x.device)
    else:
        _arg(out, "bn1d_fwd out", torch.float32, (B, D), rows=True, out=True, like=x)
    sm = torch.empty(D, dtype=torch.float32, device=x.device) if save and training else None
    sr = torch.empty(D, dtype=torch.float32, device=x.device) if save and training else None
    call("ldmae_bn1d_fwd", F32, ptr(x), _ld(x), ptr(out), _ld(out), ptr(run_mean), ptr(run_var), ptr(sm), ptr(sr), B, D, float(eps), float(momentum),
         1 if training else 0, stream())
    return (out, sm, sr) if save and training else out


def softmax_xent(logits, labels, num_classes=None, grad_scale=None, dlogits=None):
    """logits [B, W] f32 (rows may be strided; the first num_classes columns count, default all), labels [B]: a HOST vector (checked against
    [0, C) and uploaded here) or the device vector check_labels returned -> (loss [B] f32, rank [B] i32, dlogits or None).  grad_scale given:
    dlogits [B, C] = (softmax - onehot) * grad_scale, written into `dlogits` if passed (rows may be strided; columns beyond C untouched).
    rank = #{c : l[c] > l[y]} + #{c < y : l[c] == l[y]}: top-1 is rank == 0, top-5 rank < 5."""
    _arg(logits, "softmax_xent logits", torch.float32, ("B", "W"), rows=True, copy=False)
    B, W = logits.shape
    C = W if num_classes is None else int(num_classes)
    if not 1 <= C <= W:
        raise RuntimeError(f"softmax_xent: {C} classes in rows of {W} logits")
    labels = _device_labels(labels, C, logits, B, "softmax_xent labels")
    if grad_scale is None:
        if dlogits is not None:
            raise RuntimeError("softmax_xent: dlogits needs grad_scale")
    elif dlogits is None:
        dlogits = torch.empty(B, C, dtype=torch.float32, device=logits.device)
    else:
        _arg(dlogits, "softmax_xent dlogits", torch.float32, (B, "W >= C"), rows=True, out=True, like=logits)
        if dlogits.shape[1] < C:
            raise RuntimeError(f"softmax_xent dlogits: {dlogits.shape[1]} columns for {C} classes")
    labels = _device_labels(labels, C, logits, B, "softmax_xent labels")      # (idempotent: the device vector made above passes as it is)
    loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    rank = torch.empty(B, dtype=torch.int32, device=logits.device)
    call("ldmae_softmax_xent", F32, ptr(logits), _ld(logits), ptr(labels), ptr(loss), ptr(dlogits), 0 if dlogits is None else max(_ld(dlogits), C),
         ptr(rank), B, C, float(grad_scale or 0.0), stream())
    return loss, rank, dlogits


def lars_norms(p, g, weight_decay=0.0, out=None):
    """(|p|, |g + wd p|) of two f32 tensors of one size -> f32 [2] on the device (two-stage fixed-order reduction, sums in f64)."""
    _arg(p, "lars_norms p", torch.float32, copy=False)
    _arg(g, "lars_norms g", torch.float32, numel=p.numel(), copy=False, like=p)
    if p.numel() < 1:
        raise RuntimeError("lars_norms: empty tensor")
    if out is None:
        out = torch.empty(2, dtype=torch.float32, device=p.device)
    else:
        _arg(out, "lars_norms out", torch.float32, (2,), out=True, like=p)
    nbytes = _ws_bytes("ldmae_lars_workspace_bytes", p.numel())
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=p.device)
    call("ldmae_lars_norms", F32, ptr(p), ptr(g), p.numel(), float(weight_decay), ptr(ws), ptr(out), stream())
    return out


def lars_step(p, g, mu, lr, norms=None, weight_decay=0.0, momentum=0.9, trust=0.001):
    """One LARS update of p and mu IN PLACE (the reference's util/lars.py).  norms (f32 [2] from lars_norms, read on the device): the tensor has
    more than one dimension -- dp = (g + wd p) * q, q = trust |p| / |dp| where both are positive, else 1.  norms None: a bias -- dp = g.
    Then mu = momentum mu + dp, p -= lr mu."""
    _arg(p, "lars_step p", torch.float32, out=True)
    _arg(g, "lars_step g", torch.float32, numel=p.numel(), copy=False, like=p)
    _arg(mu, "lars_step mu", torch.float32, numel=p.numel(), out=True, like=p)
    _arg(norms, "lars_step norms", torch.float32, (2,), copy=False, like=p)
    if p.numel() < 1:
        raise RuntimeError("lars_step: empty tensor")
    call("ldmae_lars_step", F32, ptr(p), ptr(g), ptr(mu), p.numel(), ptr(norms), float(lr), float(weight_decay), float(momentum), float(trust), stream())
    return p


def l2_normalize(x):
    """f32 [M, D] -> x / max(|x_m|, 1e-12) row by row (F.normalize): row_sqnorms, then one scaling pass."""
    _arg(x, "l2_normalize x", torch.float32, ("M", "D"), copy=False)
    out = torch.empty_like(x)
    call("ldmae_l2_normalize", ptr(x), ptr(row_sqnorms(x)), ptr(out), x.shape[0], x.shape[1], stream())
    return out


def topk_empty(m, k, device):
    """All-empty running lists of topk_merge: (values [m, k] = -inf, indices [m, k] = -1)."""
    if not 1 <= int(k) <= TOPK_MAX_K:
        raise ValueError(f"topk: k = {k} neighbours; the merge kernel keeps 1 .. {TOPK_MAX_K}")
    return (torch.full((m, k), float("-inf"), dtype=torch.float32, device=device), torch.full((m, k), -1, dtype=torch.int32, device=device))


def topk_merge(sims, col0, vals, idx):
    """Merge the chunk sims [M, Nc] f32 (rows may be strided; column j is bank row col0 + j) into the running lists vals / idx [M, k] IN PLACE:
    sorted by value descending, then index ascending, empty slots (-inf, -1) last.  Exact: comparisons only."""
    _arg(sims, "topk_merge sims", torch.float32, ("M", "Nc"), rows=True, copy=False)
    M, Nc = sims.shape
    _arg(vals, "topk_merge vals", torch.float32, (M, "k"), out=True, like=sims)
    k = vals.shape[1]
    if not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f"topk_merge: k = {k} neighbours; the kernel keeps 1 .. {TOPK_MAX_K}")
    _arg(idx, "topk_merge idx", torch.int32, (M, k), out=True, like=sims)
    if col0 < 0 or col0 + Nc >= 2 ** 31:
        raise RuntimeError(f"topk_merge: bank rows [{col0}, {col0 + Nc}) leave the int32 index range")
    call("ldmae_topk_merge", ptr(sims), _ld(sims), M, Nc, int(col0), ptr(vals), ptr(idx), k, stream())
    return vals, idx


def knn_vote(vals, idx, bank_labels, query_labels, num_classes, temperature=0.07, return_scores=False):
    """The weighted k-NN vote (DINO's protocol): score[c] = sum of exp(sim / T) over the neighbours of class c, in list order -> rank [M] i32 of
    the query's own class (softmax_xent's rule, ties to the lower class).  vals / idx [M, k] from topk_merge; the label vectors are HOST
    vectors (checked here) or what check_labels returned.  return_scores: also the f32 [M, C] scores."""
    _arg(vals, "knn_vote vals", torch.float32, ("M", "k"), copy=False)
    M, k = vals.shape
    _arg(idx, "knn_vote idx", torch.int32, (M, k), copy=False, like=vals)
    C = int(num_classes)
    if not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f"knn_vote: k = {k} neighbours; the kernel takes 1 .. {TOPK_MAX_K}")
    if not 1 <= C <= KNN_VOTE_MAX_C:
        raise ValueError(f"knn_vote: {C} classes; the scores of a query are held in LDS, KNN_VOTE_MAX_C = {KNN_VOTE_MAX_C} fit")
    nbank = int(torch.as_tensor(bank_labels).numel())
    bank_labels = _device_labels(bank_labels, C, vals, nbank, "knn_vote bank_labels")
    query_labels = _device_labels(query_labels, C, vals, M, "knn_vote query_labels")
    rank = torch.empty(M, dtype=torch.int32, device=vals.device)
    scores = torch.empty(M, C, dtype=torch.float32, device=vals.device) if return_scores else None
    call("ldmae_knn_vote", ptr(vals), ptr(idx), M, k, ptr(bank_labels), nbank, ptr(query_labels), C, float(temperature), ptr(rank), ptr(scores), stream())
    return (rank, scores) if return_scores else rank


# ----------------------------------------------------------------------------- FID evaluation (csrc/inception.hip), NHWC f32
# A channel slice is (tensor [B, H, W, Ctot], offset, C): the kernels read / write channels [offset, offset + C) of every pixel.
# From here to the end of the file the kernels work on the caller's tensors as they are: every _arg below says copy=False, or out=True for an output.

def conv2d_nhwc(x, w, bias=None, stride=(1, 1), padding=(0, 0), relu=True, xoff=0, cin=None, out=None, ooff=0):
    """Implicit-GEMM convolution on the exact-f32 MFMA.  x [B, H, W, ldx] read at channels [xoff, xoff + cin); w [Cout, kh, kw, Cin] f32;
    out [B, Ho, Wo, ldo] written at channels [ooff, ooff + Cout) (allocated as [B, Ho, Wo, Cout] when None); bias + ReLU epilogue."""
    _arg(x, "conv2d_nhwc x", torch.float32, "NHWC", copy=False)
    B, H, W, ldx = x.shape
    _arg(w, "conv2d_nhwc weight", torch.float32, ("Cout", "kh", "kw", "Cin" if cin is None else cin), copy=False, like=x)
    Cout, kh, kw, Cin = w.shape
    _arg(bias, "conv2d_nhwc bias", torch.float32, (Cout,), copy=False, like=x)
    sh, sw = stride
    ph, pw = padding
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    if out is None:
        out = torch.empty(B, Ho, Wo, Cout, dtype=torch.float32, device=x.device)
    _arg(out, "conv2d_nhwc out", torch.float32, (B, Ho, Wo, "ldo"), out=True, like=x)
    call("ldmae_conv2d_nhwc_f32", ptr(x), ldx, xoff, ptr(w), ptr(bias), ptr(out), out.shape[3], ooff, B, H, W, Cin, Cout, kh, kw, sh, sw, ph, pw,
         1 if relu else 0, stream())
    return out


def pool2d_nhwc(x, mode, k=3, stride=1, pad=0, xoff=0, c=None, out=None, ooff=0):
    """3x3-style pooling of channel slices: mode "max" (padding never wins) or "avg" (count_include_pad=False)."""
    _arg(x, "pool2d_nhwc x", torch.float32, "NHWC", copy=False)
    B, H, W, ldx = x.shape
    c = ldx - xoff if c is None else c
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if out is None:
        out = torch.empty(B, Ho, Wo, c, dtype=torch.float32, device=x.device)
    _arg(out, "pool2d_nhwc out", torch.float32, (B, Ho, Wo, "ldo"), out=True, like=x)
    call("ldmae_pool2d_nhwc_f32", {"max": 0, "avg": 1}[mode], ptr(x), ldx, xoff, ptr(out), out.shape[3], ooff, B, H, W, c, k, stride, pad, stream())
    return out


def global_avgpool_nhwc(x, xoff=0, c=None):
    """[B, H, W, ldx] (or [B, HW, ldx]) -> [B, c]: the mean over all pixels of channels [xoff, xoff + c)."""
    _arg(x, "global_avgpool_nhwc x", torch.float32, ("B", "HW", "C") if x.dim() == 3 else "NHWC", copy=False)
    B, ldx = x.shape[0], x.shape[-1]
    HW = x[0, ..., 0].numel()
    c = ldx - xoff if c is None else c
    out = torch.empty(B, c, dtype=torch.float32, device=x.device)
    call("ldmae_global_avgpool_nhwc_f32", ptr(x), ldx, xoff, ptr(out), B, HW, c, stream())
    return out


def _preprocess(op, img, size):
    """fid_preprocess / adm_preprocess: one wrapper, two resampling rules (entry point ldmae_<op>)."""
    _arg(img, op + " img", torch.uint8, ("B", "H", "W", 3), copy=False)
    B, H, W, _ = img.shape
    out = torch.empty(B, size, size, 3, dtype=torch.float32, device=img.device)
    call("ldmae_" + op, ptr(img), ptr(out), B, H, W, size, size, stream())
    return out


def fid_preprocess(img, size=299):
    """uint8 [B, H, W, 3] RGB -> f32 [B, size, size, 3] = F.interpolate(img / 255, (size, size), bilinear, align_corners=False) * 2 - 1."""
    return _preprocess("fid_preprocess", img, size)


def fid_stats_accumulate(feats, shift, s1, s2):
    """s1 [D] += sum_r (f_r - shift); s2 [D, D] += sum_r (f_r - shift)(f_r - shift)^T, f64 accumulators on the device."""
    _arg(feats, "fid_stats_accumulate feats", torch.float32, ("n", "D"), copy=False)
    n, D = feats.shape
    _arg(shift, "fid_stats_accumulate shift", torch.float32, (D,), copy=False, like=feats)
    _arg(s1, "fid_stats_accumulate s1", torch.float64, (D,), out=True, like=feats)
    _arg(s2, "fid_stats_accumulate s2", torch.float64, (D, D), out=True, like=feats)
    call("ldmae_fid_stats_accumulate", ptr(feats), n, D, ptr(shift), ptr(s1), ptr(s2), stream())


# ----------------------------------------------------------------------------- ADM evaluator (csrc/adm_eval.hip), f32
def adm_preprocess(img, size=299):
    """uint8 [B, H, W, 3] RGB -> f32 [B, size, size, 3] = (TF1 legacy ResizeBilinear(img) - 128) / 128: the ADM Inception graph's
    pre-processing (src = dst * in / out, no half-pixel centres)."""
    return _preprocess("adm_preprocess", img, size)


def adm_spatial_tap(x, xoff=0, c=7):
    """[B, H, W, ldx] -> f32 [B, H * W * c]: channels [xoff, xoff + c) of every pixel, flattened in (h, w, c) order (TF's NHWC reshape)."""
    _arg(x, "adm_spatial_tap x", torch.float32, "NHWC", copy=False)
    B, H, W, ldx = x.shape
    if xoff < 0 or c <= 0 or xoff + c > ldx:
        raise RuntimeError(f"adm_spatial_tap: channel slice [{xoff}, {xoff + c}) of {ldx}")
    out = torch.empty(B, H * W * c, dtype=torch.float32, device=x.device)
    call("ldmae_adm_spatial_tap", ptr(x), ldx, xoff, ptr(out), B, H * W, c, stream())
    return out


def row_sqnorms(x):
    """f32 [M, D] -> f32 [M]: |x_m|^2 accumulated in f64, rounded once."""
    _arg(x, "row_sqnorms x", torch.float32, ("M", "D"), copy=False)
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    call("ldmae_row_sqnorms_f32", ptr(x), x.shape[0], x.shape[1], ptr(out), stream())
    return out


def pairwise_logits(u, w):
    """u [M, D] . w [N, D]^T -> f32 [M, N] on the exact-f32 MFMA, no bias (the ADM softmax graph's MatMul)."""
    _arg(u, "pairwise_logits u", torch.float32, ("M", "D"), copy=False)
    _arg(w, "pairwise_logits w", torch.float32, ("N", u.shape[1]), copy=False, like=u)
    out = torch.empty(u.shape[0], w.shape[0], dtype=torch.float32, device=u.device)
    call("ldmae_pairwise_logits", ptr(u), u.shape[0], u.shape[1], ptr(w), w.shape[0], ptr(out), stream())
    return out


def _pair_tiles(n):
    return (n + 127) // 128, (n + 63) // 64


def default_col_splits(m, n):
    """Column splits of a pairwise pass: enough (row tile, split) workgroups to fill the chip (~2048), at most one per 64-column tile."""
    row_tiles, col_tiles = _pair_tiles(m)[0], _pair_tiles(n)[1]
    return max(1, min(col_tiles, -(-2048 // row_tiles)))


def _nhood(nhood_sizes):
    nh = [int(k) for k in nhood_sizes]
    if not nh or len(nh) > 8 or min(nh) < 0 or max(nh) > 7:
        raise RuntimeError(f"nhood_sizes {tuple(nhood_sizes)}: 1..8 sizes, each in [0, 7]")
    return nh


def knn_radii(x, nhood_sizes=(3,), norms=None, nsplit=None):
    """f32 [N, D] -> f32 [N, len(nhood_sizes)]: column t is the value at sorted index nhood_sizes[t] of the row's squared distances
    max(|x_i|^2 - 2 x_i.x_j + |x_j|^2, 0) to every row (itself included), as np.partition(d, seq)[:, k].  nsplit: column splits of the
    pass (default default_col_splits); the result is bitwise the same for every nsplit."""
    _arg(x, "knn_radii x", torch.float32, ("N", "D"), copy=False)
    N, D = x.shape
    nh = _nhood(nhood_sizes)
    if N <= max(nh):
        raise RuntimeError(f"knn_radii: {N} rows hold no neighbour at sorted index {max(nh)}")
    norms = row_sqnorms(x) if norms is None else norms
    _arg(norms, "knn_radii norms", torch.float32, (N,), copy=False, like=x)
    nsplit = default_col_splits(N, N) if nsplit is None else int(nsplit)
    if nsplit < 1:
        raise RuntimeError(f"knn_radii: nsplit {nsplit} (>= 1)")
    nbytes = L.load().ldmae_knn_partials_bytes(N, nsplit)
    part = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    radii = torch.empty(N, len(nh), dtype=torch.float32, device=x.device)
    arr = (ctypes.c_int * len(nh))(*nh)
    call("ldmae_knn_radii", ptr(x), ptr(norms), N, D, arr, len(nh), nsplit, ptr(part), ptr(radii), stream())
    return radii


def pr_flags(u, ru, v, rv, nu=None, nv=None, nsplit=None):
    """Manifold membership between u [M, D] (radii ru [M, K]) and v [N, D] (radii rv [N, K]): (u_in [M, K], v_in [N, K]) int32, with
    u_in[i, k] = any_j d(i, j) <= rv[j, k] and v_in[j, k] = any_i d(i, j) <= ru[i, k] (evaluator.py DistanceBlock.less_thans)."""
    _arg(u, "pr_flags u", torch.float32, ("M", "D"), copy=False)
    M, D = u.shape
    _arg(v, "pr_flags v", torch.float32, ("N", D), copy=False, like=u)
    N = v.shape[0]
    _arg(ru, "pr_flags ru", torch.float32, (M, "K"), copy=False, like=u)
    K = ru.shape[1]
    _arg(rv, "pr_flags rv", torch.float32, (N, K), copy=False, like=u)
    if not 1 <= K <= 8:
        raise RuntimeError(f"pr_flags: radii {tuple(ru.shape)} / {tuple(rv.shape)}: 1..8 columns")
    nu = row_sqnorms(u) if nu is None else nu
    nv = row_sqnorms(v) if nv is None else nv
    _arg(nu, "pr_flags nu", torch.float32, (M,), copy=False, like=u)
    _arg(nv, "pr_flags nv", torch.float32, (N,), copy=False, like=u)
    nsplit = default_col_splits(M, N) if nsplit is None else int(nsplit)
    if nsplit < 1:
        raise RuntimeError(f"pr_flags: nsplit {nsplit} (>= 1)")
    u_in = torch.zeros(M, K, dtype=torch.int32, device=u.device)
    v_in = torch.zeros(N, K, dtype=torch.int32, device=u.device)
    call("ldmae_pr_flags", ptr(u), ptr(nu), ptr(ru), M, ptr(v), ptr(nv), ptr(rv), N, D, K, nsplit, ptr(u_in), ptr(v_in), stream())
    return u_in, v_in


def adm_softmax_is(logits, split=5000):
    """logits f32 [M, C] -> (h f64 [M], S f64 [ceil(M / split), C]): h[i] = sum_c p log p (0 log 0 = 0), S[s] = sum of p over rows
    [s * split, (s + 1) * split), p = softmax(logits) in f32; fixed-order sums (bitwise reproducible)."""
    _arg(logits, "adm_softmax_is logits", torch.float32, ("M", "C"), copy=False)
    M, Cc = logits.shape
    if split < 1:
        raise RuntimeError(f"adm_softmax_is: split {split} (>= 1)")
    ws = workspace(_ws_bytes("ldmae_adm_is_workspace_bytes", M, Cc, split), logits.device, "adm_is")
    h = torch.empty(M, dtype=torch.float64, device=logits.device)
    S = torch.empty(-(-M // split), Cc, dtype=torch.float64, device=logits.device)
    call("ldmae_adm_softmax_is", ptr(logits), M, Cc, split, ptr(ws), ptr(h), ptr(S), stream())
    return h, S


# ----------------------------------------------------------------------------- tokenizer evaluation (csrc/tokenizer_eval.hip), f32
# ... and LPIPS: forward, backward (csrc/lpips_bwd.hip: f32 NHWC, no atomics) and the 16-bit path (csrc/lpips_f16.hip: fp16 forward, bf16 data
# gradient).  The C side serves an f32 entry point and its 16-bit twin from one template; so does this file: one private body per pair, named
# after the f32 wrapper, with the facts that differ as parameters (op = the public name, and "ldmae_" + op the entry point unless given).

def _lpips_prep(op, input, target, out_dtype, C):
    _arg(input, op + " input", torch.float32, ("B", 3, "H", "W"), copy=False)
    _arg(target, op + " target", torch.float32, input.shape, copy=False, like=input)
    B, _, H, W = input.shape
    out = torch.empty(2 * B, H, W, C, dtype=out_dtype, device=input.device)
    call("ldmae_" + op, ptr(input), ptr(target), ptr(out), B, H, W, stream())
    return out


def lpips_prep(input, target):
    """LPIPS' ScalingLayer on both images: NCHW f32 [B, 3, H, W] x 2 -> NHWC f32 [2B, H, W, 4] = (x - shift) / scale, input first, channel 3
    zero (the Cin-4 VEC path of conv2d_nhwc)."""
    return _lpips_prep("lpips_prep", input, target, torch.float32, 4)


def _lpips_tap(op, f, lin_w, f_dtype, align):
    """The tap f [2B, h, w, C] and its lin weight [C], common to the four lpips_layer wrappers -> (lin_w, B, h, w, C)."""
    _arg(f, op + " f", f_dtype, "NHWC", copy=False, align=align)
    n, h, w, C = f.shape
    if n % 2 or C not in (64, 128, 256, 512):
        raise RuntimeError(f"{op}: features {tuple(f.shape)}: need [2B, h, w, C] with C in 64, 128, 256, 512")
    return _arg(lin_w, op + " lin_w", torch.float32, numel=C, like=f), n // 2, h, w, C


def _lpips_layer(op, f, lin_w, out, f_dtype, align):
    lin_w, B, h, w, C = _lpips_tap(op, f, lin_w, f_dtype, align)
    _arg(out, op + " out", torch.float32, (B,), out=True, like=f)
    ws = workspace(_ws_bytes("ldmae_lpips_workspace_bytes", B, h, w), f.device, "lpips")
    call("ldmae_" + op, ptr(f), ptr(lin_w), ptr(out), B, h, w, C, ptr(ws), stream())
    return out


def lpips_layer(f, lin_w, out):
    """One VGG tap f [2B, h, w, C] (C = 64, 128, 256, 512) and its lin weight [C]: out [B] += mean_hw sum_c w_c (f^_b - f^_(B+b))^2, f^ the
    channel-normalised features (f / (|f| + 1e-10)).  out is accumulated in place (f32 [B])."""
    return _lpips_layer("lpips_layer", f, lin_w, out, torch.float32, 0)


def _conv3x3_relu_dgrad(op, entry, dy, y, w_rot, out, y_dtype, w_dtype, multiple, align):
    _arg(y, op + " y", y_dtype, "NHWC", copy=False, align=align)
    B, H, W, Cy = y.shape
    _arg(dy, op + " dy", torch.float32, y.shape, copy=False, like=y, align=align)
    _arg(w_rot, op + " rotated weight", w_dtype, ("Cx", 3, 3, Cy), copy=False, like=y, align=align)
    if Cy % multiple or dy.numel() == 0:
        raise RuntimeError(f"{op}: {Cy} gradient channels (a multiple of {multiple}) of a non-empty tensor")
    Cx = w_rot.shape[0]
    if out is None:
        out = torch.empty(B, H, W, Cx, dtype=torch.float32, device=dy.device)
    _arg(out, op + " out", torch.float32, (B, H, W, Cx), out=True, like=y)
    call(entry, ptr(dy), ptr(y), ptr(w_rot), ptr(out), B, H, W, Cy, Cx, stream())
    return out


def conv3x3_relu_dgrad_nhwc(dy, y, w_rot, out=None):
    """Data gradient of y = relu(conv3x3(x, w) + b) (stride 1, pad 1): dx [B, H, W, Cx] = conv3x3(dy * [y > 0], w_rot) with dy, y [B, H, W, Cy] and
    w_rot [Cx, 3, 3, Cy] (models.lpips.rotate_weight of the forward weight).  The ReLU mask is taken from y inside the operand gather."""
    return _conv3x3_relu_dgrad("conv3x3_relu_dgrad_nhwc", "ldmae_conv3x3_relu_dgrad_nhwc_f32", dy, y, w_rot, out, torch.float32, torch.float32, 4, 0)


def _maxpool2x2_bwd(op, entry, dy, x, out, x_dtype, align):
    _arg(x, op + " x", x_dtype, "NHWC", copy=False, align=align)
    B, H, W, C = x.shape
    _arg(dy, op + " dy", torch.float32, (B, H // 2, W // 2, C), copy=False, like=x)
    if C % 4 or x.numel() == 0:
        raise RuntimeError(f"{op}: x {tuple(x.shape)}: need a non-empty tensor with a multiple of 4 channels")
    if out is None:
        out = torch.empty(B, H, W, C, dtype=torch.float32, device=x.device)
    _arg(out, op + " out", torch.float32, x.shape, out=True, like=x)
    call(entry, ptr(dy) if dy.numel() else None, ptr(x), ptr(out), B, H, W, C, stream())
    return out


def maxpool2x2_bwd_nhwc(dy, x, out=None):
    """Backward of pool2d_nhwc(x, "max", k=2, stride=2): dx [B, H, W, C] from dy [B, H // 2, W // 2, C] and the pooled input x.  dy goes to the
    window's maximum (the first in row-major order on a tie, as torch); odd last rows / columns get 0; every element of dx is written."""
    return _maxpool2x2_bwd("maxpool2x2_bwd_nhwc", "ldmae_maxpool2x2_bwd_nhwc_f32", dy, x, out, torch.float32, 0)


def _lpips_layer_bwd(op, f, lin_w, g, d_input, d_target, accumulate, f_dtype, align):
    lin_w, B, h, w, C = _lpips_tap(op, f, lin_w, f_dtype, align)
    _arg(g, op + " g", torch.float32, (B,), copy=False, like=f)
    if d_input is None and d_target is None:
        raise RuntimeError(f"{op}: neither d_input nor d_target given: nothing to compute")
    _arg(d_input, op + " d_input", torch.float32, (B, h, w, C), out=True, like=f)
    _arg(d_target, op + " d_target", torch.float32, (B, h, w, C), out=True, like=f)
    call("ldmae_" + op, ptr(f), ptr(lin_w), ptr(g), ptr(d_input), ptr(d_target), B, h, w, C, 1 if accumulate else 0, stream())
    return d_input, d_target


def lpips_layer_bwd(f, lin_w, g, d_input=None, d_target=None, accumulate=False):
    """Backward of lpips_layer for one tap f [2B, h, w, C]: with g [B] the gradient of the per-pair value, the gradient to f's first (input) /
    second (target) half is written into d_input / d_target [B, h, w, C]; None = that half is not wanted (at least one is).  accumulate=True adds
    into the buffers (which then hold the following pool's backward), else they are overwritten.  A pixel whose channels are all zero in a half
    gets exactly 0 there (torch gives NaN).  -> (d_input, d_target)."""
    return _lpips_layer_bwd("lpips_layer_bwd", f, lin_w, g, d_input, d_target, accumulate, torch.float32, 0)


def _lpips_prep_bwd(op, g, C):
    _arg(g, op + " g", torch.float32, ("B", "H", "W", C), copy=False)
    B, H, W, _ = g.shape
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=g.device)
    call("ldmae_" + op, ptr(g), ptr(out), B, H, W, stream())
    return out


def lpips_prep_bwd(g):
    """Backward of lpips_prep for one half: g NHWC f32 [B, H, W, 4] (the data gradient of conv1_1) -> NCHW f32 [B, 3, H, W] = g[..., c] / scale[c]."""
    return _lpips_prep_bwd("lpips_prep_bwd", g, 4)


def lpips_prep_f16(input, target):
    """lpips_prep's f32 arithmetic, then one rounding: NCHW f32 [B, 3, H, W] x 2 -> NHWC fp16 [2B, H, W, 8], input first, channels 3 .. 7 zero
    (the Cin % 8 == 0 operand of conv3x3_relu_nhwc_f16)."""
    return _lpips_prep("lpips_prep_f16", input, target, torch.float16, 8)


def conv3x3_relu_nhwc_f16(x, w, bias=None, out=None):
    """relu(conv3x3(x, w) + bias), stride 1, pad 1, on the fp16 MFMA with f32 accumulation: x fp16 [B, H, W, Cin] (Cin % 8 == 0), w fp16
    [Cout, 3, 3, Cin], bias f32 [Cout]; the f32 result is rounded once to fp16 (saturating at +-65504) into out [B, H, W, Cout] (a contiguous
    view of a larger tensor is taken as it is; allocated when None)."""
    _arg(x, "conv3x3_relu_nhwc_f16 x", torch.float16, "NHWC", copy=False, align=16)
    B, H, W, Cin = x.shape
    _arg(w, "conv3x3_relu_nhwc_f16 weight", torch.float16, ("Cout", 3, 3, Cin), copy=False, like=x, align=16)
    if Cin % 8 or x.numel() == 0:
        raise RuntimeError(f"conv3x3_relu_nhwc_f16: x {tuple(x.shape)}: need a non-empty tensor with a multiple of 8 channels")
    Cout = w.shape[0]
    _arg(bias, "conv3x3_relu_nhwc_f16 bias", torch.float32, (Cout,), copy=False, like=x)
    if out is None:
        out = torch.empty(B, H, W, Cout, dtype=torch.float16, device=x.device)
    _arg(out, "conv3x3_relu_nhwc_f16 out", torch.float16, (B, H, W, Cout), out=True, like=x)
    call("ldmae_conv3x3_relu_nhwc_f16", ptr(x), ptr(w), ptr(bias), ptr(out), B, H, W, Cin, Cout, stream())
    return out


def maxpool2x2_nhwc_f16(x):
    """2x2 / 2 max pool of fp16 NHWC [B, H, W, C] (C % 8 == 0, H, W >= 2) -> [B, H // 2, W // 2, C]; the odd last row / column is dropped."""
    _arg(x, "maxpool2x2_nhwc_f16 x", torch.float16, "NHWC", copy=False, align=16)
    B, H, W, C = x.shape
    if C % 8 or B == 0 or H < 2 or W < 2:
        raise RuntimeError(f"maxpool2x2_nhwc_f16: x {tuple(x.shape)}: need at least 2 x 2 pixels and a multiple of 8 channels")
    out = torch.empty(B, H // 2, W // 2, C, dtype=torch.float16, device=x.device)
    call("ldmae_maxpool2x2_nhwc_f16", ptr(x), ptr(out), B, H, W, C, stream())
    return out


def lpips_layer_f16(f, lin_w, out):
    """lpips_layer on fp16 taps f [2B, h, w, C]: the same f32 arithmetic on the (exactly converted) values; out f32 [B] accumulated in place."""
    return _lpips_layer("lpips_layer_f16", f, lin_w, out, torch.float16, 16)


def conv3x3_relu_dgrad_nhwc_bf16(dy, y, w_rot, out=None):
    """conv3x3_relu_dgrad_nhwc with 16-bit operands: dy f32 [B, H, W, Cy] (Cy % 8 == 0), y the stored fp16 activation of the same shape, w_rot bf16
    [Cx, 3, 3, Cy]; dx f32 [B, H, W, Cx] = conv3x3(bf16(dy * [y > 0]), w_rot), f32 accumulation on the bf16 MFMA."""
    return _conv3x3_relu_dgrad("conv3x3_relu_dgrad_nhwc_bf16", "ldmae_conv3x3_relu_dgrad_nhwc_bf16", dy, y, w_rot, out, torch.float16,
                               torch.bfloat16, 8, 16)


def maxpool2x2_bwd_nhwc_xf16(dy, x, out=None):
    """maxpool2x2_bwd_nhwc with the pooled input x stored as fp16; dy and dx f32."""
    return _maxpool2x2_bwd("maxpool2x2_bwd_nhwc_xf16", "ldmae_maxpool2x2_bwd_nhwc_xf16", dy, x, out, torch.float16, 16)


def lpips_layer_bwd_f16(f, lin_w, g, d_input=None, d_target=None, accumulate=False):
    """lpips_layer_bwd on fp16 taps f [2B, h, w, C]; g, d_input, d_target f32, the same arithmetic.  -> (d_input, d_target)."""
    return _lpips_layer_bwd("lpips_layer_bwd_f16", f, lin_w, g, d_input, d_target, accumulate, torch.float16, 16)


def lpips_prep_bwd_c8(g):
    """lpips_prep_bwd from the 8-channel data gradient of the fp16 path's conv1_1: g NHWC f32 [B, H, W, 8] -> NCHW f32 [B, 3, H, W] = g[..., c] /
    scale[c]; channels 3 .. 7 (exactly zero: their weight rows are) are ignored."""
    return _lpips_prep_bwd("lpips_prep_bwd_c8", g, 8)


def ssim(preds, target, lo=-1.0, hi=1.0, data_range=2.0):
    """Per-image SSIM f32 [B] of NCHW f32 [B, C, H, W] (H, W >= 11): torchmetrics' default Gaussian SSIM of the inputs clamped to [lo, hi]
    (+-inf: no clamp) with c1 = (0.01 data_range)^2, c2 = (0.03 data_range)^2."""
    _arg(preds, "ssim preds", torch.float32, "BCHW", copy=False)
    _arg(target, "ssim target", torch.float32, preds.shape, copy=False, like=preds)
    B, C, H, W = preds.shape
    if H < 11 or W < 11:
        raise RuntimeError(f"ssim: {H} x {W} images are smaller than the 11 x 11 Gaussian window")
    out = torch.empty(B, dtype=torch.float32, device=preds.device)
    ws = workspace(_ws_bytes("ldmae_ssim_workspace_bytes", B, C, H, W), preds.device, "ssim")
    call("ldmae_ssim", ptr(preds), ptr(target), ptr(out), B, C, H, W, float(lo), float(hi), float(data_range), ptr(ws), stream())
    return out


def recon_quantize_sse(decoded, ref):
    """What the reference writes as PNG, for both images, and their exact squared error: NCHW f32 [B, 3, H, W] x 2 ->
    (dec8, ref8) uint8 NHWC [B, H, W, 3] = (uint8) clamp(127.5 x + 128, 0, 255), sse int64 [B] = sum of (dec8 - ref8)^2."""
    _arg(decoded, "recon_quantize decoded", torch.float32, ("B", 3, "H", "W"), copy=False)
    _arg(ref, "recon_quantize ref", torch.float32, decoded.shape, copy=False, like=decoded)
    B, _, H, W = decoded.shape
    dec8 = torch.empty(B, H, W, 3, dtype=torch.uint8, device=decoded.device)
    ref8 = torch.empty_like(dec8)
    sse = torch.empty(B, dtype=torch.int64, device=decoded.device)
    ws = workspace(_ws_bytes("ldmae_sse_workspace_bytes", B, H * W), decoded.device, "sse")
    call("ldmae_recon_quantize_psnr", ptr(decoded), ptr(ref), ptr(dec8), ptr(ref8), ptr(sse), B, H, W, ptr(ws), stream())
    return dec8, ref8, sse


def sse_u8(a, b):
    """int64 [B]: exact sum of (a - b)^2 over each image of two uint8 tensors [B, ...] of one shape."""
    _arg(a, "sse_u8 a", torch.uint8, copy=False)
    if a.dim() < 2:
        raise RuntimeError(f"sse_u8: need [B, ...] tensors of at least two dimensions, got {tuple(a.shape)}")
    _arg(b, "sse_u8 b", torch.uint8, a.shape, copy=False, like=a)
    B, n = a.shape[0], a[0].numel()
    sse = torch.empty(B, dtype=torch.int64, device=a.device)
    ws = workspace(_ws_bytes("ldmae_sse_workspace_bytes", B, n), a.device, "sse")
    call("ldmae_sse_u8", ptr(a), ptr(b), ptr(sse), B, n, ptr(ws), stream())
    return sse


# ----------------------------------------------------------------------------- convolutional KL-VAE tokenizers (csrc/conv_vae.hip), NHWC f32
VAE_PLAIN, VAE_NORM_ACT, VAE_DOWN, VAE_UP = 0, 1, 2, 3
VAE_GROUPS, VAE_EPS = 32, 1e-6          # the reference's Normalize: GroupNorm(32, C, eps=1e-6)


def groupnorm_stats_nhwc(x, groups=VAE_GROUPS, eps=VAE_EPS):
    """(mean, rstd) f32 [B, groups] of x [B, H, W, C]: biased variance over the H * W * (C / groups) elements of every (image, group)."""
    _arg(x, "groupnorm_stats_nhwc x", torch.float32, "NHWC", copy=False)
    B, H, W, C = x.shape
    mean = torch.empty(B, groups, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    call("ldmae_groupnorm_stats_nhwc_f32", ptr(x), ptr(mean), ptr(rstd), B, H * W, C, groups, float(eps), stream())
    return mean, rstd


def groupnorm_apply_nhwc(x, stats, gamma, beta, silu=False, out=None, out_dtype=torch.float32):
    """gamma (x - mean) rstd + beta of x [B, H, W, C] from groupnorm_stats_nhwc's (mean, rstd); silu=True: y * sigmoid(y) of that.
    out_dtype=torch.float16: the same f32 value stored as fp16 (round to nearest even, saturating at +-65504): the operand of the two-pass
    TF32-class convolution."""
    _arg(x, "groupnorm_apply_nhwc x", torch.float32, "NHWC", copy=False)
    B, H, W, C = x.shape
    mean, rstd = stats
    _arg(mean, "groupnorm_apply_nhwc mean", torch.float32, (B, "groups"), copy=False, like=x)
    _arg(rstd, "groupnorm_apply_nhwc rstd", torch.float32, mean.shape, copy=False, like=x)
    _arg(gamma, "groupnorm_apply_nhwc gamma", torch.float32, (C,), copy=False, like=x)
    _arg(beta, "groupnorm_apply_nhwc beta", torch.float32, (C,), copy=False, like=x)
    if out_dtype not in (torch.float32, torch.float16):
        raise RuntimeError(f"groupnorm_apply_nhwc: out_dtype {out_dtype} (float32 or float16)")
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    _arg(out, "groupnorm_apply_nhwc out", out_dtype, x.shape, out=True, like=x)
    call("ldmae_groupnorm_apply_nhwc_f32" if out_dtype == torch.float32 else "ldmae_groupnorm_apply_nhwc_f16out", ptr(x), ptr(mean), ptr(rstd),
         ptr(gamma), ptr(beta), ptr(out), B, H * W, C, mean.shape[1], 1 if silu else 0, stream())
    return out


VAE_PRECISIONS = ("f32", "tf32")


def _precision(precision, what):
    if precision not in VAE_PRECISIONS:
        raise ValueError(f"{what}: precision {precision!r} (one of {VAE_PRECISIONS})")
    return precision == "tf32"


def conv3x3_vae_nhwc(x, w, bias=None, mode=VAE_PLAIN, res=None, stats=None, gamma=None, beta=None, silu=True, precision="f32"):
    """3x3 convolution of x [B, H, W, Cin] with w [Cout, 3, 3, Cin] -> [B, Ho, Wo, Cout], + bias + res (the output's shape).
    mode VAE_PLAIN: stride 1, pad 1.  VAE_NORM_ACT: the operand is groupnorm_apply_nhwc(x, stats, gamma, beta, silu), computed while it is
    gathered; out-of-image taps are 0.  VAE_DOWN: stride 2, zero pad right and bottom only.  VAE_UP: nearest 2x upsampling, then stride 1, pad 1.
    precision "tf32": w is the fp16 pack (ops.cast of the f32 one), Cin % 8 == 0; both operands of every product are rounded once to fp16
    (saturating), accumulation, bias, residual and output are f32.  x may then be fp16 in VAE_PLAIN (groupnorm_apply_nhwc(out_dtype=float16))."""
    tf32 = _precision(precision, "conv3x3_vae_nhwc")
    _arg(x, "conv3x3_vae_nhwc x", (torch.float32, torch.float16) if tf32 else torch.float32, "NHWC", copy=False)
    B, H, W, Cin = x.shape
    _arg(w, "conv3x3_vae_nhwc weight", torch.float16 if tf32 else torch.float32, ("Cout", 3, 3, Cin), copy=False, like=x)
    Cout = w.shape[0]
    if mode == VAE_DOWN:
        Ho, Wo = (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1
        if Ho < 1 or Wo < 1:
            raise RuntimeError(f"conv3x3_vae_nhwc: down needs at least 2 x 2 pixels, got {H} x {W}")
    elif mode == VAE_UP:
        Ho, Wo = 2 * H, 2 * W
    elif mode in (VAE_PLAIN, VAE_NORM_ACT):
        Ho, Wo = H, W
    else:
        raise RuntimeError(f"conv3x3_vae_nhwc: mode {mode}")
    mean = rstd = None
    groups = 0
    if mode == VAE_NORM_ACT:
        if stats is None or gamma is None or beta is None:
            raise RuntimeError("conv3x3_vae_nhwc: norm-act needs stats, gamma and beta")
        mean, rstd = stats
        _arg(mean, "conv3x3_vae_nhwc mean", torch.float32, (B, "groups"), copy=False, like=x)
        _arg(rstd, "conv3x3_vae_nhwc rstd", torch.float32, mean.shape, copy=False, like=x)
        groups = mean.shape[1]
        _arg(gamma, "conv3x3_vae_nhwc gamma", torch.float32, (Cin,), copy=False, like=x)
        _arg(beta, "conv3x3_vae_nhwc beta", torch.float32, (Cin,), copy=False, like=x)
    _arg(bias, "conv3x3_vae_nhwc bias", torch.float32, (Cout,), copy=False, like=x)
    _arg(res, "conv3x3_vae_nhwc res", torch.float32, (B, Ho, Wo, Cout), copy=False, like=x)
    out = torch.empty(B, Ho, Wo, Cout, dtype=torch.float32, device=x.device)
    tail = (ptr(x), ptr(w), ptr(bias), ptr(res), ptr(mean), ptr(rstd), ptr(gamma if mode == VAE_NORM_ACT else None),
            ptr(beta if mode == VAE_NORM_ACT else None), groups, 1 if silu else 0, ptr(out), B, H, W, Cin, Cout, stream())
    if tf32:
        call("ldmae_conv3x3_vae_nhwc_f16", mode, dt(x.dtype), *tail)
    else:
        call("ldmae_conv3x3_vae_nhwc_f32", mode, *tail)
    return out


def conv1x1_res_nhwc(x, w, bias=None, res=None, precision="f32"):
    """x [..., Cin] (contiguous f32) times w [Cout, Cin]^T + bias + res [..., Cout]: the 1x1 convolution with a residual epilogue.
    precision "tf32": w is the fp16 pack, Cin % 8 == 0; the arithmetic contract of conv3x3_vae_nhwc."""
    tf32 = _precision(precision, "conv1x1_res_nhwc")
    _arg(x, "conv1x1_res_nhwc x", torch.float32, copy=False)
    _arg(w, "conv1x1_res_nhwc weight", torch.float16 if tf32 else torch.float32, ("Cout", x.shape[-1]), copy=False, like=x)
    Cout, Cin = w.shape
    _arg(bias, "conv1x1_res_nhwc bias", torch.float32, (Cout,), copy=False, like=x)
    _arg(res, "conv1x1_res_nhwc res", torch.float32, (*x.shape[:-1], Cout), copy=False, like=x)
    out = torch.empty(*x.shape[:-1], Cout, dtype=torch.float32, device=x.device)
    call("ldmae_conv1x1_res_nhwc_f16" if tf32 else "ldmae_conv1x1_res_nhwc_f32", ptr(x), ptr(w), ptr(bias), ptr(res), ptr(out), x.numel() // Cin, Cin,
         Cout, stream())
    return out


def softmax_rows_(s, cols, scale=1.0):
    """In place on s [rows, ld] f32 (contiguous): s[:, :cols] = softmax(scale * s[:, :cols], dim=1); s[:, cols:] = 0."""
    _arg(s, "softmax_rows_ s", torch.float32, ("rows", "ld"), out=True)
    if not 0 < cols <= s.shape[1]:
        raise RuntimeError(f"softmax_rows_: cols {cols} of rows of {s.shape[1]} (ld >= cols > 0)")
    call("ldmae_softmax_rows_f32", ptr(s), s.shape[1], s.shape[0], cols, float(scale), stream())
    return s


ATTN_WIDE_KPAD = 16                     # ldmae_gemm_nt in f32 takes K in multiples of 16: the key axis of P and of V^T is padded with zeros


def attention_wide(q, k, vt, scale, bias=None):
    """Single-head attention of any width on the f32 GEMM: out [B, N, C] = softmax(scale q k^T) v (+ bias [C]).  q, k: [B, N, C] f32 views whose
    rows are dense (the halves of one [B, N, 2C] buffer are fine); vt: [B, C, Np] f32 = v transposed, Np = N rounded up to ATTN_WIDE_KPAD with
    zeros in the padding.  Per image: S = q k^T (ldmae_gemm_nt), row softmax in place (ldmae_softmax_rows_f32), out = P (v^T)^T + bias."""
    B, N, C = q.shape
    Np = -(-N // ATTN_WIDE_KPAD) * ATTN_WIDE_KPAD
    if tuple(k.shape) != (B, N, C) or tuple(vt.shape) != (B, C, Np):
        raise RuntimeError(f"attention_wide: q {tuple(q.shape)}, k {tuple(k.shape)}, vt {tuple(vt.shape)} must be [B, N, C] x 2 and [B, C, {Np}]")
    out = torch.empty(B, N, C, dtype=torch.float32, device=q.device)
    s = torch.empty(N, Np, dtype=torch.float32, device=q.device)
    for b in range(B):
        gemm_nt(q[b], k[b], out=s[:, :N])
        softmax_rows_(s, N, scale)
        gemm_nt(s, vt[b], bias=bias, out=out[b])
    return out


# ----------------------------------------------------------------------------- adaptive dopri5 ODE sampler (csrc/ode.hip), f32
# State vectors are addressed flat: _arg(numel=n).  Device scalars (h, t, the error ratio) and scratch are f32 memory of at_least= so many
# elements.  Everything shares the device of the state.

def _ode_slab(k, n, y):
    _arg(k, "ode: the stage slab", torch.float32, (7, "ld"), copy=False, like=y)
    if k.shape[1] < n or k.shape[1] % 4:
        raise RuntimeError(f"ode: the stage slab must be a contiguous f32 [7, ld] tensor with ld % 4 == 0 and ld >= {n}, got {tuple(k.shape)}")
    return k


def ode_slab_ld(n):
    """Row length of the [7, ld] stage slab for a state of n elements: n rounded up to a multiple of 4 (every row 16-byte aligned)."""
    return (n + 3) // 4 * 4


def ode_partials(n):
    """Number of per-block partial sums ldmae_dopri5_finish_f32 / ldmae_rms_norm_scaled_f32 write for n elements (a function of n alone)."""
    return int(L.load().ldmae_ode_partials(n))


def rk_stage(y, k_slab, coef, h_dev, out, t_dev=None, ct=0.0, t_out=None):
    """out = y + h * sum_j coef[j] * k_slab[j] (one pass, fixed left-to-right order); h read from the device scalar h_dev.  With t_out (f32 [B]):
    every element of t_out = t + ct * h as well, the time vector of the next model evaluation.  Returns out."""
    n = y.numel()
    m = len(coef)
    _arg(y, "rk_stage y", torch.float32, copy=False)
    _arg(out, "rk_stage out", torch.float32, numel=n, out=True, like=y)
    _ode_slab(k_slab, n, y)
    _arg(h_dev, "rk_stage h_dev", torch.float32, copy=False, like=y, at_least=1)
    if t_out is not None:
        _arg(t_dev, "rk_stage t_dev", torch.float32, copy=False, like=y, at_least=1)
        _arg(t_out, "rk_stage t_out", torch.float32, out=True, like=y)
    cf = (ctypes.c_float * 7)(*[float(c) for c in coef])
    call("ldmae_rk_stage_f32", ptr(y), ptr(k_slab), k_slab.shape[1], cf, m, ptr(h_dev), ptr(out), n, ptr(t_dev), float(ct), ptr(t_out),
         0 if t_out is None else t_out.numel(), stream())
    return out


def dopri5_finish(y, k_slab, h_dev, atol, rtol, y1, partial, ratio_dev):
    """y1 = y + h * sum b_j k_j and ratio_dev = rms over ALL elements of (h * sum e_j k_j) / (atol + rtol * max(|y|, |y1|)), in one pass plus a
    one-block fold; fixed summation order (bitwise reproducible), no atomics.  partial: >= ode_partials(n) f32."""
    n = y.numel()
    _arg(y, "dopri5_finish y", torch.float32, copy=False)
    _arg(y1, "dopri5_finish y1", torch.float32, numel=n, out=True, like=y)
    _ode_slab(k_slab, n, y)
    _arg(h_dev, "dopri5_finish h_dev", torch.float32, copy=False, like=y, at_least=1)
    _arg(partial, "dopri5_finish partial", torch.float32, out=True, like=y, at_least=ode_partials(n))
    _arg(ratio_dev, "dopri5_finish ratio_dev", torch.float32, out=True, like=y, at_least=1)
    call("ldmae_dopri5_finish_f32", ptr(y), ptr(k_slab), k_slab.shape[1], ptr(h_dev), float(atol), float(rtol), ptr(y1), ptr(partial), ptr(ratio_dev),
         n, stream())
    return y1


def rms_norm_scaled(x, y, atol, rtol, partial, out_dev):
    """out_dev = sqrt(mean((x / (atol + rtol * |y|))^2)) (y None: y = x), the norm of the starting-step rule; same two-stage fold as dopri5_finish."""
    n = x.numel()
    _arg(x, "rms_norm_scaled x", torch.float32, copy=False)
    _arg(y, "rms_norm_scaled y", torch.float32, numel=n, copy=False, like=x)
    _arg(partial, "rms_norm_scaled partial", torch.float32, out=True, like=x, at_least=ode_partials(n))
    _arg(out_dev, "rms_norm_scaled out_dev", torch.float32, out=True, like=x, at_least=1)
    call("ldmae_rms_norm_scaled_f32", ptr(x), ptr(y), float(atol), float(rtol), ptr(partial), ptr(out_dev), n, stream())
    return out_dev


def dopri5_interp(y0, y1, y_mid, k_slab, h_dev, t0_dev, t_eval, out):
    """out = the quartic through y0, y1, y_mid with end slopes k_slab[0], k_slab[6], at x = (t_eval - t0) / h; coefficients never stored."""
    n = y0.numel()
    for t, w in ((y0, "y0"), (y1, "y1"), (y_mid, "y_mid"), (out, "out")):
        _arg(t, "dopri5_interp " + w, torch.float32, numel=n, copy=False, like=y0)
    _ode_slab(k_slab, n, y0)
    _arg(h_dev, "dopri5_interp h_dev", torch.float32, copy=False, like=y0, at_least=1)
    _arg(t0_dev, "dopri5_interp t0_dev", torch.float32, copy=False, like=y0, at_least=1)
    call("ldmae_dopri5_interp_f32", ptr(y0), ptr(y1), ptr(y_mid), ptr(k_slab), k_slab.shape[1], ptr(h_dev), ptr(t0_dev), float(t_eval), ptr(out), n, stream())
    return out


def dopri5_advance(ratio_dev, h_dev, t_dev, status_dev):
    """The step-size controller on the device (one thread): status_dev[0..5] = (accepted, ratio, t, h, t', h'); t_dev, h_dev updated in place."""
    for t, w, n in ((ratio_dev, "ratio_dev", 1), (h_dev, "h_dev", 1), (t_dev, "t_dev", 1), (status_dev, "status_dev", 6)):
        _arg(t, "dopri5_advance " + w, torch.float32, copy=False, like=ratio_dev, at_least=n)
    call("ldmae_dopri5_advance", ptr(ratio_dev), ptr(h_dev), ptr(t_dev), ptr(status_dev), stream())


def dopri5_initial_step(d_dev, phase, h_dev):
    """The Hairer-Norsett-Wanner starting step from the norms d_dev = (d0, d1, d2 * h0, h0): phase 0 writes h0, phase 1 the step, to h_dev."""
    _arg(d_dev, "dopri5_initial_step d_dev", torch.float32, out=True, at_least=4)
    _arg(h_dev, "dopri5_initial_step h_dev", torch.float32, out=True, like=d_dev, at_least=1)
    call("ldmae_dopri5_initial_step", ptr(d_dev), int(phase), ptr(h_dev), stream())


# ----------------------------------------------------------------------------- likelihood evaluation (csrc/ode.hip), f32
def rademacher(shape, seed, counter, device):
    """+-1.0 of the given shape from Philox4x32-10 keyed by `seed`, counter words (counter, element index / 4); one sign per 32-bit word (its top
    bit).  A function of (seed, counter, element index) alone; transport/probe.py restates it in numpy bit for bit."""
    out = torch.empty(shape, dtype=torch.float32, device=device)
    if out.numel() == 0:
        raise RuntimeError("rademacher: empty shape")
    call("ldmae_rademacher_f32", ptr(out), out.numel(), int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1), stream())
    return out


def rowdot(a, b=None, out=None):
    """out[r] = sum over everything but dim 0 of a[r] * b[r] (b None: b = a, the row sums of squares); f32, contiguous, two-stage fixed-order sum."""
    b = a if b is None else b
    _arg(a, "rowdot a", torch.float32, copy=False)
    _arg(b, "rowdot b", torch.float32, a.shape, copy=False, like=a)
    B, m, out, partial = _row_reduce_out("rowdot", L.load().ldmae_rowdot_partials, a, out)
    call("ldmae_rowdot_f32", ptr(a), ptr(b), ptr(out), B, m, ptr(partial), stream())
    return out


def likelihood_finish(sumsq, delta, m):
    """logp[b] = (-m / 2 log(2 pi) - sumsq[b] / 2) - delta[b]: transport.prior_logp of a state with row sums of squares `sumsq` minus the
    integrated divergence."""
    import math
    B = sumsq.numel()
    _arg(sumsq, "likelihood_finish sumsq", torch.float32, copy=False)
    _arg(delta, "likelihood_finish delta", torch.float32, numel=B, copy=False, like=sumsq)
    out = torch.empty(B, dtype=torch.float32, device=sumsq.device)
    call("ldmae_likelihood_finish_f32", ptr(sumsq), ptr(delta), -m / 2.0 * math.log(2 * math.pi), ptr(out), B, stream())
    return out


# ----------------------------------------------------------------------------- SDE sampler (csrc/ode.hip), f32
def normal(shape, seed, counter, device, out=None):
    """Standard normals of the given shape from Philox4x32-10 keyed by `seed`, counter words (counter, element index / 4), Box-Muller on the four
    words of a block (include/ldmae_hip.h).  A function of (seed, counter, element index) alone; transport/probe.normal restates it in f64."""
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=device)
    if out.numel() == 0:
        raise RuntimeError("normal: empty shape")
    _arg(out, "normal out", torch.float32, out=True)
    call("ldmae_normal_f32", ptr(out), out.numel(), int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1), stream())
    return out


def sde_combine(ins, coef, out, noise_coef=0.0, z=None, seed=None, counter=0, mean_out=None, t_next=0.0, t_out=None):
    """out = sum_j coef[j] * ins[j] + noise_coef * z in one pass (1 to 4 inputs, fixed left-to-right fma order, the noise term last).  z: a tensor,
    or None with `seed` given: the draw normal(seed, counter), generated inside the kernel and never stored; neither: no noise term.
    mean_out: the sum without the noise term.  t_out (f32 [B]): every element = t_next as well, the time vector of the next model evaluation.
    out / mean_out may be one of the inputs (in place).  Returns out."""
    n, m = out.numel(), len(ins)
    if not 1 <= m <= 4 or len(coef) != m:
        raise RuntimeError(f"sde_combine: 1 to 4 inputs with one coefficient each, got {m} inputs and {len(coef)} coefficients")
    _arg(out, "sde_combine out", torch.float32, out=True)
    for j, t in enumerate(ins):
        _arg(t, f"sde_combine input {j}", torch.float32, numel=n, copy=False, like=out)
    _arg(z, "sde_combine z", torch.float32, numel=n, copy=False, like=out)
    _arg(mean_out, "sde_combine mean_out", torch.float32, numel=n, out=True, like=out)
    _arg(t_out, "sde_combine t_out", torch.float32, out=True, like=out)
    mode = 1 if z is not None else (2 if seed is not None else 0)
    p = [ptr(t) for t in ins] + [None] * (4 - m)
    cf = (ctypes.c_float * 4)(*([float(c) for c in coef] + [0.0] * (4 - m)))
    call("ldmae_sde_combine_f32", p[0], p[1], p[2], p[3], cf, m, ptr(z), float(noise_coef), mode, int(seed or 0) & (2 ** 64 - 1),
         int(counter) & (2 ** 64 - 1), ptr(out), ptr(mean_out), n, float(t_next), ptr(t_out), 0 if t_out is None else t_out.numel(), stream())
    return out


# ----------------------------------------------------------------------------- Dispersive Loss (csrc/dispersive.hip)
# ops.dispersive_fwd / ops.dispersive_bwd: written in dispersive.py on this module's argument checker (_arg), workspace and stream
from .dispersive import dispersive_bwd, dispersive_fwd      # noqa: E402,F401
