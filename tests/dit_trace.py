"""Launch traces of the LightningDiT: which C entry points a forward / backward calls, in which order, with which scalars, and which of
their pointer arguments are null.  Not a test module: tests/test_gpu_dit_trace.py replays CASES against tests/golden/dit_call_trace.json,
tests/golden/make_golden_dit_trace.py writes that file.

`recording()` replaces ops.call (ops binds `call` by name at import, so patching _lib.call would not take effect) with a wrapper that notes
[entry point, argument, ...] and calls through.  A scalar is noted as given (floats through repr); a parameter that include/ldmae_hip.h
declares as a pointer only as "null" / "ptr": which optional outputs were requested -- and, the default stream being null, which stream a
weight-gradient GEMM went to.  Everything below uses names that are as old as the input-gradient-only backward, so this file runs
unmodified on either side of a change to models/lightningdit.py."""
import contextlib
import ctypes
import os

import torch

from ldmae_amd import _lib, ops

# the A/B switches that change launches: with one of them set the golden file does not apply
SWITCHES = ("LDMAE_FUSED_QKV", "LDMAE_FUSED_RESNORM", "LDMAE_FUSED_QKN_BWD", "LDMAE_TN_STREAM", "LDMAE_BATCHED_ADALN")


def switch_set():
    return next((s for s in SWITCHES if s in os.environ), None)


# the one scalar that is no property of the launch: `workspace_bytes`, the last argument but one of these entry points, is the capacity of
# ops.workspace's grow-only scratch buffer, i.e. the largest request this PROCESS has made so far (other tests included)
_CAPACITY = ("ldmae_gemm_tn", "ldmae_thin_tn")


def _note(name, args):
    types = _lib.SIGNATURES[name][1]
    assert len(args) == len(types), name
    out = [name]
    for i, (a, ty) in enumerate(zip(args, types)):
        if name in _CAPACITY and i == len(args) - 2:
            out.append("capacity")
        elif ty is ctypes.c_void_p:
            out.append("null" if a is None or (isinstance(a, int) and a == 0) else "ptr")
        elif isinstance(a, float):
            out.append(repr(a))
        else:
            out.append(int(a))
    return out


@contextlib.contextmanager
def recording():
    log, real = [], ops.call

    def call(name, *args):
        log.append(_note(name, args))
        return real(name, *args)

    # the GEMM launch mode and the half-line switch are process-wide and travel in the `epi` argument: pinned to their defaults while
    # recording, so that a test which left one of them set cannot change a trace by running first
    mode, half = ops._GEMM_MODE, ops._HALF_LINES
    ops.set_gemm_launch_mode("persistent")
    ops.set_gemm_half_lines(False)
    ops.call = call
    try:
        yield log
    finally:
        ops.call = real
        ops._GEMM_MODE, ops._HALF_LINES = mode, half


# ----------------------------------------------------------------------------- the cases
# base: width 128, 2 heads of 64, 64 tokens of 16 channels, SwiGLU width 341 (the zero-padded path)
BASE = dict(input_size=8, patch_size=1, in_channels=16, hidden_size=128, depth=2, num_heads=2, num_classes=10, use_qknorm=True,
            use_swiglu=True, use_rope=True, use_rmsnorm=True)
LN_QK = dict(use_rmsnorm=False)                                      # nn.LayerNorm QK-norm, LayerNorm modulate
TIMM = dict(use_swiglu=False, wo_shift=True, use_rope=False, use_qknorm=False)


def _case(cid, kind, prec, B, cfg=None, has=(), lacks=(), **opt):
    return dict(id=cid, kind=kind, prec=prec, B=B, cfg=cfg or {}, has=tuple(has), lacks=tuple(lacks), **opt)


# has / lacks: entry points the case's trace must / must not contain -- the branch it is named for (checked before a golden file is written)
CASES = [
    _case("train-f32-b2", "train", "f32", 2, has=("ldmae_attention_fwd", "ldmae_attention_bwd", "ldmae_qknorm_rope_bwd"),
          lacks=("ldmae_cast_stack", "ldmae_attention_fwd_pv_bounded")),
    _case("train-bf16-b2", "train", "bf16", 2, has=("ldmae_attention_fwd_pv_bounded", "ldmae_attention_bwd_pv_qknorm"),
          lacks=("ldmae_cast_stack", "ldmae_qknorm_rope_bwd", "ldmae_gemm_nt_qkv_rope")),
    _case("train-bf16-b8", "train", "bf16", 8, has=("ldmae_cast_stack", "ldmae_res_rmsnorm_modulate_fwd", "ldmae_rmsnorm_modulate_bwd_gate_recompute"),
          lacks=("ldmae_gate_bwd",)),
    _case("train-bf16-b8-direct", "train", "bf16", 8, dict(mlp_ratio=3.0), has=("ldmae_multi_add",), direct=True),
    # 256 tokens; the fused qkv epilogue also wants 3 * H * 64 % 256 == 0 (ldmae_gemm_nt_qkv_rope_ok), so 4 heads of 64: width 256
    _case("train-bf16-b2-n256", "train", "bf16", 2, dict(input_size=16, hidden_size=256, num_heads=4), has=("ldmae_gemm_nt_qkv_rope",), lacks=("ldmae_qknorm_rope_fwd",)),
    _case("train-bf16-b2-hd32", "train", "bf16", 2, dict(num_heads=4), has=("ldmae_attention_bwd_pv", "ldmae_qknorm_rope_bwd"),
          lacks=("ldmae_attention_bwd_pv_qknorm",)),
    _case("train-bf16-b8-hook", "train", "bf16", 8, has=("ldmae_gate_bwd",), lacks=("ldmae_cast_stack", "ldmae_res_rmsnorm_modulate_fwd"), hook=True),
    _case("train-bf16-b2-checkpoint", "train", "bf16", 2, dict(use_checkpoint=True), has=("ldmae_gate_bwd",)),
    _case("train-f32-b2-lnqk", "train", "f32", 2, LN_QK, has=("ldmae_layernorm_fwd", "ldmae_layernorm_bwd_cast", "ldmae_layernorm_modulate_bwd_gate")),
    _case("train-bf16-b2-lnqk", "train", "bf16", 2, LN_QK, has=("ldmae_layernorm_fwd", "ldmae_layernorm_bwd_cast", "ldmae_layernorm_modulate_bwd_gate"),
          lacks=("ldmae_attention_fwd_pv_bounded",)),
    _case("train-bf16-b2-timm", "train", "bf16", 2, TIMM, has=("ldmae_gelu_tanh_fwd", "ldmae_gelu_tanh_bwd", "ldmae_attention_fwd_pv"),
          lacks=("ldmae_attention_fwd_pv_bounded",)),
    _case("io-f32-b2", "io", "f32", 2, has=("ldmae_attention_bwd", "ldmae_qknorm_rope_bwd"), lacks=("ldmae_gemm_tn", "ldmae_colsum")),
    _case("io-bf16-b2", "io", "bf16", 2, has=("ldmae_attention_bwd_pv_qknorm",), lacks=("ldmae_gemm_tn",)),
    _case("io-bf16-b8", "io", "bf16", 8, has=("ldmae_attention_bwd_pv_qknorm",), lacks=("ldmae_gemm_tn", "ldmae_res_rmsnorm_modulate_fwd")),
    _case("io-bf16-b2-lnqk", "io", "bf16", 2, LN_QK, has=("ldmae_layernorm_bwd_cast",), lacks=("ldmae_gemm_tn",)),
    _case("cfg-f32-b4", "cfg", "f32", 4, has=("ldmae_attention_fwd",), lacks=("ldmae_gemm_tn",)),
    _case("cfg-bf16-b4", "cfg", "bf16", 4, has=("ldmae_attention_fwd_pv_bounded",), lacks=("ldmae_cast_stack",)),
    _case("cfg-bf16-b16", "cfg", "bf16", 16, has=("ldmae_cast_stack",)),
    _case("mx8-n64", "cfg", "bf16", 4, dict(mlp_ratio=3.0), has=("ldmae_gemm_nt_mx8", "ldmae_qknorm_rope_fwd"), lacks=("ldmae_gemm_nt_qkv_rope_mx8",), mx8=True),
    _case("mx8-n256", "cfg", "bf16", 4, dict(mlp_ratio=3.0, input_size=16), has=("ldmae_gemm_nt_qkv_rope_mx8",), lacks=("ldmae_qknorm_rope_fwd",), mx8=True),
    _case("attn-f32", "attn", "f32", 2, has=("ldmae_attention_fwd", "ldmae_attention_bwd", "ldmae_qknorm_rope_bwd")),
    _case("attn-bf16", "attn", "bf16", 2, has=("ldmae_attention_bwd_pv", "ldmae_qknorm_rope_bwd"), lacks=("ldmae_attention_bwd_pv_qknorm",)),
    _case("attn-bf16-lnqk", "attn", "bf16", 2, LN_QK, has=("ldmae_layernorm_fwd", "ldmae_layernorm_bwd_cast")),
    _case("block-bf16-b2", "block", "bf16", 2, has=("ldmae_gate_bwd", "ldmae_attention_bwd_pv_qknorm"), lacks=("ldmae_cast_stack",)),
]
IDS = [c["id"] for c in CASES]


def _model(cfg):
    """A fresh model on a fixed seed; adaLN and final-layer weights re-drawn (their zero initialisation would hide everything), as _dit() in
    tests/test_gpu_likelihood.py does."""
    from ldmae_amd.models.lightningdit import LightningDiT
    torch.manual_seed(0)
    m = LightningDiT(**dict(BASE, **cfg))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "adaLN_modulation" in n or n.startswith("final_layer.linear"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return m.cuda()


def _grads(m, out):
    out.update({"grad." + n: p.grad for n, p in m.named_parameters() if p.grad is not None})


def run_case(case):
    """-> (the recorded calls, {name: tensor}: the output, dx and every parameter gradient)."""
    m = _model(case["cfg"])
    S, D = m.x_embedder.img_size[0], m.hidden_size
    B, kind = case["B"], case["kind"]
    g = torch.Generator().manual_seed(2)
    x, t = torch.randn(B, 16, S, S, generator=g).cuda(), torch.rand(B, generator=g).cuda()
    y, gout = torch.randint(0, 10, (B,), generator=g).cuda(), torch.randn(B, 16, S, S, generator=g).cuda()
    tok, c = torch.randn(B, S * S, D, generator=g).cuda(), torch.randn(B, D, generator=g).cuda()
    gtok = torch.randn(B, S * S, D, generator=g).cuda()
    ac = lambda: torch.autocast("cuda", dtype=torch.bfloat16, enabled=case["prec"] == "bf16")      # noqa: E731
    got = {}
    if case.get("direct"):
        m.direct_param_grads = True
        for p in m.parameters():
            if p.requires_grad:
                p.grad = torch.zeros_like(p, dtype=torch.float32).contiguous()
    if case.get("hook"):
        m.blocks[1].register_forward_hook(lambda mod, args, out: None)
    if case.get("mx8"):
        m.set_gemm_precision("mxfp8")
    ops.invalidate_weight_cache()
    with recording() as log:
        if kind == "cfg":                                            # forward-only: cold, then with the weight-copy cache warm
            m.eval()
            ycfg = torch.cat([y[:B // 2], torch.full_like(y[:B // 2], 10)])
            with torch.no_grad(), ac():
                got["out"] = m.forward_with_cfg(x, t, ycfg, 2.0, True, 0.1)
                got["out_warm"] = m.forward_with_cfg(x, t, ycfg, 2.0, True, 0.1)
        elif kind == "attn":                                         # the stand-alone Attention module
            tok.requires_grad_(True)
            with ac():
                got["out"] = m.blocks[0].attn(tok, m.feat_rope)
            got["out"].backward(gtok.to(got["out"].dtype))
            got["dx"] = tok.grad
            _grads(m, got)
        elif kind == "block":                                        # one block called on its own
            tok.requires_grad_(True)
            c.requires_grad_(True)
            with ac():
                got["out"] = m.blocks[0](tok, c, m.feat_rope)
            got["out"].backward(gtok)
            got["dx"], got["dc"] = tok.grad, c.grad
            _grads(m, got)
        else:
            m.train() if kind == "train" else m.eval()
            x.requires_grad_(True)
            with (m.input_grad_only() if kind == "io" else contextlib.nullcontext()), ac():
                got["out"] = m(x, t, y)
            got["out"].backward(gout)
            got["dx"] = x.grad
            _grads(m, got)
    torch.cuda.synchronize()
    return log, got


def check_branch(case, log):
    """The case reached the branch it is named for."""
    names = {e[0] for e in log}
    missing, extra = [n for n in case["has"] if n not in names], [n for n in case["lacks"] if n in names]
    assert not missing and not extra, f"{case['id']}: the trace lacks {missing} and holds {extra}"
    if case.get("direct"):                                           # the weight-gradient GEMMs add into .grad: beta = 1
        beta = _lib.SIGNATURES["ldmae_gemm_tn"][1].index(ctypes.c_float)      # its only float parameter
        assert any(e[0] == "ldmae_gemm_tn" and e[1 + beta] == repr(1.0) for e in log), case["id"]

