"""Characterisation of the argument checks of every public wrapper in ldmae_amd/ops.py.

Every row builds a well-formed set of CPU tensors at the smallest legal shape.  Then each tensor argument gets each single defect in turn --
another dtype, one extra leading dimension, a non-contiguous view of the same shape, a last dimension that disagrees with the others -- and the
wrapper either REFUSES with its own message (the text starts with the op's name) or GOES ON towards the device (anything else: on CPU tensors
that is `_lib.ptr`'s "no CPU fallback", or an error of the workspace allocation just before it).  tests/golden/ops_args_outcomes.json holds the
expected outcome of every (op, argument, defect); a refusal must never turn into "on".  In the rows of the training path (gemm_nt .. knn_vote)
every "on" is moreover named in ALLOWED_ON with the reason why that call may reach the device.

No GPU is needed, but the built library is (what build() leaves in the tree, like tests/test_dtype_refusals_cpu.py): several wrappers ask it for
a workspace or blob size between two checks, and the fixture records what they do with it present."""
import inspect
import json
import os
import re

import pytest
import torch

F16, BF16, F32, F64, U8, I32, I64 = torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.uint8, torch.int32, torch.int64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_args_outcomes.json")
DEFECTS = ("dtype", "dim", "strided", "shape")


def Z(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


def _lpips_bwd(name, dt):
    return (lambda: dict(f=Z(2, 2, 2, 64, dtype=dt), lin_w=Z(64), g=Z(1), d_input=Z(1, 2, 2, 64), d_target=Z(1, 2, 2, 64)),
            lambda o, a: getattr(o, name)(a["f"], a["lin_w"], a["g"], a["d_input"], a["d_target"]))


def _blob():
    """A weight blob of the size the fused VMAE encoder expects for one block (the size is the library's to say)."""
    from ldmae_amd import _lib
    return Z(_lib.load().ldmae_vmae_encoder_blob_bytes(1), dtype=U8)


def _norm_bwd(w=True, gate=False, dt=F32, **kw):
    """rmsnorm_modulate_bwd / _bwd_gate: M = 2 rows, one per sample (B = 2: the two views of a modulation pair must agree on their row stride)."""
    def make():
        a = dict(dout=Z(2, 4, dtype=dt), x=Z(2, 4), w=Z(4), scale=Z(2, 4), rstd=Z(2), dx_accum=Z(2, 4), dshift=Z(2, 4), dscale=Z(2, 4))
        if gate:
            a.update(y=Z(2, 4, dtype=dt), gate=Z(2, 4), dgate=Z(2, 4))
        if not w:
            del a["w"]
        return a

    def call(o, a):
        head = (a["dout"], a["x"], a.get("w"), a["scale"], a["rstd"], a["dx_accum"], a["dshift"], a["dscale"])
        if gate:
            return o.rmsnorm_modulate_bwd_gate(*head, a["y"], a["gate"], a["dgate"], 1, dt, **kw)
        return o.rmsnorm_modulate_bwd(*head, 1)
    return make, call


def _attn_bwd_pv(name, tables):
    def make():
        a = dict(q=Z(1, 1, 2, 16, dtype=BF16), k=Z(1, 1, 2, 16, dtype=BF16), qkv=Z(2, 48, dtype=BF16), o=Z(1, 2, 16, dtype=BF16),
                 do=Z(1, 2, 16, dtype=BF16), lse=Z(1, 1, 2))
        if tables:
            a.update(wq=Z(16), wk=Z(16), cos=Z(2, 16), sin=Z(2, 16))
        return a
    return make, lambda o, a: getattr(o, name)(a["q"], a["k"], a["qkv"], a["o"], a["do"], a["lse"], 0.25, *([a[n] for n in ("wq", "wk", "cos", "sin")] if tables else []))


_MX8 = dict(aq=(2, 128), asc=(2, 4), wq=(3, 128), wsc=(3, 4))


def _mx8(n=3, **more):
    """The four operands of a block-scaled NT product (uint8 elements and scales), N = n output columns, and what else the row passes."""
    return lambda: dict({k: Z(*((n if s[0] == 3 else s[0]), s[1]), dtype=U8) for k, s in _MX8.items()}, **{k: f() for k, f in more.items()})


# op -> (tensors of a well-formed call, the call).  Shapes: the smallest each wrapper accepts.  Where one wrapper has forms with different
# contracts there is a row per form, "op[form]".  HOST tables (label vectors, crop and KID index tables) are no tensor arguments of the
# kernels: the rows pass them as they are and do not damage them.
ROWS = {
    # ---- the training path: gemm_nt .. knn_vote
    "gemm_nt": (lambda: dict(a=Z(2, 4), b=Z(3, 4), bias=Z(3), out=Z(2, 3)), lambda o, a: o.gemm_nt(a["a"], a["b"], a["bias"], out=a["out"])),
    "gemm_nt_gate_res": (lambda: dict(a=Z(2, 4), b=Z(3, 4), bias=Z(3), xin=Z(2, 3), gate=Z(2, 3), xout=Z(2, 3)),
                         lambda o, a: o.gemm_nt_gate_res(a["a"], a["b"], a["bias"], a["xin"], a["gate"], 1, xout=a["xout"])),
    "gemm_nt_pos": (lambda: dict(a=Z(2, 4), b=Z(3, 4), bias=Z(3), pos=Z(2, 3)), lambda o, a: o.gemm_nt_pos(a["a"], a["b"], a["bias"], a["pos"], 2)),
    "gemm_nt_gelu": (lambda: dict(a=Z(2, 4), b=Z(3, 4), bias=Z(3)), lambda o, a: o.gemm_nt_gelu(a["a"], a["b"], a["bias"])),
    "gemm_nt_gelu_bwd": (lambda: dict(dy=Z(2, 4), w2t=Z(3, 4), pre=Z(2, 3)), lambda o, a: o.gemm_nt_gelu_bwd(a["dy"], a["w2t"], a["pre"])),
    "gemm_nt_swiglu": (lambda: dict(a=Z(2, 4), w12=Z(4, 4), b12=Z(4)), lambda o, a: o.gemm_nt_swiglu(a["a"], a["w12"], a["b12"])),
    "gemm_nt_swiglu[bf16]": (lambda: dict(a=Z(2, 64, dtype=BF16), w12=Z(256, 64, dtype=BF16), b12=Z(256)),
                             lambda o, a: o.gemm_nt_swiglu(a["a"], a["w12"], a["b12"])),
    "gemm_nt_qkv_rope": (lambda: dict(a=Z(2, 4), w=Z(12, 4), bias=Z(12), wq=Z(4), wk=Z(4), cos=Z(2, 4), sin=Z(2, 4)),
                         lambda o, a: o.gemm_nt_qkv_rope(a["a"], a["w"], a["bias"], a["wq"], a["wk"], a["cos"], a["sin"], 1, 2, 1, 4)),
    "mx8_quantize": (lambda: dict(x=Z(2, 128)), lambda o, a: o.mx8_quantize(a["x"])),
    "rmsnorm_modulate_fwd_mx8": (lambda: dict(x=Z(2, 128), w=Z(128), shift=Z(2, 128), scale=Z(2, 128)),
                                 lambda o, a: o.rmsnorm_modulate_fwd_mx8(a["x"], a["w"], a["shift"], a["scale"], 1)),
    "gemm_nt_mx8": (_mx8(bias=lambda: Z(3), out=lambda: Z(2, 3, dtype=BF16)),
                    lambda o, a: o.gemm_nt_mx8(a["aq"], a["asc"], a["wq"], a["wsc"], a["bias"], out=a["out"])),
    "gemm_nt_gate_res_mx8": (_mx8(bias=lambda: Z(3), xin=lambda: Z(2, 3), gate=lambda: Z(2, 3), xout=lambda: Z(2, 3)),
                             lambda o, a: o.gemm_nt_gate_res_mx8(a["aq"], a["asc"], a["wq"], a["wsc"], a["bias"], a["xin"], a["gate"], 1, xout=a["xout"])),
    "gemm_nt_swiglu_mx8": (_mx8(256, b12=lambda: Z(256)), lambda o, a: o.gemm_nt_swiglu_mx8(a["aq"], a["asc"], a["wq"], a["wsc"], a["b12"])),
    "gemm_nt_qkv_rope_mx8": (_mx8(12, bias=lambda: Z(12), nwq=lambda: Z(4), nwk=lambda: Z(4), cos=lambda: Z(2, 4), sin=lambda: Z(2, 4)),
                             lambda o, a: o.gemm_nt_qkv_rope_mx8(a["aq"], a["asc"], a["wq"], a["wsc"], a["bias"], a["nwq"], a["nwk"], a["cos"], a["sin"],
                                                                 1, 2, 1, 4)),
    "gemm_nt_swiglu_bwd": (lambda: dict(dy=Z(2, 4), w3t=Z(3, 4), h12=Z(2, 6)), lambda o, a: o.gemm_nt_swiglu_bwd(a["dy"], a["w3t"], a["h12"])),
    "gemm_nt_swiglu_bwd[bf16]": (lambda: dict(dy=Z(2, 64, dtype=BF16), w3t=Z(8, 64, dtype=BF16), h12=Z(2, 16, dtype=BF16)),
                                 lambda o, a: o.gemm_nt_swiglu_bwd(a["dy"], a["w3t"], a["h12"], with_bias=True)),
    "gemm_tn": (lambda: dict(a=Z(2, 3), b=Z(2, 4), out=Z(3, 4), dbias_out=Z(3)),
                lambda o, a: o.gemm_tn(a["a"], a["b"], out=a["out"], beta=1.0, with_bias=True, dbias_out=a["dbias_out"])),
    "colsum": (lambda: dict(x=Z(2, 3), out=Z(3)), lambda o, a: o.colsum(a["x"], out=a["out"])),
    "cast_weight": (lambda: dict(w=Z(2, 3)), lambda o, a: o.cast_weight(a["w"], BF16)),
    "cast": (lambda: dict(x=Z(2, 4)), lambda o, a: o.cast(a["x"], BF16)),
    "thin_nt": (lambda: dict(t=Z(2, 16), w=Z(4, 16), bias=Z(4), pos=Z(2, 4)), lambda o, a: o.thin_nt(a["t"], a["w"], a["bias"], a["pos"], 2)),
    "thin_tn": (lambda: dict(g=Z(2, 4), t=Z(2, 16)), lambda o, a: o.thin_tn(a["g"], a["t"])),
    "multi_add_": (lambda: dict(dst0=Z(4), dst1=Z(2, 3), src0=Z(4), src1=Z(2, 3)),
                   lambda o, a: o.multi_add_([a["dst0"], a["dst1"]], [a["src0"], a["src1"]])),
    "cast_stack": (lambda: dict(t0=Z(2, 8), t1=Z(2, 8)), lambda o, a: o.cast_stack([a["t0"], a["t1"]], BF16)),
    "rmsnorm_modulate_fwd": (lambda: dict(x=Z(2, 4), w=Z(4), shift=Z(2, 4), scale=Z(2, 4)),
                             lambda o, a: o.rmsnorm_modulate_fwd(a["x"], a["w"], a["shift"], a["scale"], 1, F32)),
    "rmsnorm_modulate_fwd[w=None]": (lambda: dict(x=Z(2, 4), shift=Z(2, 4), scale=Z(2, 4)),
                                     lambda o, a: o.rmsnorm_modulate_fwd(a["x"], None, a["shift"], a["scale"], 1, BF16)),
    "res_rmsnorm_modulate_fwd": (lambda: dict(x=Z(2, 4), ya=Z(2, 4, dtype=BF16), gate_a=Z(2, 4), yb=Z(2, 4, dtype=BF16), gate_b=Z(2, 4), w=Z(4),
                                              shift=Z(2, 4), scale=Z(2, 4)),
                                 lambda o, a: o.res_rmsnorm_modulate_fwd(a["x"], a["ya"], a["gate_a"], a["yb"], a["gate_b"], a["w"], a["shift"], a["scale"], 1,
                                                                         want_xout=True)),
    "rmsnorm_modulate_bwd": _norm_bwd(),
    "rmsnorm_modulate_bwd[w=None]": _norm_bwd(w=False),
    "rmsnorm_modulate_bwd_gate": _norm_bwd(gate=True),
    "rmsnorm_modulate_bwd_gate[w=None]": _norm_bwd(w=False, gate=True),
    "rmsnorm_modulate_bwd_gate[recompute]": _norm_bwd(gate=True, dt=BF16, recompute=True),
    "qknorm_rope_fwd": (lambda: dict(qkv=Z(2, 12), wq=Z(4), wk=Z(4), cos=Z(2, 4), sin=Z(2, 4)),
                        lambda o, a: o.qknorm_rope_fwd(a["qkv"], a["wq"], a["wk"], a["cos"], a["sin"], 1, 2, 1, 4)),
    "qknorm_rope_bwd": (lambda: dict(dq=Z(1, 1, 2, 4), dk=Z(1, 1, 2, 4), dv=Z(1, 1, 2, 4), qkv=Z(2, 12), wq=Z(4), wk=Z(4), cos=Z(2, 4), sin=Z(2, 4)),
                        lambda o, a: o.qknorm_rope_bwd(a["dq"], a["dk"], a["dv"], a["qkv"], a["wq"], a["wk"], a["cos"], a["sin"], 1, 2, 1, 4, with_bias=True)),
    "qknorm_rope_bwd[dv=None]": (lambda: dict(dq=Z(1, 1, 2, 4), dk=Z(1, 1, 2, 4), qkv=Z(2, 12), cos=Z(2, 4), sin=Z(2, 4), dqkv=Z(2, 12)),
                                 lambda o, a: o.qknorm_rope_bwd(a["dq"], a["dk"], None, a["qkv"], None, None, a["cos"], a["sin"], 1, 2, 1, 4, dqkv=a["dqkv"])),
    "rope": (lambda: dict(t=Z(1, 2, 4), cos=Z(2, 4), sin=Z(2, 4)), lambda o, a: o.rope(a["t"], a["cos"], a["sin"])),
    "attention_fwd": (lambda: dict(q=Z(1, 1, 2, 16), k=Z(1, 1, 2, 16), v=Z(1, 1, 2, 16)), lambda o, a: o.attention_fwd(a["q"], a["k"], a["v"], 0.25)),
    "attention_bwd": (lambda: dict(q=Z(1, 1, 2, 16), k=Z(1, 1, 2, 16), v=Z(1, 1, 2, 16), o=Z(1, 2, 16), do=Z(1, 2, 16), lse=Z(1, 1, 2)),
                      lambda o, a: o.attention_bwd(a["q"], a["k"], a["v"], a["o"], a["do"], a["lse"], 0.25)),
    "qk_score_bound": (lambda: dict(wq=Z(16), wk=Z(16)), lambda o, a: o.qk_score_bound(a["wq"], a["wk"], 16, 0.25)),
    "attention_fwd_pv": (lambda: dict(q=Z(1, 1, 2, 16, dtype=BF16), k=Z(1, 1, 2, 16, dtype=BF16), qkv=Z(2, 48, dtype=BF16)),
                         lambda o, a: o.attention_fwd_pv(a["q"], a["k"], a["qkv"], 0.25)),
    "attention_fwd_pv[bound]": (lambda: dict(q=Z(1, 1, 2, 16, dtype=BF16), k=Z(1, 1, 2, 16, dtype=BF16), qkv=Z(2, 48, dtype=BF16), bound=Z(1)),
                                lambda o, a: o.attention_fwd_pv(a["q"], a["k"], a["qkv"], 0.25, bound=a["bound"])),
    "attention_bwd_pv": _attn_bwd_pv("attention_bwd_pv", False),
    "attention_bwd_pv_qknorm": _attn_bwd_pv("attention_bwd_pv_qknorm", True),
    "attention_fwd_qkv": (lambda: dict(qkv=Z(2, 48, dtype=BF16)), lambda o, a: o.attention_fwd_qkv(a["qkv"], 1, 2, 1, 16, 0.25)),
    "attention_fwd_qkv[f32]": (lambda: dict(qkv=Z(2, 48)), lambda o, a: o.attention_fwd_qkv(a["qkv"], 1, 2, 1, 16, 0.25)),
    "attention_bwd_qkv": (lambda: dict(qkv=Z(2, 48, dtype=BF16), o=Z(1, 2, 16, dtype=BF16), do=Z(1, 2, 16, dtype=BF16), lse=Z(1, 1, 2)),
                          lambda o, a: o.attention_bwd_qkv(a["qkv"], a["o"], a["do"], a["lse"], 1, 2, 1, 16, 0.25)),
    "swiglu_fwd": (lambda: dict(h12=Z(2, 4)), lambda o, a: o.swiglu_fwd(a["h12"])),
    "swiglu_bwd": (lambda: dict(dhid=Z(2, 2), h12=Z(2, 4)), lambda o, a: o.swiglu_bwd(a["dhid"], a["h12"])),
    "gate_bwd": (lambda: dict(dxout=Z(2, 4), y=Z(2, 4), gate=Z(2, 4), dgate=Z(2, 4)),
                 lambda o, a: o.gate_bwd(a["dxout"], a["y"], a["gate"], a["dgate"], 1, F32, with_bias=True)),
    "timestep_embedding": (lambda: dict(t=Z(2)), lambda o, a: o.timestep_embedding(a["t"])),
    "silu_fwd": (lambda: dict(x=Z(2, 8)), lambda o, a: o.silu_fwd(a["x"])),
    "silu_bwd": (lambda: dict(dy=Z(2, 8), x=Z(2, 8)), lambda o, a: o.silu_bwd(a["dy"], a["x"])),
    "label_embed_fwd": (lambda: dict(table=Z(3, 4), y=Z(2, dtype=I64), drop=Z(2, dtype=U8)), lambda o, a: o.label_embed_fwd(a["table"], a["y"], a["drop"], 2)),
    "label_embed_bwd": (lambda: dict(dout=Z(2, 4), y=Z(2, dtype=I64), drop=Z(2, dtype=U8)), lambda o, a: o.label_embed_bwd(a["dout"], a["y"], a["drop"], 2, 3)),
    "cached_weight_copy": (lambda: dict(w=Z(2, 3)), lambda o, a: o.cached_weight_copy(a["w"], BF16)),
    "cached_weight_mx8": (lambda: dict(w=Z(2, 128)), lambda o, a: o.cached_weight_mx8(a["w"])),
    "cached_stack_copy": (lambda: dict(t0=Z(2, 8), t1=Z(2, 8)), lambda o, a: o.cached_stack_copy([a["t0"], a["t1"]], BF16)),
    "adamw_ema": (lambda: dict(p=Z(4), g=Z(4), m=Z(4), v=Z(4), ema=Z(4)),
                  lambda o, a: o.adamw_ema(a["p"], a["g"], a["m"], a["v"], a["ema"], 1, 1e-3, 0.9, 0.95, 1e-8, 0.0, 0.999)),
    "ema_only": (lambda: dict(ema=Z(4), p=Z(4)), lambda o, a: o.ema_only(a["ema"], a["p"], 0.999)),
    "adamw_ema_tracks": (lambda: dict(p=Z(4), g=Z(4), m=Z(4), v=Z(4), ema=Z(4), track=Z(4)),
                         lambda o, a: o.adamw_ema_tracks(a["p"], a["g"], a["m"], a["v"], a["ema"], [a["track"]], [0.5], 1, 1e-3, 0.9, 0.95, 1e-8, 0.0, 0.999)),
    "ema_tracks_only": (lambda: dict(p=Z(4), track=Z(4)), lambda o, a: o.ema_tracks_only(a["p"], [a["track"]], [0.5])),
    "snapshot_accumulate": (lambda: dict(acc=Z(4, dtype=F64), x=Z(4)), lambda o, a: o.snapshot_accumulate(a["acc"], a["x"], 0.5)),
    "snapshot_finish": (lambda: dict(acc=Z(4, dtype=F64), out=Z(4)), lambda o, a: o.snapshot_finish(a["acc"], a["out"])),
    "random_masking": (lambda: dict(noise=Z(2, 16)), lambda o, a: o.random_masking(a["noise"], 4)),
    "patch_embed_kept": (lambda: dict(img=Z(1, 1, 2, 2), ids_keep=Z(1, 2, dtype=I64), pos=Z(4, 4), w2d=Z(4, 1), bias=Z(4)),
                         lambda o, a: o.patch_embed_kept(a["img"], a["ids_keep"], a["pos"], a["w2d"], a["bias"], 1, F32)),
    "latent_prologue": (lambda: dict(moments=Z(1, 4, 2, 2), noise=Z(1, 2, 2, 2), lat_mean=Z(2), lat_std=Z(2)),
                        lambda o, a: o.latent_prologue(a["moments"], a["noise"], a["lat_mean"], a["lat_std"])),
    "fm_valid_plan": (lambda: dict(stored=Z(1, 4, 2, 2), idx=Z(1, dtype=I64), t=Z(1), lat_mean=Z(2), lat_std=Z(2)),
                      lambda o, a: o.fm_valid_plan(a["stored"], a["idx"], a["t"], a["lat_mean"], a["lat_std"])),
    "row_mse": (lambda: dict(a=Z(2, 4), u=Z(2, 4), out=Z(2)), lambda o, a: o.row_mse(a["a"], a["u"], a["out"])),
    "guidance_combine": (lambda: dict(pos=Z(1, 2, 2, 2), neg=Z(1, 2, 2, 2), out=Z(1, 2, 2, 2)),
                         lambda o, a: o.guidance_combine("cfg", a["pos"], a["neg"], 1.5, out=a["out"])),
    "guidance_combine[apg]": (lambda: dict(pos=Z(1, 2, 2, 2), neg=Z(1, 2, 2, 2), x=Z(1, 2, 2, 2), t=Z(1), mom=Z(1, 8), out=Z(1, 2, 2, 2)),
                              lambda o, a: o.guidance_combine("apg", a["pos"], a["neg"], 1.5, x=a["x"], t=a["t"], momentum=0.5, mom=a["mom"], out=a["out"])),
    "crop_resize_flip": (lambda: dict(blob=Z(12, dtype=U8), out=Z(1, 3, 2, 2)),
                         lambda o, a: o.crop_resize_flip(a["blob"], torch.zeros(1, dtype=I64), torch.tensor([[2, 2, 0, 0, 2, 2, 0, 0]], dtype=I32), 2, out=a["out"])),
    "gather_rows": (lambda: dict(x=Z(1, 2, 4), ids=Z(1, 2, dtype=I64)), lambda o, a: o.gather_rows(a["x"], a["ids"])),
    "scatter_rows": (lambda: dict(dout=Z(1, 2, 4), ids=Z(1, 2, dtype=I64)), lambda o, a: o.scatter_rows(a["dout"], a["ids"], 4)),
    "restore_tokens": (lambda: dict(x=Z(1, 2, 4), mask_token=Z(4), pos=Z(4, 4), ids_restore=Z(1, 4, dtype=I64)),
                       lambda o, a: o.restore_tokens(a["x"], a["mask_token"], a["pos"], a["ids_restore"])),
    "restore_tokens_bwd": (lambda: dict(dout=Z(1, 4, 4), ids_restore=Z(1, 4, dtype=I64)), lambda o, a: o.restore_tokens_bwd(a["dout"], a["ids_restore"], 2)),
    "vmae_encoder_fwd": (lambda: dict(x=Z(1, 2, 4), blob=_blob()), lambda o, a: o.vmae_encoder_fwd(a["x"], a["blob"], 1, 4, 1, 8)),
    "vmae_encoder_fwd_tiled": (lambda: dict(x=Z(1, 2, 4), blob=_blob()), lambda o, a: o.vmae_encoder_fwd_tiled(a["x"], a["blob"], 1, 4, 1, 8)),
    "heads_split": (lambda: dict(qkv=Z(2, 24)), lambda o, a: o.heads_split(a["qkv"], 1, 2, 1, 8)),
    "heads_merge": (lambda: dict(dq=Z(1, 1, 2, 8), dk=Z(1, 1, 2, 8), dv=Z(1, 1, 2, 8)), lambda o, a: o.heads_merge(a["dq"], a["dk"], a["dv"], 1, 2, 1, 8)),
    "conv3x3": (lambda: dict(x=Z(1, 3, 2, 2), w=Z(3, 3, 3, 3), b=Z(3)), lambda o, a: o.conv3x3(a["x"], a["w"], a["b"])),
    "conv3x3_bwd": (lambda: dict(dout=Z(1, 3, 2, 2), x=Z(1, 3, 2, 2), w=Z(3, 3, 3, 3)), lambda o, a: o.conv3x3_bwd(a["dout"], a["x"], a["w"])),
    "mae_loss_fwd": (lambda: dict(pred_img=Z(1, 1, 2, 2), imgs=Z(1, 1, 2, 2), mask=Z(1, 4)), lambda o, a: o.mae_loss_fwd(a["pred_img"], a["imgs"], a["mask"], 1)),
    "mae_loss_bwd": (lambda: dict(pred_img=Z(1, 1, 2, 2), imgs=Z(1, 1, 2, 2), mask=Z(1, 4), coef=Z(2)),
                     lambda o, a: o.mae_loss_bwd(a["pred_img"], a["imgs"], a["mask"], a["coef"], 1)),
    "layernorm_fwd": (lambda: dict(x=Z(2, 4), w=Z(4), b=Z(4)), lambda o, a: o.layernorm_fwd(a["x"], a["w"], a["b"], F32)),
    "layernorm_bwd": (lambda: dict(dout=Z(2, 4), x=Z(2, 4), w=Z(4), mean=Z(2), rstd=Z(2), dx_accum=Z(2, 4)),
                      lambda o, a: o.layernorm_bwd(a["dout"], a["x"], a["w"], a["mean"], a["rstd"], a["dx_accum"])),
    "layernorm_bwd[cast]": (lambda: dict(dout=Z(2, 4, dtype=BF16), x=Z(2, 4), w=Z(4), mean=Z(2), rstd=Z(2), dx_accum=Z(2, 4)),
                            lambda o, a: o.layernorm_bwd(a["dout"], a["x"], a["w"], a["mean"], a["rstd"], a["dx_accum"], cast=True)),
    "gelu_bwd": (lambda: dict(dout=Z(2, 4), pre=Z(2, 4)), lambda o, a: o.gelu_bwd(a["dout"], a["pre"])),
    "gelu_tanh_fwd": (lambda: dict(x=Z(2, 4)), lambda o, a: o.gelu_tanh_fwd(a["x"])),
    "gelu_tanh_bwd": (lambda: dict(dout=Z(2, 4), pre=Z(2, 4)), lambda o, a: o.gelu_tanh_bwd(a["dout"], a["pre"])),
    "ball_counts": (lambda: dict(u=Z(2, 4), ru=Z(2), v=Z(3, 4), nu=Z(2), nv=Z(3)), lambda o, a: o.ball_counts(a["u"], a["ru"], a["v"], a["nu"], a["nv"])),
    "kid_sums": (lambda: dict(a=Z(2, 4), b=Z(2, 4)), lambda o, a: o.kid_sums(a["a"], a["b"], [[0, 1]], [[0, 1]], 1.0)),
    "token_mean": (lambda: dict(x=Z(1, 2, 4)), lambda o, a: o.token_mean(a["x"])),
    "bn1d_fwd": (lambda: dict(x=Z(2, 4), run_mean=Z(4), run_var=Z(4), out=Z(2, 4)), lambda o, a: o.bn1d_fwd(a["x"], a["run_mean"], a["run_var"], out=a["out"])),
    "softmax_xent": (lambda: dict(logits=Z(2, 4)), lambda o, a: o.softmax_xent(a["logits"], [0, 1])),
    "lars_norms": (lambda: dict(p=Z(4), g=Z(4), out=Z(2)), lambda o, a: o.lars_norms(a["p"], a["g"], out=a["out"])),
    "lars_step": (lambda: dict(p=Z(4), g=Z(4), mu=Z(4), norms=Z(2)), lambda o, a: o.lars_step(a["p"], a["g"], a["mu"], 0.1, a["norms"])),
    "l2_normalize": (lambda: dict(x=Z(2, 4)), lambda o, a: o.l2_normalize(a["x"])),
    "topk_merge": (lambda: dict(sims=Z(2, 3), vals=Z(2, 2), idx=Z(2, 2, dtype=I32)), lambda o, a: o.topk_merge(a["sims"], 0, a["vals"], a["idx"])),
    "knn_vote": (lambda: dict(vals=Z(2, 2), idx=Z(2, 2, dtype=I32)), lambda o, a: o.knn_vote(a["vals"], a["idx"], [0, 1, 0], [0, 1], 2)),
    # ---- evaluation, tokenizers, samplers: conv2d_nhwc .. sde_combine
    "conv2d_nhwc": (lambda: dict(x=Z(1, 4, 4, 4), w=Z(8, 3, 3, 4), bias=Z(8), out=Z(1, 2, 2, 8)),
                    lambda o, a: o.conv2d_nhwc(a["x"], a["w"], a["bias"], out=a["out"])),
    "pool2d_nhwc": (lambda: dict(x=Z(1, 4, 4, 4), out=Z(1, 2, 2, 4)), lambda o, a: o.pool2d_nhwc(a["x"], "max", out=a["out"])),
    "global_avgpool_nhwc": (lambda: dict(x=Z(1, 2, 2, 4)), lambda o, a: o.global_avgpool_nhwc(a["x"])),
    "fid_preprocess": (lambda: dict(img=Z(1, 4, 4, 3, dtype=U8)), lambda o, a: o.fid_preprocess(a["img"], 8)),
    "fid_stats_accumulate": (lambda: dict(feats=Z(2, 4), shift=Z(4), s1=Z(4, dtype=F64), s2=Z(4, 4, dtype=F64)),
                             lambda o, a: o.fid_stats_accumulate(a["feats"], a["shift"], a["s1"], a["s2"])),
    "adm_preprocess": (lambda: dict(img=Z(1, 4, 4, 3, dtype=U8)), lambda o, a: o.adm_preprocess(a["img"], 8)),
    "adm_spatial_tap": (lambda: dict(x=Z(1, 2, 2, 8)), lambda o, a: o.adm_spatial_tap(a["x"])),
    "row_sqnorms": (lambda: dict(x=Z(2, 4)), lambda o, a: o.row_sqnorms(a["x"])),
    "pairwise_logits": (lambda: dict(u=Z(2, 4), w=Z(3, 4)), lambda o, a: o.pairwise_logits(a["u"], a["w"])),
    "knn_radii": (lambda: dict(x=Z(4, 4), norms=Z(4)), lambda o, a: o.knn_radii(a["x"], (3,), a["norms"])),
    "pr_flags": (lambda: dict(u=Z(2, 4), ru=Z(2, 2), v=Z(3, 4), rv=Z(3, 2), nu=Z(2), nv=Z(3)),
                 lambda o, a: o.pr_flags(a["u"], a["ru"], a["v"], a["rv"], a["nu"], a["nv"])),
    "adm_softmax_is": (lambda: dict(logits=Z(2, 4)), lambda o, a: o.adm_softmax_is(a["logits"])),
    "lpips_prep": (lambda: dict(input=Z(1, 3, 2, 2), target=Z(1, 3, 2, 2)), lambda o, a: o.lpips_prep(a["input"], a["target"])),
    "lpips_layer": (lambda: dict(f=Z(2, 2, 2, 64), lin_w=Z(64), out=Z(1)), lambda o, a: o.lpips_layer(a["f"], a["lin_w"], a["out"])),
    "conv3x3_relu_dgrad_nhwc": (lambda: dict(dy=Z(1, 4, 4, 8), y=Z(1, 4, 4, 8), w_rot=Z(4, 3, 3, 8), out=Z(1, 4, 4, 4)),
                                lambda o, a: o.conv3x3_relu_dgrad_nhwc(a["dy"], a["y"], a["w_rot"], a["out"])),
    "maxpool2x2_bwd_nhwc": (lambda: dict(dy=Z(1, 2, 2, 4), x=Z(1, 4, 4, 4), out=Z(1, 4, 4, 4)),
                            lambda o, a: o.maxpool2x2_bwd_nhwc(a["dy"], a["x"], a["out"])),
    "lpips_layer_bwd": _lpips_bwd("lpips_layer_bwd", F32),
    "lpips_prep_bwd": (lambda: dict(g=Z(1, 2, 2, 4)), lambda o, a: o.lpips_prep_bwd(a["g"])),
    "lpips_prep_f16": (lambda: dict(input=Z(1, 3, 2, 2), target=Z(1, 3, 2, 2)), lambda o, a: o.lpips_prep_f16(a["input"], a["target"])),
    "conv3x3_relu_nhwc_f16": (lambda: dict(x=Z(1, 4, 4, 8, dtype=F16), w=Z(16, 3, 3, 8, dtype=F16), bias=Z(16), out=Z(1, 4, 4, 16, dtype=F16)),
                              lambda o, a: o.conv3x3_relu_nhwc_f16(a["x"], a["w"], a["bias"], a["out"])),
    "maxpool2x2_nhwc_f16": (lambda: dict(x=Z(1, 2, 2, 8, dtype=F16)), lambda o, a: o.maxpool2x2_nhwc_f16(a["x"])),
    "lpips_layer_f16": (lambda: dict(f=Z(2, 2, 2, 64, dtype=F16), lin_w=Z(64), out=Z(1)),
                        lambda o, a: o.lpips_layer_f16(a["f"], a["lin_w"], a["out"])),
    "conv3x3_relu_dgrad_nhwc_bf16": (lambda: dict(dy=Z(1, 4, 4, 8), y=Z(1, 4, 4, 8, dtype=F16), w_rot=Z(8, 3, 3, 8, dtype=BF16), out=Z(1, 4, 4, 8)),
                                     lambda o, a: o.conv3x3_relu_dgrad_nhwc_bf16(a["dy"], a["y"], a["w_rot"], a["out"])),
    "maxpool2x2_bwd_nhwc_xf16": (lambda: dict(dy=Z(1, 2, 2, 4), x=Z(1, 4, 4, 4, dtype=F16), out=Z(1, 4, 4, 4)),
                                 lambda o, a: o.maxpool2x2_bwd_nhwc_xf16(a["dy"], a["x"], a["out"])),
    "lpips_layer_bwd_f16": _lpips_bwd("lpips_layer_bwd_f16", F16),
    "lpips_prep_bwd_c8": (lambda: dict(g=Z(1, 2, 2, 8)), lambda o, a: o.lpips_prep_bwd_c8(a["g"])),
    "ssim": (lambda: dict(preds=Z(1, 1, 11, 11), target=Z(1, 1, 11, 11)), lambda o, a: o.ssim(a["preds"], a["target"])),
    "recon_quantize_sse": (lambda: dict(decoded=Z(1, 3, 2, 2), ref=Z(1, 3, 2, 2)), lambda o, a: o.recon_quantize_sse(a["decoded"], a["ref"])),
    "sse_u8": (lambda: dict(a=Z(1, 4, dtype=U8), b=Z(1, 4, dtype=U8)), lambda o, a: o.sse_u8(a["a"], a["b"])),
    "groupnorm_stats_nhwc": (lambda: dict(x=Z(1, 2, 2, 32)), lambda o, a: o.groupnorm_stats_nhwc(a["x"])),
    "groupnorm_apply_nhwc": (lambda: dict(x=Z(1, 2, 2, 32), mean=Z(1, 32), rstd=Z(1, 32), gamma=Z(32), beta=Z(32), out=Z(1, 2, 2, 32)),
                             lambda o, a: o.groupnorm_apply_nhwc(a["x"], (a["mean"], a["rstd"]), a["gamma"], a["beta"], out=a["out"])),
    "conv3x3_vae_nhwc": (lambda: dict(x=Z(1, 2, 2, 32), w=Z(4, 3, 3, 32), bias=Z(4), res=Z(1, 2, 2, 4), mean=Z(1, 32), rstd=Z(1, 32), gamma=Z(32),
                                      beta=Z(32)),
                         lambda o, a: o.conv3x3_vae_nhwc(a["x"], a["w"], a["bias"], o.VAE_NORM_ACT, a["res"], (a["mean"], a["rstd"]), a["gamma"],
                                                         a["beta"])),
    "conv3x3_vae_nhwc[tf32]": (lambda: dict(x=Z(1, 2, 2, 8, dtype=F16), w=Z(4, 3, 3, 8, dtype=F16), bias=Z(4), res=Z(1, 2, 2, 4)),
                               lambda o, a: o.conv3x3_vae_nhwc(a["x"], a["w"], a["bias"], o.VAE_PLAIN, a["res"], precision="tf32")),
    "conv1x1_res_nhwc": (lambda: dict(x=Z(1, 2, 2, 4), w=Z(8, 4), bias=Z(8), res=Z(1, 2, 2, 8)),
                         lambda o, a: o.conv1x1_res_nhwc(a["x"], a["w"], a["bias"], a["res"])),
    "conv1x1_res_nhwc[tf32]": (lambda: dict(x=Z(1, 2, 2, 8), w=Z(8, 8, dtype=F16), bias=Z(8), res=Z(1, 2, 2, 8)),
                               lambda o, a: o.conv1x1_res_nhwc(a["x"], a["w"], a["bias"], a["res"], precision="tf32")),
    "softmax_rows_": (lambda: dict(s=Z(2, 4)), lambda o, a: o.softmax_rows_(a["s"], 3)),
    "attention_wide": (lambda: dict(q=Z(1, 2, 16), k=Z(1, 2, 16), vt=Z(1, 16, 16), bias=Z(16)),
                       lambda o, a: o.attention_wide(a["q"], a["k"], a["vt"], 1.0, a["bias"])),
    "rk_stage": (lambda: dict(y=Z(2, 2), k_slab=Z(7, 4), h_dev=Z(2), out=Z(2, 2), t_dev=Z(2), t_out=Z(3)),
                 lambda o, a: o.rk_stage(a["y"], a["k_slab"], (0.5, 0.5), a["h_dev"], a["out"], a["t_dev"], 0.5, a["t_out"])),
    "dopri5_finish": (lambda: dict(y=Z(2, 2), k_slab=Z(7, 4), h_dev=Z(2), y1=Z(2, 2), partial=Z(64), ratio_dev=Z(2)),
                      lambda o, a: o.dopri5_finish(a["y"], a["k_slab"], a["h_dev"], 1e-6, 1e-3, a["y1"], a["partial"], a["ratio_dev"])),
    "rms_norm_scaled": (lambda: dict(x=Z(2, 2), y=Z(2, 2), partial=Z(64), out_dev=Z(2)),
                        lambda o, a: o.rms_norm_scaled(a["x"], a["y"], 1e-6, 1e-3, a["partial"], a["out_dev"])),
    "dopri5_interp": (lambda: dict(y0=Z(2, 2), y1=Z(2, 2), y_mid=Z(2, 2), k_slab=Z(7, 4), h_dev=Z(2), t0_dev=Z(2), out=Z(2, 2)),
                      lambda o, a: o.dopri5_interp(a["y0"], a["y1"], a["y_mid"], a["k_slab"], a["h_dev"], a["t0_dev"], 0.5, a["out"])),
    "dopri5_advance": (lambda: dict(ratio_dev=Z(2), h_dev=Z(2), t_dev=Z(2), status_dev=Z(6)),
                       lambda o, a: o.dopri5_advance(a["ratio_dev"], a["h_dev"], a["t_dev"], a["status_dev"])),
    "dopri5_initial_step": (lambda: dict(d_dev=Z(4), h_dev=Z(2)), lambda o, a: o.dopri5_initial_step(a["d_dev"], 0, a["h_dev"])),
    "rowdot": (lambda: dict(a=Z(2, 4), b=Z(2, 4), out=Z(2)), lambda o, a: o.rowdot(a["a"], a["b"], a["out"])),
    "likelihood_finish": (lambda: dict(sumsq=Z(2), delta=Z(2)), lambda o, a: o.likelihood_finish(a["sumsq"], a["delta"], 4)),
    "normal": (lambda: dict(out=Z(2, 4)), lambda o, a: o.normal(None, 1, 0, "cpu", out=a["out"])),
    "sde_combine": (lambda: dict(in0=Z(2, 2), in1=Z(2, 2), out=Z(2, 2), z=Z(2, 2), mean_out=Z(2, 2), t_out=Z(3)),
                    lambda o, a: o.sde_combine([a["in0"], a["in1"]], (0.5, 0.5), a["out"], 0.1, a["z"], mean_out=a["mean_out"], t_out=a["t_out"])),
}
FIRST_HALF = tuple(ROWS)[:tuple(ROWS).index("conv2d_nhwc")]
# a message that opens with one of these is the wrapper's own refusal (some families name their shared contract instead of the op)
PREFIX = {"recon_quantize_sse": ("recon_quantize",), "attention_wide": ("attention_wide", "gemm_nt", "softmax_rows_"),
          **{op: (op, "ode:") for op in ("rk_stage", "dopri5_finish", "dopri5_interp")},
          "rmsnorm_modulate_bwd_gate": ("rmsnorm_modulate_bwd",), "vmae_encoder_fwd_tiled": ("vmae_encoder_fwd",),
          "mae_loss_fwd": ("mae_loss",), "mae_loss_bwd": ("mae_loss",), "gemm_nt_swiglu": ("gemm_nt",), "gemm_nt_swiglu_bwd": ("gemm_nt", "swiglu_bwd"),
          "cached_weight_copy": ("cast_weight",), "cached_weight_mx8": ("mx8_quantize",), "cached_stack_copy": ("cast_stack",),
          "l2_normalize": ("l2_normalize", "row_sqnorms")}
# public names of ops.py that pass no tensor to the library, each with why: nothing to characterise
NO_TENSOR_ARGS = {
    "stream": "the current stream's handle", "workspace": "makes the scratch buffer itself", "side_stream": "a stream per device", "set_gemm_launch_mode": "a mode string",
    "set_gemm_half_lines": "a flag", "gemm_launch_mode": "reads the mode", "thin_ok": "two integers", "invalidate_weight_cache": "bumps a counter",
    "gemm_nt_qkv_rope_ok": "a predicate on strides and shapes: reads attributes only", "gemm_nt_qkv_rope_mx8_ok": "a predicate, as above",
    "check_crop_table": "checks HOST tables", "check_kid_index_table": "checks a HOST table", "check_labels": "checks and uploads a HOST vector",
    "topk_empty": "makes its tensors itself", "default_col_splits": "two integers", "ode_slab_ld": "one integer", "ode_partials": "one integer",
    "rademacher": "makes its tensor itself: a shape, a seed, a counter"}

# ---- why a call of the training path with one damaged tensor may still reach the device.  Each reason stands for a rule:
COPIED = "strided: an input of another layout is copied first (_arg's copy=True), as the wrapper did before it had checks"
CONVERTED = "dtype: the wrapper converts this input to float32 by its documented contract and checks the result"
FLAT = "dim: the kernel addresses this operand flat; numel= still holds and its shape is not used"
# ... and two the defect generator itself makes: the damaged tensor IS a well-formed argument, so refusing it would change behaviour
DISPATCH = "dtype: the entry dispatches on this tensor's type and has a kernel for the other one (f32 <-> f16 / bf16); nothing else states it"
EXTENT = "shape: the wrapper takes this extent from this very tensor and no other argument states it: the doubled tensor is a well-formed call"
_GEMM = {"gemm_nt": "a b bias", "gemm_nt_gate_res": "a b bias gate xin", "gemm_nt_pos": "a b bias pos", "gemm_nt_gelu": "a b bias",
         "gemm_nt_gelu_bwd": "dy pre w2t", "gemm_nt_swiglu": "a b12 w12", "gemm_nt_swiglu[bf16]": "a b12 w12",
         "gemm_nt_qkv_rope": "a bias cos sin w wk wq", "mx8_quantize": "x", "gemm_nt_mx8": "aq asc bias wq wsc",
         "gemm_nt_gate_res_mx8": "aq asc bias gate wq wsc xin", "gemm_nt_swiglu_mx8": "aq asc b12 wq wsc",
         "gemm_nt_qkv_rope_mx8": "aq asc bias cos nwk nwq sin wq wsc", "gemm_nt_swiglu_bwd": "dy h12 w3t", "gemm_nt_swiglu_bwd[bf16]": "dy h12 w3t",
         "gemm_tn": "a b", "colsum": "x", "cast_weight": "w", "cast": "x", "thin_nt": "bias pos t w", "thin_tn": "g t", "multi_add_": "src0 src1",
         "cast_stack": "t0 t1", "cached_weight_copy": "w", "cached_weight_mx8": "w", "cached_stack_copy": "t0 t1"}
_NORM_BWD = {"rmsnorm_modulate_bwd": "dout rstd w x", "rmsnorm_modulate_bwd[w=None]": "dout rstd x", "rmsnorm_modulate_bwd_gate": "dout rstd w x y",
             "rmsnorm_modulate_bwd_gate[w=None]": "dout rstd x y", "rmsnorm_modulate_bwd_gate[recompute]": "dout rstd w x y"}
# reason -> {op: the arguments it holds for}.  The modulation and gate views (shift, scale, gate of the backward forms) are read in place at
# their row stride and are NOT here: a view of another layout is refused.
_ALLOWED = {
    COPIED: {**_GEMM, **_NORM_BWD, "rmsnorm_modulate_fwd_mx8": "w x", "rmsnorm_modulate_fwd": "w x", "rmsnorm_modulate_fwd[w=None]": "x",
             "res_rmsnorm_modulate_fwd": "gate_a gate_b w x ya yb", "qknorm_rope_fwd": "cos qkv sin wk wq",
             "qknorm_rope_bwd": "cos dk dq dv qkv sin wk wq", "qknorm_rope_bwd[dv=None]": "cos dk dq qkv sin", "rope": "cos sin t",
             "attention_fwd": "k q v", "attention_bwd": "do k lse o q v", "qk_score_bound": "wk wq", "attention_fwd_pv": "k q qkv",
             "attention_fwd_pv[bound]": "k q qkv", "attention_bwd_pv": "do k lse o q qkv", "attention_bwd_pv_qknorm": "cos do k lse o q qkv sin wk wq",
             "attention_fwd_qkv": "qkv", "attention_fwd_qkv[f32]": "qkv", "attention_bwd_qkv": "do lse o qkv", "swiglu_fwd": "h12",
             "swiglu_bwd": "dhid h12", "gate_bwd": "dxout y", "timestep_embedding": "t", "silu_fwd": "x", "silu_bwd": "dy x",
             "label_embed_fwd": "drop table y", "label_embed_bwd": "dout drop y", "random_masking": "noise",
             "patch_embed_kept": "bias ids_keep img pos w2d", "latent_prologue": "lat_mean lat_std moments noise",
             "fm_valid_plan": "lat_mean lat_std stored", "row_mse": "a u", "guidance_combine": "neg pos", "guidance_combine[apg]": "neg pos x",
             "gather_rows": "ids x", "scatter_rows": "dout ids", "restore_tokens": "ids_restore mask_token pos x",
             "restore_tokens_bwd": "dout ids_restore", "vmae_encoder_fwd": "x", "vmae_encoder_fwd_tiled": "x", "heads_split": "qkv",
             "heads_merge": "dk dq dv", "conv3x3": "b w x", "conv3x3_bwd": "dout w x", "mae_loss_fwd": "imgs mask pred_img",
             "mae_loss_bwd": "coef imgs mask pred_img", "layernorm_fwd": "b w x", "layernorm_bwd": "dout mean rstd w x",
             "layernorm_bwd[cast]": "dout mean rstd w x", "gelu_bwd": "dout pre", "gelu_tanh_fwd": "x", "gelu_tanh_bwd": "dout pre"},
    CONVERTED: {"timestep_embedding": "t", "patch_embed_kept": "img", "latent_prologue": "lat_mean lat_std moments noise", "vmae_encoder_fwd": "x",
                "vmae_encoder_fwd_tiled": "x"},
    # flat operands: residual streams and tables of the GEMM epilogues, packed qkv / o / do of the attention, optimizer and snapshot slabs,
    # pointwise inputs, the weight blob; lat_mean / lat_std are flattened by the wrapper; rope takes t [..., N, hd] with any leading dimensions
    FLAT: {"gemm_nt_gate_res": "xin xout", "gemm_nt_pos": "pos", "gemm_nt_gelu_bwd": "pre", "gemm_nt_gate_res_mx8": "xin xout",
           "gemm_nt_swiglu_bwd": "h12", "gemm_nt_swiglu_bwd[bf16]": "h12", "cast": "x", "thin_nt": "pos", "multi_add_": "dst0 dst1 src0 src1",
           "cast_stack": "t0 t1", "cached_stack_copy": "t0 t1", "qknorm_rope_fwd": "qkv", "qknorm_rope_bwd": "qkv",
           "qknorm_rope_bwd[dv=None]": "dqkv qkv", "rope": "t", "attention_bwd": "do o", "attention_fwd_pv": "qkv",
           "attention_fwd_pv[bound]": "bound qkv", "attention_bwd_pv": "do o qkv", "attention_bwd_pv_qknorm": "do o qkv", "attention_fwd_qkv": "qkv",
           "attention_fwd_qkv[f32]": "qkv", "attention_bwd_qkv": "do o qkv", "silu_fwd": "x", "adamw_ema": "ema g m p v", "ema_only": "ema p",
           "adamw_ema_tracks": "ema g m p track v", "ema_tracks_only": "p track", "snapshot_accumulate": "acc x", "snapshot_finish": "acc out",
           "latent_prologue": "lat_mean lat_std", "fm_valid_plan": "lat_mean lat_std", "row_mse": "out", "vmae_encoder_fwd": "blob",
           "vmae_encoder_fwd_tiled": "blob", "heads_split": "qkv", "gelu_tanh_fwd": "x", "lars_norms": "g p", "lars_step": "g mu p"},
    # f32 <-> f16: colsum, cast, layernorm_bwd and token_mean have kernels for all three float types; attention_fwd_qkv at head_dim 16 too
    DISPATCH: {"colsum": "x", "cast": "x", "attention_fwd_qkv": "qkv", "attention_fwd_qkv[f32]": "qkv", "layernorm_bwd": "dout",
               "layernorm_bwd[cast]": "dout", "token_mean": "x"},
    # the doubled last dimension is K, D, W, the token count, the kept-token count or the blob length, and the row passes nothing else that
    # states it (where a weight, a bias, a second operand or an output does, the same defect is refused)
    EXTENT: {"mx8_quantize": "x", "cast_weight": "w", "cast": "x", "thin_tn": "g t", "swiglu_fwd": "h12", "timestep_embedding": "t", "silu_fwd": "x",
             "label_embed_fwd": "table", "label_embed_bwd": "dout", "cached_weight_copy": "w", "cached_weight_mx8": "w", "random_masking": "noise",
             "patch_embed_kept": "ids_keep", "fm_valid_plan": "stored", "crop_resize_flip": "blob", "gather_rows": "ids x", "scatter_rows": "dout",
             "restore_tokens_bwd": "dout", "conv3x3": "x", "gelu_tanh_fwd": "x", "token_mean": "x", "softmax_xent": "logits", "l2_normalize": "x",
             "topk_merge": "sims"},
}
_DEFECT_OF = {COPIED: "strided", CONVERTED: "dtype", FLAT: "dim", DISPATCH: "dtype", EXTENT: "shape"}
ALLOWED_ON = {}      # op -> {"argument.defect": reason}
for _why, _ops in _ALLOWED.items():
    for _op, _names in _ops.items():
        ALLOWED_ON.setdefault(_op, {}).update({f"{n}.{_DEFECT_OF[_why]}": _why for n in _names.split()})
# what each wrapper of the training path WRITES in place: no dtype, strided or shape defect on one of these may go on
OUTPUTS = {"gemm_nt": "out", "gemm_nt_gate_res": "xout", "gemm_nt_mx8": "out", "gemm_nt_gate_res_mx8": "xout", "gemm_tn": "out dbias_out",
           "colsum": "out", "multi_add_": "dst0 dst1", "rmsnorm_modulate_bwd": "dx_accum dshift dscale", "rmsnorm_modulate_bwd_gate": "dx_accum dshift dscale dgate",
           "qknorm_rope_bwd": "dqkv", "gate_bwd": "dgate", "adamw_ema": "p g m v ema", "ema_only": "ema", "adamw_ema_tracks": "p g m v ema track",
           "ema_tracks_only": "track", "snapshot_accumulate": "acc", "snapshot_finish": "out", "row_mse": "out", "guidance_combine": "out mom",
           "crop_resize_flip": "out", "layernorm_bwd": "dx_accum", "bn1d_fwd": "run_mean run_var out", "lars_norms": "out", "lars_step": "p mu",
           "topk_merge": "vals idx"}


def defective(t, defect):
    """t with one defect, or None where the defect cannot be built (a one-element tensor has no non-contiguous view)."""
    if defect == "dtype":
        return t.to(F16 if t.dtype == F32 else F32)
    if defect == "dim":
        return t.unsqueeze(0)
    if defect == "strided":
        v = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype)[..., ::2]
        return None if v.is_contiguous() else v
    return torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype)


def outcome(op, call, args):
    from ldmae_amd import ops
    try:
        call(ops, args)
    except Exception as e:                                     # noqa: BLE001 -- the classification is the point
        return "refused" if str(e).startswith(PREFIX.get(op.split("[")[0], (op.split("[")[0],))) else "on"
    return "returned"


def characterise(op):
    make, call = ROWS[op]
    got = {}
    for name in make():
        for defect in DEFECTS:
            args = make()
            args[name] = defective(args[name], defect)
            if args[name] is not None:
                got[f"{name}.{defect}"] = outcome(op, call, args)
    return got


def test_every_public_wrapper_of_ops_has_a_row():
    from ldmae_amd import ops
    src = open(ops.__file__.replace(".pyc", ".py")).read()
    names = [ln[4:ln.index("(")] for ln in src.splitlines() if ln.startswith("def ") and ln[4] != "_"]
    assert names[0] == "stream" and names[-1] == "sde_combine"
    assert sorted(names) == sorted({op.split("[")[0] for op in ROWS} | set(NO_TENSOR_ARGS))
    assert not {op.split("[")[0] for op in ROWS} & set(NO_TENSOR_ARGS)
    first = names[:names.index("conv2d_nhwc")]
    assert {op.split("[")[0] for op in FIRST_HALF} == set(first) - set(NO_TENSOR_ARGS)
    for name in NO_TENSOR_ARGS:                                # a name listed here that does hand an argument to the library belongs in ROWS
        fn = getattr(ops, name)
        params = "|".join(inspect.signature(fn).parameters) or "$^"
        assert not re.search(rf"(?<![\w.])ptr\(\s*(?:{params})\b", inspect.getsource(fn)), name


@pytest.mark.parametrize("op", list(ROWS))
def test_argument_checks(op):
    make, call = ROWS[op]
    assert outcome(op, call, make()) == "on", "the well-formed call must pass every check and stop only at the device"
    with open(GOLDEN) as f:
        want = json.load(f)[op]
    got = characterise(op)
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}


@pytest.mark.parametrize("op", FIRST_HALF)
def test_every_on_of_the_training_path_is_allowed(op):
    """What goes on with a damaged tensor is exactly what ALLOWED_ON names -- no more (an unexplained way to the device) and no less (a stale
    entry); and the reasons respect their rules: a shape defect only where the tensor itself sets the extent, nothing at all on an output."""
    on = {k for k, v in characterise(op).items() if v != "refused"}
    assert on == set(ALLOWED_ON.get(op, {})), (sorted(on - set(ALLOWED_ON.get(op, {}))), sorted(set(ALLOWED_ON.get(op, {})) - on))
    for key in ALLOWED_ON.get(op, {}):
        arg, defect = key.split(".")
        assert defect == "dim" or arg not in OUTPUTS.get(op.split("[")[0], "").split(), (op, key, "an output of another type or layout must be refused")


if __name__ == "__main__":                                     # regenerate the fixture: python tests/test_ops_args_cpu.py
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        json.dump({op: characterise(op) for op in ROWS}, f, indent=1, sort_keys=True)
        f.write("\n")
