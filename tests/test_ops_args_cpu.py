"""Characterisation of the argument checks of the evaluation / tokenizer / sampler wrappers in ldmae_amd/ops.py (conv2d_nhwc .. sde_combine).

Every row builds a well-formed set of CPU tensors at the smallest legal shape.  Then each tensor argument gets each single defect in turn --
another dtype, one extra leading dimension, a non-contiguous view of the same shape, a last dimension that disagrees with the others -- and the
wrapper either REFUSES with its own message (the text starts with the op's name) or GOES ON towards the device (anything else: on CPU tensors
that is `_lib.ptr`'s "no CPU fallback", or an error of the workspace allocation just before it).  tests/golden/ops_args_outcomes.json holds the
expected outcome of every (op, argument, defect); a refusal must never turn into "on"."""
import json
import os

import pytest
import torch

F16, BF16, F32, F64, U8 = torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.uint8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_args_outcomes.json")
DEFECTS = ("dtype", "dim", "strided", "shape")


def Z(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


def _lpips_bwd(name, dt):
    return (lambda: dict(f=Z(2, 2, 2, 64, dtype=dt), lin_w=Z(64), g=Z(1), d_input=Z(1, 2, 2, 64), d_target=Z(1, 2, 2, 64)),
            lambda o, a: getattr(o, name)(a["f"], a["lin_w"], a["g"], a["d_input"], a["d_target"]))


# op -> (tensors of a well-formed call, the call).  Shapes: the smallest each wrapper accepts.
ROWS = {
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
# a message that opens with one of these is the wrapper's own refusal (two families name their shared contract instead of the op)
PREFIX = {"recon_quantize_sse": ("recon_quantize",), "attention_wide": ("attention_wide", "gemm_nt", "softmax_rows_"),
          **{op: (op, "ode:") for op in ("rk_stage", "dopri5_finish", "dopri5_interp")}}
# public names of that part of ops.py that take no tensor argument: nothing to characterise
NO_TENSOR_ARGS = ("default_col_splits", "ode_slab_ld", "ode_partials", "rademacher")


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
        return "refused" if str(e).startswith(PREFIX.get(op, (op.split("[")[0],))) else "on"
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


def test_every_public_wrapper_of_the_second_half_has_a_row():
    from ldmae_amd import ops
    src = open(ops.__file__.replace(".pyc", ".py")).read()
    names = [ln[4:ln.index("(")] for ln in src[src.index("\ndef conv2d_nhwc("):].splitlines() if ln.startswith("def ") and ln[4] != "_"]
    assert names[0] == "conv2d_nhwc" and names[-1] == "sde_combine"
    assert sorted(names) == sorted({op.split("[")[0] for op in ROWS} | set(NO_TENSOR_ARGS))


@pytest.mark.parametrize("op", list(ROWS))
def test_argument_checks(op):
    make, call = ROWS[op]
    assert outcome(op, call, make()) == "on", "the well-formed call must pass every check and stop only at the device"
    with open(GOLDEN) as f:
        want = json.load(f)[op]
    got = characterise(op)
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}


if __name__ == "__main__":                                     # regenerate the fixture: python tests/test_ops_args_cpu.py
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(GOLDEN, "w") as f:
        json.dump({op: characterise(op) for op in ROWS}, f, indent=1, sort_keys=True)
        f.write("\n")
