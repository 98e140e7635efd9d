"""The opt-in 16-bit LPIPS path (models/lpips.py precision="fp16"), the parts that need no GPU: the precision argument, the fp16 weight packs and the
bf16 rotated weights, the C ABI's declarations, and the drivers' flag."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ldmae_lpips_prep_f16", "ldmae_conv3x3_relu_nhwc_f16", "ldmae_maxpool2x2_nhwc_f16", "ldmae_lpips_layer_f16",
               "ldmae_conv3x3_relu_dgrad_nhwc_bf16", "ldmae_maxpool2x2_bwd_nhwc_xf16", "ldmae_lpips_layer_bwd_f16", "ldmae_lpips_prep_bwd_c8")
STAGE3 = ["--synthetic", "--tune_decoder", "--perceptual_loss_ratio", "10.0", "--mask_ratio", "0.0"]


@pytest.mark.parametrize("bad", ["int8", "bf16", "FP16", "", None, torch.float16])
def test_unknown_precision_is_a_value_error_before_the_device_check(bad):
    from ldmae_amd.models.lpips import LPIPS, random_state_dict
    with pytest.raises(ValueError, match="precision"):
        LPIPS(state_dict=random_state_dict(0), device="cpu", precision=bad)          # device="cpu" would be a RuntimeError: the value is checked first


def test_precision_is_an_attribute_and_defaults_to_f32(monkeypatch):
    from ldmae_amd.models import lpips as lp
    assert lp.LPIPS.precision == "f32" and lp.PRECISIONS == ("f32", "fp16")
    for p in ("f32", "fp16"):
        with pytest.raises(RuntimeError, match="HIP device"):                        # accepted values get as far as the device check
            lp.LPIPS(state_dict=lp.random_state_dict(0), device="cpu", precision=p)
    m = lp.LPIPS.__new__(lp.LPIPS)
    assert m.precision == "f32"
    # never inferred from autocast state or torch.backends
    monkeypatch.setattr(torch.backends.cudnn, "allow_tf32", True)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert lp.LPIPS.__new__(lp.LPIPS).precision == "f32"


def test_fp16_pack_is_the_f32_pack_rounded_with_conv1_1_padded_to_8():
    from ldmae_amd.models.lpips import CONVS, conv_weights, conv_weights_f16, random_state_dict
    sd = random_state_dict(5)
    f32, f16 = conv_weights(sd), conv_weights_f16(sd)
    assert len(f32) == len(f16) == len(CONVS)
    for j, ((w, b, s), (w16, b16, s16)) in enumerate(zip(f32, f16)):
        assert w16.dtype == torch.float16 and w16.is_contiguous() and b16.dtype == torch.float32 and torch.equal(b16, b) and s16 == s
        if j == 0:
            assert tuple(w.shape) == (64, 3, 3, 4) and tuple(w16.shape) == (64, 3, 3, 8)
            assert torch.equal(w16[..., :4], w.half()) and torch.count_nonzero(w16[..., 3:]) == 0 and torch.count_nonzero(w16[..., :3]) > 0
        else:
            assert w16.shape == w.shape and torch.equal(w16, w.half())
        assert w16.shape[3] % 8 == 0                                                   # every layer meets the fp16 kernel's Cin rule


def test_bf16_rotated_weight_is_the_rotation_rounded_once():
    from ldmae_amd.models.lpips import conv_weights_c8, random_state_dict, rotate_weight, rotate_weight_bf16
    packs = conv_weights_c8(random_state_dict(5))
    for j, (w, _, _) in enumerate(packs):
        r = rotate_weight_bf16(w)
        assert r.dtype == torch.bfloat16 and r.is_contiguous() and torch.equal(r, rotate_weight(w).to(torch.bfloat16))
        assert tuple(r.shape) == (w.shape[3], 3, 3, w.shape[0])
    r0 = rotate_weight_bf16(packs[0][0])
    assert r0.shape[0] == 8 and torch.count_nonzero(r0[3:]) == 0 and torch.count_nonzero(r0[:3]) > 0       # rows 3 .. 7: exactly zero gradients
    # rounded from the f32 weight, not through fp16 (11 -> 8 bits can round twice)
    w = torch.full((8, 3, 3, 8), 1.0 + 2.0 ** -8 + 2.0 ** -12)
    assert float(rotate_weight_bf16(w)[0, 0, 0, 0]) == 1.0 + 2.0 ** -7 and float(w.half().to(torch.bfloat16)[0, 0, 0, 0]) == 1.0


def test_abi_symbols_are_declared_and_exported():
    from ldmae_amd import _lib
    header = open(os.path.join(ROOT, "include", "ldmae_hip.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "ldmae_amd", "libldmae_hip.so"))
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
        assert hasattr(lib, name), name
    assert "v_mfma_f32_16x16x32_bf16" in header and "rounded ONCE to fp16" in header


def test_ops_wrappers_refuse_wrong_dtypes_without_a_device():
    from ldmae_amd import ops
    x32, x16 = torch.zeros(1, 4, 4, 8), torch.zeros(1, 4, 4, 8, dtype=torch.float16)
    w16 = torch.zeros(16, 3, 3, 8, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="float16 NHWC"):
        ops.conv3x3_relu_nhwc_f16(x32, w16)
    with pytest.raises(RuntimeError, match="weight"):
        ops.conv3x3_relu_nhwc_f16(x16, w16.float())
    with pytest.raises(RuntimeError, match="weight"):
        ops.conv3x3_relu_nhwc_f16(x16, torch.zeros(16, 3, 3, 16, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.conv3x3_relu_nhwc_f16(torch.zeros(1, 4, 4, 4, dtype=torch.float16), torch.zeros(16, 3, 3, 4, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="float16 NHWC"):
        ops.maxpool2x2_nhwc_f16(x32)
    with pytest.raises(RuntimeError, match="2 x 2"):
        ops.maxpool2x2_nhwc_f16(torch.zeros(1, 1, 4, 8, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="rotated weight"):
        ops.conv3x3_relu_dgrad_nhwc_bf16(x32, x16, torch.zeros(8, 3, 3, 8))             # an f32 weight
    with pytest.raises(RuntimeError, match="float16 NHWC"):
        ops.conv3x3_relu_dgrad_nhwc_bf16(x32, x32, torch.zeros(8, 3, 3, 8, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match=r"\[B, H, W, 8\]"):
        ops.lpips_prep_bwd_c8(torch.zeros(1, 4, 4, 4))


def _weights(tmp_path):
    vgg, lin = tmp_path / "vgg16-397923af.pth", tmp_path / "vgg.pth"
    torch.save({}, vgg)
    torch.save({}, lin)
    return ["--lpips_vgg", str(vgg), "--lpips_lin", str(lin)]


def test_driver_flag_is_accepted_with_stage3_and_refused_without(tmp_path, capsys):
    from ldmae_amd import vmae_pretrain as vp
    files = _weights(tmp_path)
    args = vp.parse_args(STAGE3 + files + ["--lpips_precision", "fp16"])
    assert args.stage3 and args.lpips_precision == "fp16"
    assert vp.parse_args(STAGE3 + files).lpips_precision == "f32"                     # the default
    assert vp.parse_args(STAGE3 + files + ["--lpips_precision", "f32"]).lpips_precision == "f32"
    for argv in (["--synthetic", "--lpips_precision", "fp16"], ["--synthetic", "--lpips_precision", "f32"],
                 ["--synthetic", "--tune_decoder", "--lpips_precision", "fp16"]):
        with pytest.raises(SystemExit) as e:
            vp.main(argv)
        assert e.value.code == 2
        assert "lpips_precision" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                                              # not a choice
        vp.parse_args(STAGE3 + files + ["--lpips_precision", "bf16"])
    assert e.value.code == 2
    plain = vp.parse_args(["--synthetic"])                                           # stages 1 / 2: untouched
    assert not plain.stage3 and plain.lpips_precision == "f32"


def test_evaluate_tokenizer_parses_the_flag():
    from ldmae_amd.evaluate_tokenizer import build_parser
    ap = build_parser()
    assert ap.parse_args([]).lpips_precision is None                                  # not given: today's output, byte for byte
    assert ap.parse_args(["--lpips_precision", "fp16"]).lpips_precision == "fp16"
    assert ap.parse_args(["--lpips_precision", "f32"]).lpips_precision == "f32"
    with pytest.raises(SystemExit):
        ap.parse_args(["--lpips_precision", "tf32"])


def test_train_ae_passes_lpips_precision(tmp_path):
    import subprocess
    shim = tmp_path / "bin"
    shim.mkdir()
    (shim / "python").write_text('#!/bin/bash\necho "ARGS $@"\n')
    os.chmod(shim / "python", 0o755)
    for env, want in (({}, "--lpips_precision f32"), ({"LPIPS_PRECISION": "fp16"}, "--lpips_precision fp16")):
        r = subprocess.run(["bash", os.path.join(ROOT, "ldmae_amd", "train_ae.sh")], capture_output=True, text=True,
                           env={"PATH": f"{shim}:/usr/bin:/bin", "GPUS_PER_NODE": "1", "DATA_PATH": "/d", "OUT": str(tmp_path / "w"), **env})
        assert r.returncode == 0, r.stderr
        cmds = [l for l in r.stdout.splitlines() if l.startswith("ARGS ")]
        assert len(cmds) == 3 and want in cmds[2] and "lpips_precision" not in cmds[0] and "lpips_precision" not in cmds[1]
