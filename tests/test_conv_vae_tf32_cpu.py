"""The TF32-class mode of the convolutional KL-VAE tokenizers without a GPU: set_precision and its propagation, the Cin % 8 fallback rule, the
fp16 weight-pack cache, the C ABI's declarations, the command line's flag, the host rounding helper and the golden file's keys."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from convvae_weights import CASE_A, CASE_A_DIFFUSERS, CASE_B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ldmae_conv3x3_vae_nhwc_f16", "ldmae_conv1x1_res_nhwc_f16", "ldmae_groupnorm_apply_nhwc_f16out")


def _kernel_modules(m):
    from ldmae_amd.tokenizer.autoencoder import _Kernels
    return [k for k in m.modules() if isinstance(k, _Kernels)]


def test_set_precision_accepts_rejects_and_propagates():
    from ldmae_amd.tokenizer.autoencoder import AutoencoderKL, Decoder, Encoder
    from ldmae_amd.tokenizer.marvae import MAR_VAE
    from ldmae_amd.tokenizer.sdvae import Diffusers_AutoencoderKL
    from ldmae_amd.tokenizer.vavae import VA_VAE
    enc, dec = Encoder(double_z=True, **CASE_A), Decoder(**CASE_A)
    for m in (enc, dec):
        mods = _kernel_modules(m)
        assert len(mods) > 10 and all(k.precision == "f32" for k in mods)
        assert m.set_precision("tf32") is m and all(k.precision == "tf32" for k in mods)
        for bad in ("bf16", "fp16", "TF32", None, torch.float16):
            with pytest.raises(ValueError, match="precision"):
                m.set_precision(bad)
        assert all(k.precision == "tf32" for k in mods)                      # a refused value changes nothing
        m.set_precision("f32")
        assert all(k.precision == "f32" for k in mods)
    kl = AutoencoderKL(**CASE_B)
    sd = Diffusers_AutoencoderKL(**CASE_A_DIFFUSERS)
    va, mar = object.__new__(VA_VAE), object.__new__(MAR_VAE)               # the wrappers' methods; their constructors need a GPU and a checkpoint
    va.model, mar.model = AutoencoderKL(**CASE_B), AutoencoderKL(model_type="marvae", **CASE_B)
    for top, model in ((kl, kl), (sd, sd), (va, va.model), (mar, mar.model)):
        assert model.precision == "f32"
        assert top.set_precision("tf32") is top
        assert model.precision == "tf32" and all(k.precision == "tf32" for k in _kernel_modules(model))
        with pytest.raises(ValueError, match="precision"):
            top.set_precision("half")
        top.set_precision("f32")
        assert all(k.precision == "f32" for k in _kernel_modules(model))


@pytest.mark.parametrize("flag", [True, False])
def test_default_is_f32_whatever_torch_backends_say(flag, monkeypatch):
    from ldmae_amd.tokenizer.autoencoder import AutoencoderKL
    monkeypatch.setattr(torch.backends.cudnn, "allow_tf32", flag)
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = flag
    try:
        m = AutoencoderKL(**CASE_B)
        assert m.precision == "f32" and all(k.precision == "f32" for k in _kernel_modules(m))
    finally:
        torch.backends.cuda.matmul.allow_tf32 = old


def test_cin_fallback_rule():
    from ldmae_amd.tokenizer.autoencoder import Decoder, conv3x3_layers, uses_tf32
    from ldmae_amd.tokenizer.sdvae import Diffusers_AutoencoderKL
    assert not uses_tf32("f32", 128) and uses_tf32("tf32", 128) and uses_tf32("tf32", 8) and uses_tf32("tf32", 16)
    assert not uses_tf32("tf32", 3) and not uses_tf32("tf32", 4) and not uses_tf32("tf32", 12)
    with pytest.raises(ValueError, match="precision"):
        uses_tf32("bf16", 128)
    with torch.device("meta"):                                               # shapes only: the drivers' configuration
        vae = Diffusers_AutoencoderKL(img_size=256, layers_per_block=2, latent_channels=16, block_out_channels=(128, 256, 512, 512),
                                      use_quant_conv=False, use_post_quant_conv=False)
        sd1 = Decoder(ch=128, ch_mult=(1, 2, 4, 4), num_res_blocks=2, attn_resolutions=(), resolution=256, z_channels=4)
    layers = conv3x3_layers(vae)
    f32 = [n for n, cin, _ in layers if not uses_tf32("tf32", cin)]
    assert f32 == ["encoder.conv_in"]                                        # the 3-channel image convolution; the 16-channel latent conv_in is covered
    names = [n for n, _, _ in layers]
    for n in ("decoder.conv_in", "decoder.conv_out", "encoder.conv_out", "encoder.down.0.downsample.conv", "decoder.up.1.upsample.conv",
              "encoder.mid.attn_1.proj_out", "decoder.up.3.block.0.conv1"):
        assert n in names, n
    assert not any(n.endswith(("nin_shortcut", ".q", ".k", ".v", "quant_conv")) for n in names)      # these stay f32 in every mode
    assert [n for n, cin, _ in conv3x3_layers(sd1) if not uses_tf32("tf32", cin)] == ["conv_in"]      # the 4-channel latent of SD-1.x shapes


def test_f16_pack_cache_follows_the_weight(monkeypatch):
    from ldmae_amd import ops
    from ldmae_amd.tokenizer import autoencoder as ae
    calls = []

    def cast(t, dtype):                                                      # ops.cast needs a device; the cache logic does not
        calls.append(dtype)
        return t.to(dtype)

    monkeypatch.setattr(ops, "cast", cast)
    conv = torch.nn.Conv2d(8, 16, 3)
    a = ae._packed_f16(conv)
    assert a.dtype == torch.float16 and tuple(a.shape) == (16, 3, 3, 8) and torch.equal(a, conv.weight.detach().permute(0, 2, 3, 1).half())
    assert ae._packed_f16(conv) is a and len(calls) == 1
    assert conv.__dict__["_ldmae_pack_f16"][0] == conv.__dict__["_ldmae_pack"][0] == ae._pack_key(conv.weight)
    with torch.no_grad():
        conv.weight.mul_(2.0)                                                # an in-place write: the key's version moves
    b = ae._packed_f16(conv)
    assert b is not a and len(calls) == 2 and torch.equal(b, conv.weight.detach().permute(0, 2, 3, 1).half())
    conv.load_state_dict({"weight": torch.ones(16, 8, 3, 3), "bias": torch.zeros(16)})
    assert float(ae._packed_f16(conv).min()) == 1.0 and float(ae._packed(conv).min()) == 1.0 and len(calls) == 3


def test_abi_symbols_are_declared_and_exported():
    from ldmae_amd import _lib
    header = open(os.path.join(ROOT, "include", "ldmae_hip.h")).read()
    lib = ctypes.CDLL(os.path.join(ROOT, "ldmae_amd", "libldmae_hip.so"))
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
        assert hasattr(lib, name), name
    assert "saturating at +-65504" in header and "accumulated in f32" in header


def test_cli_parses_precision():
    from ldmae_amd.evaluate_conv_tokenizer import build_parser
    ap = build_parser()
    assert ap.parse_args(["--family", "sdvae"]).precision == "f32"
    assert ap.parse_args(["--family", "vavae", "--precision", "tf32"]).precision == "tf32"
    with pytest.raises(SystemExit):
        ap.parse_args(["--family", "sdvae", "--precision", "bf16"])


def test_host_rounding_helper_saturates():
    from make_golden_convvae_tf32 import round_f16
    x = torch.tensor([1e5, -1e5, 65504.0, 65519.0, 65520.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -26, float("inf")], dtype=torch.float64)
    want = torch.tensor([65504.0, -65504.0, 65504.0, 65504.0, 65504.0, 1.0, 1.0 + 2.0 ** -9, 0.0, 65504.0], dtype=torch.float64)
    got = round_f16(x)
    assert got.dtype == torch.float64 and torch.equal(got, want)             # ties to even; beyond the range: the largest finite value
    assert bool(torch.isnan(round_f16(torch.tensor([float("nan")]))).all())
    assert round_f16(torch.tensor([0.1], dtype=torch.float32)).dtype == torch.float32


def test_golden_file_has_an_error_for_every_output(golden):
    base, tf32 = golden("convvae"), golden("convvae_tf32")
    keys = sorted(k[len("e_ref_"):] for k in base.files if k.startswith("e_ref_"))
    assert keys and sorted(tf32.files) == ["e_tf32_" + k for k in keys]          # those scalars and nothing else
    for k in keys:
        e = float(tf32["e_tf32_" + k])
        assert tf32["e_tf32_" + k].shape == () and 10 * 2.0 ** -11 > e > float(base["e_ref_" + k])   # fp16-rounding sized: above f32's error
