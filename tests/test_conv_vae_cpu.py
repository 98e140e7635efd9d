"""The convolutional KL-VAE tokenizers without a GPU: the diffusers <-> LDM key table, the loader's reports, the posterior's closed forms, the
image transform, the C ABI's declarations, and the drivers' standing refusals of the SD-VAE model types."""
import math
import os
import re

import numpy as np
import pytest
import torch

from convvae_weights import CASE_A, CASE_A_DIFFUSERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vae(**over):
    from ldmae_amd.tokenizer.sdvae import Diffusers_AutoencoderKL
    return Diffusers_AutoencoderKL(**{**CASE_A_DIFFUSERS, **over})


# ---------------------------------------------------------------------------------------------------- key table
@pytest.mark.parametrize("old_attention", [False, True])
def test_key_table_is_a_bijection(old_attention):
    from ldmae_amd.tokenizer import sdvae
    from ldmae_amd.tokenizer.autoencoder import Decoder, Encoder
    ldm = {}
    for half, mod in (("encoder", Encoder(double_z=True, **CASE_A)), ("decoder", Decoder(**CASE_A))):
        ldm.update({f"{half}.{k}": v for k, v in mod.state_dict().items()})
    there = {k: sdvae.ldm_to_diffusers_key(k, 4, old_attention) for k in ldm}
    assert None not in there.values() and len(set(there.values())) == len(ldm)                   # total and one to one
    assert all(sdvae.diffusers_to_ldm_key(d, 4) == k for k, d in there.items())                  # and back
    names = set(there.values())
    spelled = ("query", "key", "value", "proj_attn") if old_attention else ("to_q", "to_k", "to_v", "to_out.0")
    for n in spelled:
        assert f"encoder.mid_block.attentions.0.{n}.weight" in names and f"decoder.mid_block.attentions.0.{n}.bias" in names
    for k in ("encoder.down_blocks.1.resnets.0.conv_shortcut.weight", "encoder.down_blocks.2.downsamplers.0.conv.bias",
              "decoder.up_blocks.2.upsamplers.0.conv.weight", "decoder.up_blocks.3.resnets.0.conv_shortcut.weight",
              "decoder.mid_block.resnets.1.norm2.weight", "encoder.conv_norm_out.bias", "decoder.conv_in.weight"):
        assert k in names, k
    assert there["decoder.up.3.upsample.conv.weight"] == "decoder.up_blocks.0.upsamplers.0.conv.weight"      # levels count from the other end
    assert there["decoder.up.0.block.2.conv1.weight"] == "decoder.up_blocks.3.resnets.2.conv1.weight"
    # the module's own state dict speaks the same names, with the attention projections as Linear [C, C]
    vae = _vae()
    sd = vae.state_dict(old_attention=old_attention)
    assert set(sd) == names
    q = "encoder.mid_block.attentions.0." + spelled[0] + ".weight"
    assert sd[q].shape == (128, 128) and ldm["encoder.mid.attn_1.q.weight"].shape == (128, 128, 1, 1)
    # Linear -> 1x1 conv -> Linear round trip through load_state_dict
    new = {k: torch.randn(v.shape, generator=torch.Generator().manual_seed(i)) for i, (k, v) in enumerate(sd.items())}
    msg = vae.load_state_dict(new)
    assert not msg.missing_keys and not msg.unexpected_keys
    back = vae.state_dict(old_attention=old_attention)
    assert all(torch.equal(back[k], new[k]) for k in new)
    assert torch.equal(vae.encoder.mid.attn_1.q.weight.detach()[:, :, 0, 0], new[q])


def test_unknown_kwargs_and_block_types_are_refused_by_name():
    with pytest.raises(TypeError, match="mid_block_add_attention"):
        _vae(mid_block_add_attention=False)
    with pytest.raises(NotImplementedError, match="AttnDownEncoderBlock2D"):
        _vae(down_block_types=("DownEncoderBlock2D", "AttnDownEncoderBlock2D", "DownEncoderBlock2D", "DownEncoderBlock2D"))
    with pytest.raises(NotImplementedError, match="AttnUpDecoderBlock2D"):
        _vae(up_block_types=("AttnUpDecoderBlock2D",) * 4)
    with pytest.raises(NotImplementedError, match="'gelu'"):
        _vae(act_fn="gelu")
    with pytest.raises(NotImplementedError, match="norm_num_groups 16"):
        _vae(norm_num_groups=16)


def test_loader_reports_missing_and_unexpected_and_raises_on_no_match(capsys):
    vae = _vae()
    sd = vae.state_dict()
    del sd["decoder.conv_out.bias"]
    sd["loss.discriminator.main.0.weight"] = torch.zeros(1)
    sd["encoder.down_blocks.9.resnets.0.conv1.weight"] = torch.zeros(1)
    msg = vae.load_state_dict(sd, strict=False)
    assert msg.missing_keys == ["decoder.conv_out.bias"]
    assert sorted(msg.unexpected_keys) == ["encoder.down_blocks.9.resnets.0.conv1.weight", "loss.discriminator.main.0.weight"]
    out = capsys.readouterr().out
    assert "decoder.conv_out.bias" in out and "loss.discriminator.main.0.weight" in out
    with pytest.raises(RuntimeError, match="decoder.conv_out.bias"):
        vae.load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError, match="none of the 2 keys"):
        vae.load_state_dict({"model.diffusion_model.x": torch.zeros(1), "quant_conv.weight": torch.zeros(1)}, strict=False)


def test_quant_convs_follow_the_flags():
    assert _vae().quant_conv is None and _vae().post_quant_conv is None
    v = _vae(use_quant_conv=True, use_post_quant_conv=True)
    assert v.quant_conv.weight.shape == (32, 32, 1, 1) and v.post_quant_conv.weight.shape == (16, 16, 1, 1)
    assert "quant_conv.weight" in v.state_dict() and "post_quant_conv.bias" in v.state_dict()


def test_autoencoderkl_state_dict_keys_are_the_references():
    from ldmae_amd.tokenizer.autoencoder import AutoencoderKL
    m = AutoencoderKL(embed_dim=8, ch_mult=(1, 1, 2, 2, 4), ch=32, resolution=64)
    sd = m.state_dict()
    for k, shape in (("encoder.down.1.block.0.norm1.weight", (32,)), ("encoder.down.2.block.0.nin_shortcut.weight", (64, 32, 1, 1)),
                     ("decoder.up.3.upsample.conv.weight", (64, 64, 3, 3)), ("encoder.mid.attn_1.q.weight", (128, 128, 1, 1)),
                     ("decoder.up.2.attn.2.proj_out.bias", (64,)), ("encoder.down.2.attn.1.k.weight", (64, 64, 1, 1)),
                     ("quant_conv.weight", (16, 16, 1, 1)), ("post_quant_conv.weight", (8, 8, 1, 1))):
        assert tuple(sd[k].shape) == shape, k
    mar = AutoencoderKL(embed_dim=8, ch_mult=(1, 1, 2, 2, 4), ch=32, resolution=64, model_type="marvae", use_variational=False)
    assert not any(".attn." in k for k in mar.decoder.state_dict()) and any(".attn." in k for k in mar.encoder.state_dict())
    assert mar.quant_conv.weight.shape == (8, 16, 1, 1)
    for call in (lambda: m(torch.zeros(1, 3, 64, 64)), lambda: m.training_step(torch.zeros(1, 3, 64, 64), 0)):
        with pytest.raises(NotImplementedError, match="training"):
            call()
    with pytest.raises(FileNotFoundError, match="nothing is downloaded"):
        AutoencoderKL(embed_dim=8, ch_mult=(1,), ckpt_path="/nonexistent/vavae.pt")
    with pytest.raises(RuntimeError, match="HIP device"):                  # no CPU fallback
        m.encode(torch.zeros(1, 3, 64, 64))


# ---------------------------------------------------------------------------------------------------- posterior
def test_diagonal_gaussian_closed_forms():
    from ldmae_amd.tokenizer.autoencoder import DiagonalGaussianDistribution
    g = torch.Generator().manual_seed(0)
    mean = torch.randn(2, 4, 3, 3, generator=g, dtype=torch.float64)
    logvar = torch.randn(2, 4, 3, 3, generator=g, dtype=torch.float64) * 3
    logvar[0, 0, 0, 0], logvar[1, 1, 1, 1] = -100.0, 50.0
    d = DiagonalGaussianDistribution(torch.cat([mean, logvar], 1))
    lv = logvar.clamp(-30.0, 20.0)
    assert d.logvar[0, 0, 0, 0] == -30.0 and d.logvar[1, 1, 1, 1] == 20.0
    assert torch.equal(d.mode(), mean)
    assert torch.allclose(d.std, (0.5 * lv).exp(), rtol=1e-14) and torch.allclose(d.var, lv.exp(), rtol=1e-14)
    z = d.sample(generator=torch.Generator().manual_seed(7))
    noise = torch.randn(mean.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    assert torch.allclose(z, mean + (0.5 * lv).exp() * noise, rtol=1e-14)
    torch.manual_seed(3)
    z = d.sample()
    torch.manual_seed(3)
    assert torch.equal(z, d.mean + d.std * torch.randn(mean.shape, dtype=torch.float64))
    kl = 0.5 * (mean ** 2 + lv.exp() - 1.0 - lv).flatten(1).sum(1)
    assert torch.allclose(d.kl(), kl, rtol=1e-13)
    assert torch.allclose(d.kl(d), torch.zeros(2, dtype=torch.float64), atol=1e-9)
    unit = DiagonalGaussianDistribution(torch.zeros(2, 8, 3, 3, dtype=torch.float64))
    assert torch.allclose(d.kl(unit), kl, rtol=1e-13)
    det = DiagonalGaussianDistribution(torch.cat([mean, logvar], 1), deterministic=True)
    assert float(det.std.abs().max()) == 0.0 and torch.equal(det.sample(), mean) and float(det.kl()) == 0.0


# ---------------------------------------------------------------------------------------------------- image transform
def test_center_crop_and_img_transform():
    from PIL import Image
    from ldmae_amd.tokenizer.autoencoder import center_crop_arr
    rng = np.random.default_rng(0)
    img = Image.fromarray(rng.integers(0, 256, (300, 500, 3), dtype=np.uint8))           # 300 rows x 500 columns
    out = center_crop_arr(img, 128)
    assert out.size == (128, 128)
    # ADM's recipe by hand: one BOX halving (min side 300 >= 256), bicubic to short side 128, centre crop
    half = img.resize((250, 150), resample=Image.BOX)
    scaled = half.resize((round(250 * 128 / 150), 128), resample=Image.BICUBIC)
    arr = np.array(scaled)
    left = (arr.shape[1] - 128) // 2
    assert arr.shape[:2] == (128, 213) and np.array_equal(np.array(out), arr[:, left:left + 128])
    t = _vae(img_size=128).img_transform()(img)
    assert t.shape == (3, 128, 128) and t.dtype == torch.float32
    assert torch.equal(t, (torch.from_numpy(np.array(out)).permute(2, 0, 1).float() / 255.0 - 0.5) / 0.5)
    flipped = _vae(img_size=128).img_transform(p_hflip=1.0, img_size=64)(img)
    assert flipped.shape == (3, 64, 64) and torch.equal(flipped, _vae().img_transform(img_size=64)(img).flip(-1))


# ---------------------------------------------------------------------------------------------------- C ABI
def test_abi_symbols_are_declared():
    from ldmae_amd import _lib
    header = open(os.path.join(ROOT, "include", "ldmae_hip.h")).read()
    for name in ("ldmae_groupnorm_stats_nhwc_f32", "ldmae_groupnorm_apply_nhwc_f32", "ldmae_conv3x3_vae_nhwc_f32", "ldmae_conv1x1_res_nhwc_f32",
                 "ldmae_softmax_rows_f32"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
    for mode, val in (("PLAIN", 0), ("NORM_ACT", 1), ("DOWN", 2), ("UP", 3)):
        assert re.search(rf"#define LDMAE_VAE_{mode} {val}\b", header)
    src = open(os.path.join(ROOT, "ldmae_amd", "csrc", "Makefile")).read()
    assert "conv_vae.hip" in src


# ---------------------------------------------------------------------------------------------------- the drivers still refuse these types
@pytest.mark.parametrize("name", ["ae_f8d16", "dae_f8d16", "vae_f8d16", "sdv3_f8d16"])
def test_drivers_still_refuse_sdvae_model_types(name, tmp_path):
    """evaluate_tokenizer (model_type_of and main) and inference.build_vae.  The two refusals that sit behind the choice of a device are
    asserted on the GPU: extract_features.main in test_gpu_conv_vae.py, inference.do_sample in the existing test_gpu_drivers.py."""
    from ldmae_amd import evaluate_tokenizer, inference
    cfg = {"vae": {"model_name": name, "weight_path": "x.pt"}, "data": {"image_size": 256, "data_path": str(tmp_path)}}
    with pytest.raises(NotImplementedError, match="SD-VAE"):
        evaluate_tokenizer.model_type_of(cfg)
    p = tmp_path / "cfg.yaml"
    p.write_text(f"data:\n  data_path: '{tmp_path}'\n  image_size: 256\nvae:\n  model_name: '{name}'\n  weight_path: 'x.pt'\n")
    with pytest.raises(NotImplementedError, match="SD-VAE"):
        evaluate_tokenizer.main(["--config_path", str(p), "--synthetic", "2"])
    with pytest.raises(NotImplementedError, match="VMAE"):
        inference.build_vae(cfg, "cpu")


# ---------------------------------------------------------------------------------------------------- drop-in name resolution
def test_dropin_finder_leaves_the_new_tokenizer_names_to_the_reference(tmp_path):
    """A reference driver's `from tokenizer.sdvae import ...` (and autoencoder / vavae / marvae) keeps resolving to the reference's own files
    under the drop-in finder, although this tree now has modules of those names; mirrored names are still served from here."""
    import subprocess
    import sys
    ref = tmp_path / "LDMAE"
    (ref / "tokenizer").mkdir(parents=True)
    (ref / "tokenizer" / "__init__.py").write_text("WHO = 'reference'\n")
    names = ("autoencoder", "vavae", "marvae", "sdvae")
    for n in names:
        (ref / "tokenizer" / f"{n}.py").write_text(f"WHO = 'reference-{n}'\n")
    code = "import sys, tokenizer\n" + "".join(f"import tokenizer.{n}\nassert tokenizer.{n}.WHO == 'reference-{n}'\n" for n in names) + \
           "from tokenizer import models_mae\nassert models_mae is sys.modules['ldmae_amd.tokenizer.models_mae']\n" \
           "import ldmae_amd.tokenizer.sdvae as ours\nassert hasattr(ours, 'Diffusers_AutoencoderKL') and ours is not sys.modules['tokenizer.sdvae']\nfrom tokenizer.sdvae import WHO\nassert WHO == 'reference-sdvae'\nprint('OK')\n"
    (ref / "driver.py").write_text(code)
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    env["PYTHONPATH"] = os.path.join(ROOT, "ldmae_amd", "dropin")
    r = subprocess.run([sys.executable, "driver.py"], cwd=str(ref), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
