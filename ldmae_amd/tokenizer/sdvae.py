"""``Diffusers_AutoencoderKL`` on the HIP kernels -- counterpart of the reference's ``tokenizer/sdvae.py``, which subclasses diffusers'
``AutoencoderKL``.  The keyword set of the reference's drivers (inference.py:139-163) is mapped to this package's LDM ``Encoder`` /
``Decoder`` (tokenizer/autoencoder.py): the architectures are the same network under two naming schemes.  The state dict speaks diffusers'
key names, so ``load_state_dict(checkpoint['model'])`` takes the checkpoints the reference loads; ``KEY_TABLE`` is the whole translation.
The math is the LDM module's: GroupNorm eps 1e-6, a single attention head in the middle block, output scale 1.

diffusers is not a dependency and was not available to check the table against; it follows the library's public key names (both attention
spellings) and is tested as a bijection on this module's own parameters.
"""
from __future__ import annotations

import re
from collections import OrderedDict
from types import SimpleNamespace

import torch
import torch.nn as nn

from .autoencoder import Decoder, DiagonalGaussianDistribution, Encoder, ImgTransform, _conv1x1, _nhwc_in, center_crop_arr, images_uint8  # noqa: F401

# diffusers prefix -> LDM prefix inside "encoder." / "decoder.".  {i}, {j}: indices kept; {r}: the level counted from the other end
# (up_blocks.r is up.(L-1-r)).
KEY_TABLE = (
    ("down_blocks.{i}.resnets.{j}.", "down.{i}.block.{j}."),
    ("down_blocks.{i}.downsamplers.0.conv.", "down.{i}.downsample.conv."),
    ("mid_block.resnets.0.", "mid.block_1."),
    ("mid_block.resnets.1.", "mid.block_2."),
    ("mid_block.attentions.0.group_norm.", "mid.attn_1.norm."),
    ("mid_block.attentions.0.to_q.", "mid.attn_1.q."),
    ("mid_block.attentions.0.to_k.", "mid.attn_1.k."),
    ("mid_block.attentions.0.to_v.", "mid.attn_1.v."),
    ("mid_block.attentions.0.to_out.0.", "mid.attn_1.proj_out."),
    ("up_blocks.{r}.resnets.{j}.", "up.{i}.block.{j}."),
    ("up_blocks.{r}.upsamplers.0.conv.", "up.{i}.upsample.conv."),
    ("conv_norm_out.", "norm_out."),
)
# inside a resnet: the 1x1 shortcut
LEAF_TABLE = (("conv_shortcut.", "nin_shortcut."),)
# the older spelling of the attention block's Linears (diffusers before the Attention class): old -> current
OLD_ATTENTION = (("query.", "to_q."), ("key.", "to_k."), ("value.", "to_v."), ("proj_attn.", "to_out.0."))
ATTN = "mid_block.attentions.0."
# Linear [C, C] in diffusers, Conv2d [C, C, 1, 1] in the LDM module
LINEAR_AS_CONV = tuple(f"mid.attn_1.{n}.weight" for n in ("q", "k", "v", "proj_out"))

ENCODER_BLOCK, DECODER_BLOCK, ACT_FN = "DownEncoderBlock2D", "UpDecoderBlock2D", "silu"
KWARGS = ("sample_size", "in_channels", "out_channels", "layers_per_block", "latent_channels", "norm_num_groups", "act_fn", "block_out_channels",
          "force_upcast", "use_quant_conv", "use_post_quant_conv", "down_block_types", "up_block_types", "scaling_factor")


def _compile(pattern):
    return re.compile("^" + re.sub(r"\\\{[ijr]\\\}", lambda m: f"(?P<{m.group(0)[2]}>\\d+)", re.escape(pattern)))


def _translate(rest, levels, src, dst):
    """Rewrite the head of `rest` by the first KEY_TABLE row whose column `src` matches; None when no row does."""
    for row in KEY_TABLE:
        m = _compile(row[src]).match(rest)
        if m is None:
            continue
        idx = {k: int(v) for k, v in m.groupdict().items()}
        if "r" in idx:
            idx["i"] = levels - 1 - idx["r"]
        elif "{r}" in row[dst]:
            idx["r"] = levels - 1 - idx["i"]
        tail = rest[m.end():]
        for leaf in LEAF_TABLE:
            if tail.startswith(leaf[src]):
                tail = leaf[dst] + tail[len(leaf[src]):]
        return row[dst].format(**idx) + tail
    return None


def diffusers_to_ldm_key(key, levels):
    """The LDM name of a diffusers key (either attention spelling), or None for a key this model has no place for."""
    top, _, rest = key.partition(".")
    if top in ("quant_conv", "post_quant_conv"):
        return key
    if top not in ("encoder", "decoder"):
        return None
    if rest.startswith(ATTN):
        for old, new in OLD_ATTENTION:
            if rest.startswith(ATTN + old):
                rest = ATTN + new + rest[len(ATTN + old):]
    if rest.startswith(("conv_in.", "conv_out.")):
        return key
    out = _translate(rest, levels, 0, 1)
    return None if out is None else f"{top}.{out}"


def ldm_to_diffusers_key(key, levels, old_attention=False):
    top, _, rest = key.partition(".")
    if top in ("quant_conv", "post_quant_conv") or rest.startswith(("conv_in.", "conv_out.")):
        return key
    out = _translate(rest, levels, 1, 0)
    if out is None:
        return None
    if old_attention and out.startswith(ATTN):
        for old, new in OLD_ATTENTION:
            if out.startswith(ATTN + new):
                out = ATTN + old + out[len(ATTN + new):]
    return f"{top}.{out}"


class Diffusers_AutoencoderKL(nn.Module):
    def __init__(self, img_size=256, **kwargs):
        super().__init__()
        unknown = sorted(set(kwargs) - set(KWARGS))
        if unknown:
            raise TypeError(f"Diffusers_AutoencoderKL: unsupported keyword(s) {unknown}; supported: {list(KWARGS)}")
        boc = tuple(kwargs.get("block_out_channels", (64,)))
        down = tuple(kwargs.get("down_block_types", (ENCODER_BLOCK,) * len(boc)))
        up = tuple(kwargs.get("up_block_types", (DECODER_BLOCK,) * len(boc)))
        for name, types, want in (("down_block_types", down, ENCODER_BLOCK), ("up_block_types", up, DECODER_BLOCK)):
            bad = sorted({t for t in types if t != want})
            if bad:
                raise NotImplementedError(f"Diffusers_AutoencoderKL: {name} {bad} not built; only {want!r} is")
            if len(types) != len(boc):
                raise ValueError(f"Diffusers_AutoencoderKL: {len(types)} {name} for {len(boc)} block_out_channels")
        act_fn = kwargs.get("act_fn", ACT_FN)
        if act_fn != ACT_FN:
            raise NotImplementedError(f"Diffusers_AutoencoderKL: act_fn {act_fn!r} not built; only {ACT_FN!r} is")
        if kwargs.get("norm_num_groups", 32) != 32:
            raise NotImplementedError(f"Diffusers_AutoencoderKL: norm_num_groups {kwargs['norm_num_groups']} not built; only 32 is")
        ch = boc[0]
        if any(c % ch for c in boc):
            raise NotImplementedError(f"Diffusers_AutoencoderKL: block_out_channels {boc} are not multiples of the first")
        ch_mult = tuple(c // ch for c in boc)
        z = kwargs.get("latent_channels", 4)
        common = dict(ch=ch, ch_mult=ch_mult, num_res_blocks=kwargs.get("layers_per_block", 1), attn_resolutions=(), resolution=img_size,
                      z_channels=z, in_channels=kwargs.get("in_channels", 3))
        self.img_size = img_size
        self.levels = len(boc)
        self.latent_channels = z
        self.scaling_factor = kwargs.get("scaling_factor", 0.18215)
        self.encoder = Encoder(double_z=True, **common)
        self.decoder = Decoder(out_ch=kwargs.get("out_channels", 3), **common)
        self.quant_conv = nn.Conv2d(2 * z, 2 * z, 1) if kwargs.get("use_quant_conv", True) else None
        self.post_quant_conv = nn.Conv2d(z, z, 1) if kwargs.get("use_post_quant_conv", True) else None

    # ------------------------------------------------------------------ state dict in diffusers' names
    def state_dict(self, *args, destination=None, prefix="", keep_vars=False, old_attention=False):
        """diffusers' key names (old_attention=True: the older query / key / value / proj_attn spelling).  `destination` and `prefix` are
        honoured, so the keys also appear, renamed, in the state dict of a module that holds this one.  LOADING through a parent goes by
        nn.Module's own per-submodule routine and expects the LDM names: load checkpoints with this class's load_state_dict."""
        if args:                                                # the deprecated positional form (destination, prefix, keep_vars)
            destination, prefix, keep_vars = (list(args) + [prefix, keep_vars][len(args) - 1:])[:3]
        out = OrderedDict() if destination is None else destination
        for k, v in super().state_dict(prefix="", keep_vars=keep_vars).items():
            if k.partition(".")[2] in LINEAR_AS_CONV:
                v = v.reshape(v.shape[0], v.shape[1])
            out[prefix + ldm_to_diffusers_key(k, self.levels, old_attention)] = v
        return out

    def load_state_dict(self, state_dict, strict=True, assign=False):
        own = super().state_dict()
        sd, unexpected, matched = {}, [], 0
        for k, v in state_dict.items():
            lk = diffusers_to_ldm_key(k, self.levels)
            if lk is None or lk not in own:
                unexpected.append(k)
                continue
            if lk.partition(".")[2] in LINEAR_AS_CONV and v.dim() == 2:
                v = v.reshape(v.shape[0], v.shape[1], 1, 1)
            sd[lk] = v
            matched += lk.startswith(("encoder.", "decoder."))
        if matched == 0:
            raise RuntimeError(f"Diffusers_AutoencoderKL.load_state_dict: none of the {len(state_dict)} keys names an encoder or decoder parameter of "
                               f"this model (first keys: {list(state_dict)[:3]})")
        missing = [ldm_to_diffusers_key(k, self.levels) for k in own if k not in sd]
        msg = nn.modules.module._IncompatibleKeys(missing, unexpected)
        if strict and (missing or unexpected):
            raise RuntimeError(f"Diffusers_AutoencoderKL.load_state_dict: {msg}")
        super().load_state_dict(sd, strict=False)
        print(msg)
        return msg

    @property
    def precision(self):
        return self.encoder.precision

    def set_precision(self, precision):
        """"f32" (default) or "tf32": Encoder.set_precision on both halves (tokenizer/autoencoder.py); the quant convolutions stay f32."""
        self.encoder.set_precision(precision)
        self.decoder.set_precision(precision)
        return self

    # ------------------------------------------------------------------ diffusers' interface, as far as the reference uses it
    def encode(self, x, return_dict=True):
        with torch.no_grad():
            h = self.encoder.forward_nhwc(_nhwc_in(x, self.encoder.conv_in.weight))
            if self.quant_conv is not None:
                h = _conv1x1(self.quant_conv, h)
            posterior = DiagonalGaussianDistribution(h.permute(0, 3, 1, 2).contiguous())
        return SimpleNamespace(latent_dist=posterior) if return_dict else (posterior,)

    def decode(self, z, return_dict=True):
        with torch.no_grad():
            z = _nhwc_in(z, self.decoder.conv_in.weight)
            if self.post_quant_conv is not None:
                z = _conv1x1(self.post_quant_conv, z)
            dec = self.decoder.forward_nhwc(z).permute(0, 3, 1, 2).contiguous()
        return SimpleNamespace(sample=dec) if return_dict else (dec,)

    def forward(self, *args, **kwargs):
        raise NotImplementedError("Diffusers_AutoencoderKL.forward: training these autoencoders is not built here; use encode / decode")

    training_step = forward

    def img_transform(self, p_hflip=0, img_size=None):
        return ImgTransform(img_size if img_size is not None else self.img_size, p_hflip)

    def encode_images(self, images):
        return self.encode(images, return_dict=False)[0].mode()

    def decode_to_images(self, z):
        return images_uint8(self.decode(z, return_dict=False)[0])
