"""The LDM convolutional KL autoencoder on the HIP kernels -- counterpart of the reference's ``tokenizer/autoencoder.py``: ``Encoder``,
``Decoder``, ``DiagonalGaussianDistribution``, ``AutoencoderKL`` and ``center_crop_arr``, forward only.  The posterior class is the package's
own (tokenizer/util/misc.py: the same clamp, ``mode``, ``kl`` and ``nll``; ``sample`` draws its noise on the tensor's device, from the global
generator or the one given, where the reference draws on the host and copies).

Constructor arguments, parameter names and state-dict keys are the reference's, so its checkpoints load with ``load_state_dict``.  Parameters
are held by ``nn.Conv2d`` / ``nn.GroupNorm`` objects in the reference's layout; those objects are containers only, their ``forward`` is never
called.  Every layer runs on csrc/conv_vae.hip (GroupNorm statistics, the 3x3 implicit-GEMM convolution with its norm-act / down / up gathers
and bias + residual epilogue, the row softmax) and on the existing 1x1 convolution and f32 GEMM.  Activations are NHWC f32 inside, NCHW at
the module boundary.  Convolution weights are repacked to [Cout, kh, kw, Cin] on first use and again whenever a parameter is rewritten
(``load_state_dict``).  There is no CPU or PyTorch fallback and no training: ``forward`` / ``training_step`` raise.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .util.misc import DiagonalGaussianDistribution  # noqa: F401  (one posterior class for both tokenizer families)

# True: GroupNorm + SiLU are applied while the 3x3 convolution gathers its operand (one pass over the activation).  False: a normalise pass
# writes the activated tensor and a plain convolution reads it.  Both forms use one definition of the arithmetic (gn_act of
# csrc/conv_vae.hip); tools/bench_conv_vae.py times one against the other.
FUSED_NORM_ACT = True

# The same choice for precision "tf32" (set_precision): True rounds to fp16 while the convolution gathers from the f32 tensor; False has the
# normalise pass write the activated tensor as fp16 and a plain fp16-input convolution read it.  Identical results.  Two-pass is shipped on
# the argument of DESIGN section 15 (the fused gather re-evaluates the activation per tap and per output tile, against an MFMA loop 16x
# shorter than the f32 one); tools/bench_conv_vae.py times one against the other on the 256 x 256 x 128 and the 32 x 32 x 512 layer.
TF32_FUSED_NORM_ACT = False

PRECISIONS = ("f32", "tf32")


def Normalize(in_channels, num_groups=32):
    return nn.GroupNorm(num_groups=num_groups, num_channels=in_channels, eps=1e-6, affine=True)


def _pack_key(w):
    return (w._version, w.data_ptr(), w.device)


def _packed(conv):
    """[Cout, kh, kw, Cin] f32 copy of an nn.Conv2d's weight, cached on the module until the parameter is rewritten or moved."""
    w = conv.weight
    key = _pack_key(w)
    hit = conv.__dict__.get("_ldmae_pack")
    if hit is None or hit[0] != key:
        hit = (key, w.detach().float().permute(0, 2, 3, 1).contiguous())
        conv.__dict__["_ldmae_pack"] = hit
    return hit[1]


def _packed_f16(conv):
    """The fp16 rounding (saturating, ldmae_cast) of _packed(conv), cached next to it under the same (version, pointer, device) key."""
    key = _pack_key(conv.weight)
    hit = conv.__dict__.get("_ldmae_pack_f16")
    if hit is None or hit[0] != key:
        hit = (key, ops.cast(_packed(conv), torch.float16))
        conv.__dict__["_ldmae_pack_f16"] = hit
    return hit[1]


def check_precision(precision):
    if precision not in PRECISIONS:
        raise ValueError(f"precision {precision!r}: one of {PRECISIONS} (\"tf32\": fp16-rounded operands, f32 accumulation)")
    return precision


def uses_tf32(precision, cin):
    """Whether a 3x3 (or residual 1x1) convolution with `cin` input channels runs the fp16-MFMA kernel under `precision`.  The kernel takes
    Cin % 8 == 0; every other layer (the 3-channel image convolution, a 4-channel latent conv_in) falls back to MORE precision: exact f32."""
    return check_precision(precision) == "tf32" and cin % 8 == 0


def conv3x3_layers(module):
    """[(name, Cin, Cout)] of the 3x3 convolutions (and AttnBlock.proj_out, the residual 1x1) below `module`: the layers set_precision acts on."""
    return [(n, m.in_channels, m.out_channels) for n, m in module.named_modules()
            if isinstance(m, nn.Conv2d) and (m.kernel_size == (3, 3) or n.endswith("proj_out"))]


def _f32(p):
    return None if p is None else p.detach().float().contiguous()


def _conv3x3(conv, x, mode=ops.VAE_PLAIN, res=None, precision="f32"):
    if uses_tf32(precision, x.shape[3]):
        return ops.conv3x3_vae_nhwc(x, _packed_f16(conv), _f32(conv.bias), mode=mode, res=res, precision="tf32")
    if x.shape[3] % 4:                     # the 3-channel image: the general gather of the existing convolution
        if mode != ops.VAE_PLAIN or res is not None:
            raise RuntimeError(f"conv3x3: {x.shape[3]} input channels (not a multiple of 4) are supported by the plain convolution only")
        return ops.conv2d_nhwc(x, _packed(conv), _f32(conv.bias), stride=(1, 1), padding=(1, 1), relu=False)
    return ops.conv3x3_vae_nhwc(x, _packed(conv), _f32(conv.bias), mode=mode, res=res)


def _conv1x1(conv, x):
    return ops.conv2d_nhwc(x, _packed(conv), _f32(conv.bias), relu=False)


def _norm_act_conv(norm, conv, x, res=None, precision="f32"):
    """conv(silu(norm(x))) + res."""
    stats = ops.groupnorm_stats_nhwc(x, norm.num_groups, norm.eps)
    gamma, beta = _f32(norm.weight), _f32(norm.bias)
    if uses_tf32(precision, x.shape[3]):
        w = _packed_f16(conv)
        if TF32_FUSED_NORM_ACT:
            return ops.conv3x3_vae_nhwc(x, w, _f32(conv.bias), mode=ops.VAE_NORM_ACT, res=res, stats=stats, gamma=gamma, beta=beta, silu=True,
                                        precision="tf32")
        a = ops.groupnorm_apply_nhwc(x, stats, gamma, beta, silu=True, out_dtype=torch.float16)
        return ops.conv3x3_vae_nhwc(a, w, _f32(conv.bias), mode=ops.VAE_PLAIN, res=res, precision="tf32")
    if FUSED_NORM_ACT:
        return ops.conv3x3_vae_nhwc(x, _packed(conv), _f32(conv.bias), mode=ops.VAE_NORM_ACT, res=res, stats=stats, gamma=gamma, beta=beta, silu=True)
    a = ops.groupnorm_apply_nhwc(x, stats, gamma, beta, silu=True)
    return ops.conv3x3_vae_nhwc(a, _packed(conv), _f32(conv.bias), mode=ops.VAE_PLAIN, res=res)


class _Kernels(nn.Module):
    """Forward-only module whose arithmetic runs on the HIP kernels: NCHW at the boundary, NHWC inside (forward_nhwc)."""

    precision = "f32"          # never inferred from torch.backends.*: only set_precision changes it

    def set_precision(self, precision):
        """"f32" (default): every layer on the exact-f32 kernels.  "tf32": the 3x3 convolutions and AttnBlock.proj_out with Cin % 8 == 0 round
        both operands once to fp16 and accumulate in f32 (what the reference's drivers compute under allow_tf32); everything else stays f32."""
        check_precision(precision)
        for m in self.modules():
            if isinstance(m, _Kernels):
                m.precision = precision
        return self

    def forward(self, x, *args):
        with torch.no_grad():
            x = x.detach().float().permute(0, 2, 3, 1).contiguous()
            return self.forward_nhwc(x, *args).permute(0, 3, 1, 2).contiguous()


class Upsample(_Kernels):
    def __init__(self, in_channels, with_conv):
        super().__init__()
        self.with_conv = with_conv
        if not with_conv:
            raise NotImplementedError("Upsample(with_conv=False) is not built: the reference's Encoder / Decoder always resample with a convolution")
        self.conv = nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1)

    def forward_nhwc(self, x):
        return _conv3x3(self.conv, x, ops.VAE_UP, precision=self.precision)


class Downsample(_Kernels):
    def __init__(self, in_channels, with_conv):
        super().__init__()
        self.with_conv = with_conv
        if not with_conv:
            raise NotImplementedError("Downsample(with_conv=False) is not built: the reference's Encoder / Decoder always resample with a convolution")
        self.conv = nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=2, padding=0)

    def forward_nhwc(self, x):
        return _conv3x3(self.conv, x, ops.VAE_DOWN, precision=self.precision)


class ResnetBlock(_Kernels):
    def __init__(self, *, in_channels, out_channels=None, conv_shortcut=False, dropout, temb_channels=512):
        super().__init__()
        self.in_channels = in_channels
        out_channels = in_channels if out_channels is None else out_channels
        self.out_channels = out_channels
        self.use_conv_shortcut = conv_shortcut
        if temb_channels > 0:
            raise NotImplementedError("ResnetBlock with a timestep embedding is not built: the autoencoder uses temb_channels=0")
        if dropout:
            raise NotImplementedError("ResnetBlock dropout is a training feature; this module is forward only")
        self.norm1 = Normalize(in_channels)
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.norm2 = Normalize(out_channels)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1)
        if self.in_channels != self.out_channels:
            if self.use_conv_shortcut:
                self.conv_shortcut = nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
            else:
                self.nin_shortcut = nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=1, padding=0)

    def forward_nhwc(self, x, temb=None):
        if temb is not None:
            raise NotImplementedError("ResnetBlock: temb is not supported")
        h = _norm_act_conv(self.norm1, self.conv1, x, precision=self.precision)
        if self.in_channels != self.out_channels:
            x = _conv3x3(self.conv_shortcut, x, precision=self.precision) if self.use_conv_shortcut else _conv1x1(self.nin_shortcut, x)
        return _norm_act_conv(self.norm2, self.conv2, h, res=x, precision=self.precision)


class AttnBlock(_Kernels):
    def __init__(self, in_channels):
        super().__init__()
        self.in_channels = in_channels
        self.norm = Normalize(in_channels)
        self.q = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.k = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.v = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.proj_out = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)

    def _qk(self):
        """q and k as one [2C, 1, 1, C] convolution, cached like the packed weights."""
        key = tuple((p._version, p.data_ptr()) for p in (self.q.weight, self.k.weight, self.q.bias, self.k.bias))
        hit = self.__dict__.get("_ldmae_qk")
        if hit is None or hit[0] != key:
            w = torch.cat([_packed(self.q), _packed(self.k)], 0).contiguous()
            b = torch.cat([_f32(self.q.bias), _f32(self.k.bias)], 0).contiguous()
            hit = (key, w, b)
            self.__dict__["_ldmae_qk"] = hit
        return hit[1], hit[2]

    def forward_nhwc(self, x):
        B, H, W, C = x.shape
        N = H * W
        stats = ops.groupnorm_stats_nhwc(x, self.norm.num_groups, self.norm.eps)
        hn = ops.groupnorm_apply_nhwc(x, stats, _f32(self.norm.weight), _f32(self.norm.bias), silu=False)
        wqk, bqk = self._qk()
        qk = ops.conv2d_nhwc(hn, wqk, bqk, relu=False).view(B, N, 2 * C)
        # v is produced transposed, [C, N] per image, as the second GEMM reads it; its bias is added after the softmax-weighted sum (the
        # probabilities of a row sum to 1, so P (v + 1 b^T) = P v + b^T).  Keys are padded to the GEMM's K granule with zeros.
        Np = -(-N // ops.ATTN_WIDE_KPAD) * ops.ATTN_WIDE_KPAD
        vt = (torch.zeros if Np != N else torch.empty)(B, C, Np, dtype=torch.float32, device=x.device)
        wv = _packed(self.v).view(C, C)
        hn = hn.view(B, N, C)
        for b in range(B):
            ops.gemm_nt(wv, hn[b], out=vt[b][:, :N])
        o = ops.attention_wide(qk[:, :, :C], qk[:, :, C:], vt, float(int(C) ** (-0.5)), bias=_f32(self.v.bias))
        if uses_tf32(self.precision, C):
            return ops.conv1x1_res_nhwc(o.view(B, H, W, C), _packed_f16(self.proj_out).view(C, C), _f32(self.proj_out.bias), res=x, precision="tf32")
        return ops.conv1x1_res_nhwc(o.view(B, H, W, C), _packed(self.proj_out).view(C, C), _f32(self.proj_out.bias), res=x)


class Encoder(_Kernels):
    def __init__(self, *, ch=128, out_ch=3, ch_mult=(1, 1, 2, 2, 4), num_res_blocks=2, attn_resolutions=(16,), dropout=0.0, resamp_with_conv=True,
                 in_channels=3, resolution=256, z_channels=16, double_z=True, **ignore_kwargs):
        super().__init__()
        self.ch = ch
        self.temb_ch = 0
        self.num_resolutions = len(ch_mult)
        self.num_res_blocks = num_res_blocks
        self.resolution = resolution
        self.in_channels = in_channels
        self.conv_in = nn.Conv2d(in_channels, self.ch, kernel_size=3, stride=1, padding=1)
        curr_res = resolution
        in_ch_mult = (1,) + tuple(ch_mult)
        self.down = nn.ModuleList()
        for i_level in range(self.num_resolutions):
            block = nn.ModuleList()
            attn = nn.ModuleList()
            block_in = ch * in_ch_mult[i_level]
            block_out = ch * ch_mult[i_level]
            for i_block in range(self.num_res_blocks):
                block.append(ResnetBlock(in_channels=block_in, out_channels=block_out, temb_channels=self.temb_ch, dropout=dropout))
                block_in = block_out
                if curr_res in attn_resolutions:
                    attn.append(AttnBlock(block_in))
            down = nn.Module()
            down.block = block
            down.attn = attn
            if i_level != self.num_resolutions - 1:
                down.downsample = Downsample(block_in, resamp_with_conv)
                curr_res = curr_res // 2
            self.down.append(down)
        self.mid = nn.Module()
        self.mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch, dropout=dropout)
        self.mid.attn_1 = AttnBlock(block_in)
        self.mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch, dropout=dropout)
        self.norm_out = Normalize(block_in)
        self.conv_out = nn.Conv2d(block_in, 2 * z_channels if double_z else z_channels, kernel_size=3, stride=1, padding=1)

    def forward_nhwc(self, x):
        h = _conv3x3(self.conv_in, x, precision=self.precision)
        for i_level in range(self.num_resolutions):
            for i_block in range(self.num_res_blocks):
                h = self.down[i_level].block[i_block].forward_nhwc(h)
                if len(self.down[i_level].attn) > 0:
                    h = self.down[i_level].attn[i_block].forward_nhwc(h)
            if i_level != self.num_resolutions - 1:
                h = self.down[i_level].downsample.forward_nhwc(h)
        h = self.mid.block_1.forward_nhwc(h)
        h = self.mid.attn_1.forward_nhwc(h)
        h = self.mid.block_2.forward_nhwc(h)
        return _norm_act_conv(self.norm_out, self.conv_out, h, precision=self.precision)


class Decoder(_Kernels):
    def __init__(self, *, ch=128, out_ch=3, ch_mult=(1, 1, 2, 2, 4), num_res_blocks=2, attn_resolutions=(16,), dropout=0.0, resamp_with_conv=True,
                 in_channels=3, resolution=256, z_channels=16, give_pre_end=False, **ignore_kwargs):
        super().__init__()
        self.ch = ch
        self.temb_ch = 0
        self.num_resolutions = len(ch_mult)
        self.num_res_blocks = num_res_blocks
        self.resolution = resolution
        self.in_channels = in_channels
        self.give_pre_end = give_pre_end
        block_in = ch * ch_mult[self.num_resolutions - 1]
        curr_res = resolution // 2 ** (self.num_resolutions - 1)
        self.z_shape = (1, z_channels, curr_res, curr_res)
        self.conv_in = nn.Conv2d(z_channels, block_in, kernel_size=3, stride=1, padding=1)
        self.mid = nn.Module()
        self.mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch, dropout=dropout)
        self.mid.attn_1 = AttnBlock(block_in)
        self.mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch, dropout=dropout)
        self.up = nn.ModuleList()
        for i_level in reversed(range(self.num_resolutions)):
            block = nn.ModuleList()
            attn = nn.ModuleList()
            block_out = ch * ch_mult[i_level]
            for i_block in range(self.num_res_blocks + 1):
                block.append(ResnetBlock(in_channels=block_in, out_channels=block_out, temb_channels=self.temb_ch, dropout=dropout))
                block_in = block_out
                if curr_res in attn_resolutions:
                    attn.append(AttnBlock(block_in))
            up = nn.Module()
            up.block = block
            up.attn = attn
            if i_level != 0:
                up.upsample = Upsample(block_in, resamp_with_conv)
                curr_res = curr_res * 2
            self.up.insert(0, up)  # prepend to get consistent order
        self.norm_out = Normalize(block_in)
        self.conv_out = nn.Conv2d(block_in, out_ch, kernel_size=3, stride=1, padding=1)

    def forward_nhwc(self, z):
        self.last_z_shape = (z.shape[0], z.shape[3], z.shape[1], z.shape[2])
        h = _conv3x3(self.conv_in, z, precision=self.precision)
        h = self.mid.block_1.forward_nhwc(h)
        h = self.mid.attn_1.forward_nhwc(h)
        h = self.mid.block_2.forward_nhwc(h)
        for i_level in reversed(range(self.num_resolutions)):
            for i_block in range(self.num_res_blocks + 1):
                h = self.up[i_level].block[i_block].forward_nhwc(h)
                if len(self.up[i_level].attn) > 0:
                    h = self.up[i_level].attn[i_block].forward_nhwc(h)
            if i_level != 0:
                h = self.up[i_level].upsample.forward_nhwc(h)
        if self.give_pre_end:
            return h
        return _norm_act_conv(self.norm_out, self.conv_out, h, precision=self.precision)


def _nhwc_in(x, ref):
    return x.detach().to(ref.device).float().permute(0, 2, 3, 1).contiguous()


class AutoencoderKL(nn.Module):
    def __init__(self, embed_dim, ch_mult, use_variational=True, ckpt_path=None, model_type='vavae', **ddconfig):
        """``ddconfig`` (ch, resolution, num_res_blocks, ... of Encoder / Decoder) is this package's addition for scaled-down instances; without
        it the encoder and decoder are the reference's (ch=128, resolution=256, two res blocks)."""
        super().__init__()
        if model_type not in ('vavae', 'marvae'):
            raise ValueError(f"Invalid model type: {model_type}")
        if ckpt_path is not None and not os.path.isfile(ckpt_path):          # before the parameters are built
            raise FileNotFoundError(f"AutoencoderKL({model_type}): checkpoint {ckpt_path!r} not found; pass the path of the file (nothing is downloaded)")
        ddconfig.pop("z_channels", None)
        dec_attn = ddconfig.pop("decoder_attn_resolutions", (16,) if model_type == 'vavae' else ())
        self.encoder = Encoder(ch_mult=ch_mult, z_channels=embed_dim, **ddconfig)
        self.decoder = Decoder(ch_mult=ch_mult, z_channels=embed_dim, **{**ddconfig, "attn_resolutions": dec_attn})
        self.use_variational = use_variational
        mult = 2 if self.use_variational else 1
        self.quant_conv = nn.Conv2d(2 * embed_dim, mult * embed_dim, 1)
        self.post_quant_conv = nn.Conv2d(embed_dim, embed_dim, 1)
        self.embed_dim = embed_dim
        self.model_type = model_type
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path)

    def init_from_ckpt(self, path):
        if self.model_type == 'vavae':
            sd = torch.load(path, map_location="cpu")["state_dict"]
            sd = {k: v for k, v in sd.items() if 'loss' not in k}          # the reference's filter: the loss (discriminator / LPIPS) weights go
        else:
            sd = torch.load(path, map_location="cpu")["model"]
        msg = self.load_state_dict(sd, strict=False)
        print(msg)
        return msg

    @property
    def precision(self):
        return self.encoder.precision

    def set_precision(self, precision):
        """Encoder.set_precision on both halves; quant_conv / post_quant_conv stay f32."""
        self.encoder.set_precision(precision)
        self.decoder.set_precision(precision)
        return self

    def encode_moments(self, x):
        """The quantised encoder output [B, mult * embed_dim, h, w] (NCHW) before the posterior is formed."""
        with torch.no_grad():
            h = self.encoder.forward_nhwc(_nhwc_in(x, self.quant_conv.weight))
            return _conv1x1(self.quant_conv, h).permute(0, 3, 1, 2).contiguous()

    def encode(self, x):
        moments = self.encode_moments(x)
        if not self.use_variational:
            moments = torch.cat((moments, torch.ones_like(moments)), 1)
        return DiagonalGaussianDistribution(moments)

    def decode(self, z):
        with torch.no_grad():
            z = _conv1x1(self.post_quant_conv, _nhwc_in(z, self.post_quant_conv.weight))
            return self.decoder.forward_nhwc(z).permute(0, 3, 1, 2).contiguous()

    def forward(self, inputs, disable=True, train=True, optimizer_idx=0):
        raise NotImplementedError("AutoencoderKL.forward: training these autoencoders is not built here (no backward, no discriminator / LPIPS / "
                                  "VF losses); use encode / decode")

    def training_step(self, *args, **kwargs):
        raise NotImplementedError("AutoencoderKL.training_step: training these autoencoders is not built here; use encode / decode")

    validation_step = training_step


def center_crop_arr(pil_image, image_size):
    """
    Center cropping implementation from ADM.
    https://github.com/openai/guided-diffusion/blob/8fb3ad9197f16bbc40620447b2742e13458d2831/guided_diffusion/image_datasets.py#L126
    """
    from PIL import Image
    while min(*pil_image.size) >= 2 * image_size:
        pil_image = pil_image.resize(tuple(x // 2 for x in pil_image.size), resample=Image.BOX)
    scale = image_size / min(*pil_image.size)
    pil_image = pil_image.resize(tuple(round(x * scale) for x in pil_image.size), resample=Image.BICUBIC)
    arr = np.array(pil_image)
    crop_y = (arr.shape[0] - image_size) // 2
    crop_x = (arr.shape[1] - image_size) // 2
    return Image.fromarray(arr[crop_y: crop_y + image_size, crop_x: crop_x + image_size])


class ImgTransform:
    """center_crop_arr -> RandomHorizontalFlip(p) -> ToTensor -> Normalize(0.5, 0.5): the wrappers' ``img_transform`` without torchvision."""

    def __init__(self, img_size, p_hflip=0):
        self.img_size, self.p_hflip = img_size, p_hflip

    def __call__(self, pil_image):
        arr = np.array(center_crop_arr(pil_image.convert("RGB"), self.img_size), dtype=np.uint8)
        x = torch.from_numpy(arr).permute(2, 0, 1).float().div_(255.0)
        if self.p_hflip > 0 and torch.rand(1).item() < self.p_hflip:
            x = x.flip(-1)
        return ((x - 0.5) / 0.5).contiguous()


def images_uint8(images):
    """NCHW f32 in [-1, 1] -> uint8 NHWC on the host: clamp(127.5 x + 128, 0, 255) truncated, on the PNG quantisation kernel of the tokenizer
    evaluation, left as it is.  That kernel quantises a (decoded, reference) pair and sums their squared error; it is given the tensor twice
    and the second image and the (zero) error are dropped: twice the reads of a 3-channel image, small against the decoder in front of it."""
    dec8, _, _ = ops.recon_quantize_sse(images, images)
    return dec8.cpu().numpy()
