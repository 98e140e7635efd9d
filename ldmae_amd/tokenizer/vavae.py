"""``VA_VAE`` on the HIP kernels -- counterpart of the reference's ``tokenizer/vavae.py`` (the Vision-foundation-model Aligned VAE of
LightningDiT: the LDM KL autoencoder, f16 d32, attention at resolution 16 in both halves).  The YAML is read with PyYAML; the checkpoint path
is an argument that defaults to the reference's literal, a missing file is an error, nothing is downloaded."""
from __future__ import annotations

import torch
import yaml

from .autoencoder import AutoencoderKL, ImgTransform, center_crop_arr, images_uint8  # noqa: F401

CKPT_PATH = "pretrain_weight/vavae-imagenet256-f16d32-dinov2.pt"


class VA_VAE:
    """Vision Foundation Model Aligned VAE Implementation"""

    def __init__(self, config, img_size=256, horizon_flip=0.5, fp16=True, ckpt_path=CKPT_PATH):
        """config: path of the YAML holding model.params.embed_dim (or a dict of that shape).  fp16 is accepted and unused, as in the reference."""
        if isinstance(config, dict):
            self.config = config
        else:
            with open(config) as f:
                self.config = yaml.safe_load(f)
        self.embed_dim = self.config["model"]["params"]["embed_dim"]
        self.ckpt_path = ckpt_path
        self.img_size = img_size
        self.horizon_flip = horizon_flip
        self.load()

    def load(self):
        """Load and initialize VAE model"""
        if not torch.cuda.is_available():
            raise RuntimeError("VA_VAE needs a GPU: there is no CPU path in this package")
        self.model = AutoencoderKL(embed_dim=self.embed_dim, ch_mult=(1, 1, 2, 2, 4), ckpt_path=self.ckpt_path).cuda().eval()
        return self

    def set_precision(self, precision):
        """"f32" (default) or "tf32": AutoencoderKL.set_precision of the model (tokenizer/autoencoder.py)."""
        self.model.set_precision(precision)
        return self

    def img_transform(self, p_hflip=0, img_size=None):
        return ImgTransform(img_size if img_size is not None else self.img_size, p_hflip)

    def encode_images(self, images):
        return self.model.encode(images.cuda()).sample()

    def decode_to_images(self, z):
        return images_uint8(self.model.decode(z.cuda()))
