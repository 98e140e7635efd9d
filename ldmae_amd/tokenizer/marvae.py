"""``MAR_VAE`` on the HIP kernels -- counterpart of the reference's ``tokenizer/marvae.py`` (the KL-16 autoencoder of MAR: the LDM KL
autoencoder with no attention in the decoder's levels).  The reference leaves the checkpoint path empty for the user to fill in; here it is
an argument, a missing file is an error, nothing is downloaded."""
from __future__ import annotations

import torch

from .autoencoder import AutoencoderKL, ImgTransform, center_crop_arr, images_uint8  # noqa: F401

CKPT_PATH = ''  # <-- MAR VAE checkpoint, from its official repository (the reference's literal)


class MAR_VAE:
    def __init__(self, img_size=256, horizon_flip=0.5, fp16=True, ckpt_path=CKPT_PATH):
        self.embed_dim = 16
        self.ckpt_path = ckpt_path
        self.img_size = img_size
        self.horizon_flip = horizon_flip
        self.load()

    def load(self):
        if not torch.cuda.is_available():
            raise RuntimeError("MAR_VAE needs a GPU: there is no CPU path in this package")
        self.model = AutoencoderKL(embed_dim=self.embed_dim, ch_mult=(1, 1, 2, 2, 4), ckpt_path=self.ckpt_path, model_type='marvae').cuda().eval()
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
