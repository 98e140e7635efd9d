"""Deterministic, name-keyed weights for the convolutional KL-VAE goldens, shared by make_golden_convvae.py (which loads them into the
*reference* autoencoder) and by the tests (which load them into the HIP modules).  Weights are never stored in fixtures: both sides
regenerate them from (name, shape, seed) with torch's CPU generator (weights.det_randn)."""
import math

import numpy as np

from weights import det_randn

# the constructor arguments of the two golden cases (tests/golden/convvae.npz)
CASE_A = dict(ch=32, ch_mult=(1, 2, 4, 4), num_res_blocks=2, z_channels=16, attn_resolutions=(), resolution=32, in_channels=3, out_ch=3)
CASE_B = dict(embed_dim=8, ch_mult=(1, 1, 2, 2, 4), ch=32, resolution=64)
# case A under diffusers' keyword names
CASE_A_DIFFUSERS = dict(img_size=32, sample_size=32, in_channels=3, out_channels=3, layers_per_block=2, latent_channels=16, norm_num_groups=32,
                        act_fn="silu", block_out_channels=(32, 64, 128, 128), force_upcast=False, use_quant_conv=False, use_post_quant_conv=False,
                        down_block_types=("DownEncoderBlock2D",) * 4, up_block_types=("UpDecoderBlock2D",) * 4)


def convvae_weights(shapes: dict, seed: int = 0) -> dict:
    """Non-degenerate values for every parameter: GroupNorm scales around 1 and shifts around 0 (so silu(norm(0)) != 0), biases non-zero,
    convolutions at unit gain (variance 1 / fan_in)."""
    out = {}
    for k, shp in shapes.items():
        z = det_randn(k, shp, seed)
        if "norm" in k and k.endswith(".weight"):
            out[k] = 1.0 + 0.1 * z
        elif "norm" in k and k.endswith(".bias"):
            out[k] = 0.1 * z
        elif k.endswith(".bias"):
            out[k] = 0.05 * z
        else:
            out[k] = z / math.sqrt(int(np.prod(shp[1:])))
    return out


def weights_for(module, seed: int = 0) -> dict:
    """convvae_weights for every entry of an nn.Module's own (LDM-named) state dict."""
    return convvae_weights({k: tuple(v.shape) for k, v in module.state_dict().items()}, seed)
