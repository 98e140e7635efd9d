"""Image-quality metrics of the tokenizer evaluation on this package's kernels (csrc/tokenizer_eval.hip): SSIM as torchmetrics 1.x's
StructuralSimilarityIndexMeasure computes it with its defaults, and PSNR of 8-bit images as the reference's calculate_psnr does.
LPIPS is ldmae_amd.models.lpips.LPIPS."""
from __future__ import annotations

import math

import torch


def ssim(preds, target, data_range=(-1.0, 1.0), reduction="elementwise_mean"):
    """SSIM of NCHW images [B, C, H, W] (H, W >= 11) with torchmetrics' defaults (Gaussian 11 x 11, sigma 1.5, k1 0.01, k2 0.03).
    data_range: a (lo, hi) tuple clamps both inputs to [lo, hi] and uses hi - lo; a number is the range and nothing is clamped.
    reduction: "elementwise_mean" -> the mean over the batch (0-dim tensor, what the metric's forward returns); "none" -> per image [B]."""
    from . import ops
    if isinstance(data_range, (tuple, list)):
        lo, hi = float(data_range[0]), float(data_range[1])
        rng = hi - lo
    else:
        lo, hi, rng = -math.inf, math.inf, float(data_range)
    if not rng > 0:
        raise ValueError(f"ssim: data_range {data_range} must be positive")
    if reduction not in ("elementwise_mean", "none"):
        raise ValueError(f"ssim: reduction {reduction!r} (elementwise_mean or none)")
    per_image = ops.ssim(preds.float().contiguous(), target.float().contiguous(), lo, hi, rng)
    return per_image.mean() if reduction == "elementwise_mean" else per_image


def psnr_from_sse(sse, values_per_image):
    """Per-image PSNR f64 = 20 log10(255 / sqrt(sse / n)) from exact integer squared errors (+inf where the images are equal)."""
    mse = sse.double() / float(values_per_image)
    return 20.0 * torch.log10(255.0 / torch.sqrt(mse))


def psnr_uint8(a, b):
    """Per-image PSNR f64 [B] of two uint8 image batches [B, ...] of one shape, from the exact integer squared error: the reference's
    calculate_psnr on the same pixels (it rounds the mean to f32; this does not)."""
    from . import ops
    return psnr_from_sse(ops.sse_u8(a.contiguous(), b.contiguous()), a[0].numel())
