#!/usr/bin/env python3
"""Generate tests/golden/convvae_tf32.npz: the REFERENCE's own error under the TF32-class arithmetic of the convolutional tokenizers.

Runs only where the reference checkout is present (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_convvae_tf32.py

The reference's tokenizer/autoencoder.py is imported as make_golden_convvae.py does, and cases A and B of convvae.npz are run in f64 twice:
exactly, and with every ``nn.Conv2d`` whose kernel is 3x3 and whose Cin % 8 == 0 reading an fp16-rounded input (a forward pre-hook) and an
fp16-rounded weight (a rounded copy of the model), everything else in f64.  Rounding is to nearest even, saturating at +-65504
(``round_f16``).  Per output key

    e_tf32 = max|emulated - exact f64| / max|exact f64|

is stored, and nothing else: inputs, weights and exact outputs are those of convvae.npz (the exact run is checked against it here).
"""
import copy
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from convvae_weights import CASE_A, CASE_B, weights_for  # noqa: E402

F16_MAX = 65504.0


def round_f16(t):
    """t rounded once to fp16 (nearest even, saturating at +-65504, NaN kept), returned in t's dtype."""
    return t.clamp(-F16_MAX, F16_MAX).to(torch.float16).to(t.dtype)


def is_tf32_conv(m):
    return isinstance(m, torch.nn.Conv2d) and tuple(m.kernel_size) == (3, 3) and m.in_channels % 8 == 0


def emulated(model):
    """A copy of `model` (f64) whose 3x3 convolutions with Cin % 8 == 0 see fp16-rounded inputs and weights."""
    m = copy.deepcopy(model).double().eval()
    for mod in m.modules():
        if is_tf32_conv(mod):
            mod.weight.data = round_f16(mod.weight.data)
            mod.register_forward_pre_hook(lambda _, args: (round_f16(args[0]),) + tuple(args[1:]))
    return m


def main():
    from make_golden_convvae import import_reference
    ae = import_reference()
    fx = np.load(os.path.join(HERE, "convvae.npz"))
    e = {}

    def record(key, model, call, x):
        with torch.no_grad():
            exact = call(model.double().eval())(x.double())
            emu = call(emulated(model))(x.double())
        assert np.array_equal(exact.numpy(), fx[key]), f"{key}: the exact f64 run differs from convvae.npz"
        e[key] = float((emu - exact).abs().max() / exact.abs().max())

    enc, dec = ae.Encoder(double_z=True, **CASE_A), ae.Decoder(**CASE_A)
    enc.load_state_dict(weights_for(enc, 1))
    dec.load_state_dict(weights_for(dec, 2))
    record("A_moments", enc, lambda m: m, torch.from_numpy(fx["A_x"]))
    record("A_dec", dec, lambda m: m, torch.from_numpy(fx["A_z"]))

    def model_b(use_variational, model_type="vavae"):
        b = dict(CASE_B)
        m = ae.AutoencoderKL(embed_dim=b["embed_dim"], ch_mult=(1,), use_variational=use_variational, model_type=model_type)   # throw-away halves
        cfg = dict(ch=b["ch"], ch_mult=b["ch_mult"], resolution=b["resolution"], z_channels=b["embed_dim"])
        m.encoder, m.decoder = ae.Encoder(**cfg), ae.Decoder(attn_resolutions=(16,) if model_type == "vavae" else (), **cfg)
        m.load_state_dict(weights_for(m, 3))
        return m

    xb, zb = torch.from_numpy(fx["B_x"]), torch.from_numpy(fx["B_z"])
    record("B_moments", model_b(True), lambda m: (lambda x: m.encode(x).parameters), xb)
    record("B_moments_nv", model_b(False), lambda m: (lambda x: m.encode(x).parameters), xb)
    record("B_dec", model_b(True), lambda m: m.decode, zb)
    record("B_dec_mar", model_b(True, "marvae"), lambda m: m.decode, zb)

    for k, v in e.items():
        print(f"{k:14s} e_tf32 {v:.3e}  4 e_tf32 {4 * v:.3e}" + ("   (above the standing 1e-3 of TF32-class calls)" if 4 * v > 1e-3 else ""))
    np.savez_compressed(os.path.join(HERE, "convvae_tf32.npz"), **{"e_tf32_" + k: np.float64(v) for k, v in e.items()})


if __name__ == "__main__":
    main()
