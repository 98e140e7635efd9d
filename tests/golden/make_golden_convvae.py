#!/usr/bin/env python3
"""Generate tests/golden/convvae.npz by IMPORTING THE REFERENCE's tokenizer/autoencoder.py.

Runs only where the reference checkout is present (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_convvae.py

The reference's third-party imports that are absent (torchvision, requests, tqdm) are replaced by empty stand-ins inserted into
``sys.modules`` before the import, as make_golden.py does.  Outputs are data only: inputs, expected outputs in f64, and
e_ref = max|f32 - f64| / max|f64| of the reference's own f32 CPU run per output.  Weights are regenerated on both sides from
convvae_weights.py, so none are stored.
"""
import importlib
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/LDMAE"
sys.path.insert(0, HERE)
from convvae_weights import CASE_A, CASE_B, weights_for  # noqa: E402
from weights import det_randn  # noqa: E402


def import_reference():
    for name in ("requests", "tqdm", "torchvision"):
        try:
            importlib.import_module(name)
        except ImportError:
            m = types.ModuleType(name)
            m.tqdm = lambda it=None, *a, **k: it
            m.transforms = types.ModuleType(name + ".transforms")
            sys.modules[name] = m
            sys.modules[name + ".transforms"] = m.transforms
    sys.path.insert(0, REF)
    return importlib.import_module("tokenizer.autoencoder")


def run(fn, x):
    """(f64 output, e_ref of the f32 run)."""
    with torch.no_grad():
        y64 = fn(torch.float64)(x.double())
        y32 = fn(torch.float32)(x.float())
    return y64.numpy(), float((y32.double() - y64).abs().max() / y64.abs().max())


def main():
    ae = import_reference()
    torch.manual_seed(0)
    out, e_ref = {}, {}

    # ---- case A: the driver shape scaled down, bare Encoder / Decoder
    enc, dec = ae.Encoder(double_z=True, **CASE_A), ae.Decoder(**CASE_A)
    enc.load_state_dict(weights_for(enc, 1))
    dec.load_state_dict(weights_for(dec, 2))
    out["A_x"] = det_randn("convvae.A.x", (2, 3, 32, 32)).clamp(-1, 1).numpy()
    out["A_z"] = det_randn("convvae.A.z", (2, 16, 4, 4)).numpy()
    out["A_moments"], e_ref["A_moments"] = run(lambda dt: enc.to(dt).eval(), torch.from_numpy(out["A_x"]))
    out["A_dec"], e_ref["A_dec"] = run(lambda dt: dec.to(dt).eval(), torch.from_numpy(out["A_z"]))

    # ---- case B: the VA-VAE shape scaled down, AutoencoderKL with quant convs; attention at resolution 16 in both halves
    def model_b(use_variational, model_type="vavae"):
        b = dict(CASE_B)
        m = ae.AutoencoderKL(embed_dim=b["embed_dim"], ch_mult=(1,), use_variational=use_variational, model_type=model_type)   # throw-away halves
        cfg = dict(ch=b["ch"], ch_mult=b["ch_mult"], resolution=b["resolution"], z_channels=b["embed_dim"])
        m.encoder, m.decoder = ae.Encoder(**cfg), ae.Decoder(attn_resolutions=(16,) if model_type == "vavae" else (), **cfg)
        m.load_state_dict(weights_for(m, 3))
        return m

    mb, mb_nv = model_b(True), model_b(False)
    out["B_x"] = det_randn("convvae.B.x", (1, 3, 64, 64)).clamp(-1, 1).numpy()
    out["B_z"] = det_randn("convvae.B.z", (1, 8, 4, 4)).numpy()
    xb, zb = torch.from_numpy(out["B_x"]), torch.from_numpy(out["B_z"])
    out["B_moments"], e_ref["B_moments"] = run(lambda dt: (lambda x: mb.to(dt).eval().encode(x).parameters), xb)
    out["B_moments_nv"], e_ref["B_moments_nv"] = run(lambda dt: (lambda x: mb_nv.to(dt).eval().encode(x).parameters), xb)
    out["B_dec"], e_ref["B_dec"] = run(lambda dt: mb.to(dt).eval().decode, zb)
    mb_mar = model_b(True, "marvae")                          # the MAR-VAE decoder: no attention in its levels
    out["B_dec_mar"], e_ref["B_dec_mar"] = run(lambda dt: mb_mar.to(dt).eval().decode, zb)

    for k, v in out.items():
        print(f"{k:14s} {v.shape} {v.dtype} max|.| {np.abs(v).max():.4g}" + (f"  e_ref {e_ref[k]:.3e}  8 e_ref {8 * e_ref[k]:.3e}" if k in e_ref else ""))
    np.savez_compressed(os.path.join(HERE, "convvae.npz"), **out, **{"e_ref_" + k: np.float64(v) for k, v in e_ref.items()})


if __name__ == "__main__":
    main()
