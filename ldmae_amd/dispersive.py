"""Tensor-level wrappers of csrc/dispersive.hip, reached as ``ops.dispersive_fwd`` / ``ops.dispersive_bwd`` (ops.py re-exports them).

They are written like ``ops.guidance_combine`` / ``ops.row_mse``: every tensor goes through the one argument checker ``ops._arg``, the
scratch comes from ``ops.workspace``, the kernels are enqueued on torch's current stream, and nothing is computed in PyTorch.  The
contract of the two entry points is in include/ldmae_hip.h; DESIGN.md section 28 has the kernels.
"""
from __future__ import annotations

import torch

from ._lib import call, ptr

DISPERSIVE_MAX_B = 1024


def _dispersive_z(op, z):
    """z [B, K] f32 as the two kernels read it (dense, in place: 805 MB at the bench shape is not copied behind the caller's back) -> (B, K)."""
    from . import ops
    z = ops._arg(z, op + " z", torch.float32, ("B", "K"), copy=False, align=16)
    B, K = z.shape
    if not 1 <= B <= DISPERSIVE_MAX_B:
        raise RuntimeError(f"{op} z: B = {B} samples, expected 1 .. {DISPERSIVE_MAX_B} (shape {tuple(z.shape)})")
    if K < 4 or K % 4:
        raise RuntimeError(f"{op} z: K = {K} features per sample, expected a positive multiple of 4 (16-byte accesses; shape {tuple(z.shape)})")
    return B, K


def dispersive_fwd(z, tau):
    """(loss [1] f32, C [B, B] f32) of the Dispersive Loss L = log mean_ij exp(-||z_i - z_j||^2 / (K tau)) of z [B, K] f32 (the contract of
    ldmae_dispersive_fwd: exact-f32 MFMA Gram matrix, split along K, no atomics -- bitwise reproducible); dL/dz = C z (dispersive_bwd)."""
    from . import ops
    B, K = _dispersive_z("dispersive_fwd", z)
    tau = float(tau)
    if not 0.0 < tau < float("inf"):
        raise RuntimeError(f"dispersive_fwd tau: {tau!r}, expected a finite value > 0")
    loss = torch.empty(1, dtype=torch.float32, device=z.device)
    C = torch.empty(B, B, dtype=torch.float32, device=z.device)
    ws = ops.workspace(ops._ws_bytes("ldmae_dispersive_workspace_bytes", B, K), z.device, "dispersive")
    call("ldmae_dispersive_fwd", ptr(z), ptr(loss), ptr(C), B, K, tau, ptr(ws), ops.stream())
    return loss, C


def dispersive_bwd(C, z, g, out=None):
    """dz [B, K] = g * (C z): the gradient of g * L with respect to z, from the C of dispersive_fwd(z, tau).  g: a python number (upstream
    gradient times the loss weight, passed by value).  One writer per element, a fixed order over j: bitwise reproducible."""
    from . import ops
    B, K = _dispersive_z("dispersive_bwd", z)
    C = ops._arg(C, "dispersive_bwd C", torch.float32, (B, B), like=z)
    if out is None:
        out = torch.empty(B, K, dtype=torch.float32, device=z.device)
    else:
        ops._arg(out, "dispersive_bwd out", torch.float32, (B, K), out=True, like=z, align=16)
    call("ldmae_dispersive_bwd", ptr(C), ptr(z), float(g), ptr(out), B, K, ops.stream())
    return out
