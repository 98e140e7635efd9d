#!/usr/bin/env python3
"""Records what the norm + modulate and gate row entry points answer to arguments they refuse: tests/golden/row_refusals.json.

    LDMAE_HIP_LIB=/path/to/the/OLD/libldmae_hip.so python tests/golden/make_golden_row_refusals.py

The file is a record of behaviour that must not change, so it is generated from a build of the commit BEFORE the change under test, never
from the code a test then checks against it.  The one committed here was written by the library of 2d3f7e5 ("One block backward and one
attention branch for the LightningDiT block"), the parent of the commit that gave the row kernels one text (csrc/norm_mod_rows.inc) and
the backward entries one named argument struct.

Entries: ldmae_rmsnorm_modulate_fwd, ldmae_layernorm_modulate_fwd, ldmae_res_rmsnorm_modulate_fwd, ldmae_rmsnorm_modulate_bwd,
ldmae_rmsnorm_modulate_bwd_gate, ldmae_rmsnorm_modulate_bwd_gate_recompute, ldmae_layernorm_modulate_bwd, ldmae_layernorm_modulate_bwd_gate,
ldmae_gate_bwd and ldmae_rmsnorm_modulate_fwd_mx8.  (The three *_workspace_bytes functions of the family refuse nothing.)  At least one
call per LDMAE_REQUIRE of each entry, and one per clause where a refusal joins several conditions (D % 4 and mod_ld % 4, null and empty);
every argument list is a valid small problem with one thing wrong, on dummy pointers (16: aligned, 20: not 16-byte aligned, 18: not 4-byte
aligned -- the only alignment ldmae_rmsnorm_modulate_fwd_mx8 asks of q -- and null), so a call that is not refused would reach a launch: run
this where no GPU is present, like the test.  "D > 2048" is the refusal of row_nch_dispatch (csrc/common.h), which every entry reaches
after its own checks.

Refusals that cannot be provoked, and are not listed:
  * "rows_per_batch=%d must be a multiple of 4" of the five backward entries and of ldmae_gate_bwd: pick_rows_per_wg ends at 1 row per
    workgroup and never returns 0 once rows_per_batch > 0 and M % rows_per_batch == 0 hold, which the check before it requires;
  * the `center` half of "bf16 activations and the RMSNorm form only": no LayerNorm entry sets recompute; and the "dtype %d (f32 or bf16)"
    refusal of ldmae_rmsnorm_modulate_bwd_gate_recompute, which that refusal of everything but bf16 comes before;
  * row_nch_dispatch's refusal inside ldmae_rmsnorm_modulate_fwd_mx8: the entry's own D <= 2048 comes first.
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from ldmae_amd import _lib  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "row_refusals.json")
P, P20, P18, NUL = 16, 20, 18, None
F32, BF16, F16 = 0, 1, 2


def _args(names, defaults, k):
    a = dict(defaults)
    assert set(k) <= set(a), k
    a.update(k)
    return [a[n] for n in names.split()] + [None]               # + stream


def fwd(layernorm=False, **k):
    d = dict(out_dtype=BF16, x=P, w=P, shift=P, scale=P, mod_ld=64, out=P, rstd=P, M=16, D=64, rpb=4, eps=1e-6)
    return _args("out_dtype x shift scale mod_ld out rstd M D rpb eps" if layernorm else "out_dtype x w shift scale mod_ld out rstd M D rpb eps", d, k)


def res_fwd(**k):
    d = dict(dtype=BF16, x=P, ya=P, gate_a=P, gate_a_ld=64, yb=P, gate_b=P, gate_b_ld=64, xout=32, w=P, shift=P, scale=P, mod_ld=64, out=P,
             rstd=P, M=16, D=64, rpb=4, eps=1e-6)
    return _args("dtype x ya gate_a gate_a_ld yb gate_b gate_b_ld xout w shift scale mod_ld out rstd M D rpb eps", d, k)


def bwd(layernorm=False, gate=False, **k):
    d = dict(dtype=BF16, dout=P, x=P, w=P, scale=P, mod_ld=64, rstd=P, dx=P, beta_x=1.0, dshift=P, dscale=P, dmod_ld=64, dw=P, beta_w=0.0,
             y=P, gate=P, gate_ld=64, dy=P, dgate=P, dgate_ld=64, dbias=P, M=16, D=64, rpb=4, ws=P)
    names = "dtype dout x w scale mod_ld rstd dx beta_x dshift dscale dmod_ld dw beta_w y gate gate_ld dy dgate dgate_ld dbias M D rpb ws".split()
    drop = (["w", "dw", "beta_w"] if layernorm else []) + ([] if gate else "y gate gate_ld dy dgate dgate_ld dbias".split())
    return _args(" ".join(n for n in names if n not in drop), d, k)


def gate_bwd(**k):
    d = dict(dtype=BF16, dxout=P, y=P, gate=P, gate_ld=64, dy=P, dgate=P, dgate_ld=64, dbias=P, M=16, D=64, rpb=4, ws=P)
    return _args("dtype dxout y gate gate_ld dy dgate dgate_ld dbias M D rpb ws", d, k)


def fwd_mx8(**k):
    d = dict(x=P, w=P, shift=P, scale=P, mod_ld=128, q=P, scales=P, rstd=P, M=16, D=128, rpb=4, eps=1e-6)
    return _args("x w shift scale mod_ld q scales rstd M D rpb eps", d, k)


def cases():
    c = []
    add = lambda entry, what, args: c.append({"id": f"{entry[6:]}-{what}", "entry": entry, "args": args})
    for e, ln in (("ldmae_rmsnorm_modulate_fwd", False), ("ldmae_layernorm_modulate_fwd", True)):
        add(e, "null", fwd(ln, x=NUL))
        if not ln:
            add(e, "null_w", fwd(ln, w=NUL))
        add(e, "empty", fwd(ln, M=0))
        add(e, "D_multiple", fwd(ln, D=6))
        add(e, "mod_ld_multiple", fwd(ln, mod_ld=66))
        add(e, "rows_per_batch", fwd(ln, rpb=3))
        add(e, "rows_per_batch_nonpositive", fwd(ln, rpb=0))
        add(e, "dtype", fwd(ln, out_dtype=F16))
        add(e, "D_too_wide", fwd(ln, D=4096))
    e = "ldmae_res_rmsnorm_modulate_fwd"
    add(e, "dtype", res_fwd(dtype=F32))
    add(e, "null", res_fwd(ya=NUL))
    add(e, "no_output", res_fwd(xout=NUL, out=NUL))
    add(e, "empty", res_fwd(M=0))
    add(e, "yb_without_gate_b", res_fwd(gate_b=NUL))
    add(e, "norm_without_weight", res_fwd(w=NUL))
    add(e, "rstd_without_norm", res_fwd(out=NUL, w=NUL, shift=NUL, scale=NUL))
    add(e, "xout_is_x", res_fwd(xout=P))
    add(e, "D_multiple", res_fwd(D=6))
    add(e, "gate_a_ld_multiple", res_fwd(gate_a_ld=66))
    add(e, "gate_b_ld_multiple", res_fwd(gate_b_ld=66))
    add(e, "mod_ld_multiple", res_fwd(mod_ld=66))
    add(e, "rows_per_batch", res_fwd(rpb=3))
    add(e, "misaligned", res_fwd(ya=P20))
    add(e, "D_too_wide", res_fwd(D=4096))
    for e, ln, g in (("ldmae_rmsnorm_modulate_bwd", False, False), ("ldmae_rmsnorm_modulate_bwd_gate", False, True),
                     ("ldmae_rmsnorm_modulate_bwd_gate_recompute", False, True), ("ldmae_layernorm_modulate_bwd", True, False),
                     ("ldmae_layernorm_modulate_bwd_gate", True, True)):
        if g:
            add(e, "gate_null", bwd(ln, g, y=NUL))
            add(e, "gate_ld_multiple", bwd(ln, g, gate_ld=66))
        add(e, "null", bwd(ln, g, dout=NUL))
        if not ln:
            add(e, "null_dw", bwd(ln, g, dw=NUL))
        add(e, "D_multiple", bwd(ln, g, D=6))
        add(e, "empty", bwd(ln, g, M=0))
        add(e, "rows_per_batch", bwd(ln, g, rpb=3))
        add(e, "beta_x", bwd(ln, g, beta_x=0.5))
        if e.endswith("recompute"):
            add(e, "recompute_f32", bwd(ln, g, dtype=F32))
        else:
            add(e, "dtype", bwd(ln, g, dtype=F16))
        add(e, "D_too_wide", bwd(ln, g, D=4096))
    e = "ldmae_gate_bwd"
    add(e, "null", gate_bwd(dxout=NUL))
    add(e, "empty", gate_bwd(M=0))
    add(e, "D_multiple", gate_bwd(D=6))
    add(e, "rows_per_batch", gate_bwd(rpb=3))
    add(e, "dgate_without_y", gate_bwd(y=NUL))
    add(e, "dgate_without_workspace", gate_bwd(dbias=NUL, ws=NUL))
    add(e, "dbias_without_workspace", gate_bwd(dgate=NUL, ws=NUL))
    add(e, "dtype", gate_bwd(dtype=F16))
    add(e, "D_too_wide", gate_bwd(D=4096))
    e = "ldmae_rmsnorm_modulate_fwd_mx8"
    add(e, "null", fwd_mx8(w=NUL))
    add(e, "empty", fwd_mx8(M=0))
    add(e, "D_multiple", fwd_mx8(D=64, mod_ld=64))
    add(e, "D_too_wide", fwd_mx8(D=2176, mod_ld=2176))
    add(e, "mod_ld_multiple", fwd_mx8(mod_ld=130))
    add(e, "rows_per_batch", fwd_mx8(rpb=3))
    add(e, "misaligned", fwd_mx8(q=P18))
    return c


def main():
    import torch
    if torch.cuda.is_available():
        sys.exit("run this where no GPU is present: a call that is not refused would launch a kernel on address 16")
    lib = _lib.load()
    out = cases()
    for c in out:
        c["rc"] = getattr(lib, c["entry"])(*c["args"])
        c["message"] = _lib.last_error()
        if c["rc"] != -1:
            sys.exit(f"{c['id']}: not refused (rc {c['rc']}: {c['message']!r})")
    head = ("Recorded by tests/golden/make_golden_row_refusals.py from the library of commit 2d3f7e5, BEFORE the row kernels moved onto "
            "csrc/norm_mod_rows.inc and the backward entries onto one argument struct: the old behaviour, never the code under test.")
    with open(OUT, "w") as f:
        json.dump({"_comment": head, "cases": out}, f, indent=1)
        f.write("\n")
    print(f"{len(out)} refusals from {_lib.LIB_PATH} -> {OUT}")


if __name__ == "__main__":
    main()
