#!/usr/bin/env python3
"""Records what the flat f32 entry points answer to arguments they refuse: tests/golden/flat_refusals.json.

    LDMAE_HIP_LIB=/path/to/the/OLD/libldmae_hip.so python tests/golden/make_golden_flat_refusals.py

The file is a record of behaviour that must not change, so it is generated from a build of the commit BEFORE the change under test, never
from the code a test then checks against it.  The one committed here was written by the library of 9f442bc ("Add sample.guidance:
all-channel CFG, rescale, APG, autoguidance in HIP"), the parent of the commit that gave the flat kernels one walker, one row reduction
(csrc/flat_common.h) and one block sum (csrc/common.h).

Entries: every entry of csrc/ode.hip (ldmae_rk_stage_f32, ldmae_dopri5_finish_f32, ldmae_rms_norm_scaled_f32, ldmae_dopri5_interp_f32,
ldmae_dopri5_advance, ldmae_dopri5_initial_step, ldmae_rademacher_f32, ldmae_normal_f32, ldmae_sde_combine_f32, ldmae_rowdot_f32,
ldmae_likelihood_finish_f32) and of csrc/fm_valid.hip (ldmae_fm_valid_plan_f32, ldmae_row_mse), and ldmae_guidance_combine.  (The three
*_partials functions refuse nothing: they return 0.)  At least one call per LDMAE_REQUIRE of each entry, and one per clause where a refusal
joins several conditions; every argument list is a valid small problem with one thing wrong, on dummy pointers (multiples of 0x1000:
aligned; + 4: not 16-byte aligned; + 2: not 4-byte aligned; + 1: not 2-byte aligned; null), so a call that is not refused would reach a
launch: run this where no GPU is present, like the test.  "@coef" stands for a host array of floats: the two entries that take coefficients
read them on the host, ldmae_sde_combine_f32 before its later checks.

Refusals that cannot be provoked, and are not listed:
  * the second "dtype %d (f32 or bf16)" of ldmae_row_mse and of ldmae_guidance_combine (the answer of dtype_dispatch): the same check on
    the code comes first in both entries.
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from ldmae_amd import _lib  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "flat_refusals.json")
NUL, COEF = None, "@coef"
F32, BF16, F16 = 0, 1, 2
A, B_, C_, D, E, F, G, H = (0x1000 * i for i in range(1, 9))       # eight dummy buffers 4096 bytes apart
N_MAX = 0x7fffffff * 4096                                           # the largest n one grid of 1024-item blocks covers


def materialize(args):
    return [(ctypes.c_float * 7)(*[0.5] * 7) if a == COEF else a for a in args]


def _args(names, defaults, k):
    a = dict(defaults)
    assert set(k) <= set(a), k
    a.update(k)
    return [a[n] for n in names.split()] + [None]               # + stream


def rk_stage(**k):
    return _args("y k ld coef m h out n t_dev ct t_out nt", dict(y=A, k=B_, ld=64, coef=COEF, m=3, h=C_, out=D, n=61, t_dev=E, ct=0.5, t_out=F, nt=3), k)


def finish(**k):
    return _args("y k ld h atol rtol y1 partial ratio n", dict(y=A, k=B_, ld=64, h=C_, atol=1e-3, rtol=1e-3, y1=D, partial=E, ratio=F, n=61), k)


def rms(**k):
    return _args("x y atol rtol partial out n", dict(x=A, y=B_, atol=1e-3, rtol=1e-3, partial=C_, out=D, n=61), k)


def interp(**k):
    return _args("y0 y1 ym k ld h t0 t_eval out n", dict(y0=A, y1=B_, ym=C_, k=D, ld=64, h=E, t0=F, t_eval=0.5, out=G, n=61), k)


def draw(**k):
    return _args("out n seed counter", dict(out=A, n=61, seed=7, counter=3), k)


def sde(**k):
    d = dict(in0=A, in1=B_, in2=NUL, in3=NUL, coef=COEF, m=2, z=C_, noise_coef=0.1, mode=1, seed=7, counter=3, out=D, mean_out=E, n=61, t_next=0.5,
             t_out=F, nt=3)
    return _args("in0 in1 in2 in3 coef m z noise_coef mode seed counter out mean_out n t_next t_out nt", d, k)


def rowdot(**k):
    return _args("a b out B m partial", dict(a=A, b=B_, out=C_, B=2, m=61, partial=D), k)


def plan(**k):
    d = dict(stored=A, idx=B_, t=C_, mean=D, std=E, mult=1.0, sample=1, seed=7, xt=F, ut=G, B=2, C=4, HW=16)
    return _args("stored idx t mean std mult sample seed xt ut B C HW", d, k)


def row_mse(**k):
    return _args("dtype a u loss B m partial", dict(dtype=F32, a=A, u=B_, loss=C_, B=2, m=61, partial=D), k)


def guide(**k):
    d = dict(rule=2, dtype=F32, pos=A, neg=B_, x=C_, t=D, mom=E, out=F, B=2, C=4, HW=16, k=2, scale=2.0, phi=0.5, eta=0.0, r=1.0, momentum=-0.5)
    return _args("rule dtype pos neg x t mom out B C HW k scale phi eta r momentum", d, k)


def cases():
    c = []

    def add(entry, what, args):
        c.append({"id": f"{entry[6:]}-{what}", "entry": entry, "args": args})

    def each(entry, make, **wrong):                                  # one call per keyword: that argument alone is wrong
        for name, v in wrong.items():
            add(entry, f"{name}_{'null' if v is None else v}", make(**{name: v}))

    e = "ldmae_rk_stage_f32"
    each(e, rk_stage, y=NUL, k=NUL, coef=NUL, h=NUL, out=NUL, n=0, m=0)
    add(e, "m_8", rk_stage(m=8))
    each(e, rk_stage, ld=60)
    add(e, "ld_multiple", rk_stage(ld=62, n=60))
    add(e, "y_misaligned", rk_stage(y=A + 4))
    add(e, "k_misaligned", rk_stage(k=B_ + 4))
    add(e, "out_misaligned", rk_stage(out=D + 4))
    each(e, rk_stage, t_dev=NUL, nt=0)
    add(e, "n_too_large", rk_stage(n=N_MAX + 1, ld=N_MAX + 4))
    e = "ldmae_dopri5_finish_f32"
    each(e, finish, y=NUL, k=NUL, h=NUL, y1=NUL, partial=NUL, ratio=NUL, n=0, ld=60)
    add(e, "ld_multiple", finish(ld=62, n=60))
    add(e, "y_misaligned", finish(y=A + 4))
    add(e, "k_misaligned", finish(k=B_ + 4))
    add(e, "y1_misaligned", finish(y1=D + 4))
    add(e, "y1_is_y", finish(y1=A))
    e = "ldmae_rms_norm_scaled_f32"
    each(e, rms, x=NUL, partial=NUL, out=NUL, n=0)
    add(e, "x_misaligned", rms(x=A + 4))
    add(e, "y_misaligned", rms(y=B_ + 4))
    add(e, "x_misaligned_as_y", rms(x=A + 4, y=NUL))
    e = "ldmae_dopri5_interp_f32"
    each(e, interp, y0=NUL, y1=NUL, ym=NUL, k=NUL, h=NUL, t0=NUL, out=NUL, n=0, ld=60)
    add(e, "ld_multiple", interp(ld=62, n=60))
    for name, base in (("y0", A), ("y1", B_), ("ym", C_), ("k", D), ("out", G)):
        add(e, f"{name}_misaligned", interp(**{name: base + 4}))
    e = "ldmae_dopri5_advance"
    for i, name in enumerate(("ratio", "h", "t", "status")):
        add(e, f"{name}_null", [NUL if j == i else (A, B_, C_, D)[j] for j in range(4)] + [None])
    e = "ldmae_dopri5_initial_step"
    add(e, "d_null", [NUL, 0, B_, None])
    add(e, "h_null", [A, 0, NUL, None])
    add(e, "phase_2", [A, 2, B_, None])
    add(e, "phase_negative", [A, -1, B_, None])
    for e in ("ldmae_rademacher_f32", "ldmae_normal_f32"):
        each(e, draw, out=NUL, n=0)
        add(e, "out_misaligned", draw(out=A + 2))
        add(e, "n_too_large", draw(n=N_MAX + 1))
    e = "ldmae_sde_combine_f32"
    each(e, sde, coef=NUL, out=NUL, n=0, m=0)
    add(e, "m_5", sde(m=5))
    each(e, sde, mode=-1)
    add(e, "mode_3", sde(mode=3))
    add(e, "z_missing", sde(z=NUL))
    add(e, "z_unasked", sde(mode=0))
    add(e, "z_unasked_philox", sde(mode=2))
    each(e, sde, nt=0)
    add(e, "t_out_misaligned", sde(t_out=F + 2))
    add(e, "n_too_large", sde(n=N_MAX + 1, t_out=NUL))
    each(e, sde, in0=NUL, in1=NUL)
    add(e, "in0_misaligned", sde(in0=A + 4))
    add(e, "in1_misaligned", sde(in1=B_ + 4))
    add(e, "out_misaligned", sde(out=D + 4))
    add(e, "mean_out_misaligned", sde(mean_out=E + 4))
    add(e, "z_misaligned", sde(z=C_ + 4))
    add(e, "mean_out_is_out", sde(mean_out=D))
    add(e, "mean_out_overlaps_out_above", sde(mean_out=D + 16))
    add(e, "mean_out_overlaps_out_below", sde(mean_out=D - 16))
    add(e, "out_overlaps_in0", sde(out=A + 16))
    add(e, "out_overlaps_in1", sde(out=B_ - 16))
    add(e, "mean_out_overlaps_in0", sde(mean_out=A + 16))
    add(e, "mean_out_overlaps_in1", sde(mean_out=B_ - 16))
    add(e, "out_overlaps_z", sde(out=C_ + 16))
    add(e, "mean_out_overlaps_z", sde(mean_out=C_ - 16))
    for name, base in (("in0", A), ("in1", B_), ("z", C_), ("out", D), ("mean_out", E)):
        add(e, f"t_out_overlaps_{name}", sde(t_out=base + 240))
        add(e, f"t_out_below_{name}", sde(t_out=base - 8))
    e = "ldmae_rowdot_f32"
    each(e, rowdot, a=NUL, b=NUL, out=NUL, partial=NUL, B=0, m=0)
    add(e, "a_misaligned", rowdot(a=A + 2))
    add(e, "b_misaligned", rowdot(b=B_ + 2))
    add(e, "too_many_blocks", rowdot(B=0x7fffffff, m=4097))
    e = "ldmae_likelihood_finish_f32"
    for i, name in enumerate(("sumsq", "delta")):
        add(e, f"{name}_null", [NUL if j == i else (A, B_)[j] for j in range(2)] + [0.5, C_, 2, None])
    add(e, "logp_null", [A, B_, 0.5, NUL, 2, None])
    add(e, "B_0", [A, B_, 0.5, C_, 0, None])
    e = "ldmae_fm_valid_plan_f32"
    each(e, plan, stored=NUL, idx=NUL, t=NUL, xt=NUL, ut=NUL, B=0, C=0, HW=0)
    add(e, "HW_multiple", plan(HW=18))
    each(e, plan, mean=NUL, std=NUL, sample=2)
    add(e, "sample_negative", plan(sample=-1))
    add(e, "stored_misaligned", plan(stored=A + 4))
    add(e, "xt_misaligned", plan(xt=F + 4))
    add(e, "ut_misaligned", plan(ut=G + 4))
    add(e, "idx_misaligned", plan(idx=B_ + 4))
    add(e, "t_misaligned", plan(t=C_ + 2))
    add(e, "ut_overlaps_xt_above", plan(ut=F + 16))
    add(e, "ut_overlaps_xt_below", plan(ut=F - 16))
    add(e, "too_many_blocks", plan(B=0x7fffffff, C=1, HW=1028, ut=1 << 48))
    e = "ldmae_row_mse"
    each(e, row_mse, dtype=F16)
    add(e, "dtype_unknown", row_mse(dtype=7))
    each(e, row_mse, a=NUL, u=NUL, loss=NUL, partial=NUL, B=0, m=0)
    add(e, "too_many_blocks", row_mse(B=0x7fffffff, m=4097))
    add(e, "a_misaligned_f32", row_mse(a=A + 2))
    add(e, "a_misaligned_bf16", row_mse(dtype=BF16, a=A + 1))
    add(e, "u_misaligned", row_mse(u=B_ + 2))
    e = "ldmae_guidance_combine"
    each(e, guide, rule=3, dtype=F16, pos=NUL, neg=NUL, out=NUL, B=0, C=0, HW=0, k=0)
    add(e, "rule_negative", guide(rule=-1))
    add(e, "k_5", guide(k=5))
    add(e, "pos_misaligned", guide(pos=A + 2))
    add(e, "neg_misaligned_bf16", guide(dtype=BF16, neg=B_ + 1))
    add(e, "out_misaligned", guide(out=F + 2))
    add(e, "out_is_pos_bf16", guide(dtype=BF16, out=A))
    add(e, "out_overlaps_pos", guide(out=A + 16))
    add(e, "out_overlaps_neg", guide(out=B_ - 16))
    add(e, "phi_negative", guide(rule=1, phi=-0.25))
    add(e, "phi_above_1", guide(rule=1, phi=1.5))
    add(e, "rescale_one_element", guide(rule=1, C=1, HW=1, k=1))
    each(e, guide, x=NUL, t=NUL)
    add(e, "x_misaligned", guide(x=C_ + 2))
    add(e, "t_misaligned", guide(t=D + 2))
    add(e, "mom_misaligned", guide(mom=E + 2))
    add(e, "norm_threshold_negative", guide(r=-1.0))
    add(e, "momentum_without_buffer", guide(mom=NUL))
    add(e, "out_overlaps_x", guide(out=C_ + 16))
    add(e, "mom_overlaps_out", guide(mom=F + 16))
    add(e, "mom_overlaps_pos", guide(mom=A + 16))
    add(e, "mom_overlaps_neg", guide(mom=B_ + 16))
    add(e, "mom_overlaps_x", guide(mom=C_ - 16))
    return c


def main():
    import torch
    if torch.cuda.is_available():
        sys.exit("run this where no GPU is present: a call that is not refused would launch a kernel on a dummy address")
    lib = _lib.load()
    out = cases()
    assert len({c["id"] for c in out}) == len(out)
    for c in out:
        c["rc"] = getattr(lib, c["entry"])(*materialize(c["args"]))
        c["message"] = _lib.last_error()
        if c["rc"] != -1:
            sys.exit(f"{c['id']}: not refused (rc {c['rc']}: {c['message']!r})")
    head = ("Recorded by tests/golden/make_golden_flat_refusals.py from the library of commit 9f442bc, BEFORE the flat kernels moved onto "
            "csrc/flat_common.h and the block sums onto csrc/common.h: the old behaviour, never the code under test.")
    with open(OUT, "w") as f:
        json.dump({"_comment": head, "cases": out}, f, indent=1)
        f.write("\n")
    print(f"{len(out)} refusals from {_lib.LIB_PATH} -> {OUT}")
    count = {}
    for c in out:
        count[c["entry"]] = count.get(c["entry"], 0) + 1
    print(count)


if __name__ == "__main__":
    main()
