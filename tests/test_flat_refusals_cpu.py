"""The flat f32 entry points refuse what they refused before their kernels shared one walker and one row reduction (csrc/flat_common.h)
and the host predicates moved to csrc/common.h, in the same words.

tests/golden/flat_refusals.json holds the calls of tests/golden/make_golden_flat_refusals.py against every entry of csrc/ode.hip and
csrc/fm_valid.hip and against ldmae_guidance_combine -- null pointer, empty, a slab row that is short or no multiple of 4, misalignment,
aliasing and partial overlap, an unknown mode / rule / dtype code, a problem beyond one grid -- with the return code and the exact
ldmae_last_error() text the library gave BEFORE that change (generated at the parent commit, so the file records the old behaviour and
not the code under test; the generator's docstring names the refusals that cannot be provoked).  Each call must return LDMAE_ERR_INVALID
(-1) with that text.  Every device pointer is a dummy: a check that went missing would reach the HIP runtime, which has no device on the
machines this test runs on, and return LDMAE_ERR_HIP (-2).  "@coef" in an argument list is a host array of floats.

With a GPU present the test skips itself: a missed check would launch a kernel on a dummy address.
"""
import ctypes
import json
import os

import pytest
import torch

from ldmae_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers: only where no kernel can be launched")

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flat_refusals.json")) as _f:
    CASES = json.load(_f)["cases"]

# entry -> the recorded calls it has (one per clause of each LDMAE_REQUIRE of the entry)
REFUSALS = {
    "ldmae_rk_stage_f32": 16, "ldmae_dopri5_finish_f32": 13, "ldmae_rms_norm_scaled_f32": 7, "ldmae_dopri5_interp_f32": 15,
    "ldmae_dopri5_advance": 4, "ldmae_dopri5_initial_step": 4, "ldmae_rademacher_f32": 4, "ldmae_normal_f32": 4, "ldmae_sde_combine_f32": 39,
    "ldmae_rowdot_f32": 9, "ldmae_likelihood_finish_f32": 4, "ldmae_fm_valid_plan_f32": 21, "ldmae_row_mse": 12, "ldmae_guidance_combine": 32,
}


def test_golden_covers_every_entry():
    count = {}
    for c in CASES:
        count[c["entry"]] = count.get(c["entry"], 0) + 1
        assert c["rc"] == -1 and c["message"], c
        assert len(c["args"]) == len(_lib.SIGNATURES[c["entry"]][1]), c["id"]
    assert count == REFUSALS


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_refusal_is_unchanged(case):
    args = [(ctypes.c_float * 7)(*[0.5] * 7) if a == "@coef" else a for a in case["args"]]
    rc = getattr(_lib.load(), case["entry"])(*args)
    msg = _lib.last_error()
    assert rc == -1, f"{case['id']} returned {rc}: {msg!r}"
    assert msg == case["message"]
