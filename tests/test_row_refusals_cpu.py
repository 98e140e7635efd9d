"""The norm + modulate and gate row entry points refuse what they refused before the row kernels shared csrc/norm_mod_rows.inc and the
backward entries one named argument struct, in the same words.

tests/golden/row_refusals.json holds the calls of tests/golden/make_golden_row_refusals.py against ldmae_rmsnorm_modulate_fwd,
ldmae_layernorm_modulate_fwd, ldmae_res_rmsnorm_modulate_fwd, ldmae_rmsnorm_modulate_bwd(_gate(_recompute)),
ldmae_layernorm_modulate_bwd(_gate), ldmae_gate_bwd and ldmae_rmsnorm_modulate_fwd_mx8 -- null pointer, empty, D % 4, mod_ld % 4,
gate_ld % 4, M % rows_per_batch, beta_x outside {0, 1}, recompute with a dtype that is not bf16, an unknown dtype code, xout == x,
misalignment, D > 2048 -- with the return code and the exact ldmae_last_error() text the library gave BEFORE that change (generated at
the parent commit, so the file records the old behaviour and not the code under test; the generator's docstring names the refusals that
cannot be provoked).  Each call must return LDMAE_ERR_INVALID (-1) with that text.  Every pointer is a dummy (16, 18, 20, 32 or null): a
check that went missing would reach the HIP runtime, which has no device on the machines this test runs on, and return LDMAE_ERR_HIP (-2).

With a GPU present the test skips itself: a missed check would launch a kernel on address 16.  tests/test_gpu_row_paths.py makes
entry-point refusals there on real buffers.
"""
import json
import os

import pytest
import torch

from ldmae_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers: only where no kernel can be launched")

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_refusals.json")) as _f:
    CASES = json.load(_f)["cases"]

# entry -> the recorded calls it has (one per clause of each LDMAE_REQUIRE of the entry, of the core it forwards to and of row_nch_dispatch)
REFUSALS = {
    "ldmae_rmsnorm_modulate_fwd": 9, "ldmae_layernorm_modulate_fwd": 8, "ldmae_res_rmsnorm_modulate_fwd": 15,
    "ldmae_rmsnorm_modulate_bwd": 8, "ldmae_rmsnorm_modulate_bwd_gate": 10, "ldmae_rmsnorm_modulate_bwd_gate_recompute": 10,
    "ldmae_layernorm_modulate_bwd": 7, "ldmae_layernorm_modulate_bwd_gate": 9, "ldmae_gate_bwd": 9, "ldmae_rmsnorm_modulate_fwd_mx8": 7,
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
    rc = getattr(_lib.load(), case["entry"])(*case["args"])
    msg = _lib.last_error()
    assert rc == -1, f"{case['id']} returned {rc}: {msg!r}"
    assert msg == case["message"]
