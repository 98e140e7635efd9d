"""The LightningDiT calls the C entry points it called before models/lightningdit.py got one block backward and one attention front end:
the same entry points in the same order, with the same scalars, the same optional outputs requested and the same streams, in every case of
tests/dit_trace.py (every arm of the attention front end and backward, both adaLN forms, the chain hand-offs, direct gradient accumulation,
the input-gradient-only backward, forward-only sampling cold and warm, the MXFP8 mode, the stand-alone Attention module and block).
tests/golden/dit_call_trace.json was recorded at the parent of that change (tests/golden/make_golden_dit_trace.py, which also says how a
change that alters launches on purpose regenerates it)."""
import json
import os

import pytest

import dit_trace as T

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(T.switch_set() is not None, reason=f"{T.switch_set()} is set: the golden trace is that of the default environment")]

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dit_call_trace.json")) as _f:
    GOLDEN = json.load(_f)


def test_golden_covers_every_case():
    assert list(GOLDEN) == T.IDS
    for case in T.CASES:
        T.check_branch(case, GOLDEN[case["id"]])


@pytest.mark.parametrize("case", T.CASES, ids=T.IDS)
def test_launches_are_unchanged(case):
    log, _ = T.run_case(case)
    want = GOLDEN[case["id"]]
    first = next((i for i, (a, b) in enumerate(zip(log, want)) if a != b), min(len(log), len(want)))
    assert log == want, (f"{len(log)} calls, {len(want)} recorded; first difference at call {first}: "
                         f"{log[first] if first < len(log) else None} against {want[first] if first < len(want) else None}")
