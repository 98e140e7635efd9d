"""The flat f32 kernels, the two-stage row reductions and every kernel on the shared 256-thread block sum give the bits they gave before
they shared csrc/flat_common.h and the reductions of csrc/common.h.

tests/golden/flat_bits.json holds one SHA-256 of the raw output bytes per case of tests/golden/make_golden_flat_bits.py, recorded on an
MI355X from the tree of the parent commit (named in the file), so it records the old behaviour and not the code under test.  The cases
are computed once, by the generator's own cases(): hash-made inputs, the smallest shapes at which the walker, its tail, the chunk map and
each block sum can go wrong (the generator's docstring lists them)."""
import json
import os

import pytest
import torch

from make_golden_flat_bits import cases, digest

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flat_bits.json")) as _f:
    GOLDEN = json.load(_f)["sha256"]


@pytest.fixture(scope="module")
def computed():
    from ldmae_amd import _lib, ops
    assert _lib.load().ldmae_arch() == b"gfx950"
    out = {name: digest(outputs) for name, outputs in cases(ops, torch)}
    torch.cuda.synchronize()
    return out


def test_every_recorded_case_is_computed(computed):
    assert sorted(computed) == sorted(GOLDEN)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_bits_are_unchanged(computed, name):
    assert computed[name] == GOLDEN[name]
