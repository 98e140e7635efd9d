"""The eight convolution entry points refuse what they refused before they shared csrc/conv_igemm_common.h, in the same words.

tests/golden/conv_refusals.json holds one call per LDMAE_REQUIRE of ldmae_conv2d_nhwc_f32, ldmae_conv3x3_relu_dgrad_nhwc_{f32,bf16},
ldmae_conv3x3_relu_nhwc_f16, ldmae_conv3x3_vae_nhwc_{f32,f16} and ldmae_conv1x1_res_nhwc_{f32,f16} -- null pointer, non-positive size, channel
multiple, misalignment (pointer 20), bad mode, fp16 input outside plain mode, norm-act without statistics, Cin % G, down on a 1 x N image,
channel slice out of range, kernel larger than the padded input, each "too large" bound -- with the return code and the exact
ldmae_last_error() text the library gave BEFORE that change (tests/golden/make_golden_conv_refusals.py: generated at the parent commit, so
the file records the old behaviour and not the code under test).  Each call must return LDMAE_ERR_INVALID (-1) with that text.  Every
pointer is a dummy (16, 20 or null): a check that went missing would reach the HIP runtime, which has no device on the machines this test
runs on, and return LDMAE_ERR_HIP (-2).

With a GPU present the test skips itself: a missed check would launch a kernel on address 16.  tests/test_gpu_conv_vae.py and
tests/test_gpu_conv_vae_tf32.py make the entry-point refusals there on real buffers.
"""
import json
import os

import pytest
import torch

from ldmae_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers: only where no kernel can be launched")

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_refusals.json")) as _f:
    CASES = json.load(_f)["cases"]

# entry -> the refusals it has today (the LDMAE_REQUIREs of the entry and of the geometry helper it calls, one call each)
REFUSALS = {
    "ldmae_conv2d_nhwc_f32": 7, "ldmae_conv3x3_relu_dgrad_nhwc_f32": 7, "ldmae_conv3x3_relu_dgrad_nhwc_bf16": 8,
    "ldmae_conv3x3_relu_nhwc_f16": 8, "ldmae_conv3x3_vae_nhwc_f32": 14, "ldmae_conv3x3_vae_nhwc_f16": 16,
    "ldmae_conv1x1_res_nhwc_f32": 7, "ldmae_conv1x1_res_nhwc_f16": 8,
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
