"""train.dispersive without a GPU: parsing and defaults, every refusal (all of them when the configuration is read), the two symbols in the
header and the library, the split plan's host arithmetic, the ops refusals that need no device, and create_transport's unchanged signature."""
import copy
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ldmae_amd import _lib, ops, train_accum as ta                      # noqa: E402
from ldmae_amd.transport import create_transport                        # noqa: E402
from ldmae_amd.transport.transport import Transport, dispersive_options  # noqa: E402

IMAGENET = os.path.join(ROOT, "ldmae_amd", "configs", "imagenet", "lightningdit_b_vmae_f8d16_cfg.yaml")
CELEBA = os.path.join(ROOT, "ldmae_amd", "configs", "celeba_hq", "lightningdit_b_vmae_f8d16_cfg.yaml")
NEW_SYMBOLS = ("ldmae_dispersive_fwd", "ldmae_dispersive_bwd", "ldmae_dispersive_slabs", "ldmae_dispersive_workspace_bytes")


def config(path=IMAGENET, **dispersive):
    c = yaml.safe_load(open(path))
    c['train']['dispersive'] = dispersive
    return c


# ----------------------------------------------------------------------------- parsing and defaults
def test_the_key_is_absent_from_the_shipped_configurations():
    for path in (IMAGENET, CELEBA):
        c = yaml.safe_load(open(path))
        assert 'dispersive' not in c['train'] and ta.dispersive_config(c, 12) is None


def test_defaults_and_every_key():
    assert ta.dispersive_config(config(), 12) == {"weight": 0.5, "tau": 0.5, "block": 3}             # block = depth // 4, counted from 0
    assert ta.dispersive_config(config(), 28)["block"] == 7 and ta.dispersive_config(config(), 2)["block"] == 0
    got = ta.dispersive_config(config(weight=0.25, tau=1, block=11), 12)
    assert got == {"weight": 0.25, "tau": 1.0, "block": 11} and type(got["tau"]) is float and type(got["block"]) is int
    assert ta.dispersive_config(config(weight=0), 12)["weight"] == 0.0                               # weight 0 is allowed: the term is logged only
    # the YAML text a user writes
    c = yaml.safe_load("train:\n  global_batch_size: 256\n  dispersive: {weight: 0.5, tau: 0.5}\nmodel: {}\n")
    assert ta.dispersive_config(c, 12) == {"weight": 0.5, "tau": 0.5, "block": 3}


@pytest.mark.parametrize("bad,word", [
    (dict(weight=-0.1), "train.dispersive.weight"), (dict(weight="0.5"), "train.dispersive.weight"), (dict(weight=float("nan")), "train.dispersive.weight"),
    (dict(tau=0), "train.dispersive.tau"), (dict(tau=-1.0), "train.dispersive.tau"), (dict(tau=float("inf")), "train.dispersive.tau"),
    (dict(tau=True), "train.dispersive.tau"),
    (dict(block=12), "train.dispersive.block"), (dict(block=-1), "train.dispersive.block"), (dict(block=1.0), "train.dispersive.block"),
    (dict(block=True), "train.dispersive.block"), (dict(blocks=[1, 2]), "train.dispersive must be a mapping"),
])
def test_refusals_name_the_key(bad, word):
    with pytest.raises(ValueError, match=re.escape(word)):
        ta.dispersive_config(config(**bad), 12)


def test_refusals_of_the_surrounding_configuration():
    c = config()
    c['train']['dispersive'] = [0.5, 0.5]
    with pytest.raises(ValueError, match="train.dispersive must be a mapping"):
        ta.dispersive_config(c, 12)
    c = config()
    c['train']['global_batch_size'] = 8
    with pytest.raises(ValueError, match="per-GPU batch of at least 2"):
        ta.dispersive_config(c, 12, world=8)
    assert ta.dispersive_config(c, 12, world=4) is not None
    c = config()
    c['model']['use_checkpoint'] = True
    with pytest.raises(ValueError, match="use_checkpoint"):
        ta.dispersive_config(c, 12)
    # the absent key never looks at the rest
    c = yaml.safe_load(open(IMAGENET))
    c['model']['use_checkpoint'] = True
    c['train']['global_batch_size'] = 1
    assert ta.dispersive_config(c, 12) is None


def test_transport_takes_the_option_by_keyword_only():
    """create_transport keeps the reference's positional order; dispersive is keyword-only and None by default."""
    p = inspect.signature(create_transport).parameters
    names = list(p)
    assert names == ["path_type", "prediction", "loss_weight", "train_eps", "sample_eps", "use_cosine_loss", "use_lognorm", "partitial_train",
                     "partial_ratio", "shift_lg", "dispersive"]
    assert [p[n].kind for n in names[:-1]] == [inspect.Parameter.POSITIONAL_OR_KEYWORD] * 10
    assert [p[n].default for n in names[:-1]] == ['Linear', "velocity", None, None, None, None, None, None, 1.0, False]
    assert p["dispersive"].kind is inspect.Parameter.KEYWORD_ONLY and p["dispersive"].default is None
    assert inspect.signature(Transport.__init__).parameters["dispersive"].kind is inspect.Parameter.KEYWORD_ONLY
    assert create_transport("Linear", "velocity", None, None, None).dispersive is None
    opt = dispersive_options({"tau": 0.25}, 4)
    assert create_transport(dispersive=opt).dispersive == {"weight": 0.5, "tau": 0.25, "block": 1}
    with pytest.raises(TypeError):
        create_transport("Linear", "velocity", None, None, None, None, None, None, 1.0, False, opt)


def test_transport_refuses_a_model_without_a_tap():
    tr = create_transport(dispersive=dispersive_options({}, 4))
    torch.manual_seed(0)
    with pytest.raises(RuntimeError, match="tap_block"):
        tr.training_losses(lambda x, t: x, torch.zeros(2, 4, 2, 2))


# ----------------------------------------------------------------------------- the model's tap, as far as it goes without a device
def _dit(**over):
    from ldmae_amd.models.lightningdit import LightningDiT
    kw = dict(input_size=8, patch_size=1, in_channels=16, hidden_size=192, depth=4, num_heads=3, num_classes=10, use_qknorm=True, use_swiglu=True,
              use_rope=True, use_rmsnorm=True)
    kw.update(over)
    return LightningDiT(**kw)


def test_tap_block_refusals_and_state():
    m = _dit()
    assert m._tap is None and m.tapped is None and "tapped" not in m.state_dict() and "_tap" not in m.state_dict()
    for bad in (4, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="tap_block index"):
            with m.tap_block(bad):
                pass
    with m.tap_block(1) as mm:
        assert mm is m and m._tap == 1
        with pytest.raises(NotImplementedError, match="input_grad_only"):
            with m.input_grad_only():
                m(torch.zeros(2, 16, 8, 8, requires_grad=True), torch.zeros(2), torch.zeros(2, dtype=torch.long))
    assert m._tap is None and m.tapped is None
    with m.input_grad_only():
        with pytest.raises(NotImplementedError, match="tap_block with input_grad_only"):
            with m.tap_block(1):
                pass
    with pytest.raises(NotImplementedError, match="tap_block with use_checkpoint"):
        with _dit(use_checkpoint=True).tap_block(1):
            pass


# ----------------------------------------------------------------------------- the library
def test_new_symbols_in_header_signatures_and_library():
    header = open(os.path.join(ROOT, "include", "ldmae_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        m = re.search(r"^(?:int|long) " + name + r"\s*\(([^;]*?)\)\s*;", header, re.S | re.M)      # the prototype, not a mention in the contract
        assert m, name + " is not declared in include/ldmae_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
        assert hasattr(handle, name), name
    C = ctypes
    assert _lib.SIGNATURES["ldmae_dispersive_fwd"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_void_p, C.c_void_p])
    assert _lib.SIGNATURES["ldmae_dispersive_bwd"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_long, C.c_void_p])
    for text in ("d_ij = ||z_i - z_j||^2", "L    = log S - 2 log B", "C_ij = 4 / (S K tau) (e_ij - delta_ij r_i)"):
        assert text in header, text


def test_split_plan_and_workspace_are_host_arithmetic():
    """slab = max(1024, ceil(K pairs / 512) rounded up to 64) with pairs = T (T + 1) / 2, T = ceil(B / 128); workspace = r [B] f64 (rounded up
    to 16 bytes) + (slabs + 1) B^2 f32.  The bench shape: 171 slabs of 4608, 45 MB."""
    lib = _lib.load()

    def plan(B, K):
        T = -(-B // 128)
        pairs = T * (T + 1) // 2
        slab = max(1024, -(-(-(-K * pairs // 512)) // 64) * 64)
        return -(-K // slab), slab

    for B, K in [(1, 64), (2, 64), (5, 1000), (37, 4100), (130, 2052), (256, 4096), (8, 3172), (256, 786432), (1024, 786432), (129, 1 << 20), (1, 4)]:
        slabs, _ = plan(B, K)
        assert lib.ldmae_dispersive_slabs(B, K) == slabs, (B, K)
        assert lib.ldmae_dispersive_workspace_bytes(B, K) == (B * 8 + 15) // 16 * 16 + (slabs + 1) * B * B * 4, (B, K)
    assert plan(256, 786432) == (171, 4608) and plan(8, 3172) == (4, 1024) and 3172 % 1024 % 64 != 0
    assert lib.ldmae_dispersive_workspace_bytes(256, 786432) == 2048 + 172 * 65536 * 4
    for B, K in [(0, 64), (1025, 64), (4, 62), (4, 0)]:
        assert lib.ldmae_dispersive_slabs(B, K) == -1 and lib.ldmae_dispersive_workspace_bytes(B, K) == -1
    assert "dispersive" in _lib.last_error()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """LDMAE_ERR_INVALID with a message that names the problem, from host pointers that are never dereferenced."""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p16 = (p + 15) // 16 * 16
    for args, word in [((p16, p16 + 128, p16 + 160, 1025, 4, 0.5, p16 + 192, None), "B = 1025"),
                       ((p16, p16 + 128, p16 + 160, 2, 6, 0.5, p16 + 192, None), "K = 6"),
                       ((p16, p16 + 128, p16 + 160, 2, 4, 0.0, p16 + 192, None), "tau"),
                       ((p16 + 4, p16 + 128, p16 + 160, 2, 4, 0.5, p16 + 192, None), "aligned"),
                       ((p16, p16 + 128, p16 + 16, 2, 4, 0.5, p16 + 192, None), "overlap"),
                       ((None, p16 + 128, p16 + 160, 2, 4, 0.5, p16 + 192, None), "null")]:
        assert lib.ldmae_dispersive_fwd(*args) == -1 and word in _lib.last_error(), (word, _lib.last_error())
    for args, word in [((p16, p16 + 64, 1.0, p16 + 128, 0, 4, None), "B = 0"), ((p16, p16 + 64, 1.0, p16 + 128, 2, 10, None), "K = 10"),
                       ((p16, p16 + 64, 1.0, p16 + 72, 2, 4, None), "aligned"), ((p16, p16 + 64, 1.0, p16 + 80, 2, 4, None), "overlaps")]:
        assert lib.ldmae_dispersive_bwd(*args) == -1 and word in _lib.last_error(), (word, _lib.last_error())


def test_ops_refuse_by_name_without_a_device():
    """The checks of ops._arg come before any device work: dtype, layout, K % 4, B > 1024 name the argument."""
    z = torch.zeros(4, 64)
    for bad, word in [(z.double(), "dispersive_fwd z: dtype"), (z.t(), "dispersive_fwd z: the kernel reads a contiguous tensor"),
                      (torch.zeros(4, 62), "dispersive_fwd z: K = 62"), (torch.zeros(1025, 4), "dispersive_fwd z: B = 1025"),
                      (torch.zeros(4, 8, 8), "dispersive_fwd z: shape")]:
        with pytest.raises(RuntimeError, match=re.escape(word)):
            ops.dispersive_fwd(bad, 0.5)
    with pytest.raises(RuntimeError, match="dispersive_fwd tau"):
        ops.dispersive_fwd(z, 0.0)
    with pytest.raises(RuntimeError, match=re.escape("dispersive_bwd C: shape")):
        ops.dispersive_bwd(torch.zeros(4, 5), z, 1.0)
    with pytest.raises(RuntimeError, match=re.escape("dispersive_bwd out: shape")):
        ops.dispersive_bwd(torch.zeros(4, 4), z, 1.0, out=torch.zeros(4, 60))
    with pytest.raises(RuntimeError, match=re.escape("dispersive_bwd out: dtype")):
        ops.dispersive_bwd(torch.zeros(4, 4), z, 1.0, out=torch.zeros(4, 64, dtype=torch.bfloat16))
