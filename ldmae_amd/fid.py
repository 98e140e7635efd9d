"""FID evaluation on the MI355X: pytorch-fid's Inception-v3 feature extractor in HIP (csrc/inception.hip) and the interface of the
reference's tools/calculate_fid.py (calculate_fid_given_paths, compute_statistics_of_path, calculate_frechet_distance).

The network is pytorch-fid's fid_inception_v3() (calculate_fid.py:64-425 of the reference): 94 BasicConv2d layers (conv without bias ->
BatchNorm eps 1e-3 -> ReLU) in NHWC f32.  BatchNorm is folded into each conv's weight and bias in f64 at load time; every conv runs on the
exact-f32 MFMA, every pool / resize / statistic on a kernel of this package.  Features are accumulated into f64 mean / covariance sums on
the device, so 50 000 x 2048 activations never reach the host.

Weights: the user's pt_inception-2015-12-05-6726825d.pth (a torchvision-style state dict), found from the `weights=` argument, then
$LDMAE_FID_WEIGHTS, then torch.hub's checkpoint directory (where the reference's loader has already put it).  Nothing is downloaded.

    python -m ldmae_amd.fid PATH1 PATH2 [--batch-size 50] [--dims 2048] [--weights P] [--sp-len N]
    python -m ldmae_amd.fid --save-stats SRC_FOLDER DST.npz
"""
from __future__ import annotations

import argparse
import os
import pathlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

WEIGHTS_NAME = "pt_inception-2015-12-05-6726825d.pth"
WEIGHTS_ENV = "LDMAE_FID_WEIGHTS"
IMAGE_EXTENSIONS = {"bmp", "jpg", "jpeg", "pgm", "png", "ppm", "tif", "tiff", "webp"}      # calculate_fid.py:431
BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}                                     # InceptionV3.BLOCK_INDEX_BY_DIM
BN_EPS = 1e-3
MAX_DECODE_THREADS = 16


def _layer_table():
    """name -> (Cin, Cout, kh, kw, stride, ph, pw), in execution order: torchvision's Inception3.__init__ with pytorch-fid's FID blocks."""
    t = {}

    def c(name, cin, cout, k, s=1, p=(0, 0)):
        kh, kw = (k, k) if isinstance(k, int) else k
        t[name] = (cin, cout, kh, kw, s, p[0], p[1])

    c("Conv2d_1a_3x3", 3, 32, 3, 2)
    c("Conv2d_2a_3x3", 32, 32, 3)
    c("Conv2d_2b_3x3", 32, 64, 3, 1, (1, 1))
    c("Conv2d_3b_1x1", 64, 80, 1)
    c("Conv2d_4a_3x3", 80, 192, 3)
    for blk, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        c(f"{blk}.branch1x1", cin, 64, 1)
        c(f"{blk}.branch5x5_1", cin, 48, 1)
        c(f"{blk}.branch5x5_2", 48, 64, 5, 1, (2, 2))
        c(f"{blk}.branch3x3dbl_1", cin, 64, 1)
        c(f"{blk}.branch3x3dbl_2", 64, 96, 3, 1, (1, 1))
        c(f"{blk}.branch3x3dbl_3", 96, 96, 3, 1, (1, 1))
        c(f"{blk}.branch_pool", cin, pf, 1)
    c("Mixed_6a.branch3x3", 288, 384, 3, 2)
    c("Mixed_6a.branch3x3dbl_1", 288, 64, 1)
    c("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 1, (1, 1))
    c("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 2)
    for blk, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        c(f"{blk}.branch1x1", 768, 192, 1)
        c(f"{blk}.branch7x7_1", 768, c7, 1)
        c(f"{blk}.branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        c(f"{blk}.branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        c(f"{blk}.branch7x7dbl_1", 768, c7, 1)
        c(f"{blk}.branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        c(f"{blk}.branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        c(f"{blk}.branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        c(f"{blk}.branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        c(f"{blk}.branch_pool", 768, 192, 1)
    c("Mixed_7a.branch3x3_1", 768, 192, 1)
    c("Mixed_7a.branch3x3_2", 192, 320, 3, 2)
    c("Mixed_7a.branch7x7x3_1", 768, 192, 1)
    c("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
    c("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    c("Mixed_7a.branch7x7x3_4", 192, 192, 3, 2)
    for blk, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        c(f"{blk}.branch1x1", cin, 320, 1)
        c(f"{blk}.branch3x3_1", cin, 384, 1)
        c(f"{blk}.branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
        c(f"{blk}.branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        c(f"{blk}.branch3x3dbl_1", cin, 448, 1)
        c(f"{blk}.branch3x3dbl_2", 448, 384, 3, 1, (1, 1))
        c(f"{blk}.branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
        c(f"{blk}.branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        c(f"{blk}.branch_pool", cin, 192, 1)
    return t


LAYERS = _layer_table()
# 1x1 convs of one Mixed block that read the same input and feed only further convs: run as ONE GEMM with concatenated weights into a scratch
# tensor whose channel slices the next convs read (one pass over the block input instead of two)
FUSED_1X1 = {f"{b}": (f"{b}.branch5x5_1", f"{b}.branch3x3dbl_1") for b in ("Mixed_5b", "Mixed_5c", "Mixed_5d")}
FUSED_1X1.update({b: (f"{b}.branch7x7_1", f"{b}.branch7x7dbl_1") for b in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e")})
FUSED_1X1["Mixed_7a"] = ("Mixed_7a.branch3x3_1", "Mixed_7a.branch7x7x3_1")
FUSED_1X1.update({b: (f"{b}.branch3x3_1", f"{b}.branch3x3dbl_1") for b in ("Mixed_7b", "Mixed_7c")})


def param_shapes():
    """Every conv / bn key of the state dict with its shape (fc.* and bn.num_batches_tracked are accepted and ignored)."""
    out = {}
    for name, (cin, cout, kh, kw, *_) in LAYERS.items():
        out[f"{name}.conv.weight"] = (cout, cin, kh, kw)
        for k in ("weight", "bias", "running_mean", "running_var"):
            out[f"{name}.bn.{k}"] = (cout,)
    return out


# input resolution of every conv (after the 299 x 299 resize): the stride-2 convs end their branches, so a block's convs all read its input size
_INPUT_HW = {"Conv2d_1a_3x3": 299, "Conv2d_2a_3x3": 149, "Conv2d_2b_3x3": 147, "Conv2d_3b_1x1": 73, "Conv2d_4a_3x3": 73,
             "Mixed_5b": 35, "Mixed_5c": 35, "Mixed_5d": 35, "Mixed_6a": 35, "Mixed_6b": 17, "Mixed_6c": 17, "Mixed_6d": 17, "Mixed_6e": 17,
             "Mixed_7a": 17, "Mixed_7b": 8, "Mixed_7c": 8}


def conv_geometries():
    """name -> (H, W, Cin, Cout, kh, kw, stride, ph, pw, Ho, Wo) of the 94 convolutions of one 299 x 299 image."""
    out = {}
    for name, (cin, cout, kh, kw, s, ph, pw) in LAYERS.items():
        h = w = _INPUT_HW[name.split(".")[0]]
        out[name] = (h, w, cin, cout, kh, kw, s, ph, pw, (h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1)
    return out


def conv_flops_per_image():
    """2 x multiply-adds of the 94 convolutions for one image (pools, resize and the statistics not counted): 11.42 GFLOP."""
    return sum(2 * ho * wo * cout * kh * kw * cin for (_, _, cin, cout, kh, kw, _, _, _, ho, wo) in conv_geometries().values())


def random_state_dict(seed=0):
    """A state dict in the real key set and layout with random values that keep activations O(1) through all 94 layers: He-scaled conv
    weights, gamma in [0.5, 1.5], beta and running_mean ~ N(0, 0.1), running_var in [0.5, 2] (tests and tools/bench_fid.py)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, (cin, cout, kh, kw, *_) in LAYERS.items():
        sd[f"{name}.conv.weight"] = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
        sd[f"{name}.bn.weight"] = torch.rand(cout, generator=g) + 0.5
        sd[f"{name}.bn.bias"] = torch.randn(cout, generator=g) * 0.1
        sd[f"{name}.bn.running_mean"] = torch.randn(cout, generator=g) * 0.1
        sd[f"{name}.bn.running_var"] = torch.rand(cout, generator=g) * 1.5 + 0.5
        sd[f"{name}.bn.num_batches_tracked"] = torch.tensor(0)
    sd["fc.weight"] = torch.zeros(1008, 2048)
    sd["fc.bias"] = torch.zeros(1008)
    return sd


def check_state_dict(sd):
    """Refuse a missing, extra or wrongly shaped conv / bn key, naming it."""
    want = param_shapes()
    ignored = {"fc.weight", "fc.bias"} | {f"{n}.bn.num_batches_tracked" for n in LAYERS}
    missing = [k for k in want if k not in sd]
    if missing:
        raise KeyError(f"Inception state dict lacks {missing[0]}" + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
    extra = [k for k in sd if k not in want and k not in ignored]
    if extra:
        raise KeyError(f"Inception state dict has an unexpected key {extra[0]}" + (f" (and {len(extra) - 1} more)" if len(extra) > 1 else ""))
    for k, shape in want.items():
        if tuple(sd[k].shape) != shape:
            raise ValueError(f"Inception state dict: {k} has shape {tuple(sd[k].shape)}, expected {shape}")


def fold_bn(sd):
    """name -> (weight [Cout, kh, kw, Cin] f32, bias [Cout] f32): BatchNorm(eps 1e-3) folded into the bias-free conv in f64, the weight packed
    channels-last (the kernel's K order: ky, kx, ci)."""
    check_state_dict(sd)
    out = {}
    for name in LAYERS:
        w = sd[f"{name}.conv.weight"].double()
        gamma, beta = sd[f"{name}.bn.weight"].double(), sd[f"{name}.bn.bias"].double()
        mean, var = sd[f"{name}.bn.running_mean"].double(), sd[f"{name}.bn.running_var"].double()
        scale = gamma / torch.sqrt(var + BN_EPS)
        wf = (w * scale[:, None, None, None]).permute(0, 2, 3, 1).contiguous().float()
        bf = (beta - mean * scale).float()
        out[name] = (wf, bf)
    return out


def weight_locations(weights=None):
    """The three places looked at, in order: the argument, $LDMAE_FID_WEIGHTS, torch.hub's checkpoint directory."""
    hub = os.path.join(torch.hub.get_dir(), "checkpoints", WEIGHTS_NAME)
    return [("weights= argument", weights), (f"${WEIGHTS_ENV}", os.environ.get(WEIGHTS_ENV)), ("torch.hub checkpoints", hub)]


def resolve_weights(weights=None):
    """Path of the Inception weights, or FileNotFoundError naming every place looked at.  Never downloads."""
    locs = weight_locations(weights)
    for _, p in locs:
        if p and os.path.isfile(p):
            return p
    where = "; ".join(f"{what}: {p if p else '(not set)'}" for what, p in locs)
    raise FileNotFoundError(f"Inception FID weights {WEIGHTS_NAME} not found ({where}).  Place the file in one of these; "
                            "this package never downloads it.")


class InceptionFID:
    """pytorch-fid's InceptionV3([BLOCK_INDEX_BY_DIM[dims]]) on the HIP kernels.  features(uint8 [B, H, W, 3]) -> f32 [B, dims] on the device:
    the block output followed by a global average, as get_activations does."""

    def __init__(self, weights=None, dims=2048, device="cuda", state_dict=None, fuse_1x1=True):
        from . import ops
        self._ops = ops
        if dims not in BLOCK_INDEX_BY_DIM:
            raise ValueError(f"dims must be one of {sorted(BLOCK_INDEX_BY_DIM)}, got {dims}")
        self.dims, self.block = dims, BLOCK_INDEX_BY_DIM[dims]
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"InceptionFID runs on a HIP device (no CPU fallback); got {device}")
        if state_dict is None:
            self.weights_path = resolve_weights(weights)
            state_dict = torch.load(self.weights_path, map_location="cpu", weights_only=True)
        folded = fold_bn(state_dict)
        self.fuse_1x1 = fuse_1x1
        if fuse_1x1:
            for blk, (a, b) in FUSED_1X1.items():
                folded[f"{blk}.fused_1x1"] = (torch.cat([folded[a][0], folded[b][0]]), torch.cat([folded[a][1], folded[b][1]]))
        self.params = {k: (w.to(self.device), b.to(self.device)) for k, (w, b) in folded.items()}
        self._fc_weight_src = state_dict.get("fc.weight")      # the ADM softmax graph's weight (adm_logits_weight); not used by features()
        self._fc_weight = None

    # ---------------------------------------------------------------- building blocks
    def _conv(self, name, x, xoff=0, out=None, ooff=0):
        w, b = self.params[name]
        geo = LAYERS.get(name)
        s, ph, pw = (geo[4], geo[5], geo[6]) if geo else (1, 0, 0)
        return self._ops.conv2d_nhwc(x, w, b, (s, s), (ph, pw), True, xoff, w.shape[3], out, ooff)

    def _pair_1x1(self, blk, x):
        """(tensor, offset of the first conv's channels, offset of the second's) of the two shared-input 1x1 convs of a block."""
        a, b = FUSED_1X1[blk]
        if self.fuse_1x1:
            return self._conv(f"{blk}.fused_1x1", x), 0, LAYERS[a][1]
        ta, tb = self._conv(a, x), self._conv(b, x)
        return (ta, tb), 0, 0

    @staticmethod
    def _pick(t, i):
        return t[i] if isinstance(t, tuple) else t

    def _empty(self, x, h, w, c):
        return torch.empty(x.shape[0], h, w, c, dtype=torch.float32, device=self.device)

    def _block_a(self, blk, x):
        B, H, W, _ = x.shape
        pf = LAYERS[f"{blk}.branch_pool"][1]
        out = self._empty(x, H, W, 224 + pf)
        self._conv(f"{blk}.branch1x1", x, out=out, ooff=0)
        t, oa, ob = self._pair_1x1(blk, x)
        self._conv(f"{blk}.branch5x5_2", self._pick(t, 0), oa, out=out, ooff=64)
        d = self._conv(f"{blk}.branch3x3dbl_2", self._pick(t, 1), ob)
        self._conv(f"{blk}.branch3x3dbl_3", d, out=out, ooff=128)
        p = self._ops.pool2d_nhwc(x, "avg", 3, 1, 1)
        self._conv(f"{blk}.branch_pool", p, out=out, ooff=224)
        return out

    def _block_b(self, x):
        B, H, W, C = x.shape
        ho, wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        out = self._empty(x, ho, wo, 384 + 96 + C)
        self._conv("Mixed_6a.branch3x3", x, out=out, ooff=0)
        d = self._conv("Mixed_6a.branch3x3dbl_1", x)
        d = self._conv("Mixed_6a.branch3x3dbl_2", d)
        self._conv("Mixed_6a.branch3x3dbl_3", d, out=out, ooff=384)
        self._ops.pool2d_nhwc(x, "max", 3, 2, 0, out=out, ooff=480)
        return out

    def _block_c(self, blk, x):
        B, H, W, _ = x.shape
        out = self._empty(x, H, W, 768)
        self._conv(f"{blk}.branch1x1", x, out=out, ooff=0)
        t, oa, ob = self._pair_1x1(blk, x)
        a = self._conv(f"{blk}.branch7x7_2", self._pick(t, 0), oa)
        self._conv(f"{blk}.branch7x7_3", a, out=out, ooff=192)
        d = self._conv(f"{blk}.branch7x7dbl_2", self._pick(t, 1), ob)
        d = self._conv(f"{blk}.branch7x7dbl_3", d)
        d = self._conv(f"{blk}.branch7x7dbl_4", d)
        self._conv(f"{blk}.branch7x7dbl_5", d, out=out, ooff=384)
        p = self._ops.pool2d_nhwc(x, "avg", 3, 1, 1)
        self._conv(f"{blk}.branch_pool", p, out=out, ooff=576)
        return out

    def _block_d(self, x):
        B, H, W, C = x.shape
        ho, wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        out = self._empty(x, ho, wo, 320 + 192 + C)
        t, oa, ob = self._pair_1x1("Mixed_7a", x)
        self._conv("Mixed_7a.branch3x3_2", self._pick(t, 0), oa, out=out, ooff=0)
        d = self._conv("Mixed_7a.branch7x7x3_2", self._pick(t, 1), ob)
        d = self._conv("Mixed_7a.branch7x7x3_3", d)
        self._conv("Mixed_7a.branch7x7x3_4", d, out=out, ooff=320)
        self._ops.pool2d_nhwc(x, "max", 3, 2, 0, out=out, ooff=512)
        return out

    def _block_e(self, blk, x, pool):
        B, H, W, _ = x.shape
        out = self._empty(x, H, W, 2048)
        self._conv(f"{blk}.branch1x1", x, out=out, ooff=0)
        t, oa, ob = self._pair_1x1(blk, x)
        self._conv(f"{blk}.branch3x3_2a", self._pick(t, 0), oa, out=out, ooff=320)
        self._conv(f"{blk}.branch3x3_2b", self._pick(t, 0), oa, out=out, ooff=704)
        d = self._conv(f"{blk}.branch3x3dbl_2", self._pick(t, 1), ob)
        self._conv(f"{blk}.branch3x3dbl_3a", d, out=out, ooff=1088)
        self._conv(f"{blk}.branch3x3dbl_3b", d, out=out, ooff=1472)
        p = self._ops.pool2d_nhwc(x, pool, 3, 1, 1)
        self._conv(f"{blk}.branch_pool", p, out=out, ooff=1856)
        return out

    # ---------------------------------------------------------------- forward
    def _uint8_images(self, images, what):
        if not isinstance(images, torch.Tensor):
            images = torch.from_numpy(np.ascontiguousarray(images))
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
            raise ValueError(f"{what}() takes uint8 [B, H, W, 3] RGB images, got {tuple(images.shape)} {images.dtype}")
        return images.to(self.device, non_blocking=True).contiguous()

    @torch.no_grad()
    def features(self, images):
        """uint8 [B, H, W, 3] RGB (host or device) -> f32 [B, dims] on the device."""
        return self._forward(self._ops.fid_preprocess(self._uint8_images(images, "features")))

    @torch.no_grad()
    def adm_features(self, images):
        """The ADM evaluator's two tensors in one forward (reference tools/evaluator.py:24,601-615): uint8 [B, H, W, 3] RGB ->
        (pool f32 [B, 2048], spatial f32 [B, 2023]) on the device.  Pre-processing is the TF graph's (ops.adm_preprocess), not
        pytorch-fid's; pool is TF pool_3 (the global average of Mixed_7c); spatial is TF mixed_6/conv[..., :7] = channels 0..6 of Mixed_6d's
        branch1x1 after BatchNorm + ReLU (TF mixed_4..mixed_7 are Mixed_6b..6e), flattened in NHWC order: index (h * 17 + w) * 7 + c."""
        if self.block != 3:
            raise ValueError(f"adm_features() needs the full network (dims=2048), this model has dims={self.dims}")
        taps = []
        pool = self._forward(self._ops.adm_preprocess(self._uint8_images(images, "adm_features")), taps)
        return pool, taps[0]

    def adm_logits_weight(self):
        """fc.weight [1008, 2048] f32 on the device: the ADM softmax graph's MatMul weight (softmax/logits/MatMul; no bias is added).
        KeyError if the state dict had no fc.weight, ValueError on a wrong shape."""
        if self._fc_weight is None:
            w = self._fc_weight_src
            if w is None:
                raise KeyError("Inception state dict lacks fc.weight [1008, 2048], which the Inception Score needs")
            if tuple(w.shape) != (1008, 2048):
                raise ValueError(f"Inception state dict: fc.weight has shape {tuple(w.shape)}, expected (1008, 2048)")
            self._fc_weight = w.detach().float().contiguous().to(self.device)
        return self._fc_weight

    def _forward(self, x, taps=None):
        """Pre-processed f32 [B, 299, 299, 3] -> f32 [B, dims]; taps (a list) receives Mixed_6d's sFID tap [B, 17 * 17 * 7]."""
        ops = self._ops
        x = self._conv("Conv2d_1a_3x3", x)
        x = self._conv("Conv2d_2a_3x3", x)
        x = self._conv("Conv2d_2b_3x3", x)
        x = ops.pool2d_nhwc(x, "max", 3, 2, 0)
        if self.block == 0:
            return ops.global_avgpool_nhwc(x)
        x = self._conv("Conv2d_3b_1x1", x)
        x = self._conv("Conv2d_4a_3x3", x)
        x = ops.pool2d_nhwc(x, "max", 3, 2, 0)
        if self.block == 1:
            return ops.global_avgpool_nhwc(x)
        for blk in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            x = self._block_a(blk, x)
        x = self._block_b(x)
        for blk in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = self._block_c(blk, x)
            if taps is not None and blk == "Mixed_6d":
                taps.append(ops.adm_spatial_tap(x, 0, 7))      # branch1x1 is written at channel offset 0 of the block output
        if self.block == 2:
            return ops.global_avgpool_nhwc(x)
        x = self._block_d(x)
        x = self._block_e("Mixed_7b", x, "avg")
        x = self._block_e("Mixed_7c", x, "max")
        return ops.global_avgpool_nhwc(x)


class FeatureStats:
    """Running f64 sums of shifted features on the device: mu / sigma come out as np.mean / np.cov(rowvar=False) give them.  The shift is
    the first batch's mean, so the covariance sums do not cancel."""

    def __init__(self, dims, device="cuda"):
        self.dims, self.device, self.n = dims, torch.device(device), 0
        self.shift = None
        self.s1 = torch.zeros(dims, dtype=torch.float64, device=self.device)
        self.s2 = torch.zeros(dims, dims, dtype=torch.float64, device=self.device)

    def update(self, feats):
        from . import ops
        feats = feats.contiguous()
        if feats.shape[1] != self.dims:
            raise ValueError(f"features of width {feats.shape[1]}, expected {self.dims}")
        if self.shift is None:
            self.shift = ops.global_avgpool_nhwc(feats.view(1, feats.shape[0], self.dims)).view(self.dims)
        ops.fid_stats_accumulate(feats, self.shift, self.s1, self.s2)
        self.n += feats.shape[0]

    def finalize(self):
        if self.n < 2:
            raise ValueError(f"FID statistics need at least 2 images, got {self.n}")
        s1, s2 = self.s1.cpu().numpy(), self.s2.cpu().numpy()
        shift = self.shift.double().cpu().numpy()
        d = s1 / self.n
        mu = shift + d
        sigma = (s2 - self.n * np.outer(d, d)) / (self.n - 1)
        return mu, sigma


# ---------------------------------------------------------------------------------------------------- the reference's interface
def list_images(path, sp_len=None):
    """The reference's file list: every file of IMAGE_EXTENSIONS directly in `path`, sorted, cut to sp_len."""
    path = pathlib.Path(path)
    files = sorted([f for ext in IMAGE_EXTENSIONS for f in path.glob(f"*.{ext}")])
    if sp_len is not None:
        files = files[:sp_len]
    return files


def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def _batches(files, batch_size, threads):
    """uint8 [b, H, W, 3] arrays of consecutive files, decoded on a thread pool one batch ahead; a run of images of one size per array."""
    with ThreadPoolExecutor(max_workers=threads) as pool:
        chunks = [files[i:i + batch_size] for i in range(0, len(files), batch_size)]
        pending = pool.map(_decode, chunks[0]) if chunks else None
        for i in range(len(chunks)):
            ims = list(pending)
            if i + 1 < len(chunks):
                pending = pool.map(_decode, chunks[i + 1])
            j = 0
            while j < len(ims):
                k = j + 1
                while k < len(ims) and ims[k].shape == ims[j].shape:
                    k += 1
                yield np.stack(ims[j:k])
                j = k


_MODELS = {}


def _model(dims, device, weights=None):
    key = (resolve_weights(weights), dims, str(device))
    if key not in _MODELS:
        _MODELS.clear()
        _MODELS[key] = InceptionFID(key[0], dims, device)
    return _MODELS[key]


def calculate_activation_statistics(files, model, batch_size=50, dims=2048, device="cuda", num_workers=1, sp_len=None):
    """mu, sigma of the pool features of `files` (the reference's function of this name; statistics accumulated on the device)."""
    if batch_size > len(files):
        print("Warning: batch size is bigger than the data size. Setting batch size to data size")
        batch_size = len(files)
    stats = FeatureStats(model.dims, model.device)
    threads = max(1, min(MAX_DECODE_THREADS, int(num_workers or 1) * 2))
    for arr in _batches(files, batch_size, threads):
        stats.update(model.features(torch.from_numpy(arr).pin_memory() if torch.cuda.is_available() else torch.from_numpy(arr)))
    return stats.finalize()


def compute_statistics_of_path(path, model, batch_size, dims, device, num_workers=1, sp_len=None):
    """`.npz` -> its mu / sigma; a folder -> the statistics of its images (list_images order, cut to sp_len).  `model` may be None: the
    Inception weights are then resolved (and loaded once) only when a folder needs them."""
    path = str(path)
    if path.endswith(".npz"):
        with np.load(path) as f:
            return f["mu"][:], f["sigma"][:]
    files = list_images(path, sp_len)
    if model is None:
        model = _model(dims, device)
    return calculate_activation_statistics(files, model, batch_size, dims, device, num_workers)


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """d^2 = |mu1 - mu2|^2 + Tr(S1 + S2 - 2 sqrt(S1 S2)) in f64 (the reference's stable form: eps on the diagonals when the product's square
    root is not finite, ValueError when its diagonal has an imaginary part beyond 1e-3)."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1).astype(np.float64), np.atleast_1d(mu2).astype(np.float64)
    sigma1, sigma2 = np.atleast_2d(sigma1).astype(np.float64), np.atleast_2d(sigma2).astype(np.float64)
    assert mu1.shape == mu2.shape, "Training and test mean vectors have different lengths"
    assert sigma1.shape == sigma2.shape, "Training and test covariances have different dimensions"
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        print(f"fid calculation produces singular product; adding {eps} to diagonal of cov estimates")
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))


def calculate_fid_given_paths(paths, batch_size, device, dims, num_workers=1, model_name="inception_v3", sp_len=None):
    """The FID of two paths (folders of images or .npz statistics), with the reference's signature (tools/calculate_fid.py)."""
    for p in paths:
        if not os.path.exists(p):
            raise RuntimeError("Invalid path: %s" % p)
    if model_name != "inception_v3":
        raise NotImplementedError(f"Model {model_name} not implemented")
    if dims not in BLOCK_INDEX_BY_DIM:
        raise ValueError(f"dims must be one of {sorted(BLOCK_INDEX_BY_DIM)}, got {dims}")
    m1, s1 = compute_statistics_of_path(paths[0], None, batch_size, dims, device, num_workers, sp_len)
    m2, s2 = compute_statistics_of_path(paths[1], None, batch_size, dims, device, num_workers, sp_len)
    return calculate_frechet_distance(m1, s1, m2, s2)


def save_fid_stats(paths, batch_size, device, dims, num_workers=1, sp_len=None):
    """Write mu / sigma of the folder paths[0] to paths[1] (pytorch-fid's --save-stats)."""
    if not os.path.exists(paths[0]):
        raise RuntimeError("Invalid path: %s" % paths[0])
    if os.path.exists(paths[1]):
        raise RuntimeError("Existing output file: %s" % paths[1])
    m, s = compute_statistics_of_path(paths[0], None, batch_size, dims, device, num_workers, sp_len)
    np.savez_compressed(paths[1], mu=m, sigma=s)


def main(argv=None):
    ap = argparse.ArgumentParser(description="FID of two image folders / .npz statistics on the HIP Inception-v3")
    ap.add_argument("path", nargs=2, help="folders of images or .npz statistics files (with --save-stats: SRC folder, DST .npz)")
    ap.add_argument("--batch-size", type=int, default=50)
    ap.add_argument("--dims", type=int, default=2048, choices=sorted(BLOCK_INDEX_BY_DIM))
    ap.add_argument("--weights", default=None, help=f"{WEIGHTS_NAME} (default: ${WEIGHTS_ENV}, then torch.hub's checkpoints directory)")
    ap.add_argument("--sp-len", type=int, default=None, help="use only the first N images of a folder (sorted)")
    ap.add_argument("--num-workers", type=int, default=8, help="image decoding threads / 2 (at most 16 threads)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--save-stats", action="store_true", help="write mu / sigma of SRC to DST.npz instead of computing a distance")
    a = ap.parse_args(argv)
    if a.weights:
        os.environ[WEIGHTS_ENV] = a.weights
    if a.save_stats:
        save_fid_stats(a.path, a.batch_size, a.device, a.dims, a.num_workers, a.sp_len)
        return None
    fid = calculate_fid_given_paths(a.path, a.batch_size, a.device, a.dims, a.num_workers, sp_len=a.sp_len)
    print("FID: ", fid)
    return fid


if __name__ == "__main__":
    main()
