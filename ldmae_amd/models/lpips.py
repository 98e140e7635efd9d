"""LPIPS (VGG16 + learned linear heads) with the interface of the reference's models/lpips.py, forward only, on this package's kernels.

    d(x, y) = sum_k mean_hw sum_c w_k[c] (f^_k(x) - f^_k(y))^2,   f^ = f / (sqrt(sum_c f^2) + 1e-10)

with f_k the VGG16 taps relu1_2, relu2_2, relu3_3, relu4_3 and relu5_3 of the ScalingLayer'd image.  The 13 convolutions (3x3, padding 1,
ReLU fused) run on conv2d_nhwc (the exact-f32 MFMA implicit GEMM), the four 2x2 / 2 max pools on pool2d_nhwc, the ScalingLayer and the
heads on csrc/tokenizer_eval.hip.  Input and target run as ONE batch of 2B images, so every conv is one launch.

Weights are the user's files, never downloaded:
  - torchvision's vgg16-397923af.pth (keys features.{0,2,5,...,28}.weight|bias): the `vgg_weights` argument, then $LDMAE_LPIPS_VGG, then
    torch.hub's checkpoints/ directory;
  - taming's vgg.pth (keys lin{0..4}.model.1.weight [1, C, 1, 1]): the `lin_weights` argument, then $LDMAE_LPIPS_LIN, then the reference's
    relative path movqgan/modules/losses/lpips/vgg.pth.
A `state_dict` in the reference module's own keys (net.slice{1..5}.{i}.weight|bias, lin{k}.model.1.weight) replaces both files.
"""
from __future__ import annotations

import os

import torch

VGG_NAME = "vgg16-397923af.pth"
LIN_NAME = "vgg.pth"
VGG_ENV = "LDMAE_LPIPS_VGG"
LIN_ENV = "LDMAE_LPIPS_LIN"
LIN_REL_PATH = os.path.join("movqgan", "modules", "losses", "lpips", LIN_NAME)
CHANNELS = (64, 128, 256, 512, 512)

# (torchvision features index, reference slice, Cin, Cout); a pool precedes the first conv of slices 2..5 (features 4, 9, 16, 23)
CONVS = ((0, 1, 3, 64), (2, 1, 64, 64),
         (5, 2, 64, 128), (7, 2, 128, 128),
         (10, 3, 128, 256), (12, 3, 256, 256), (14, 3, 256, 256),
         (17, 4, 256, 512), (19, 4, 512, 512), (21, 4, 512, 512),
         (24, 5, 512, 512), (26, 5, 512, 512), (28, 5, 512, 512))
# scaling_layer.shift / .scale are buffers of the reference module (constants here); torchvision's classifier is not used
_IGNORED_PREFIXES = ("scaling_layer.",)


def vgg_param_shapes():
    """torchvision VGG16 key -> shape of the 13 convolutions LPIPS uses."""
    out = {}
    for i, _, cin, cout in CONVS:
        out[f"features.{i}.weight"] = (cout, cin, 3, 3)
        out[f"features.{i}.bias"] = (cout,)
    return out


def lin_param_shapes():
    return {f"lin{k}.model.1.weight": (1, c, 1, 1) for k, c in enumerate(CHANNELS)}


def param_shapes():
    """The reference module's state-dict keys (net.slice{s}.{i}.*, lin{k}.model.1.weight) -> shape."""
    out = {}
    for i, s, cin, cout in CONVS:
        out[f"net.slice{s}.{i}.weight"] = (cout, cin, 3, 3)
        out[f"net.slice{s}.{i}.bias"] = (cout,)
    out.update(lin_param_shapes())
    return out


def _check(sd, want, what, ignored=()):
    """Refuse a missing, extra or wrongly shaped key, naming it (fid.check_state_dict's rule)."""
    missing = [k for k in want if k not in sd]
    if missing:
        raise KeyError(f"{what} lacks {missing[0]}" + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
    extra = [k for k in sd if k not in want and not any(k.startswith(p) for p in ignored)]
    if extra:
        raise KeyError(f"{what} has an unexpected key {extra[0]}" + (f" (and {len(extra) - 1} more)" if len(extra) > 1 else ""))
    for k, shape in want.items():
        if tuple(sd[k].shape) != shape:
            raise ValueError(f"{what}: {k} has shape {tuple(sd[k].shape)}, expected {shape}")


def check_state_dict(sd):
    _check(sd, param_shapes(), "LPIPS state dict", _IGNORED_PREFIXES)


def vgg_to_lpips(vgg_sd):
    """torchvision VGG16 state dict -> the net.slice* keys (the features.* convs only; classifier.* is accepted and dropped)."""
    feats = {k: v for k, v in vgg_sd.items() if not k.startswith("classifier.")}
    _check(feats, vgg_param_shapes(), f"VGG16 state dict ({VGG_NAME})")
    return {f"net.slice{s}.{i}.{p}": feats[f"features.{i}.{p}"] for i, s, _, _ in CONVS for p in ("weight", "bias")}


def load_lin(lin_sd):
    """taming's vgg.pth -> its five lin{k}.model.1.weight tensors (scaling_layer.* buffers accepted and ignored)."""
    _check(lin_sd, lin_param_shapes(), f"LPIPS lin state dict ({LIN_NAME})", _IGNORED_PREFIXES)
    return {k: lin_sd[k] for k in lin_param_shapes()}


def weight_locations(vgg_weights=None, lin_weights=None):
    """(file name, [(where, path), ...]) for both files, in search order."""
    hub = os.path.join(torch.hub.get_dir(), "checkpoints", VGG_NAME)
    return [(VGG_NAME, [("vgg_weights= argument", vgg_weights), (f"${VGG_ENV}", os.environ.get(VGG_ENV)), ("torch.hub checkpoints", hub)]),
            (LIN_NAME, [("lin_weights= argument", lin_weights), (f"${LIN_ENV}", os.environ.get(LIN_ENV)),
                        ("reference relative path", LIN_REL_PATH)])]


def resolve_weights(vgg_weights=None, lin_weights=None):
    """(vgg path, lin path), or one FileNotFoundError that names both files and every place looked at.  Never downloads."""
    found, report = [], []
    for name, locs in weight_locations(vgg_weights, lin_weights):
        hit = next((p for _, p in locs if p and os.path.isfile(p)), None)
        found.append(hit)
        where = "; ".join(f"{what}: {p if p else '(not set)'}" for what, p in locs)
        report.append(f"{name} {'found at ' + hit if hit else 'NOT found'} ({where})")
    if None in found:
        raise FileNotFoundError(f"LPIPS needs two weight files, {VGG_NAME} (torchvision VGG16) and {LIN_NAME} (taming's LPIPS heads): "
                                + " | ".join(report) + ".  Place them in one of these; this package never downloads them.")
    return found[0], found[1]


def load_state_dict_from_files(vgg_weights=None, lin_weights=None):
    vgg_path, lin_path = resolve_weights(vgg_weights, lin_weights)
    sd = vgg_to_lpips(torch.load(vgg_path, map_location="cpu", weights_only=True))
    sd.update(load_lin(torch.load(lin_path, map_location="cpu", weights_only=True)))
    return sd


def random_state_dict(seed=0):
    """The reference module's keys with random values (tests, tools/bench_tokenizer_eval.py): He-scaled conv weights, biases ~ N(0, 0.01)
    keeping the ReLU taps O(1) through 13 layers, lin weights in [0, 0.1) (non-negative, as the trained heads are)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, s, cin, cout in CONVS:
        sd[f"net.slice{s}.{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
        sd[f"net.slice{s}.{i}.bias"] = torch.randn(cout, generator=g) * 0.01
    for k, c in enumerate(CHANNELS):
        sd[f"lin{k}.model.1.weight"] = torch.rand(1, c, 1, 1, generator=g) * 0.1
    return sd


def conv_weights(sd):
    """[(weight [Cout, 3, 3, Cin'] f32, bias [Cout] f32, slice)] in execution order, channels-last (the conv kernel's K order: ky, kx, ci);
    conv1_1's weight zero-padded from Cin 3 to 4 to match lpips_prep's 4-channel output."""
    check_state_dict(sd)
    out = []
    for i, s, cin, _ in CONVS:
        w = sd[f"net.slice{s}.{i}.weight"].float().permute(0, 2, 3, 1)
        if cin == 3:
            w = torch.nn.functional.pad(w, (0, 1))
        out.append((w.contiguous(), sd[f"net.slice{s}.{i}.bias"].float().contiguous(), s))
    return out


def conv_flops_per_image(H, W):
    """2 x multiply-adds of the 13 VGG convolutions for ONE image at H x W (a pair runs two): 2 x 15.35 GMAC = 30.7 GFLOP at 224^2,
    40.1 GFLOP at 256^2 (the real Cin 3 of conv1_1, not the padded 4)."""
    flops, h, w, prev = 0, H, W, 1
    for _, s, cin, cout in CONVS:
        if s != prev:
            h, w, prev = h // 2, w // 2, s
        flops += 2 * h * w * cout * 9 * cin
    return flops


class LPIPS:
    """forward(input, target): NCHW f32 [B, 3, H, W] in [-1, 1] -> f32 [B, 1, 1, 1], as the reference's LPIPS().eval().  Forward only."""

    def __init__(self, vgg_weights=None, lin_weights=None, state_dict=None, device="cuda"):
        from .. import ops
        self._ops = ops
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"LPIPS runs on a HIP device (no CPU fallback); got {device}")
        if state_dict is None:
            state_dict = load_state_dict_from_files(vgg_weights, lin_weights)
        self.convs = [(w.to(self.device), b.to(self.device), s) for w, b, s in conv_weights(state_dict)]
        self.lins = [state_dict[f"lin{k}.model.1.weight"].float().reshape(-1).contiguous().to(self.device) for k in range(len(CHANNELS))]

    def to(self, device):
        if torch.device(device) != self.device:
            raise RuntimeError("LPIPS: construct it on its device (device=...)")
        return self

    def eval(self):
        return self

    def __call__(self, input, target):
        return self.forward(input, target)

    def forward(self, input, target):
        if torch.is_grad_enabled() and (input.requires_grad or target.requires_grad):
            raise RuntimeError("LPIPS here is forward-only: its kernels have no backward, so it cannot serve as a perceptual training loss. "
                               "Call it under torch.no_grad() or on tensors that do not require grad.")
        if input.dim() != 4 or input.shape[1] != 3 or tuple(input.shape) != tuple(target.shape):
            raise RuntimeError(f"LPIPS: input {tuple(input.shape)} and target {tuple(target.shape)} must both be [B, 3, H, W]")
        x = input.detach().to(self.device, torch.float32).contiguous()
        y = target.detach().to(self.device, torch.float32).contiguous()
        h = self._ops.lpips_prep(x, y)
        out = torch.zeros(x.shape[0], dtype=torch.float32, device=self.device)
        prev = 1
        for w, b, s in self.convs:
            if s != prev:                              # end of slice prev: its last ReLU output is tap prev - 1; then the 2x2 / 2 max pool
                self._ops.lpips_layer(h, self.lins[prev - 1], out)
                h = self._ops.pool2d_nhwc(h, "max", k=2, stride=2, pad=0)
                prev = s
            h = self._ops.conv2d_nhwc(h, w, b, (1, 1), (1, 1), True)
        self._ops.lpips_layer(h, self.lins[prev - 1], out)
        return out.view(-1, 1, 1, 1)
