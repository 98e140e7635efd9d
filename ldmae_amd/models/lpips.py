"""LPIPS (VGG16 + learned linear heads) with the interface of the reference's models/lpips.py on this package's kernels: forward only by default,
differentiable on request (`LPIPS(..., differentiable=True)`: the perceptual loss of the stage-3 decoder tuning, VMAE/train_ae.sh:84-106).

    d(x, y) = sum_k mean_hw sum_c w_k[c] (f^_k(x) - f^_k(y))^2,   f^ = f / (sqrt(sum_c f^2) + 1e-10)

with f_k the VGG16 taps relu1_2, relu2_2, relu3_3, relu4_3 and relu5_3 of the ScalingLayer'd image.  The 13 convolutions (3x3, padding 1,
ReLU fused) run on conv2d_nhwc (the exact-f32 MFMA implicit GEMM), the four 2x2 / 2 max pools on pool2d_nhwc, the ScalingLayer and the
heads on csrc/tokenizer_eval.hip.  Input and target run as ONE batch of 2B images, so every conv is one launch.

Backward (csrc/lpips_bwd.hip; only with differentiable=True, only for the halves that require grad -- stage 3 needs the second argument alone:
perceptual_loss(imgs, unpatchify(pred))): per tap the head backward, per pool the max-pool backward (the two sum into one buffer: the pool backward
writes it, the head backward adds to it -- always in this order), per conv the data gradient with the ReLU mask taken from the saved output inside
the operand gather, on weights rotated once per object (rotate_weight); no weight gradients (the network is frozen), no atomics: two backward runs
give the same bits.  Activation memory: the forward keeps the 13 conv outputs of each half that requires grad (17.7 M floats = 71 MB per 256 x 256
image; 1.13 GB at the recipe's batch of 16) and only the five taps (the first of them is the largest: 16.8 MB per image) of a half that does not.
Nothing is copied to keep them: when one half requires grad every layer runs as two launches of B images (LPIPS._run).
One deliberate difference from torch: at a pixel whose channels are all zero in a half, that half's gradient is exactly 0 (torch: NaN, from sqrt's
backward at 0).  The value is bitwise the forward-only value.

precision="fp16" (opt-in; the default "f32" is the exact-f32 path above, unchanged) runs the VGG in 16 bits, the reference's autocast arithmetic
without its GradScaler (csrc/lpips_f16.hip).  Forward: every conv operand fp16 (round to nearest even, saturating at +-65504), products exact in f32
and accumulated in f32 on the fp16 MFMA, bias and ReLU in f32, ONE rounding to fp16 at the store; activations live in memory as fp16 (half the kept
bytes: 35 MB per 256 x 256 image), the pool runs on fp16 (exact), the heads read fp16 taps and compute in f32.  The ScalingLayer'd image has 8
channels (3 real, 5 zero) and conv1_1 a weight zero-padded to Cin 8, so all 13 convolutions are one kernel.  Backward: gradients stay f32 in memory;
the data gradient rounds dy * [y > 0] (at the fetch) and w_rot (once per object) to bf16 and accumulates in f32 on the bf16 MFMA -- bf16 because the
gradient scales as 1 / (h w) and is below fp16's smallest normal already at 33 x 47; the mask is y > 0 on the stored fp16 activation.  The launch
structure, the "one half requires grad" rule, the bitwise value and the all-zero-pixel rule are those of the f32 path.  The precision is an argument,
never inferred from torch.backends or autocast state.

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


PRECISIONS = ("f32", "fp16")


def check_precision(precision):
    if not isinstance(precision, str) or precision not in PRECISIONS:
        raise ValueError(f"LPIPS precision {precision!r}: one of {PRECISIONS}")
    return precision


def conv_weights_c8(sd):
    """conv_weights with conv1_1's weight zero-padded from Cin 3 to 8 (f32): the shapes of the fp16 path, matching lpips_prep_f16's 8 channels."""
    return [(torch.nn.functional.pad(w, (0, 4)).contiguous() if w.shape[3] == 4 else w, b, s) for w, b, s in conv_weights(sd)]


def conv_weights_f16(sd):
    """[(weight [Cout, 3, 3, Cin'] fp16, bias [Cout] f32, slice)]: conv_weights_c8 with each weight rounded once to fp16 (round to nearest even; VGG
    weights are far inside fp16's range)."""
    return [(w.half().contiguous(), b, s) for w, b, s in conv_weights_c8(sd)]


def rotate_weight_bf16(w):
    """rotate_weight of the f32 channels-last forward weight, rounded once to bf16: the data gradient's weight of the fp16 path."""
    return rotate_weight(w.float()).to(torch.bfloat16).contiguous()


class _Family:
    """The kernels of one precision under one set of names: _run and _LPIPSFn are written once over them."""

    def __init__(self, ops, precision):
        f32 = precision == "f32"
        self.act_dtype = torch.float32 if f32 else torch.float16
        self.prep = ops.lpips_prep if f32 else ops.lpips_prep_f16
        self.conv = (lambda x, w, b, out=None: ops.conv2d_nhwc(x, w, b, (1, 1), (1, 1), True, out=out)) if f32 else ops.conv3x3_relu_nhwc_f16
        self.pool = (lambda x: ops.pool2d_nhwc(x, "max", k=2, stride=2, pad=0)) if f32 else ops.maxpool2x2_nhwc_f16
        self.head = ops.lpips_layer if f32 else ops.lpips_layer_f16
        self.dgrad = ops.conv3x3_relu_dgrad_nhwc if f32 else ops.conv3x3_relu_dgrad_nhwc_bf16
        self.pool_bwd = ops.maxpool2x2_bwd_nhwc if f32 else ops.maxpool2x2_bwd_nhwc_xf16
        self.head_bwd = ops.lpips_layer_bwd if f32 else ops.lpips_layer_bwd_f16
        self.prep_bwd = ops.lpips_prep_bwd if f32 else ops.lpips_prep_bwd_c8


def conv_flops_per_image(H, W):
    """2 x multiply-adds of the 13 VGG convolutions for ONE image at H x W (a pair runs two): 2 x 15.35 GMAC = 30.7 GFLOP at 224^2,
    40.1 GFLOP at 256^2 (the real Cin 3 of conv1_1, not the padded 4)."""
    flops, h, w, prev = 0, H, W, 1
    for _, s, cin, cout in CONVS:
        if s != prev:
            h, w, prev = h // 2, w // 2, s
        flops += 2 * h * w * cout * 9 * cin
    return flops


def rotate_weight(w):
    """Channels-last forward weight [Cout, 3, 3, Cin] -> the data gradient's weight [Cin, 3, 3, Cout] in the conv kernel's K order (ky, kx, channel):
    w_rot[ci][ky][kx][co] = w[co][2 - ky][2 - kx][ci], so that dx = conv3x3(dy, w_rot) with padding 1 (conv_transpose2d of a stride-1 conv)."""
    if w.dim() != 4 or tuple(w.shape[1:3]) != (3, 3):
        raise ValueError(f"rotate_weight: weight {tuple(w.shape)} is not [Cout, 3, 3, Cin]")
    return w.flip(1, 2).permute(3, 1, 2, 0).contiguous()


def _last_of_slice(i):
    return i + 1 == len(CONVS) or CONVS[i + 1][1] != CONVS[i][1]


class _LPIPSFn(torch.autograd.Function):
    """LPIPS.forward with a backward (see the module docstring).  Saved: the five taps [2B, ...] and, per half that requires grad, the other eight
    conv outputs of that half [B, ...] (tensors of their own when one half requires grad, views of the [2B, ...] outputs when both do; the tap
    entries of a half are views of the saved taps)."""

    @staticmethod
    def forward(ctx, mod, input, target):
        need = (ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        out, taps, acts = mod._run(input, target, need)
        ctx.mod, ctx.need, ctx.dtypes, ctx.devices = mod, need, (input.dtype, target.dtype), (input.device, target.device)
        ctx.save_for_backward(*taps, *[a for half in acts if half is not None for a in half if a is not None])
        return out

    @staticmethod
    def backward(ctx, gout):
        mod, k_ = ctx.mod, ctx.mod._k
        saved = list(ctx.saved_tensors)
        taps, rest = saved[:len(CHANNELS)], saved[len(CHANNELS):]
        B = taps[0].shape[0] // 2
        g = gout.detach().reshape(B).to(torch.float32).contiguous()
        per_half = len(CONVS) - len(CHANNELS)          # saved per half besides the taps, in execution order, the input half's first
        grads = [None, None]
        for half in (0, 1):
            if not ctx.need[half]:
                continue
            inner, rest = rest[:per_half], rest[per_half:]
            d = None
            for i in reversed(range(len(CONVS))):
                k = CONVS[i][1] - 1
                if _last_of_slice(i):
                    y = taps[k][half * B:(half + 1) * B]
                    # gradient of tap k: the following pool's backward writes the buffer, the head backward adds to it (fixed order)
                    buf = k_.pool_bwd(d, y) if d is not None else torch.empty(y.shape, dtype=torch.float32, device=y.device)
                    k_.head_bwd(taps[k], mod.lins[k], g, d_input=buf if half == 0 else None, d_target=buf if half == 1 else None,
                                accumulate=d is not None)
                    d = buf
                else:
                    y = inner.pop()
                d = k_.dgrad(d, y, mod.wrot[i])
            grads[half] = k_.prep_bwd(d).to(ctx.devices[half], ctx.dtypes[half])
        return None, grads[0], grads[1]


class LPIPS:
    """forward(input, target): NCHW f32 [B, 3, H, W] in [-1, 1] -> f32 [B, 1, 1, 1], as the reference's LPIPS().eval().  Forward only unless built with
    differentiable=True (then a torch.autograd.Function with the same value, bit for bit; activation memory: module docstring).
    precision "f32" (default: the exact-f32 path) or "fp16" (fp16 VGG forward, bf16 data gradient: module docstring); anything else is a ValueError."""

    differentiable = False
    precision = "f32"

    def __init__(self, vgg_weights=None, lin_weights=None, state_dict=None, device="cuda", differentiable=False, precision="f32"):
        self.precision = check_precision(precision)
        from .. import ops
        self._ops = ops
        self._k = _Family(ops, self.precision)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"LPIPS runs on a HIP device (no CPU fallback); got {device}")
        if state_dict is None:
            state_dict = load_state_dict_from_files(vgg_weights, lin_weights)
        packs = conv_weights(state_dict) if self.precision == "f32" else conv_weights_f16(state_dict)
        self.convs = [(w.to(self.device), b.to(self.device), s) for w, b, s in packs]
        self.lins = [state_dict[f"lin{k}.model.1.weight"].float().reshape(-1).contiguous().to(self.device) for k in range(len(CHANNELS))]
        if differentiable:
            self.differentiable = True
            # once per object; conv1_1's padded rows are zero.  fp16 path: the f32 weight rounded once to bf16 (not through fp16)
            self.wrot = ([rotate_weight(w) for w, _, _ in self.convs] if self.precision == "f32" else
                         [rotate_weight_bf16(w).to(self.device) for w, _, _ in conv_weights_c8(state_dict)])

    def to(self, device):
        if torch.device(device) != self.device:
            raise RuntimeError("LPIPS: construct it on its device (device=...)")
        return self

    def eval(self):
        return self

    def __call__(self, input, target):
        return self.forward(input, target)

    def _run(self, input, target, keep=(False, False)):
        """-> (value [B, 1, 1, 1], the five taps [2B, ...], per half in `keep` its other conv outputs in execution order (None at the taps))."""
        if input.dim() != 4 or input.shape[1] != 3 or tuple(input.shape) != tuple(target.shape):
            raise RuntimeError(f"LPIPS: input {tuple(input.shape)} and target {tuple(target.shape)} must both be [B, 3, H, W]")
        x = input.detach().to(self.device, torch.float32).contiguous()
        y = target.detach().to(self.device, torch.float32).contiguous()
        B = x.shape[0]
        k_ = self._k
        h = k_.prep(x, y)
        out = torch.zeros(B, dtype=torch.float32, device=self.device)
        taps, acts = [], [[] if k else None for k in keep]
        # ONE half kept: each layer runs as two launches of B images, so the kept half's outputs are tensors of their own (kept without a copy)
        # and the other half's are freed layer by layer; the taps are still one [2B, ...] tensor, written half by half.  Both or none: one launch
        # of 2B images per layer, the kept entries are views of it.  Every output element is the same sum either way: the value is bitwise one.
        split = keep[0] != keep[1]
        hs = [h[:B], h[B:]] if split else [h]
        prev = 1
        for i, (w, b, s) in enumerate(self.convs):
            if s != prev:                              # end of slice prev: its last ReLU output is tap prev - 1; then the 2x2 / 2 max pool
                k_.head(h, self.lins[prev - 1], out)
                taps.append(h)
                hs = [k_.pool(t) for t in hs]
                prev = s
            if split and _last_of_slice(i):            # a tap: both halves into one tensor
                h = torch.empty(2 * B, hs[0].shape[1], hs[0].shape[2], w.shape[0], dtype=k_.act_dtype, device=self.device)
                hs = [k_.conv(t, w, b, out=h[j * B:(j + 1) * B]) for j, t in enumerate(hs)]
            else:
                hs = [k_.conv(t, w, b) for t in hs]
                h = hs[0]                              # (read only where it is the whole batch: not split)
            for half, a in enumerate(acts):
                if a is not None:
                    a.append(None if _last_of_slice(i) else (hs[half] if split else h[half * B:(half + 1) * B]))
        k_.head(h, self.lins[prev - 1], out)
        taps.append(h)
        return out.view(-1, 1, 1, 1), taps, acts

    def forward(self, input, target):
        if torch.is_grad_enabled() and (input.requires_grad or target.requires_grad):
            if not self.differentiable:
                raise RuntimeError("LPIPS here is forward-only: its kernels have no backward, so it cannot serve as a perceptual training loss. "
                                   "Call it under torch.no_grad() or on tensors that do not require grad -- or build it with differentiable=True.")
            return _LPIPSFn.apply(self, input, target)
        return self._run(input, target)[0]
