"""The opt-in 16-bit LPIPS path (csrc/lpips_f16.hip; models/lpips.py precision="fp16") on the MI355X.

Kernels whose arithmetic is exact (the fp16 prep, pool, heads, pool backward, prep backward) are compared bit for bit with the f32 kernels fed the
same numbers.  The two convolutions are checked per element against f64 on the operands the kernel reads, with bounds derived from the number
formats.  End to end, the GPU is held against an f64 run of the exact network, with the error an f64 EMULATION of the arithmetic contract makes on
the same fixture as the yardstick (times 4: the standing margin for two independent realisations of the same rounding noise):

    forward : every conv reads its input and weight rounded to fp16 and stores its output rounded to fp16; everything else f64;
    backward: every data gradient reads dy * mask and the weight rounded to bf16; everything else f64;
    ReLU masks and pool picks of both gradient runs are forced to the ones the GPU's fp16 forward took (the gradient is discontinuous in them).
"""
import functools
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHIFT = torch.tensor([-0.030, -0.088, -0.188], dtype=torch.float64).view(1, 3, 1, 1)
SCALE = torch.tensor([0.458, 0.448, 0.450], dtype=torch.float64).view(1, 3, 1, 1)
MARGIN = 4.0            # two independent realisations of the same rounding noise (f32 against f64 accumulation flips individual roundings)
GRID = [(3, 5, 7), (2, 12, 11), (2, 1, 1)]


def _ops():
    from ldmae_amd import ops
    return ops


def r16(t):
    """f64 -> the nearest fp16 (ties to even), saturating at +-65504, as f64."""
    return t.clamp(-65504.0, 65504.0).to(torch.float16).to(t.dtype)


def rb16(t):
    """f64 -> the nearest bf16, as f64."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------------- kernels that are exact
@pytest.mark.parametrize("bhw", [(2, 5, 7), (1, 1, 1), (3, 16, 19)])
def test_prep_fp16_is_the_f32_prep_rounded_once(bhw):
    B, H, W = bhw
    gen = torch.Generator().manual_seed(H)
    x, y = (torch.rand(B, 3, H, W, generator=gen) * 2 - 1).cuda(), (torch.rand(B, 3, H, W, generator=gen) * 2 - 1).cuda()
    ops = _ops()
    got, ref = ops.lpips_prep_f16(x, y), ops.lpips_prep(x, y)
    assert got.dtype == torch.float16 and tuple(got.shape) == (2 * B, H, W, 8)
    assert torch.equal(got[..., :3], ref[..., :3].half()) and torch.count_nonzero(got[..., 3:]) == 0


@pytest.mark.parametrize("shape", [(2, 5, 7, 64), (1, 2, 2, 8), (3, 16, 16, 128)])
def test_pool_fp16_equals_torch(shape):
    gen = torch.Generator().manual_seed(shape[1])
    x = torch.randn(*shape, generator=gen).half()
    x[0, 0:2, 0:2, 1] = 0.5                                      # a tie
    got = _ops().maxpool2x2_nhwc_f16(x.cuda()).cpu()
    want = nhwc(F.max_pool2d(nchw(x.float()), 2, 2)).half()      # max is exact in either format
    assert got.dtype == torch.float16 and torch.equal(got, want)


@pytest.mark.parametrize("C", [64, 128, 256, 512])
@pytest.mark.parametrize("hw", [(1, 1), (5, 4), (17, 23)])
def test_heads_on_fp16_taps_equal_the_f32_heads(C, hw):
    gen = torch.Generator().manual_seed(C + hw[0])
    B = 3
    f = F.relu(torch.randn(2 * B, *hw, C, generator=gen)).half()
    f[1, 0, 0] = 0.0                                             # an all-zero pixel of the input half, image 1
    w, g = torch.rand(C, generator=gen).cuda(), torch.tensor([0.5, -1.25, 2.0]).cuda()
    ops, f16, f32 = _ops(), f.cuda(), f.cuda().float()
    start = torch.rand(B, generator=gen).cuda()
    got, want = ops.lpips_layer_f16(f16, w, start.clone()), ops.lpips_layer(f32, w, start.clone())
    assert torch.equal(got, want) and not torch.equal(got, start)
    new = lambda: torch.full((B, *hw, C), float("nan"), device="cuda")
    d0, d1 = ops.lpips_layer_bwd_f16(f16, w, g, d_input=new(), d_target=new())
    e0, e1 = ops.lpips_layer_bwd(f32, w, g, d_input=new(), d_target=new())
    assert torch.equal(d0, e0) and torch.equal(d1, e1) and torch.isfinite(d0).all() and torch.isfinite(d1).all()
    assert torch.count_nonzero(d0[1, 0, 0]) == 0                 # the all-zero pixel: exactly 0
    t0, t1 = ops.lpips_layer_bwd_f16(f16, w, g, d_target=new())
    assert t0 is None and torch.equal(t1, e1)
    pre = torch.randn(B, *hw, C, generator=gen).cuda()
    a16, a32 = pre.clone(), pre.clone()
    ops.lpips_layer_bwd_f16(f16, w, g, d_input=a16, accumulate=True)
    ops.lpips_layer_bwd(f32, w, g, d_input=a32, accumulate=True)
    assert torch.equal(a16, a32) and torch.equal(a16, pre + e0)
    with pytest.raises(RuntimeError, match="neither"):
        ops.lpips_layer_bwd_f16(f16, w, g)
    with pytest.raises(RuntimeError, match="float16"):
        ops.lpips_layer_f16(f32, w, start.clone())


def test_pool_backward_on_fp16_equals_the_f32_kernel():
    ops = _ops()
    gen = torch.Generator().manual_seed(3)
    for shape in [(2, 5, 7, 64), (1, 2, 2, 8), (3, 16, 16, 128)]:       # odd edges, one window, several blocks
        B, H, W, C = shape
        x = F.relu(torch.randn(*shape, generator=gen)).half()            # about half zeros: ties inside many windows
        x[0, 0:2, 0:2] = 0.0                                              # a window that is all zero in every channel
        x[-1, 0:2, 0:2, 5] = 1.5                                          # a four-way tie of a non-zero value
        dy = torch.randn(B, H // 2, W // 2, C, generator=gen).cuda()
        got = ops.maxpool2x2_bwd_nhwc_xf16(dy, x.cuda(), out=torch.full(shape, float("nan"), device="cuda"))
        want = ops.maxpool2x2_bwd_nhwc(dy, x.cuda().float())
        assert got.dtype == torch.float32 and torch.equal(got, want)
        assert torch.equal(got[0, 0, 0].cpu(), dy[0, 0, 0].cpu()) and torch.count_nonzero(got[0, 0, 1]) == 0      # the tie goes to the first element
        assert torch.count_nonzero(got[:, 2 * (H // 2):]) == 0 and torch.count_nonzero(got[:, :, 2 * (W // 2):]) == 0
    x = torch.randn(1, 3, 1, 64).half().cuda()                            # W // 2 == 0: no window, dy is empty
    got = ops.maxpool2x2_bwd_nhwc_xf16(torch.zeros(1, 1, 0, 64, device="cuda"), x, out=torch.full((1, 3, 1, 64), float("nan"), device="cuda"))
    assert torch.count_nonzero(got) == 0
    with pytest.raises(RuntimeError, match="dy"):
        ops.maxpool2x2_bwd_nhwc_xf16(torch.zeros(1, 1, 1, 64, device="cuda"), x)


def test_prep_backward_from_8_channels_equals_the_4_channel_one():
    ops = _ops()
    g = torch.randn(2, 5, 6, 8, device="cuda")                            # channels 3 .. 7 hold junk here: they must be ignored
    assert torch.equal(ops.lpips_prep_bwd_c8(g), ops.lpips_prep_bwd(g[..., :4].contiguous()))


# ---------------------------------------------------------------------------------------------------- forward conv
def _fwd_case(cin, cout, B, H, W, scale=1.0):
    gen = torch.Generator().manual_seed(cin + cout + H)
    x = (torch.randn(B, H, W, cin, generator=gen) * scale).half()
    w = (torch.randn(cout, 3, 3, cin, generator=gen) * (2.0 / (cin * 9)) ** 0.5 * scale).half()
    b = torch.randn(cout, generator=gen) * 0.1
    xd, wd = nchw(x.double()), w.double().permute(0, 3, 1, 2)
    pre = nhwc(F.conv2d(xd, wd, b.double(), padding=1))
    S = nhwc(F.conv2d(xd.abs(), wd.abs(), b.double().abs(), padding=1))
    return x, w, b, pre, S


def _fwd_bound(ref, S, cin):
    """f32 accumulation of K = 9 Cin + 1 terms (the bias is one), then ONE rounding to fp16 of a value within that of ref, then fp16's subnormal
    spacing; ReLU and the saturation are 1-Lipschitz."""
    K = 9 * cin + 1
    return K * 2.0 ** -23 * S * (1 + 2.0 ** -11) + 2.0 ** -11 * ref.abs() + 2.0 ** -25


@pytest.mark.parametrize("chan", [(8, 64), (64, 64), (128, 256), (512, 512)])
@pytest.mark.parametrize("bhw", GRID)
def test_conv_forward_fp16(chan, bhw):
    from gemm_check import check
    x, w, b, pre, S = _fwd_case(*chan, *bhw)
    got = _ops().conv3x3_relu_nhwc_f16(x.cuda(), w.cuda(), b.cuda()).cpu()
    assert got.dtype == torch.float16 and tuple(got.shape) == (*bhw, chan[1])
    ref = pre.clamp(min=0.0)
    worst = check(f"conv fp16 {chan} {bhw}", got, ref, _fwd_bound(ref, S, chan[0]))
    print(f"conv fp16 {chan} {bhw}: worst err / bound {worst:.3e}")
    assert 0.2 < float((got > 0).float().mean()) < 0.8                   # the ReLU is exercised on both sides


def test_conv_forward_saturates_at_65504():
    from gemm_check import check
    x, w, b, pre, S = _fwd_case(64, 64, 2, 12, 11, scale=168.0)           # pre-activations ~ N(0, (168^2 sqrt(2))^2 = 39900^2): about 5 % beyond 65504
    got = _ops().conv3x3_relu_nhwc_f16(x.cuda(), w.cuda(), b.cuda()).cpu()
    assert torch.isfinite(got).all()
    ref = pre.clamp(0.0, 65504.0)
    bound = _fwd_bound(ref, S, 64)
    check("conv fp16 saturating", got, ref, bound)
    over = pre > 65504.0 + bound                                          # beyond the largest finite fp16 whatever the accumulation order
    print(f"saturating: {int(over.sum())} of {over.numel()} outputs beyond 65504, max {float(pre.max()):.4g}")
    assert int(over.sum()) > 0 and bool((got[over] == 65504.0).all())


def test_conv_forward_writes_only_the_given_view():
    x, w, b, pre, S = _fwd_case(64, 64, 2, 5, 7)
    ops = _ops()
    alone = ops.conv3x3_relu_nhwc_f16(x.cuda(), w.cuda(), b.cuda())
    big = torch.full((6, 5, 7, 64), -3.0, dtype=torch.float16, device="cuda")
    view = big[2:4]
    assert ops.conv3x3_relu_nhwc_f16(x.cuda(), w.cuda(), b.cuda(), out=view) is view
    assert torch.equal(big[2:4], alone) and bool((big[:2] == -3.0).all()) and bool((big[4:] == -3.0).all())
    with pytest.raises(RuntimeError, match="out"):
        ops.conv3x3_relu_nhwc_f16(x.cuda(), w.cuda(), b.cuda(), out=big[:3])
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.conv3x3_relu_nhwc_f16(x.cuda(), w.cuda(), b.cuda(), out=torch.empty(2, 5, 7, 128, dtype=torch.float16, device="cuda")[..., :64])


# ---------------------------------------------------------------------------------------------------- data gradient
@pytest.mark.parametrize("chan", [(8, 64), (64, 64), (128, 256), (512, 512)])
@pytest.mark.parametrize("bhw", GRID)
def test_conv_dgrad_bf16(chan, bhw):
    """dx = conv_transpose(bf16(dy * [y > 0]), bf16(w)) with f32 accumulation: (1) against f64 on the host-rounded operands within the f32 dot-product
    bound over K = 9 Cy terms (bf16 products are exact in f32); (2) against the unrounded f64 convolution within the two operand roundings, u = 2^-8
    each: (2u + u^2) sum |dy| |w|, plus the accumulation; (3) the same with dy scaled to 1e-8: nothing vanishes (bf16 has f32's exponent range)."""
    from gemm_check import check
    from ldmae_amd.models.lpips import rotate_weight, rotate_weight_bf16
    cx, cy = chan
    B, H, W = bhw
    gen = torch.Generator().manual_seed(cx + cy + H)
    w = torch.randn(cy, 3, 3, cx, generator=gen) * (2.0 / (cx * 9)) ** 0.5                  # channels-last forward weight [Cout, 3, 3, Cin]
    if cx == 8:
        w[..., 3:] = 0.0                                                                    # conv1_1: the padding channels
    y = F.relu(torch.randn(B, H, W, cy, generator=gen)).half()                              # the mask is an INPUT here
    assert 0.3 < float((y > 0).float().mean()) < 0.7
    dy1 = torch.randn(B, H, W, cy, generator=gen)
    w_rot = rotate_weight_bf16(w)
    assert torch.equal(w_rot, rotate_weight(w).to(torch.bfloat16))
    wt, wt_r = w.double().permute(0, 3, 1, 2), w.to(torch.bfloat16).double().permute(0, 3, 1, 2)      # [Cout, Cin, ky, kx]
    K, u = 9 * cy, 2.0 ** -8
    nonzero = []
    for scale in (1.0, 1e-8):
        dy = dy1 * scale                                                                    # f32
        got = _ops().conv3x3_relu_dgrad_nhwc_bf16(dy.cuda(), y.cuda(), w_rot.cuda()).cpu()
        assert got.dtype == torch.float32 and tuple(got.shape) == (B, H, W, cx)
        dm = nchw(dy.double() * (y > 0))
        dm_r = nchw((dy * (y > 0)).to(torch.bfloat16).double())
        ref_r = nhwc(F.conv_transpose2d(dm_r, wt_r, padding=1))
        S_r = nhwc(F.conv_transpose2d(dm_r.abs(), wt_r.abs(), padding=1))
        worst1 = check(f"dgrad bf16 {chan} {bhw} x{scale:g} rounded operands", got, ref_r, K * 2.0 ** -23 * S_r)
        ref = nhwc(F.conv_transpose2d(dm, wt, padding=1))
        S = nhwc(F.conv_transpose2d(dm.abs(), wt.abs(), padding=1))
        worst2 = check(f"dgrad bf16 {chan} {bhw} x{scale:g} exact operands", got, ref, (2 * u + u * u) * S + K * 2.0 ** -23 * S)
        print(f"dgrad bf16 {chan} {bhw} x{scale:g}: worst err / bound {worst1:.3e} (rounded operands) {worst2:.3e} (exact operands)")
        nonzero.append(int(torch.count_nonzero(got)))
        if cx == 8:
            assert torch.count_nonzero(got[..., 3:]) == 0 and torch.count_nonzero(got[..., :3]) > 0
    assert nonzero[1] == nonzero[0] > 0                                                     # 1e-8 did not vanish anywhere


def test_conv_dgrad_bf16_refuses_mismatched_operands():
    ops = _ops()
    dy, y = torch.zeros(1, 4, 4, 64, device="cuda"), torch.zeros(1, 4, 4, 64, device="cuda", dtype=torch.float16)
    wb = lambda *s: torch.zeros(*s, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="rotated weight"):
        ops.conv3x3_relu_dgrad_nhwc_bf16(dy, y, wb(64, 3, 3, 128))
    with pytest.raises(RuntimeError, match="rotated weight"):
        ops.conv3x3_relu_dgrad_nhwc_bf16(dy, y, torch.zeros(64, 3, 3, 64, device="cuda"))
    with pytest.raises(RuntimeError):
        ops.conv3x3_relu_dgrad_nhwc_bf16(dy, torch.zeros(1, 4, 5, 64, device="cuda", dtype=torch.float16), wb(64, 3, 3, 64))
    with pytest.raises(RuntimeError, match="float16"):
        ops.conv3x3_relu_dgrad_nhwc_bf16(dy, y.float(), wb(64, 3, 3, 64))
    with pytest.raises(RuntimeError, match="out"):
        ops.conv3x3_relu_dgrad_nhwc_bf16(dy, y, wb(64, 3, 3, 64), out=torch.zeros(1, 4, 4, 32, device="cuda"))


# ---------------------------------------------------------------------------------------------------- end to end
def ref_head(f0, f1, w):
    n0 = f0 / (torch.sqrt((f0 ** 2).sum(-1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt((f1 ** 2).sum(-1, keepdim=True)) + 1e-10)
    return ((n0 - n1) ** 2 * w).sum(-1).mean(dim=(1, 2))


def _first_argmax_2x2(a):
    """a NCHW -> index in {0..3} (row-major inside the window) of the first maximum of every 2x2 / 2 window."""
    N, C, H, W = a.shape
    Ho, Wo = H // 2, W // 2
    v = a[:, :, :2 * Ho, :2 * Wo].reshape(N, C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, Ho, Wo, 4)
    hit = v == v.max(-1, keepdim=True).values
    return torch.where(hit, torch.arange(4), torch.tensor(4)).min(-1).values


def gpu_decisions_fp16(m, x, y):
    """The fp16 forward chain on the kernels -> per conv the mask (stored fp16 y > 0), per pool the index of the first maximum, as NCHW CPU tensors."""
    ops = _ops()
    h = ops.lpips_prep_f16(x.cuda().float().contiguous(), y.cuda().float().contiguous())
    masks, picks, prev = [], [], 1
    for w, b, s in m.convs:
        if s != prev:
            picks.append(_first_argmax_2x2(nchw(h.cpu().float())))
            h = ops.maxpool2x2_nhwc_f16(h)
            prev = s
        h = ops.conv3x3_relu_nhwc_f16(h, w, b)
        masks.append(nchw((h > 0).cpu()))
    return masks, picks


class _EmuConv(torch.autograd.Function):
    """The contract's convolution in f64: forward on fp16-rounded input and weight with the output rounded to fp16; backward on bf16-rounded dy * mask
    and weight.  mask None: a free ReLU (the mask is the output's own sign)."""

    @staticmethod
    def forward(ctx, h, w, b, mask):
        pre = F.conv2d(r16(h), r16(w), b, padding=1)
        y = r16(pre * mask if mask is not None else pre.clamp(min=0.0))
        ctx.save_for_backward(w, (mask if mask is not None else y > 0).to(h.dtype))
        return y

    @staticmethod
    def backward(ctx, dy):
        w, mask = ctx.saved_tensors
        return F.conv_transpose2d(rb16(dy * mask), rb16(w), padding=1), None, None, None


def f64_lpips(sd, x, y, masks=None, picks=None, emulate=False):
    """The reference LPIPS forward in f64; masks / picks: the decisions forced (relu(pre) -> pre * mask, max pool -> a gather); emulate: the 16-bit
    contract (module docstring)."""
    from ldmae_amd.models.lpips import CONVS
    B = x.shape[0]
    h = torch.cat([(x - SHIFT) / SCALE, (y - SHIFT) / SCALE])
    out, prev, pool = 0, 1, 0

    def head(k):
        f = h.permute(0, 2, 3, 1)
        return ref_head(f[:B], f[B:], sd[f"lin{k}.model.1.weight"].double().reshape(-1))
    for j, (i, s, _, _) in enumerate(CONVS):
        if s != prev:
            out = out + head(prev - 1)
            if picks is None:
                h = F.max_pool2d(h, 2, 2)
            else:
                N, C, H, W = h.shape
                v = h[:, :, :2 * (H // 2), :2 * (W // 2)].reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
                h = torch.gather(v, -1, picks[pool].unsqueeze(-1)).squeeze(-1)
            pool, prev = pool + 1, s
        w, b = sd[f"net.slice{s}.{i}.weight"].double(), sd[f"net.slice{s}.{i}.bias"].double()
        mask = masks[j] if masks is not None else None
        if emulate:
            h = _EmuConv.apply(h, w, b, mask)
        else:
            pre = F.conv2d(h, w, b, padding=1)
            h = pre * mask if mask is not None else F.relu(pre)
    return out + head(prev - 1)


def emulated_errors(sd, m, x, y, wts):
    """-> (exact value, e_val, {half: (exact gradient, e_l2, e_max)}): the free exact value; the forced exact and forced emulated gradients of
    sum_b wts[b] value[b]; e_val = max_b |emulated - exact| / |exact| of the value, e_l2 / e_max the emulated gradient's rel L2 / max|err| / max|g|."""
    masks, picks = gpu_decisions_fp16(m, x, y)
    with torch.no_grad():
        val = f64_lpips(sd, x.double(), y.double())
    grads = {}
    for emulate in (False, True):
        xd, yd = x.double().requires_grad_(), y.double().requires_grad_()
        v = f64_lpips(sd, xd, yd, masks, picks, emulate=emulate)
        (v * wts).sum().backward()
        grads[emulate] = (v.detach(), xd.grad, yd.grad)
    e_val = float(((grads[True][0] - val).abs() / val.abs()).max())
    halves = {}
    for name, k in (("input", 1), ("target", 2)):
        g, ge = grads[False][k], grads[True][k]
        halves[name] = (g, float((ge - g).norm() / g.norm()), float((ge - g).abs().max() / g.abs().max()))
    return val, e_val, halves


@functools.lru_cache(maxsize=None)
def _e2e(B, H, W, seed):
    from ldmae_amd.models.lpips import LPIPS, random_state_dict
    sd = random_state_dict(3)
    m = LPIPS(state_dict=sd, device="cuda", differentiable=True, precision="fp16")
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, H, W, generator=gen) * 2 - 1
    y = (x + torch.randn(B, 3, H, W, generator=gen) * 0.2).clamp(-1, 1)
    wts = torch.arange(1, B + 1, dtype=torch.float64)
    val, e_val, halves = emulated_errors(sd, m, x, y, wts)
    print(f"lpips fp16 {(B, H, W, seed)}: emulated e_val {e_val:.3e}  " + "  ".join(f"{n}: e_l2 {h[1]:.3e} e_max {h[2]:.3e}" for n, h in halves.items()))
    return sd, m, x, y, val, e_val, halves


@pytest.mark.parametrize("fixture", [(2, 20, 24, 20), (3, 16, 16, 16), (1, 33, 47, 35)])
@pytest.mark.parametrize("which", ["target", "input", "both"])
def test_lpips_fp16_end_to_end(fixture, which):
    """Measured on the MI355X (share = GPU error / (4 x emulated error)): value 0.004 .. 0.30, gradient rel L2 0.24 .. 0.26, max|err| / max|g| 0.22 .. 0.28
    over the nine cases -- the GPU's error is the emulated arithmetic's own.  DESIGN.md section 18 has the table."""
    from ldmae_amd.models.lpips import LPIPS
    sd, m, x, y, val, e_val, halves = _e2e(*fixture)
    B = fixture[0]
    assert m.precision == "fp16"
    wts = torch.arange(1, B + 1, dtype=torch.float32, device="cuda")
    need_x, need_y = which in ("input", "both"), which in ("target", "both")

    def run():
        xg, yg = x.cuda().requires_grad_(need_x), y.cuda().requires_grad_(need_y)
        out = m(xg, yg)
        (out.view(-1) * wts).sum().backward()
        return out.detach(), xg.grad, yg.grad
    out, dx, dy = run()
    with torch.no_grad():
        fwd_only = LPIPS(state_dict=sd, device="cuda", precision="fp16")(x.cuda(), y.cuda())
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, 1, 1, 1) and torch.equal(out, fwd_only)      # bitwise the forward-only fp16 value
    v_err = float(((out.view(-1).cpu().double() - val).abs() / val.abs()).max())
    print(f"lpips fp16 {fixture} {which}: value rel err {v_err:.3e}  bound {MARGIN * e_val:.3e}  share {v_err / (MARGIN * e_val):.3f}")
    assert (dx is None) == (not need_x) and (dy is None) == (not need_y)            # a half that does not require grad gets None
    out2, dx2, dy2 = run()
    assert torch.equal(out, out2)
    shares = [v_err / (MARGIN * e_val)]
    for got, again, name in ((dx, dx2, "input"), (dy, dy2, "target")):
        if got is None:
            continue
        want, e_l2, e_max = halves[name]
        assert got.dtype == torch.float32 and torch.isfinite(got).all() and torch.equal(got, again)   # no atomics: the same bits from call to call
        d = got.double().cpu() - want
        l2, mx = float(d.norm() / want.norm()), float(d.abs().max() / want.abs().max())
        print(f"lpips fp16 {fixture} {which}/{name}: rel L2 {l2:.3e} bound {MARGIN * e_l2:.3e} share {l2 / (MARGIN * e_l2):.3f}   "
              f"max|err|/max|g| {mx:.3e} bound {MARGIN * e_max:.3e} share {mx / (MARGIN * e_max):.3f}")
        shares += [l2 / (MARGIN * e_l2), mx / (MARGIN * e_max)]
    assert max(shares) <= 1.0, shares


def test_all_zero_taps_give_an_exactly_zero_gradient():
    """Biases so negative that every ReLU output is 0: every tap pixel is all zero in both halves -- the value is 0 and the gradient exactly 0 (torch: NaN)."""
    from ldmae_amd.models.lpips import LPIPS, random_state_dict
    sd = random_state_dict(3)
    for k in sd:
        if k.endswith(".bias"):
            sd[k] = torch.full_like(sd[k], -1e3)
    m = LPIPS(state_dict=sd, device="cuda", differentiable=True, precision="fp16")
    gen = torch.Generator().manual_seed(1)
    x = (torch.rand(2, 3, 16, 16, generator=gen) * 2 - 1).cuda().requires_grad_()
    y = (torch.rand(2, 3, 16, 16, generator=gen) * 2 - 1).cuda().requires_grad_()
    out = m(x, y)
    out.sum().backward()
    assert torch.count_nonzero(out) == 0
    for g in (x.grad, y.grad):
        assert torch.isfinite(g).all() and torch.count_nonzero(g) == 0


# ---------------------------------------------------------------------------------------------------- the default is untouched
def test_default_is_the_f32_path_and_fp16_is_another():
    from ldmae_amd.models.lpips import LPIPS, random_state_dict
    sd = random_state_dict(3)
    gen = torch.Generator().manual_seed(9)
    x = torch.rand(2, 3, 20, 24, generator=gen) * 2 - 1
    y = (x + torch.randn(2, 3, 20, 24, generator=gen) * 0.2).clamp(-1, 1)
    res = {}
    for name, kw in (("default", {}), ("f32", {"precision": "f32"}), ("fp16", {"precision": "fp16"})):
        m = LPIPS(state_dict=sd, device="cuda", differentiable=True, **kw)
        xg, yg = x.cuda().requires_grad_(), y.cuda().requires_grad_()
        out = m(xg, yg)
        out.sum().backward()
        res[name] = (out.detach(), xg.grad, yg.grad, m)
    assert res["default"][3].precision == "f32" and res["default"][3].convs[0][0].dtype == torch.float32 and res["fp16"][3].convs[0][0].dtype == torch.float16
    assert res["fp16"][3].wrot[0].dtype == torch.bfloat16 and tuple(res["fp16"][3].wrot[0].shape) == (8, 3, 3, 64)
    for a, b in zip(res["default"][:3], res["f32"][:3]):
        assert torch.equal(a, b)
    for a, b in zip(res["default"][:3], res["fp16"][:3]):
        assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape and not torch.equal(a, b)      # a switch that does something
    assert torch.allclose(res["default"][0], res["fp16"][0], rtol=1e-2)


# ---------------------------------------------------------------------------------------------------- the stage-3 step
def test_stage3_step_with_fp16_lpips_stays_near_the_f32_lpips_step():
    """One step of the 32 x 32 / 24-block stage-3 model with precision="fp16" against the same step with the f32 LPIPS.  Loss: the two differ in the
    perceptual term alone, weighted by its ratio: |loss16 - loss32| <= ratio x 4 e_val x p_loss32, e_val emulated in f64 on this step's own image
    pair.  Gradients: rel L2 per trainable parameter below 2e-2, the bound the bf16 leg of test_stage3_step_matches_the_oracle_f32_and_bf16 uses."""
    from ldmae_amd.models.lpips import LPIPS, random_state_dict
    from ldmae_amd.tokenizer import models_mae
    lsd = random_state_dict(3)
    torch.manual_seed(0)
    m = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, smooth_output=True, kl_loss_weight=0.0, img_size=32,
                                            perceptual_loss=LPIPS(state_dict=lsd, device="cuda", differentiable=True), perceptual_loss_ratio=10.0).cuda()
    imgs = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)) * 2 - 1
    out32 = m(imgs.cuda(), mask_ratio=0.0)
    out32[0].backward()
    g32 = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    pimg = m.unpatchify(out32[1]).detach().float().cpu()
    m.zero_grad(set_to_none=True)
    m.perceptual_loss = LPIPS(state_dict=lsd, device="cuda", differentiable=True, precision="fp16")
    out16 = m(imgs.cuda(), mask_ratio=0.0)
    out16[0].backward()
    assert abs(float(out16[3].detach()) - float(out32[3].detach())) <= 1e-6 * abs(float(out32[3].detach()))            # vis_loss: nothing outside LPIPS changed
    _, e_val, _ = emulated_errors(lsd, m.perceptual_loss, imgs, pimg, torch.ones(2, dtype=torch.float64))
    loss32, loss16, p32, p16 = float(out32[0]), float(out16[0]), float(out32[4]), float(out16[4])
    bound = 10.0 * MARGIN * e_val * abs(p32)
    print(f"stage-3 step: loss f32-LPIPS {loss32:.8f} fp16-LPIPS {loss16:.8f}  p_loss {p32:.8f} / {p16:.8f}  |diff| {abs(loss16 - loss32):.3e}  bound {bound:.3e} "
          f"(e_val {e_val:.3e})")
    assert loss16 != loss32 and abs(loss16 - loss32) <= bound
    worst = ("", 0.0)
    for k, p in m.named_parameters():
        if not p.requires_grad:
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all() and k in g32, k
        rel = float((p.grad - g32[k]).norm() / g32[k].norm())
        worst = max(worst, (k, rel), key=lambda t: t[1])
        assert rel < 2e-2, (k, rel)
    print(f"stage-3 step: worst gradient rel L2 to the f32-LPIPS step {worst[1]:.3e} ({worst[0]})")


# ---------------------------------------------------------------------------------------------------- the driver
def test_stage3_driver_with_fp16_lpips_and_its_checkpoint_resumes_in_f32(tmp_path, capsys):
    from ldmae_amd import vmae_pretrain as vp
    from ldmae_amd.models.lpips import CONVS, random_state_dict
    from ldmae_amd.tokenizer import models_mae
    sd = random_state_dict(3)
    torch.save({f"features.{i}.{p}": sd[f"net.slice{s}.{i}.{p}"] for i, s, _, _ in CONVS for p in ("weight", "bias")}, tmp_path / "vgg16-397923af.pth")
    torch.save({k: v for k, v in sd.items() if k.startswith("lin")}, tmp_path / "vgg.pth")
    torch.manual_seed(7)
    m = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=False, no_cls=True, smooth_output=True, kl_loss_weight=1e-6, img_size=32)     # a stage-1 checkpoint
    torch.save({"model": m.state_dict(), "optimizer": {"junk": 1}, "epoch": 90, "scaler": None}, tmp_path / "checkpoint-90.pth")
    common = ["--synthetic", "--tune_decoder", "--perceptual_loss_ratio", "10.0", "--mask_ratio", "0.0", "--input_size", "32", "--batch_size", "4", "--epochs", "1",
              "--steps-per-epoch", "2", "--print_freq", "1", "--kl_loss_weight", "0.0", "--warmup_epochs", "0", "--blr", "1e-2", "--no_cls", "--smooth_output",
              "--lpips_vgg", str(tmp_path / "vgg16-397923af.pth"), "--lpips_lin", str(tmp_path / "vgg.pth")]

    def p_losses():
        log = capsys.readouterr().out
        vals = [float(v) for v in re.findall(r"p_loss: ([0-9.eE+-]+|nan|inf)", log)]
        assert len(vals) == 2 and all(torch.isfinite(torch.tensor(vals))) and all(v > 0 for v in vals), log
        return log, vals
    vp.main(common + ["--resume", str(tmp_path / "checkpoint-90.pth"), "--output_dir", str(tmp_path / "out16"), "--lpips_precision", "fp16"])
    log16, p16 = p_losses()
    assert "Using Perceptual loss with ratio = 10.0; LPIPS precision fp16" in log16
    ck = tmp_path / "out16" / "checkpoint-0.pth"
    assert ck.is_file() and torch.load(ck, map_location="cpu", weights_only=False)["args"]["lpips_precision"] == "fp16"
    vp.main(common + ["--resume", str(ck), "--output_dir", str(tmp_path / "out32")])          # the f32 driver takes the fp16 run's checkpoint
    log32, p32 = p_losses()
    assert "LPIPS precision f32" in log32 and f"Resume checkpoint {ck}" in log32 and (tmp_path / "out32" / "checkpoint-0.pth").is_file()
