"""The LPIPS backward (csrc/lpips_bwd.hip) and the stage-3 decoder tuning built on it, on the MI355X: every kernel against an f64 restatement written
here, the end-to-end gradient against an f64 reference with the ReLU / max-pool DECISIONS forced to the ones the GPU forward took (the gradient is
discontinuous in them: one flipped decision moves a free reference by 1e-2), the ldmae_mode training step against the CPU oracle, and the driver."""
import functools
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import mae as omae

pytestmark = pytest.mark.gpu

SHIFT = torch.tensor([-0.030, -0.088, -0.188], dtype=torch.float64).view(1, 3, 1, 1)
SCALE = torch.tensor([0.458, 0.448, 0.450], dtype=torch.float64).view(1, 3, 1, 1)
F32_BAR = 1e-4          # the project's f32 bar: max |err| <= 1e-4 max |want| per tensor


def _ops():
    from ldmae_amd import ops
    return ops


def ref_head(f0, f1, w):
    """models/lpips.py: normalize_tensor, (f0 - f1)^2, the 1x1 lin conv, spatial_average -- on NHWC [B, h, w, C], f64."""
    n0 = f0 / (torch.sqrt((f0 ** 2).sum(-1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt((f1 ** 2).sum(-1, keepdim=True)) + 1e-10)
    return ((n0 - n1) ** 2 * w).sum(-1).mean(dim=(1, 2))


def within_bar(got, want, what=""):
    err = (got.double().cpu() - want).abs().max().item()
    top = want.abs().max().item()
    print(f"{what}: max|err| {err:.3e}  max|want| {top:.3e}  ratio {err / max(top, 1e-300):.3e}")
    assert torch.isfinite(got).all() and err <= F32_BAR * top, (what, err, top)


# ---------------------------------------------------------------------------------------------------- head backward
@pytest.mark.parametrize("C", [64, 128, 256, 512])
@pytest.mark.parametrize("hw", [(1, 1), (5, 4), (17, 23)])
def test_lpips_head_backward(C, hw):
    gen = torch.Generator().manual_seed(C + hw[0])
    B = 3
    f = F.relu(torch.randn(2 * B, *hw, C, generator=gen))
    f[1, 0, 0] = 0.0                                             # an all-zero pixel of the input half, image 1
    w = torch.rand(C, generator=gen)
    g = torch.tensor([0.5, -1.25, 2.0])
    f0 = f[:B].double().requires_grad_()
    f1 = f[B:].double().requires_grad_()
    (ref_head(f0, f1, w.double()) * g.double()).sum().backward()
    want0, want1 = f0.grad.clone(), f1.grad.clone()
    assert torch.isnan(want0[1, 0, 0]).all()                     # torch: sqrt's backward at 0; here the pixel's gradient is DEFINED as 0
    want0[1, 0, 0] = 0.0
    assert torch.isfinite(want0).all() and torch.isfinite(want1).all()
    ops = _ops()
    fc, wc, gc = f.cuda(), w.cuda(), g.cuda()
    new = lambda: torch.full((B, *hw, C), float("nan"), device="cuda")        # overwritten, never read
    d0, d1 = ops.lpips_layer_bwd(fc, wc, gc, d_input=new(), d_target=new())
    within_bar(d0, want0, "both / input")
    within_bar(d1, want1, "both / target")
    assert torch.count_nonzero(d0[1, 0, 0]) == 0                                # finite (checked above) and exactly zero
    t0, t1 = ops.lpips_layer_bwd(fc, wc, gc, d_target=new())
    assert t0 is None and torch.equal(t1, d1)
    i0, i1 = ops.lpips_layer_bwd(fc, wc, gc, d_input=new())
    assert i1 is None and torch.equal(i0, d0)
    # accumulate: adds to what the buffer holds (the pool backward's gradient)
    pre = torch.randn(B, *hw, C, generator=gen) * want1.abs().max().float()
    acc = pre.cuda()
    ops.lpips_layer_bwd(fc, wc, gc, d_target=acc, accumulate=True)
    assert torch.equal(acc, pre.cuda() + d1)
    err = (acc.double().cpu() - (pre.double() + want1)).abs().max().item()
    assert err <= F32_BAR * want1.abs().max().item() + 2.0 ** -23 * pre.abs().max().item()     # + one f32 rounding of the sum
    with pytest.raises(RuntimeError, match="neither"):
        ops.lpips_layer_bwd(fc, wc, gc)
    with pytest.raises(RuntimeError, match="d_target"):
        ops.lpips_layer_bwd(fc, wc, gc, d_target=torch.zeros(B, *hw, C // 2, device="cuda"))


# ---------------------------------------------------------------------------------------------------- pool backward
def _torch_pool_bwd(x, dy):
    xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_()
    F.max_pool2d(xt, 2, 2).backward(dy.permute(0, 3, 1, 2).contiguous())
    return xt.grad.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("shape", [(2, 5, 7, 64), (1, 2, 2, 4), (3, 16, 16, 128)])
def test_maxpool_backward_equals_torch(shape):
    gen = torch.Generator().manual_seed(shape[1])
    B, H, W, C = shape
    n = B * H * W * C
    x = (torch.randperm(n, generator=gen).float() - n // 2).reshape(shape) / 8.0          # distinct values: no ties
    dy = torch.randn(B, H // 2, W // 2, C, generator=gen)
    out = torch.full(shape, float("nan"), device="cuda")                                   # every element is written: no memset needed
    got = _ops().maxpool2x2_bwd_nhwc(dy.cuda(), x.cuda(), out=out).cpu()
    assert torch.equal(got, _torch_pool_bwd(x, dy))
    assert torch.count_nonzero(got[:, 2 * (H // 2):]) == 0 and torch.count_nonzero(got[:, :, 2 * (W // 2):]) == 0     # the odd row / column


def test_maxpool_backward_ties_go_to_the_first_element():
    gen = torch.Generator().manual_seed(3)
    B, H, W, C = 2, 5, 7, 64
    x = F.relu(torch.randn(B, H, W, C, generator=gen))
    x[0, 0:2, 0:2] = 0.0                                        # a window that is all zero in every channel
    x[1, 2:4, 4:6, :32] = 0.0
    x[1, 0:2, 2:4, 5] = 1.5                                     # a four-way tie of a non-zero value
    dy = torch.randn(B, H // 2, W // 2, C, generator=gen).abs() + 0.5
    got = _ops().maxpool2x2_bwd_nhwc(dy.cuda(), x.cuda()).cpu()
    assert torch.equal(got[0, 0, 0], dy[0, 0, 0]) and torch.count_nonzero(got[0, 0, 1]) == 0 and torch.count_nonzero(got[0, 1, 0:2]) == 0
    assert torch.equal(got[1, 2, 4, :32], dy[1, 1, 2, :32]) and torch.count_nonzero(got[1, 2, 5, :32]) == 0 and torch.count_nonzero(got[1, 3, 4:6, :32]) == 0
    assert got[1, 0, 2, 5] == dy[1, 0, 1, 5] and got[1, 0, 3, 5] == 0 and got[1, 1, 2, 5] == 0 and got[1, 1, 3, 5] == 0
    # every window hands its gradient to exactly one element
    s = got[:, :4, :6].reshape(B, 2, 2, 3, 2, C).sum(dim=(2, 4))
    assert torch.equal(s, dy) and torch.equal((got[:, :4, :6] != 0).reshape(B, 2, 2, 3, 2, C).sum(dim=(2, 4)), torch.ones(B, 2, 3, C, dtype=torch.long))
    assert torch.equal(got, _torch_pool_bwd(x, dy))             # torch's CPU kernel keeps the first maximum too


def test_maxpool_backward_without_a_window_is_all_zero():
    x = torch.randn(1, 3, 1, 64)                                # W // 2 == 0: dy is empty
    dy = torch.zeros(1, 1, 0, 64)
    got = _ops().maxpool2x2_bwd_nhwc(dy.cuda(), x.cuda(), out=torch.full((1, 3, 1, 64), float("nan"), device="cuda"))
    assert torch.count_nonzero(got) == 0
    with pytest.raises(RuntimeError, match="dy"):
        _ops().maxpool2x2_bwd_nhwc(torch.zeros(1, 1, 1, 64, device="cuda"), x.cuda())


# ---------------------------------------------------------------------------------------------------- conv data gradient
@pytest.mark.parametrize("chan", [(4, 64), (64, 64), (128, 256), (512, 512)])
@pytest.mark.parametrize("bhw", [(3, 5, 7), (2, 12, 11), (2, 1, 1)])
def test_conv_dgrad_with_relu_mask(chan, bhw):
    """dx = conv_transpose(dy * [y > 0], w) per element within the f32 dot-product bound over K = 9 Cout terms: |err| <= K 2^-23 sum |dy w|."""
    from gemm_check import check
    from ldmae_amd.models.lpips import rotate_weight
    cin, cout = chan
    B, H, W = bhw
    gen = torch.Generator().manual_seed(cin + cout + H)
    w = torch.randn(cout, 3, 3, cin, generator=gen) * (2.0 / (cin * 9)) ** 0.5               # channels-last forward weight
    if cin == 4:
        w[..., 3] = 0.0                                                                     # conv1_1: the padding channel
    dy = torch.randn(B, H, W, cout, generator=gen)
    y = F.relu(torch.randn(B, H, W, cout, generator=gen))                                   # about half zeros: the mask is an INPUT here
    assert 0.3 < float((y > 0).float().mean()) < 0.7
    got = _ops().conv3x3_relu_dgrad_nhwc(dy.cuda(), y.cuda(), rotate_weight(w).cuda()).cpu()
    assert tuple(got.shape) == (B, H, W, cin)
    dm = (dy.double() * (y > 0)).permute(0, 3, 1, 2)
    wt = w.double().permute(0, 3, 1, 2)                                                     # [Cout, Cin, ky, kx]
    ref = F.conv_transpose2d(dm, wt, padding=1).permute(0, 2, 3, 1)
    S = F.conv_transpose2d(dm.abs(), wt.abs(), padding=1).permute(0, 2, 3, 1)
    K = 9 * cout
    worst = check(f"dgrad {chan} {bhw}", got, ref, K * 2.0 ** -23 * S)
    print(f"dgrad {chan} {bhw}: worst err / bound {worst:.3e}")
    if cin == 4:
        assert torch.count_nonzero(got[..., 3]) == 0
    xg = torch.zeros(B, cin, H, W, dtype=torch.float64, requires_grad=True)                 # and it is the autograd gradient of relu(conv)
    pre = F.conv2d(xg, wt, padding=1)
    (gx,) = torch.autograd.grad(pre, xg, dm)
    assert torch.allclose(gx.permute(0, 2, 3, 1), ref, rtol=1e-12, atol=1e-12)


def test_conv_dgrad_refuses_mismatched_operands():
    ops = _ops()
    dy, y = torch.zeros(1, 4, 4, 64, device="cuda"), torch.zeros(1, 4, 4, 64, device="cuda")
    with pytest.raises(RuntimeError, match="rotated weight"):
        ops.conv3x3_relu_dgrad_nhwc(dy, y, torch.zeros(64, 3, 3, 128, device="cuda"))
    with pytest.raises(RuntimeError):
        ops.conv3x3_relu_dgrad_nhwc(dy, torch.zeros(1, 4, 5, 64, device="cuda"), torch.zeros(64, 3, 3, 64, device="cuda"))
    g = torch.randn(2, 5, 6, 4, device="cuda")
    out = ops.lpips_prep_bwd(g).cpu().double()
    assert torch.allclose(out, g.cpu().double()[..., :3].permute(0, 3, 1, 2) / SCALE, rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------------- end to end, decisions forced
def _first_argmax_2x2(a):
    """a NCHW -> index in {0..3} (row-major inside the window) of the first maximum of every 2x2 / 2 window."""
    N, C, H, W = a.shape
    Ho, Wo = H // 2, W // 2
    v = a[:, :, :2 * Ho, :2 * Wo].reshape(N, C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, Ho, Wo, 4)
    hit = v == v.max(-1, keepdim=True).values
    return torch.where(hit, torch.arange(4), torch.tensor(4)).min(-1).values


def gpu_decisions(m, x, y):
    """The forward chain of LPIPS on the kernels -> per conv the mask (y > 0), per pool the argmax index (first in row-major order), as NCHW CPU tensors."""
    ops = _ops()
    h = ops.lpips_prep(x.cuda().float().contiguous(), y.cuda().float().contiguous())
    masks, picks, prev = [], [], 1
    for w, b, s in m.convs:
        if s != prev:
            picks.append(_first_argmax_2x2(h.cpu().permute(0, 3, 1, 2)))
            h = ops.pool2d_nhwc(h, "max", k=2, stride=2, pad=0)
            prev = s
        h = ops.conv2d_nhwc(h, w, b, (1, 1), (1, 1), True)
        masks.append((h > 0).cpu().permute(0, 3, 1, 2))
    return masks, picks


def forced_lpips(sd, x, y, masks, picks):
    """The reference LPIPS forward in the dtype of x / y with relu(pre) replaced by pre * mask and the max pool by a gather at the given indices."""
    from ldmae_amd.models.lpips import CONVS
    dt = x.dtype
    B = x.shape[0]
    h = torch.cat([(x - SHIFT.to(dt)) / SCALE.to(dt), (y - SHIFT.to(dt)) / SCALE.to(dt)])
    out, prev, pool = 0, 1, 0

    def head(k):
        f = h.permute(0, 2, 3, 1)
        return ref_head(f[:B], f[B:], sd[f"lin{k}.model.1.weight"].to(dt).reshape(-1))
    for j, (i, s, _, _) in enumerate(CONVS):
        if s != prev:
            out = out + head(prev - 1)
            N, C, H, W = h.shape
            v = h[:, :, :2 * (H // 2), :2 * (W // 2)].reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
            h = torch.gather(v, -1, picks[pool].unsqueeze(-1)).squeeze(-1)
            pool, prev = pool + 1, s
        h = F.conv2d(h, sd[f"net.slice{s}.{i}.weight"].to(dt), sd[f"net.slice{s}.{i}.bias"].to(dt), padding=1) * masks[j]
    return out + head(prev - 1)


@functools.lru_cache(maxsize=None)
def _e2e(B, H, W, seed):
    from ldmae_amd.models.lpips import LPIPS, random_state_dict
    sd = random_state_dict(3)
    m = LPIPS(state_dict=sd, device="cuda", differentiable=True)
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, H, W, generator=gen) * 2 - 1
    y = (x + torch.randn(B, 3, H, W, generator=gen) * 0.2).clamp(-1, 1)
    masks, picks = gpu_decisions(m, x, y)
    xd, yd = x.double().requires_grad_(), y.double().requires_grad_()
    wts = torch.arange(1, B + 1, dtype=torch.float64)
    val = forced_lpips(sd, xd, yd, masks, picks)
    (val * wts).sum().backward()
    return sd, m, x, y, val.detach(), xd.grad, yd.grad


@pytest.mark.parametrize("fixture", [(2, 20, 24, 20), (3, 16, 16, 16), (1, 33, 47, 35)])
@pytest.mark.parametrize("which", ["target", "input", "both"])
def test_lpips_gradient_end_to_end(fixture, which):
    from ldmae_amd.models.lpips import LPIPS
    sd, m, x, y, val, gx, gy = _e2e(*fixture)
    B = fixture[0]
    wts = torch.arange(1, B + 1, dtype=torch.float32, device="cuda")
    need_x, need_y = which in ("input", "both"), which in ("target", "both")

    def run():
        xg, yg = x.cuda().requires_grad_(need_x), y.cuda().requires_grad_(need_y)
        out = m(xg, yg)
        (out.view(-1) * wts).sum().backward()
        return out.detach(), xg.grad, yg.grad
    out, dx, dy = run()
    fwd_only = LPIPS(state_dict=sd, device="cuda")
    with torch.no_grad():
        assert torch.equal(out, fwd_only(x.cuda(), y.cuda()))                      # the differentiable value IS the forward-only value
    assert tuple(out.shape) == (B, 1, 1, 1) and torch.allclose(out.view(-1).cpu().double(), val, rtol=1e-4, atol=0)
    assert (dx is None) == (not need_x) and (dy is None) == (not need_y)            # a half that does not require grad gets None
    out2, dx2, dy2 = run()
    for got, again, want, name in ((dx, dx2, gx, "input"), (dy, dy2, gy, "target")):
        if got is None:
            continue
        assert torch.equal(got, again)                                               # no atomics: the same bits from call to call
        rel = float((got.double().cpu() - want).norm() / want.norm())
        print(f"lpips grad {fixture} {which}/{name}: rel L2 {rel:.3e}")
        assert rel <= 1e-4, (name, rel)
        within_bar(got, want, f"lpips grad {fixture} {which}/{name}")


def test_forward_only_lpips_still_refuses_grad():
    from ldmae_amd.models.lpips import LPIPS, random_state_dict
    m = LPIPS(state_dict=random_state_dict(3), device="cuda")
    assert m.differentiable is False and not hasattr(m, "wrot")
    with pytest.raises(RuntimeError, match="forward-only"):
        m(torch.zeros(1, 3, 16, 16, device="cuda", requires_grad=True), torch.zeros(1, 3, 16, 16, device="cuda"))


# ---------------------------------------------------------------------------------------------------- the ldmae_mode training step
CHECKED = ("decoder_pred.linear_pred.weight", "decoder_pred.conv_smoother.weight", "decoder_pred.conv_smoother.bias", "decoder_blocks.5.attn.qkv.weight",
           "decoder_blocks.5.mlp.fc1.weight", "decoder_blocks.5.norm1.weight", "from_latent.weight", "to_latent.weight", "patch_embed.proj.weight")
ENCODER = ("to_latent.weight", "patch_embed.proj.weight", "blocks.0.attn.qkv.weight", "norm.weight")


def _stage3_model(seed=0):
    from ldmae_amd.models.lpips import LPIPS, random_state_dict
    from ldmae_amd.tokenizer import models_mae
    lsd = random_state_dict(3)
    torch.manual_seed(seed)
    m = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, smooth_output=True, kl_loss_weight=0.0, img_size=32,
                                            perceptual_loss=LPIPS(state_dict=lsd, device="cuda", differentiable=True), perceptual_loss_ratio=10.0).cuda()
    gen = torch.Generator().manual_seed(seed + 1)
    imgs = torch.rand(2, 3, 32, 32, generator=gen) * 2 - 1
    return m, lsd, imgs


def _oracle_step(m, lsd, imgs, pimg_gpu, eps=None):
    """forward_ldmae restated on the CPU oracle in f64 (encode_moments -> posterior mode, or mean + std eps -> decode -> MSE + 10 LPIPS), LPIPS with the
    decisions of the GPU forward on (imgs, the GPU's predicted image)."""
    cfg = omae.MAEConfig(img_size=32, ldmae_mode=True)
    osd = {k: v.detach().cpu().double().requires_grad_(k in CHECKED) for k, v in m.state_dict().items()}
    x = imgs.double()
    mom = omae.encode_moments(osd, x, cfg)
    mean, logvar = mom[:, :16], mom[:, 16:].clamp(-30.0, 20.0)
    z = mean if eps is None else mean + torch.exp(0.5 * logvar) * eps.double().reshape(mean.shape)
    if eps is not None:
        z = z.detach()                                                            # the encoder ran under no_grad
    img = omae.decode(osd, z, cfg)
    masks, picks = gpu_decisions(m.perceptual_loss, imgs, pimg_gpu.detach().cpu())
    vis = ((img - x) ** 2).mean()
    p = forced_lpips(lsd, x, img, masks, picks).mean()
    loss = vis + 10.0 * p
    loss.backward()
    return loss.item(), vis.item(), p.item(), {k: osd[k].grad for k in CHECKED}


def _check_step(m, out, want, expect_none=()):
    loss, pred, mask, vis, p, kl = out
    wl, wv, wp, wg = want
    assert mask is None and kl is None and tuple(pred.shape) == (2, 16, 192)
    for got, w, name in ((loss, wl, "loss"), (vis, wv, "vis_loss"), (p, wp, "p_loss")):
        print(f"{name}: got {float(got.detach()):.8f} want {w:.8f}")
        assert abs(float(got.detach()) - w) <= F32_BAR * abs(w), name
    params = dict(m.named_parameters())
    for k in CHECKED:
        if k in expect_none:
            assert params[k].grad is None, k
        else:
            within_bar(params[k].grad, wg[k], k)


def test_stage3_step_matches_the_oracle_f32_and_bf16():
    """mask_ratio 0.0: the encoder trains through the posterior mode; loss, vis_loss, p_loss and gradients from the prediction head down to the patch
    embedding against the f64 oracle; then the same step under bf16 autocast within the pre-training step's bf16 tolerance (tests/test_gpu_mae.py: 2e-2)."""
    m, lsd, imgs = _stage3_model()
    out = m(imgs.cuda(), mask_ratio=0.0)
    out[0].backward()
    pimg = m.unpatchify(out[1])
    _check_step(m, out, _oracle_step(m, lsd, imgs, pimg))
    assert all(p.grad is not None for p in m.parameters() if p.requires_grad)           # nothing is frozen: the encoder trains too
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out16 = m(imgs.cuda(), mask_ratio=0.0)
    out16[0].backward()
    assert torch.isfinite(out16[0]) and abs(float(out16[0]) - float(out[0])) < 2e-2 * abs(float(out[0])), (float(out16[0]), float(out[0]))
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    assert m.decoder_blocks[0].last_dtype == torch.bfloat16 and m.blocks[0].last_dtype == torch.bfloat16


def test_stage3_step_with_a_mask_ratio_samples_and_leaves_the_encoder_alone():
    """mask_ratio > 0: the encoder runs under no_grad (no gradient reaches it) and the posterior is SAMPLED, by the draw torch.randn makes on the device."""
    m, lsd, imgs = _stage3_model(seed=2)
    with torch.no_grad():
        m.to_latent.bias[16:] += 1.0                                              # a visible posterior std, so that the draw matters
    torch.manual_seed(5)
    eps = torch.randn(2, 16, 16, device="cuda")                                   # [B, latent, N]: the shape sample() draws
    out = m(imgs.cuda(), mask_ratio=0.25, _eps=eps)
    out[0].backward()
    _check_step(m, out, _oracle_step(m, lsd, imgs, m.unpatchify(out[1]), eps=eps.cpu()), expect_none=("to_latent.weight", "patch_embed.proj.weight"))
    params = dict(m.named_parameters())
    assert all(params[k].grad is None for k in ENCODER)
    torch.manual_seed(5)
    again = m(imgs.cuda(), mask_ratio=0.25)                                       # the same draw, made inside
    assert torch.equal(again[0], out[0])
    mode = m(imgs.cuda(), mask_ratio=0.0)
    assert abs(float(mode[0]) - float(out[0])) > 1e-3 * abs(float(out[0]))         # sampled, not the mode


# ---------------------------------------------------------------------------------------------------- the driver
def _write_stage3_inputs(tmp_path):
    from ldmae_amd.models.lpips import CONVS, random_state_dict
    from ldmae_amd.tokenizer import models_mae
    sd = random_state_dict(3)
    vgg = {f"features.{i}.{p}": sd[f"net.slice{s}.{i}.{p}"] for i, s, _, _ in CONVS for p in ("weight", "bias")}
    lin = {k: v for k, v in sd.items() if k.startswith("lin")}
    torch.save(vgg, tmp_path / "vgg16-397923af.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    torch.manual_seed(7)
    m = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=False, no_cls=True, smooth_output=True, kl_loss_weight=1e-6, img_size=32)     # a stage-1 checkpoint
    start = {k: v.clone() for k, v in m.state_dict().items()}
    torch.save({"model": start, "optimizer": {"junk": 1}, "epoch": 90, "scaler": None}, tmp_path / "checkpoint-90.pth")
    return start


@pytest.mark.parametrize("mask_ratio", ["0.0", "0.75"])
def test_stage3_driver(tmp_path, capsys, mask_ratio):
    from ldmae_amd import vmae_pretrain as vp
    from ldmae_amd.tokenizer import models_mae
    start = _write_stage3_inputs(tmp_path)
    out_dir = tmp_path / "out"
    vp.main(["--synthetic", "--tune_decoder", "--perceptual_loss_ratio", "10.0", "--mask_ratio", mask_ratio, "--input_size", "32", "--batch_size", "4", "--epochs", "1",
             "--steps-per-epoch", "3", "--print_freq", "1", "--kl_loss_weight", "0.0", "--warmup_epochs", "0", "--blr", "1e-2", "--no_cls", "--smooth_output",
             "--resume", str(tmp_path / "checkpoint-90.pth"), "--lpips_vgg", str(tmp_path / "vgg16-397923af.pth"), "--lpips_lin", str(tmp_path / "vgg.pth"),
             "--output_dir", str(out_dir)])
    log = capsys.readouterr().out
    p_losses = [float(v) for v in re.findall(r"p_loss: ([0-9.eE+-]+|nan|inf)", log)]
    assert len(p_losses) == 3 and all(torch.isfinite(torch.tensor(p_losses))) and all(v > 0 for v in p_losses), log
    assert "mask_loss: 0.000000" in log and "kl_loss: 0.000000" in log and "vis_loss: " in log
    assert "With optim & sched!" not in log                                        # the model alone is restored (the checkpoint's optimizer entry is junk)
    ck = torch.load(out_dir / "checkpoint-0.pth", map_location="cpu", weights_only=False)
    ref_keys = set(models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, smooth_output=True, kl_loss_weight=0.0, img_size=32).state_dict())
    assert set(ck["model"]) == ref_keys and "mask_token" not in ck["model"] and not any("perceptual" in k for k in ck["model"])
    moved = {k: not torch.equal(ck["model"][k], start[k]) for k in ref_keys}
    assert moved["decoder_pred.linear_pred.weight"] and moved["decoder_blocks.3.mlp.fc1.weight"] and moved["from_latent.weight"]
    encoder = [k for k in ref_keys if "decoder" not in k and "from_latent" not in k]
    assert "patch_embed.proj.weight" in encoder and "blocks.0.attn.qkv.weight" in encoder and "to_latent.weight" in encoder
    if mask_ratio == "0.75":
        assert not any(moved[k] for k in encoder), [k for k in encoder if moved[k]]      # frozen: bitwise unchanged
        assert "parameters frozen" in log
    else:
        assert moved["patch_embed.proj.weight"] and moved["blocks.0.attn.qkv.weight"]     # the shipped flags freeze nothing (the reference's quirk)
        assert "No layers are frozen" in log
