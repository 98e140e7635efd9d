"""Tokenizer evaluation on the MI355X: every kernel of csrc/tokenizer_eval.hip against an f64 torch restatement written here, LPIPS end to end
against F.conv2d in f64, and the evaluate_tokenizer driver on synthetic images with random VMAE, LPIPS and Inception weights."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHIFT = torch.tensor([-0.030, -0.088, -0.188], dtype=torch.float64).view(1, 3, 1, 1)
SCALE = torch.tensor([0.458, 0.448, 0.450], dtype=torch.float64).view(1, 3, 1, 1)


def _ops():
    from ldmae_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------- f64 restatements
def ref_head(f0, f1, w):
    """models/lpips.py: normalize_tensor, (f0 - f1)^2, the 1x1 lin conv, spatial_average -- on NHWC [B, h, w, C], f64."""
    n0 = f0 / (torch.sqrt((f0 ** 2).sum(-1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt((f1 ** 2).sum(-1, keepdim=True)) + 1e-10)
    return ((n0 - n1) ** 2 * w).sum(-1).mean(dim=(1, 2))


def ref_ssim(x, y, lo=-1.0, hi=1.0):
    """torchmetrics 1.x _ssim_update with its defaults, per image, f64."""
    x, y = x.double().clamp(lo, hi), y.double().clamp(lo, hi)
    C = x.shape[1]
    d = torch.arange(-5, 6, dtype=torch.float64)
    g = torch.exp(-((d / 1.5) ** 2) / 2)
    g = g / g.sum()
    k = (g[:, None] * g[None, :]).expand(C, 1, 11, 11)
    xp, yp = F.pad(x, (5, 5, 5, 5), mode="reflect"), F.pad(y, (5, 5, 5, 5), mode="reflect")
    o = F.conv2d(torch.cat([xp, yp, xp * xp, yp * yp, xp * yp]), k, groups=C).split(x.shape[0])
    c1, c2 = (0.01 * (hi - lo)) ** 2, (0.03 * (hi - lo)) ** 2
    mx2, my2, mxy = o[0] ** 2, o[1] ** 2, o[0] * o[1]
    sx, sy, sxy = (o[2] - mx2).clamp(min=0), (o[3] - my2).clamp(min=0), o[4] - mxy
    m = ((2 * mxy + c1) * (2 * sxy + c2)) / ((mx2 + my2 + c1) * (sx + sy + c2))
    return m[..., 5:-5, 5:-5].reshape(x.shape[0], -1).mean(-1)


def ref_lpips(sd, x, y):
    """The reference LPIPS forward (ScalingLayer, VGG16 slices, heads) with F.conv2d / max_pool2d in f64 on the CPU."""
    from ldmae_amd.models.lpips import CONVS
    out = torch.zeros(x.shape[0], dtype=torch.float64)
    hs = [(x.double() - SHIFT) / SCALE, (y.double() - SHIFT) / SCALE]
    prev = 1

    def head(k):
        w = sd[f"lin{k}.model.1.weight"].double().reshape(-1)
        return ref_head(hs[0].permute(0, 2, 3, 1), hs[1].permute(0, 2, 3, 1), w)

    for i, s, _, _ in CONVS:
        if s != prev:
            out += head(prev - 1)
            hs = [F.max_pool2d(h, 2, 2) for h in hs]
            prev = s
        w, b = sd[f"net.slice{s}.{i}.weight"].double(), sd[f"net.slice{s}.{i}.bias"].double()
        hs = [F.relu(F.conv2d(h, w, b, padding=1)) for h in hs]
    return out + head(prev - 1)


# ---------------------------------------------------------------------------------------------------- kernels
def test_lpips_prep():
    g = torch.Generator().manual_seed(0)
    x, y = torch.rand(3, 3, 17, 23, generator=g) * 2.4 - 1.2, torch.rand(3, 3, 17, 23, generator=g) * 2 - 1
    out = _ops().lpips_prep(x.cuda(), y.cuda()).cpu()
    assert tuple(out.shape) == (6, 17, 23, 4)
    want = torch.cat([(x.double() - SHIFT) / SCALE, (y.double() - SHIFT) / SCALE]).permute(0, 2, 3, 1)
    assert torch.allclose(out[..., :3].double(), want, rtol=1e-6, atol=1e-6)
    assert torch.count_nonzero(out[..., 3]) == 0


@pytest.mark.parametrize("C", [64, 128, 256, 512])
@pytest.mark.parametrize("hw", [(17, 23), (1, 1), (64, 64)])
def test_lpips_head(C, hw):
    g = torch.Generator().manual_seed(C + hw[0])
    B = 3
    f = F.relu(torch.randn(2 * B, *hw, C, generator=g))
    f[1, 0, 0] = 0.0                                          # an all-zero pixel: the 1e-10 guard, no NaN
    w = torch.rand(C, generator=g)
    out = torch.full((B,), 0.25, device="cuda")              # accumulates into out
    _ops().lpips_layer(f.cuda(), w.cuda(), out)
    want = 0.25 + ref_head(f[:B].double(), f[B:].double(), w.double())
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6), (got, want)
    same = torch.zeros(B, device="cuda")
    _ops().lpips_layer(torch.cat([f[:B], f[:B]]).cuda(), w.cuda(), same)
    assert torch.count_nonzero(same) == 0


@pytest.mark.parametrize("shape", [(2, 3, 11, 11), (3, 3, 37, 53), (2, 3, 256, 256)])
def test_ssim(shape):
    from ldmae_amd.metrics import ssim
    g = torch.Generator().manual_seed(shape[2])
    y = torch.randn(*shape, generator=g) * 0.7                      # partly outside [-1, 1]: the clamp matters
    x = y + torch.randn(*shape, generator=g) * 0.3
    got = ssim(x.cuda(), y.cuda(), reduction="none").cpu().double()
    want = ref_ssim(x, y)
    assert torch.allclose(got, want, rtol=0, atol=2e-5), (got, want)
    assert float(ssim(x.cuda(), y.cuda())) == pytest.approx(float(want.mean()), abs=2e-5)
    same = ssim(x.cuda(), x.cuda(), reduction="none").cpu()
    assert torch.allclose(same, torch.ones_like(same), atol=1e-5)
    const = torch.full(shape, 0.3, device="cuda")
    c = ssim(const, const, reduction="none").cpu()
    assert torch.equal(c, torch.ones_like(c))                      # moments about a per-tile shift: exactly 0 variance, exactly 1
    c2 = ssim(const, -const, reduction="none").cpu().double()
    assert torch.isfinite(c2).all() and torch.allclose(c2, ref_ssim(const.cpu(), -const.cpu()), atol=1e-5)


def test_ssim_unclamped_data_range():
    from ldmae_amd.metrics import ssim
    g = torch.Generator().manual_seed(5)
    y = torch.randn(2, 3, 40, 31, generator=g)
    x = y + torch.randn(2, 3, 40, 31, generator=g) * 0.5
    got = ssim(x.cuda(), y.cuda(), data_range=4.0, reduction="none").cpu().double()
    xd, yd = x.double(), y.double()
    d = torch.arange(-5, 6, dtype=torch.float64)
    gk = torch.exp(-((d / 1.5) ** 2) / 2)
    gk = gk / gk.sum()
    k = (gk[:, None] * gk[None, :]).expand(3, 1, 11, 11)
    o = F.conv2d(torch.cat([xd, yd, xd * xd, yd * yd, xd * yd]), k, groups=3).split(2)
    c1, c2 = 0.04 ** 2, 0.12 ** 2
    m = ((2 * o[0] * o[1] + c1) * (2 * (o[4] - o[0] * o[1]) + c2)) / \
        ((o[0] ** 2 + o[1] ** 2 + c1) * ((o[2] - o[0] ** 2).clamp(min=0) + (o[3] - o[1] ** 2).clamp(min=0) + c2))
    want = m.reshape(2, -1).mean(-1)
    assert torch.allclose(got, want, atol=2e-5)


def test_quantize_and_psnr():
    from ldmae_amd.metrics import psnr_from_sse, psnr_uint8
    g = torch.Generator().manual_seed(1)
    B, H, W = 3, 37, 29
    dec = torch.randn(B, 3, H, W, generator=g) * 0.8
    ref = torch.randn(B, 3, H, W, generator=g) * 0.8
    # rounding edges: the exact boundaries, values just around them, far outside [-1, 1]
    edge = torch.tensor([-1.0, 1.0, -1.0039216, 0.9960785, 0.0, -2.0, 3.0, 127.0 / 127.5 - 1.0, 1.0 / 255.0, -0.5, 0.5, 1e-8])
    dec.view(-1)[:edge.numel()] = edge
    ref[2] = dec[2]
    dec8, ref8, sse = _ops().recon_quantize_sse(dec.cuda(), ref.cuda())
    want_d = torch.clamp(127.5 * dec + 128.0, 0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    want_r = torch.clamp(127.5 * ref + 128.0, 0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    assert torch.equal(dec8.cpu(), want_d) and torch.equal(ref8.cpu(), want_r)
    want_sse = ((want_d.numpy().astype(np.int64) - want_r.numpy().astype(np.int64)) ** 2).reshape(B, -1).sum(1)
    assert sse.cpu().tolist() == want_sse.tolist()
    p = psnr_from_sse(sse, 3 * H * W).cpu()
    assert p[2] == float("inf")
    assert torch.allclose(p[:2], torch.from_numpy(20 * np.log10(255.0 / np.sqrt(want_sse[:2] / (3 * H * W)))), rtol=1e-12)
    assert torch.equal(psnr_uint8(dec8, ref8).cpu(), p)
    assert _ops().sse_u8(dec8, ref8).cpu().tolist() == want_sse.tolist()


# ---------------------------------------------------------------------------------------------------- LPIPS end to end
@pytest.mark.parametrize("B,S", [(3, 64), (1, 256)])
def test_lpips_matches_f64_reference(B, S):
    from ldmae_amd.models.lpips import LPIPS, random_state_dict
    sd = random_state_dict(3)
    m = LPIPS(state_dict=sd, device="cuda")
    g = torch.Generator().manual_seed(S)
    x = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    y = (x + torch.randn(B, 3, S, S, generator=g) * 0.2).clamp(-1, 1)
    got = m(x.cuda(), y.cuda())
    assert tuple(got.shape) == (B, 1, 1, 1)
    got = got.view(-1).cpu().double()
    want = ref_lpips(sd, x, y)
    rel = ((got - want).abs() / want.abs()).max().item()
    assert rel <= 1e-4, (got, want, rel)
    assert torch.count_nonzero(m(x.cuda(), x.cuda())) == 0
    assert torch.equal(m(y.cuda(), x.cuda()).view(-1).cpu().double(), got)
    with torch.no_grad():
        assert torch.equal(m(x.cuda(), y.cuda()).view(-1).cpu().double(), got)            # deterministic


# ---------------------------------------------------------------------------------------------------- the driver
def _write_inputs(tmp_path):
    from ldmae_amd import fid
    from ldmae_amd.models.lpips import CONVS, random_state_dict
    sd = random_state_dict(7)
    vgg = {}
    for i, s, _, _ in CONVS:
        vgg[f"features.{i}.weight"] = sd[f"net.slice{s}.{i}.weight"]
        vgg[f"features.{i}.bias"] = sd[f"net.slice{s}.{i}.bias"]
    torch.save(vgg, tmp_path / "vgg16-397923af.pth")
    torch.save({k: v for k, v in sd.items() if k.startswith("lin")}, tmp_path / "vgg.pth")
    torch.save(fid.random_state_dict(0), tmp_path / "inception.pth")
    feat = tmp_path / "feat"
    (tmp_path / "feat_sample").mkdir()
    torch.save({"mean": torch.zeros(1, 16, 1, 1), "std": torch.full((1, 16, 1, 1), 0.5)}, tmp_path / "feat_sample" / "latents_stats.pt")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(f"data:\n  data_path: '{feat}'\n  image_size: 256\n  sample: true\nvae:\n  model_name: 'vmae_f8d16'\n"
                   f"  weight_path: '{tmp_path / 'missing.pth'}'\n")
    return sd


def _run(tmp_path, out, eps, capsys):
    from ldmae_amd import evaluate_tokenizer as et
    argv = ["--config_path", str(tmp_path / "cfg.yaml"), "--output_path", str(out), "--epsilon", str(eps), "--synthetic", "32",
            "--batch_size", "8", "--num_workers", "0", "--lpips_vgg", str(tmp_path / "vgg16-397923af.pth"),
            "--lpips_lin", str(tmp_path / "vgg.pth"), "--fid_weights", str(tmp_path / "inception.pth")]
    res = et.main(argv)
    text = capsys.readouterr().out
    return res, text


def _load_pngs(folder, prefix, n):
    from PIL import Image
    return np.stack([np.asarray(Image.open(os.path.join(folder, f"{prefix}_rank_0_{i}.png"))) for i in range(n)])


def test_driver_end_to_end(tmp_path, capsys, monkeypatch):
    from ldmae_amd import evaluate_tokenizer as et
    from ldmae_amd.models.lpips import LPIPS
    from ldmae_amd.tokenizer import models_mae
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.setenv("LDMAE_FID_WEIGHTS", str(tmp_path / "inception.pth"))       # the driver sets it from --fid_weights; restored afterwards
    sd = _write_inputs(tmp_path)
    res0, text0 = _run(tmp_path, tmp_path / "o", 0.0, capsys)
    for name in ("rFID", "PSNR", "LPIPS", "SSIM"):
        assert f"[Tokenizer Evaluation]\x1b[0m {name}: " in text0, text0
    line = [ln for ln in text0.splitlines() if ln.startswith("{")][-1]
    js = json.loads(line)
    for k in ("rfid", "psnr", "lpips", "ssim"):
        assert np.isfinite(js[k]) and js[k] == res0[k]
    dec_dir, ref_dir = et.output_dirs(str(tmp_path / "o"), "vmae", 0.0)
    assert sorted(os.listdir(ref_dir)) == sorted(f"ref_image_rank_0_{i}.png" for i in range(32))
    assert sorted(os.listdir(dec_dir)) == sorted(f"decoded_image_rank_0_{i}.png" for i in range(32))

    # PSNR from the written PNGs, as the reference computes it (f64 here)
    dec = _load_pngs(dec_dir, "decoded_image", 32).astype(np.float64)
    ref = _load_pngs(ref_dir, "ref_image", 32).astype(np.float64)
    psnr = 20 * np.log10(255.0 / np.sqrt(((dec - ref) ** 2).reshape(32, -1).mean(1)))
    assert res0["psnr"] == pytest.approx(psnr.mean(), rel=1e-12)

    # SSIM / LPIPS from the tensors: the same random tokenizer, the same images, f64 restatements
    torch.manual_seed(42)
    model = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, kl_loss_weight=True, smooth_output=True, img_size=256).cuda().eval()
    imgs = torch.stack([et.SyntheticImages(32)[i][0] for i in range(32)])
    ssim_b, lpips_b, lp = [], [], LPIPS(state_dict=sd, device="cuda")
    with torch.no_grad():
        for b in range(4):
            x = imgs[8 * b:8 * b + 8].cuda()
            d = model.decode(model.encode(x).latent_dist.mode().float()).sample.float()
            q = torch.clamp(127.5 * d + 128.0, 0, 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
            diff = np.abs(q.astype(np.int64) - dec[8 * b:8 * b + 8].astype(np.int64))
            # a decode in this process matches the driver's PNGs up to truncation flips of values within rounding of an integer
            assert int(diff.max()) <= 1 and (diff > 0).mean() < 1e-3, (int(diff.max()), float((diff > 0).mean()))
            ssim_b.append(ref_ssim(d.cpu(), x.cpu()).mean())
            lpips_b.append(lp(d, x).mean().cpu())
    assert res0["ssim"] == pytest.approx(float(torch.stack(ssim_b).mean()), abs=2e-5)
    assert res0["lpips"] == pytest.approx(float(torch.stack(lpips_b).double().mean()), rel=1e-6)

    # epsilon > 0 changes the decoded images; the reference PNGs are reused; the same seed reproduces the run bitwise
    res1, _ = _run(tmp_path, tmp_path / "o", 0.1, capsys)
    dec1_dir = et.output_dirs(str(tmp_path / "o"), "vmae", 0.1)[0]
    dec1 = _load_pngs(dec1_dir, "decoded_image", 32)
    assert not np.array_equal(dec1, dec.astype(np.uint8))
    assert res1["psnr"] != res0["psnr"]
    res2, _ = _run(tmp_path, tmp_path / "o2", 0.1, capsys)
    dec2 = _load_pngs(et.output_dirs(str(tmp_path / "o2"), "vmae", 0.1)[0], "decoded_image", 32)
    assert np.array_equal(dec1, dec2)
    for k in ("psnr", "lpips", "ssim", "rfid"):
        assert res2[k] == res1[k], k
