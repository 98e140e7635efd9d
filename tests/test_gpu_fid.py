"""FID evaluation on the MI355X: the HIP Inception-v3 kernels (implicit-GEMM convolution, pools, pre-processing, f64 statistics) and the
reference's calculate_fid interface, against a plain torch.nn.functional CPU implementation of pytorch-fid's network written out here."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    a, b = torch.as_tensor(a).double().flatten().cpu(), torch.as_tensor(b).double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------------ CPU yardstick (f32, NCHW)
def cpu_features(sd, imgs, dims):
    """pytorch-fid's InceptionV3([block]) forward on the CPU: ToTensor -> bilinear 299 -> 2x - 1 -> fid_inception_v3 blocks -> global average."""
    def bc(name, x, stride=1, padding=0):
        y = F.conv2d(x, sd[f"{name}.conv.weight"].float(), stride=stride, padding=padding)
        y = F.batch_norm(y, sd[f"{name}.bn.running_mean"].float(), sd[f"{name}.bn.running_var"].float(), sd[f"{name}.bn.weight"].float(),
                         sd[f"{name}.bn.bias"].float(), False, 0.0, 1e-3)
        return F.relu(y)

    def avg(x):
        return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)

    def block_a(p, x):
        b1 = bc(f"{p}.branch1x1", x)
        b5 = bc(f"{p}.branch5x5_2", bc(f"{p}.branch5x5_1", x), padding=2)
        b3 = bc(f"{p}.branch3x3dbl_3", bc(f"{p}.branch3x3dbl_2", bc(f"{p}.branch3x3dbl_1", x), padding=1), padding=1)
        return torch.cat([b1, b5, b3, bc(f"{p}.branch_pool", avg(x))], 1)

    def block_c(p, x):
        b1 = bc(f"{p}.branch1x1", x)
        b7 = bc(f"{p}.branch7x7_3", bc(f"{p}.branch7x7_2", bc(f"{p}.branch7x7_1", x), padding=(0, 3)), padding=(3, 0))
        d = bc(f"{p}.branch7x7dbl_1", x)
        d = bc(f"{p}.branch7x7dbl_2", d, padding=(3, 0))
        d = bc(f"{p}.branch7x7dbl_3", d, padding=(0, 3))
        d = bc(f"{p}.branch7x7dbl_4", d, padding=(3, 0))
        d = bc(f"{p}.branch7x7dbl_5", d, padding=(0, 3))
        return torch.cat([b1, b7, d, bc(f"{p}.branch_pool", avg(x))], 1)

    def block_e(p, x, pool):
        b1 = bc(f"{p}.branch1x1", x)
        t = bc(f"{p}.branch3x3_1", x)
        b3 = torch.cat([bc(f"{p}.branch3x3_2a", t, padding=(0, 1)), bc(f"{p}.branch3x3_2b", t, padding=(1, 0))], 1)
        d = bc(f"{p}.branch3x3dbl_2", bc(f"{p}.branch3x3dbl_1", x), padding=1)
        bd = torch.cat([bc(f"{p}.branch3x3dbl_3a", d, padding=(0, 1)), bc(f"{p}.branch3x3dbl_3b", d, padding=(1, 0))], 1)
        return torch.cat([b1, b3, bd, bc(f"{p}.branch_pool", pool(x))], 1)

    def out(x):
        return x.mean((2, 3))

    x = torch.from_numpy(np.ascontiguousarray(imgs)).permute(0, 3, 1, 2).float() / 255
    x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False) * 2 - 1
    x = bc("Conv2d_2b_3x3", bc("Conv2d_2a_3x3", bc("Conv2d_1a_3x3", x, stride=2)), padding=1)
    x = F.max_pool2d(x, 3, 2)
    if dims == 64:
        return out(x)
    x = F.max_pool2d(bc("Conv2d_4a_3x3", bc("Conv2d_3b_1x1", x)), 3, 2)
    if dims == 192:
        return out(x)
    for p in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = block_a(p, x)
    b3 = bc("Mixed_6a.branch3x3", x, stride=2)
    d = bc("Mixed_6a.branch3x3dbl_3", bc("Mixed_6a.branch3x3dbl_2", bc("Mixed_6a.branch3x3dbl_1", x), padding=1), stride=2)
    x = torch.cat([b3, d, F.max_pool2d(x, 3, 2)], 1)
    for p in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        x = block_c(p, x)
    if dims == 768:
        return out(x)
    b3 = bc("Mixed_7a.branch3x3_2", bc("Mixed_7a.branch3x3_1", x), stride=2)
    d = bc("Mixed_7a.branch7x7x3_1", x)
    d = bc("Mixed_7a.branch7x7x3_2", d, padding=(0, 3))
    d = bc("Mixed_7a.branch7x7x3_3", d, padding=(3, 0))
    d = bc("Mixed_7a.branch7x7x3_4", d, stride=2)
    x = torch.cat([b3, d, F.max_pool2d(x, 3, 2)], 1)
    x = block_e("Mixed_7b", x, avg)
    x = block_e("Mixed_7c", x, lambda t: F.max_pool2d(t, 3, 1, 1))
    return out(x)


@pytest.fixture(scope="module")
def sd():
    from ldmae_amd import fid
    return fid.random_state_dict(7)


def _images(n, h, w, seed):
    """Smooth random RGB images (a few low-frequency waves plus noise), uint8 [n, h, w, 3]."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w] / max(h, w)
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        f = rng.uniform(1, 6, (3, 2))
        ph = rng.uniform(0, 6.3, 3)
        img = np.stack([np.sin(f[c, 0] * 6.3 * yy + f[c, 1] * 6.3 * xx + ph[c]) for c in range(3)], -1)
        out[i] = np.clip(127.5 + 100 * img + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)
    return out


# ------------------------------------------------------------------------------------------------ kernels
def test_conv_every_geometry_against_f64():
    from ldmae_amd import fid, ops
    g = torch.Generator().manual_seed(0)
    geos = sorted(set(fid.conv_geometries().values()))
    assert len(geos) == 43
    for (h, w, cin, cout, kh, kw, s, ph, pw, ho, wo) in geos:
        B = 2
        x = torch.randn(B, h, w, cin, generator=g)
        wt = torch.randn(cout, kh, kw, cin, generator=g) * (1.0 / (kh * kw * cin)) ** 0.5
        b = torch.randn(cout, generator=g) * 0.1
        ref = F.conv2d(x.double().permute(0, 3, 1, 2), wt.double().permute(0, 3, 1, 2), b.double(), stride=s, padding=(ph, pw)).permute(0, 2, 3, 1)
        got = ops.conv2d_nhwc(x.cuda(), wt.cuda(), b.cuda(), (s, s), (ph, pw), relu=False)
        assert got.shape == (B, ho, wo, cout)
        e = rel(got, ref)
        assert e <= 1e-5, ((h, w, cin, cout, kh, kw, s, ph, pw), e)
        if cout == 192 and kh * kw > 1:                # ReLU epilogue on a few
            assert rel(ops.conv2d_nhwc(x.cuda(), wt.cuda(), b.cuda(), (s, s), (ph, pw), relu=True), ref.clamp_min(0)) <= 1e-5


@pytest.mark.parametrize("cin,xoff,ldx,k,pad", [(48, 16, 112, 5, 2), (3, 1, 5, 3, 0), (160, 160, 320, 7, 3)])
def test_conv_channel_slices(cin, xoff, ldx, k, pad):
    """Input read from channels [xoff, xoff + cin) of a wider tensor, output written to a slice of a wider one; the rest untouched."""
    from ldmae_amd import ops
    g = torch.Generator().manual_seed(cin)
    B, H, W, cout, ldo, ooff = 3, 17, 13, 72, 200, 100
    x = torch.randn(B, H, W, ldx, generator=g)
    wt = torch.randn(cout, k, k, cin, generator=g) * (1.0 / (k * k * cin)) ** 0.5
    b = torch.randn(cout, generator=g)
    out = torch.full((B, H + 2 * pad - k + 1, W + 2 * pad - k + 1, ldo), 7.0).cuda()
    ops.conv2d_nhwc(x.cuda(), wt.cuda(), b.cuda(), (1, 1), (pad, pad), relu=True, xoff=xoff, cin=cin, out=out, ooff=ooff)
    ref = F.relu(F.conv2d(x[..., xoff:xoff + cin].double().permute(0, 3, 1, 2), wt.double().permute(0, 3, 1, 2), b.double(), padding=pad)).permute(0, 2, 3, 1)
    o = out.cpu()
    assert rel(o[..., ooff:ooff + cout], ref) <= 1e-5
    assert bool((o[..., :ooff] == 7.0).all()) and bool((o[..., ooff + cout:] == 7.0).all())


def test_pools_and_global_average():
    from ldmae_amd import ops
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 35, 35, 100, generator=g)
    xn = x[..., 20:84].permute(0, 3, 1, 2)                  # channel slice [20, 84)
    cases = [("max", 3, 2, 0, F.max_pool2d(xn, 3, 2)), ("avg", 3, 1, 1, F.avg_pool2d(xn, 3, 1, 1, count_include_pad=False)),
             ("max", 3, 1, 1, F.max_pool2d(xn, 3, 1, 1))]
    for mode, k, s, p, ref in cases:
        ho = ref.shape[2]
        out = torch.full((2, ho, ho, 90), -5.0).cuda()
        ops.pool2d_nhwc(x.cuda(), mode, k, s, p, xoff=20, c=64, out=out, ooff=10)
        o = out.cpu()
        assert rel(o[..., 10:74], ref.permute(0, 2, 3, 1)) <= 1e-6, (mode, s, p)
        assert bool((o[..., :10] == -5.0).all()) and bool((o[..., 74:] == -5.0).all())
    ga = ops.global_avgpool_nhwc(x.cuda(), xoff=20, c=64)
    assert rel(ga, xn.double().mean((2, 3))) <= 1e-6


@pytest.mark.parametrize("size", [256, 64, 300])
def test_preprocess_matches_interpolate(size):
    from ldmae_amd import ops
    imgs = _images(3, size, size + 7, size)
    ref = F.interpolate(torch.from_numpy(imgs).permute(0, 3, 1, 2).float() / 255, (299, 299), mode="bilinear", align_corners=False) * 2 - 1
    got = ops.fid_preprocess(torch.from_numpy(imgs).cuda()).cpu()
    assert float((got - ref.permute(0, 2, 3, 1)).abs().max()) <= 1e-6


@pytest.mark.parametrize("D", [200, 2048])
def test_device_statistics_match_numpy(D):
    from ldmae_amd import fid
    rng = np.random.default_rng(D)
    A = rng.standard_normal((D, D)) * 0.3 / np.sqrt(D)
    feats = [(rng.standard_normal((n, D)) @ A + 5.0).astype(np.float32) for n in (50, 37, 13)]
    feats = [np.abs(f) for f in feats]                   # ReLU-like, mean far from zero: the shift matters
    st = fid.FeatureStats(D)
    for f in feats:
        st.update(torch.from_numpy(f).cuda())
    mu, sigma = st.finalize()
    allf = np.concatenate(feats).astype(np.float64)
    assert rel(mu, allf.mean(0)) <= 1e-10
    assert rel(sigma, np.cov(allf, rowvar=False)) <= 1e-10
    assert np.array_equal(sigma, sigma.T)


# ------------------------------------------------------------------------------------------------ the network
def test_features_every_dims_against_cpu(sd, monkeypatch):
    from ldmae_amd import fid
    imgs = _images(8, 96, 80, 3)
    models = {dims: fid.InceptionFID(dims=dims, state_dict=sd) for dims in (64, 192, 768, 2048)}

    def boom(*a, **k):
        raise AssertionError("torch conv / pool / interpolate called on the FID path")
    got = {}
    with monkeypatch.context() as m:
        for n in ("conv2d", "max_pool2d", "avg_pool2d", "interpolate", "adaptive_avg_pool2d"):
            m.setattr(F, n, boom)
        for dims, model in models.items():
            got[dims] = model.features(torch.from_numpy(imgs)).cpu()
    for dims in (64, 192, 768, 2048):
        ref = cpu_features(sd, imgs, dims)
        f = got[dims]
        assert f.shape == (8, dims) and f.dtype == torch.float32
        assert rel(f, ref) <= 1e-4, (dims, rel(f, ref))
        assert float(f.std()) > 0 and float((f == 0).float().mean()) < 0.9, dims


def test_unfused_block_inputs_give_the_same_features(sd):
    """The shared-input 1x1 convs of a Mixed block as one GEMM (default) or as two: the same features up to f32 rounding."""
    from ldmae_amd import fid
    imgs = torch.from_numpy(_images(4, 64, 64, 9))
    a = fid.InceptionFID(dims=2048, state_dict=sd).features(imgs)
    b = fid.InceptionFID(dims=2048, state_dict=sd, fuse_1x1=False).features(imgs)
    assert rel(a, b) <= 1e-6


def _write_pngs(folder, imgs):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(os.path.join(folder, f"{i:06d}.png"))


def test_fid_of_two_folders_end_to_end(sd, tmp_path, monkeypatch):
    from ldmae_amd import fid
    wpath = tmp_path / "inception.pth"
    torch.save(sd, wpath)
    monkeypatch.setenv(fid.WEIGHTS_ENV, str(wpath))
    a, b = _images(300, 48, 48, 11), _images(300, 48, 48, 12)
    _write_pngs(tmp_path / "a", a)
    _write_pngs(tmp_path / "b", b)
    got = fid.calculate_fid_given_paths([str(tmp_path / "a"), str(tmp_path / "b")], 50, "cuda", 192)
    fa = torch.cat([cpu_features(sd, a[i:i + 100], 192) for i in range(0, 300, 100)]).double().numpy()
    fb = torch.cat([cpu_features(sd, b[i:i + 100], 192) for i in range(0, 300, 100)]).double().numpy()
    want = fid.calculate_frechet_distance(fa.mean(0), np.cov(fa, rowvar=False), fb.mean(0), np.cov(fb, rowvar=False))
    assert want > 0 and abs(got - want) <= 1e-4 * want, (got, want)
    # --save-stats writes mu / sigma; the distance from the saved file is the same
    fid.main([str(tmp_path / "a"), str(tmp_path / "a.npz"), "--save-stats", "--dims", "192"])
    with np.load(tmp_path / "a.npz") as f:
        assert f["mu"].shape == (192,) and f["sigma"].shape == (192, 192)
    again = fid.calculate_fid_given_paths([str(tmp_path / "a.npz"), str(tmp_path / "b")], 50, "cuda", 192)
    assert abs(again - got) <= 1e-9 * got


def test_inference_main_prints_fid(sd, tmp_path, monkeypatch, capsys):
    """The sampling driver's tail (reference inference.py:352-367): with the weights and the reference statistics present, main() prints
    `fid=` and the value of a direct calculate_fid_given_paths call on the folder it returns."""
    import copy

    import yaml
    import ldmae_amd.inference as inf
    import ldmae_amd.train_accum as t
    from ldmae_amd import fid
    from ldmae_amd.models import lightningdit as L
    from ldmae_amd.tokenizer import models_mae
    monkeypatch.setitem(L.LightningDiT_models, "LightningDiT-B/1", lambda **kw: L.LightningDiT(depth=2, hidden_size=192, patch_size=1, num_heads=3, **kw))
    cfg = copy.deepcopy(yaml.safe_load(open(os.path.join(ROOT, "ldmae_amd/configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml"))))
    cfg["data"].update(image_size=64, num_workers=0, data_path=str(tmp_path / "feat"), latent_multiplier=1.0)
    cfg["train"].update(global_batch_size=8, output_dir=str(tmp_path), exp_name="t", log_every=2, ckpt_every=3, max_steps=3)
    cfg["vae"]["weight_path"] = str(tmp_path / "vmae.pth")
    cfg["sample"].update(num_sampling_steps=2, per_proc_batch_size=4, fid_num=8, cfg_scale=4.0)
    torch.manual_seed(0)
    dit = t.build_model(cfg)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, p in dit.named_parameters():
            if "adaLN_modulation" in n or n.startswith("final_layer.linear"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    cfg["ckpt_path"] = str(tmp_path / "0000007.pt")
    torch.save({"ema": dit.state_dict(), "model": dit.state_dict()}, cfg["ckpt_path"])
    vae = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, kl_loss_weight=True, smooth_output=True, img_size=64)
    torch.save({"model": vae.state_dict()}, cfg["vae"]["weight_path"])
    os.makedirs(str(tmp_path / "feat_sample"))
    torch.save({"mean": torch.randn(1, 16, 1, 1, generator=g) * 0.1, "std": torch.rand(1, 16, 1, 1, generator=g) + 0.5},
               tmp_path / "feat_sample" / "latents_stats.pt")
    # reference statistics relative to the working directory, as the YAML's tools/fid_statistics/... path is
    monkeypatch.chdir(tmp_path)
    os.makedirs("stats")
    rng = np.random.default_rng(0)
    r = rng.standard_normal((4096, 2048)) * 0.05
    np.savez("stats/ref.npz", mu=r.mean(0) + 0.3, sigma=np.cov(r, rowvar=False))
    cfg["data"]["fid_reference_file"] = "stats/ref.npz"
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    wpath = tmp_path / "inception.pth"
    torch.save(sd, wpath)
    monkeypatch.setenv(fid.WEIGHTS_ENV, str(wpath))
    folder = inf.main(["--config", str(tmp_path / "cfg.yaml")])
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if ln.startswith("fid=")]
    assert len(line) == 1, out
    printed = float(line[0].split()[1])
    direct = fid.calculate_fid_given_paths(["stats/ref.npz", folder], 50, "cuda", 2048, sp_len=8)
    assert np.isfinite(direct) and printed == pytest.approx(direct, rel=1e-12, abs=0)
    # without the weights: today's line plus the reason, no FID
    monkeypatch.delenv(fid.WEIGHTS_ENV)
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "no_hub"))
    assert inf.main(["--config", str(tmp_path / "cfg.yaml")]) == folder
    out = capsys.readouterr().out
    assert "is not part of this package" in out and "FID skipped" in out and fid.WEIGHTS_NAME in out and "fid=" not in out
