"""Tokenizer evaluation without a GPU: the LPIPS weight loaders (torchvision VGG16 and taming's lin heads: key mapping, the Cin-4 padding of
conv1_1, strict key / shape checks, the missing-weights error), the driver's Resize / CenterCrop rule, its output layout, its aggregation
arithmetic, its refusals and its command line."""
import os

import pytest
import torch
import torch.nn.functional as F

from ldmae_amd import evaluate_tokenizer as et
from ldmae_amd.models import lpips as lp

# torchvision's vgg16().features: the conv indices and their (Cin, Cout), written out independently of the module under test
VGG_CONVS = {0: (3, 64), 2: (64, 64), 5: (64, 128), 7: (128, 128), 10: (128, 256), 12: (256, 256), 14: (256, 256), 17: (256, 512),
             19: (512, 512), 21: (512, 512), 24: (512, 512), 26: (512, 512), 28: (512, 512)}
SLICE_OF = {i: (1 if i < 4 else 2 if i < 9 else 3 if i < 16 else 4 if i < 23 else 5) for i in VGG_CONVS}      # the reference's slice ranges


def _fake_vgg(seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, (cin, cout) in VGG_CONVS.items():
        sd[f"features.{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=g)
        sd[f"features.{i}.bias"] = torch.randn(cout, generator=g)
    sd["classifier.6.bias"] = torch.zeros(10)          # a trimmed classifier: accepted and dropped
    return sd


def _fake_lin(seed=1):
    g = torch.Generator().manual_seed(seed)
    sd = {f"lin{k}.model.1.weight": torch.rand(1, c, 1, 1, generator=g) for k, c in enumerate((64, 128, 256, 512, 512))}
    sd["scaling_layer.shift"] = torch.tensor([-0.030, -0.088, -0.188]).view(1, 3, 1, 1)
    return sd


def test_loaders_map_keys_and_pad_conv1(tmp_path):
    vgg, lin = _fake_vgg(), _fake_lin()
    torch.save(vgg, tmp_path / "vgg16-397923af.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    sd = lp.load_state_dict_from_files(str(tmp_path / "vgg16-397923af.pth"), str(tmp_path / "vgg.pth"))
    want = {f"net.slice{SLICE_OF[i]}.{i}.{p}" for i in VGG_CONVS for p in ("weight", "bias")}
    want |= {f"lin{k}.model.1.weight" for k in range(5)}
    assert set(sd) == want
    for i in VGG_CONVS:
        assert torch.equal(sd[f"net.slice{SLICE_OF[i]}.{i}.weight"], vgg[f"features.{i}.weight"])
        assert torch.equal(sd[f"net.slice{SLICE_OF[i]}.{i}.bias"], vgg[f"features.{i}.bias"])
    for k in range(5):
        assert torch.equal(sd[f"lin{k}.model.1.weight"], lin[f"lin{k}.model.1.weight"])
    convs = lp.conv_weights(sd)
    assert len(convs) == 13
    w0, b0, s0 = convs[0]
    assert tuple(w0.shape) == (64, 3, 3, 4) and s0 == 1
    assert torch.equal(w0[..., :3], vgg["features.0.weight"].permute(0, 2, 3, 1))
    assert torch.count_nonzero(w0[..., 3]) == 0
    w1 = convs[1][0]
    assert tuple(w1.shape) == (64, 3, 3, 64) and torch.equal(w1, vgg["features.2.weight"].permute(0, 2, 3, 1))
    assert [s for _, _, s in convs] == [SLICE_OF[i] for i in sorted(VGG_CONVS)]


def test_loaders_are_strict():
    vgg = _fake_vgg()
    del vgg["features.12.bias"]
    with pytest.raises(KeyError, match="features.12.bias"):
        lp.vgg_to_lpips(vgg)
    vgg = _fake_vgg()
    vgg["features.19.weight"] = torch.zeros(512, 256, 3, 3)
    with pytest.raises(ValueError, match="features.19.weight"):
        lp.vgg_to_lpips(vgg)
    vgg = _fake_vgg()
    vgg["features.30.weight"] = torch.zeros(1)
    with pytest.raises(KeyError, match="features.30.weight"):
        lp.vgg_to_lpips(vgg)
    lin = _fake_lin()
    del lin["lin3.model.1.weight"]
    with pytest.raises(KeyError, match="lin3.model.1.weight"):
        lp.load_lin(lin)
    lin = _fake_lin()
    lin["lin0.model.1.weight"] = torch.zeros(1, 128, 1, 1)
    with pytest.raises(ValueError, match="lin0.model.1.weight"):
        lp.load_lin(lin)
    sd = lp.random_state_dict(0)
    lp.check_state_dict(sd)
    sd["net.slice5.28.bias"] = torch.zeros(3)
    with pytest.raises(ValueError, match="net.slice5.28.bias"):
        lp.check_state_dict(sd)


def test_missing_weights_error_names_both_files_and_every_place(tmp_path, monkeypatch):
    monkeypatch.delenv(lp.VGG_ENV, raising=False)
    monkeypatch.delenv(lp.LIN_ENV, raising=False)
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError) as e:
        lp.resolve_weights()
    msg = str(e.value)
    for s in ("vgg16-397923af.pth", "vgg.pth", "$LDMAE_LPIPS_VGG", "$LDMAE_LPIPS_LIN", str(tmp_path / "hub" / "checkpoints"),
              os.path.join("movqgan", "modules", "losses", "lpips", "vgg.pth"), "never downloads"):
        assert s in msg, s
    # one file present: the error still names the other, and says which was found
    torch.save(_fake_lin(), tmp_path / "vgg.pth")
    monkeypatch.setenv(lp.LIN_ENV, str(tmp_path / "vgg.pth"))
    with pytest.raises(FileNotFoundError, match="vgg16-397923af.pth NOT found"):
        lp.resolve_weights()
    torch.save(_fake_vgg(), tmp_path / "hub_vgg.pth")
    assert lp.resolve_weights(vgg_weights=str(tmp_path / "hub_vgg.pth")) == (str(tmp_path / "hub_vgg.pth"), str(tmp_path / "vgg.pth"))


def test_flops_per_image():
    # 20.04 GMAC per 256^2 image: about 80 GFLOP per LPIPS pair
    assert lp.conv_flops_per_image(256, 256) == 2 * sum(
        (256 >> (SLICE_OF[i] - 1)) ** 2 * cout * 9 * cin for i, (cin, cout) in VGG_CONVS.items())
    assert abs(2 * lp.conv_flops_per_image(256, 256) / 1e9 - 80.18) < 0.01


@pytest.mark.parametrize("hw,resized,crop", [((375, 500), (256, 341), (0, 42)), ((500, 333), (384, 256), (64, 0)),
                                             ((256, 256), (256, 256), (0, 0)), ((257, 999), (256, 995), (0, 370)),
                                             ((1001, 300), (854, 256), (299, 0))])
def test_resize_and_center_crop_rule(hw, resized, crop):
    assert et.resized_size(*hw) == resized
    assert et.crop_offsets(*resized) == crop
    g = torch.Generator().manual_seed(0)
    x = torch.rand(3, *hw, generator=g)
    y = et.EvalTransform().tensor(x)
    assert tuple(y.shape) == (3, 256, 256)
    r = x[None] if resized == hw else F.interpolate(x[None], size=resized, mode="bilinear", align_corners=False, antialias=True)
    want = (r[0, :, crop[0]:crop[0] + 256, crop[1]:crop[1] + 256] - 0.5) / 0.5
    assert torch.equal(y, want)


def test_output_layout():
    dec, ref = et.output_dirs("/o", "vmae", 0.05)
    assert dec == os.path.join("/o", "vmae_0.05", "decoded_images") and ref == os.path.join("/o", "ref_images")
    assert et.output_dirs("/o", "vmae", 0)[0] == os.path.join("/o", "vmae_0", "decoded_images")          # the reference's int default
    assert et.output_dirs("/o", "vmae", 0.0)[0] == os.path.join("/o", "vmae_0.0", "decoded_images")
    assert et.ref_name(3, 17) == "ref_image_rank_3_17.png"
    assert et.decoded_name(0, 120) == "decoded_image_rank_0_120.png"
    cfg = {"data": {"data_path": "/d/feat", "sample": True}}
    assert et.latent_stats_path(cfg) == os.path.join("/d/feat_sample", "latents_stats.pt")
    cfg = {"data": {"data_path": "/d/feat"}}
    assert et.latent_stats_path(cfg) == os.path.join("/d/feat", "latents_stats.pt")


def test_aggregation_arithmetic():
    lpv, ssv = torch.tensor([0.1, 0.3, 0.2]), torch.tensor([0.5, 0.7, 0.9])
    psnr = torch.tensor([20.0, 30.0, 31.0, 41.0], dtype=torch.float64)
    r = et.aggregate(lpv, ssv, psnr.sum(), psnr.numel())
    assert r["lpips"] == pytest.approx(0.2, abs=1e-7)
    assert r["ssim"] == pytest.approx(0.7, abs=1e-7)
    assert r["psnr"] == pytest.approx(30.5, abs=1e-12)
    # an equal pair makes the mean PSNR infinite, as in the reference
    assert et.aggregate(lpv, ssv, float("inf"), 4)["psnr"] == float("inf")


def test_refuses_sdvae_model_types(tmp_path):
    for mt in ("ae", "dae", "vae", "sdv3"):
        with pytest.raises(NotImplementedError, match="SD-VAE"):
            et.model_type_of({"vae": {"model_name": f"{mt}_f8d16"}})
    assert et.model_type_of({"vae": {"model_name": "vmae_f8d16"}}) == "vmae"
    cfg = tmp_path / "c.yaml"
    cfg.write_text("vae:\n  model_name: sdv3_f8c16\ndata:\n  data_path: x\n")
    with pytest.raises(NotImplementedError, match="sdv3"):
        et.main(["--config_path", str(cfg)])


def test_lpips_refuses_inputs_that_require_grad():
    m = lp.LPIPS.__new__(lp.LPIPS)                      # no device needed: the check comes first
    x = torch.zeros(1, 3, 16, 16, requires_grad=True)
    with pytest.raises(RuntimeError, match="forward-only"):
        m(x, torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="HIP device"):
        lp.LPIPS(state_dict=lp.random_state_dict(0), device="cpu")


def test_cli_accepts_every_reference_flag():
    a = et.build_parser().parse_args(["--config_path", "c.yaml", "--model_type", "vavae", "--data_path", "/d", "--output_path", "/o",
                                      "--seed", "7", "--epsilon", "0.1"])
    assert (a.config_path, a.model_type, a.data_path, a.output_path, a.seed, a.epsilon) == ("c.yaml", "vavae", "/d", "/o", 7, 0.1)
    assert a.batch_size == 8 and a.precision == "fp32" and a.synthetic == 0
    d = et.build_parser().parse_args([])
    assert d.epsilon == 0 and d.seed == 42 and d.output_path == "./rfid"
    a = et.build_parser().parse_args(["--batch_size", "16", "--lpips_vgg", "v", "--lpips_lin", "l", "--fid_weights", "f", "--precision", "bf16",
                                      "--synthetic", "32"])
    assert (a.batch_size, a.lpips_vgg, a.lpips_lin, a.fid_weights, a.precision, a.synthetic) == (16, "v", "l", "f", "bf16", 32)
    # the run_*.sh launchers pass --config: argparse takes it for --config_path
    assert et.build_parser().parse_args(["--config", "c.yaml"]).config_path == "c.yaml"


def test_robustness_script_sweeps_the_reference_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "ldmae_amd", "run_robustness_test.sh")).read()
    assert "evaluate_tokenizer.py" in text
    assert 'for eps in "" 0.01 0.05 0.1 0.2 0.3' in text
