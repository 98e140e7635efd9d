"""Stage 3 of train_ae.sh (decoder tuning with the LPIPS loss), the parts that need no GPU: the rotated-weight builder of the conv data gradient,
the driver's command line, the launcher script, and the default of the LPIPS class."""
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rotated_weight_is_the_transposed_convolution():
    """dx = conv3x3(dy, rotate_weight(w)) with padding 1 is conv_transpose2d(dy, w, padding=1): the data gradient of a stride-1 / pad-1 conv."""
    from ldmae_amd.models.lpips import rotate_weight
    g = torch.Generator().manual_seed(0)
    cout, cin = 5, 3
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)           # torch layout [Cout, Cin, ky, kx]
    dy = torch.randn(2, cout, 6, 7, generator=g, dtype=torch.float64)
    want = F.conv_transpose2d(dy, w, padding=1)
    w_rot = rotate_weight(w.permute(0, 2, 3, 1).contiguous())                    # channels-last in, [Cin, 3, 3, Cout] out
    assert tuple(w_rot.shape) == (cin, 3, 3, cout) and w_rot.is_contiguous()
    for ci in range(cin):
        for ky in range(3):
            for kx in range(3):
                assert torch.equal(w_rot[ci, ky, kx], w[:, ci, 2 - ky, 2 - kx])
    got = F.conv2d(dy, w_rot.permute(0, 3, 1, 2), padding=1)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    # and it is the autograd gradient
    x = torch.randn(2, cin, 6, 7, generator=g, dtype=torch.float64, requires_grad=True)
    (gx,) = torch.autograd.grad(F.conv2d(x, w, padding=1), x, dy)
    assert torch.allclose(got, gx, rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError):
        rotate_weight(torch.zeros(4, 3, 3))


def test_rotated_weight_of_the_padded_stem_conv_has_a_zero_row():
    from ldmae_amd.models.lpips import conv_weights, random_state_dict, rotate_weight
    w = conv_weights(random_state_dict(1))[0][0]                                 # conv1_1: [64, 3, 3, 4], channel 3 zero
    w_rot = rotate_weight(w)
    assert tuple(w_rot.shape) == (4, 3, 3, 64) and torch.count_nonzero(w_rot[3]) == 0 and torch.count_nonzero(w_rot[:3]) > 0


def test_lpips_is_forward_only_by_default():
    from ldmae_amd.models import lpips as lp
    assert lp.LPIPS.differentiable is False
    assert lp.LPIPS.__new__(lp.LPIPS).differentiable is False


def test_stage3_flags_parse_together_and_a_missing_weight_file_exits_2(tmp_path, capsys, monkeypatch):
    """`--tune_decoder --perceptual_loss_ratio R` is accepted as a pair; the LPIPS weight files are looked for BEFORE anything touches the GPU, and a
    missing one is exit code 2 that names the file (nothing is downloaded)."""
    from ldmae_amd import vmae_pretrain as vp
    monkeypatch.delenv("LDMAE_LPIPS_VGG", raising=False)
    monkeypatch.delenv("LDMAE_LPIPS_LIN", raising=False)
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "hub"))
    monkeypatch.chdir(tmp_path)
    lin = tmp_path / "vgg.pth"
    torch.save({}, lin)
    with pytest.raises(SystemExit) as e:
        vp.main(["--synthetic", "--tune_decoder", "--perceptual_loss_ratio", "10.0", "--mask_ratio", "0.0", "--lpips_vgg", str(tmp_path / "absent.pth"),
                 "--lpips_lin", str(lin)])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "vgg16-397923af.pth NOT found" in err and "absent.pth" in err and "unrecognized" not in err
    for alone in (["--tune_decoder"], ["--perceptual_loss_ratio", "10.0"]):
        with pytest.raises(SystemExit) as e:
            vp.main(["--synthetic"] + alone)
        assert e.value.code == 2


def test_perceptual_loss_belongs_to_ldmae_mode():
    from ldmae_amd.tokenizer import models_mae
    with pytest.raises(NotImplementedError):
        models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=False, img_size=32, perceptual_loss=object())
    marker = object()
    m = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, img_size=32, smooth_output=True, kl_loss_weight=0.0, perceptual_loss=marker,
                                            perceptual_loss_ratio=10.0)
    assert m.perceptual_loss is marker and m.perceptual_loss_ratio == 10.0
    assert not any("perceptual" in k or "mask_token" in k for k in m.state_dict())


def test_train_ae_runs_stage3(tmp_path):
    """train_ae.sh under a stand-in `python` that prints its arguments: a third command, after a line containing `Stage 3`, with the reference's
    stage-3 flags (VMAE/train_ae.sh:84-106) on torch.distributed.run."""
    shim = tmp_path / "bin"
    shim.mkdir()
    (shim / "python").write_text('#!/bin/bash\necho "ARGS $@"\n')
    os.chmod(shim / "python", 0o755)
    out_dir = tmp_path / "w"
    r = subprocess.run(["bash", os.path.join(ROOT, "ldmae_amd", "train_ae.sh")], capture_output=True, text=True,
                       env={"PATH": f"{shim}:/usr/bin:/bin", "GPUS_PER_NODE": "2", "DATA_PATH": "/d/imagenet", "OUT": str(out_dir), "OUT3": str(tmp_path / "w3"),
                            "LPIPS_VGG": "/w/vgg16.pth", "LPIPS_LIN": "/w/lin.pth"})
    assert r.returncode == 0, r.stderr
    cmds = [l for l in r.stdout.splitlines() if l.startswith("ARGS ")]
    assert len(cmds) == 3
    assert "Stage 1: VMAE pre-training (128 x 128, mask ratio 0.25)" in r.stdout
    before, after = r.stdout.split("Stage 3", 1)
    assert cmds[0] in before and cmds[1] in before and cmds[2] in after and "perceptual" not in before
    c = cmds[2]
    assert "-m torch.distributed.run --nproc-per-node 2" in c and " vmae_pretrain.py " in c
    for flags in ("--tune_decoder --perceptual_loss_ratio 10.0", "--batch_size 16 --accum_iter 16", "--input_size 256 --mask_ratio 0.0", "--epochs 10 --save_epochs 1",
                  "--warmup_epochs 0 --blr 1.0e-5", "--kl_loss_weight 0.0", "--data_path /d/imagenet", f"--output_dir {tmp_path / 'w3'}",
                  f"--resume {out_dir}/checkpoint-90.pth", "--lpips_vgg /w/vgg16.pth", "--lpips_lin /w/lin.pth"):
        assert flags in c, flags
