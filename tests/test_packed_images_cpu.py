"""Packed image shards and the device-side training transform, host side: the f64 restatement of ldmae_crop_resize_flip_u8 against PIL, the
checker's bound against an f32 emulation and three wrong variants of it, the packer's round trip, the crop tables against
RandomResizedCropFlip._box, the refusals of the packer and of the driver flags, and the C ABI."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import augment_check as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_folder(root, imagenet=False, n=12, seed=0):
    """A dozen generated PNGs of mixed sizes (short sides from 40 to 150) -> their (h, w) by file name."""
    from PIL import Image
    sizes = [(40, 56), (150, 200), (96, 96), (97, 130), (200, 120), (64, 333), (128, 100), (95, 95), (180, 181), (50, 40), (111, 240), (100, 75)][:n]
    out = {}
    for i, (h, w) in enumerate(sizes):
        d = os.path.join(root, "train", f"c{i % 3}") if imagenet else os.path.join(root, f"d{i % 2}")
        os.makedirs(d, exist_ok=True)
        name = os.path.join(d, f"img_{i:02d}.png")
        Image.fromarray(ac.make_image(w, h, "smooth" if i % 2 else "noise", seed + i)).save(name)
        out[name] = (h, w)
    return out


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("geom", ac.GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_restatement_is_pil_without_the_8_bit_rounding(geom, kind):
    h, w, top, left, ch, cw, S = geom
    img = ac.make_image(w, h, kind, seed=1)
    for flip in (0, 1):
        got = ac.restate(img, top, left, ch, cw, S, flip, mean=0.0, std=1.0)
        want = ac.pil_reference(img, top, left, ch, cw, S, flip)
        worst, bound = float(np.abs(got - want).max()), ac.pil_bound(ch, S)
        print(f"{geom} {kind} flip {flip}: worst {worst:.3e} bound {bound:.3e} ratio {worst / bound:.3f}")
        assert worst <= bound


def test_checker_passes_the_f32_contract_and_fails_three_wrong_variants():
    ratios = {"contract": 0.0, "image_clip": 0.0, "no_antialias": 0.0, "corner_centres": 0.0}
    for h, w, top, left, ch, cw, S in ac.GEOMS:
        img = ac.make_image(w, h, "noise", seed=2)
        ref, bound = ac.restate(img, top, left, ch, cw, S), ac.bound_f32(ch, cw, S)

        def ratio(**variant):
            return float((np.abs(ac.emulate_f32(img, top, left, ch, cw, S, **variant) - ref) / bound).max())
        r = ratio()
        assert r <= 1.0, (h, w, r)
        ratios["contract"] = max(ratios["contract"], r)
        if top > 0 or left > 0 or top + ch < h or left + cw < w:         # the full box has no pixel outside it
            v = ratio(clip="image")
            assert v > 100.0, (h, w, v)
            ratios["image_clip"] = max(ratios["image_clip"], v)
        if max(ch, cw) > S:                                               # an upscale has fs = 1 either way
            v = ratio(antialias=False)
            assert v > 100.0, (h, w, v)
            ratios["no_antialias"] = max(ratios["no_antialias"], v)
        v = ratio(half=False)
        assert v > 100.0, (h, w, v)
        ratios["corner_centres"] = max(ratios["corner_centres"], v)
    print(ratios)
    assert all(v > 0 for v in ratios.values())


def test_identity_and_one_pixel_crops_are_exact_in_the_f32_emulation():
    img = ac.make_image(20, 16, "noise", seed=3)
    got = ac.emulate_f32(img, 3, 5, 8, 8, 8)
    want = ((img[3:11, 5:13].astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.5)).transpose(2, 0, 1)
    assert np.array_equal(got, want)
    one = ac.emulate_f32(img, 7, 9, 1, 1, 8)
    assert all(np.all(one[c] == one[c, 0, 0]) for c in range(3))


@pytest.mark.parametrize("imagenet", [False, True])
def test_packer_round_trip(tmp_path, imagenet):
    from PIL import Image
    from ldmae_amd import pack_images as pk
    from ldmae_amd.datasets.packed_images import PackedImages
    root = str(tmp_path / ("imagenet_like" if imagenet else "tree"))
    files = write_folder(root, imagenet)
    out = str(tmp_path / "pack")
    S0 = 96
    assert pk.main(["--data_path", root, "--out", out, "--short_side", str(S0), "--shard_bytes", "150000", "--num_workers", "3"]) == len(files)
    ds = PackedImages(out)
    samples, classes = pk.list_samples(root)
    assert len(ds) == len(files) and ds.short_side == S0 and ds.classes == classes and len(ds.shard_bytes) > 1
    if imagenet:
        from ldmae_amd.datasets.image_folder import ImageFolder
        ref = ImageFolder(os.path.join(root, "train"))
        assert samples == ref.samples and classes == ["c0", "c1", "c2"] and ds.labels.tolist() == ref.targets
    else:
        assert [p for p, _ in samples] == sorted(files) and ds.labels.tolist() == [0] * len(files) and classes == []
    meta = json.load(open(os.path.join(out, "pack.json")))
    assert meta["version"] == 1 and meta["count"] == len(files) and meta["short_side"] == S0
    for k, n in enumerate(meta["shards"]):
        assert n % 16 == 0 and os.path.getsize(os.path.join(out, f"shard-{k:05d}.bin")) == n
    assert all(int(o) % 16 == 0 for o in ds.offset)
    seen_small = seen_large = 0
    for i, (path, label) in enumerate(samples):
        h, w = files[path]
        img = Image.open(path).convert("RGB")
        if min(h, w) > S0:
            seen_large += 1
            nh, nw = (S0, int(round(w * S0 / h))) if h <= w else (int(round(h * S0 / w)), S0)
            img = img.resize((nw, nh), Image.BICUBIC)
        else:
            seen_small += 1
            nh, nw = h, w                                            # never upscaled
        assert tuple(ds.sizes[i]) == (nh, nw) and min(nh, nw) <= S0
        got, lab = ds[i]
        assert lab == label and got.shape == (nh, nw, 3) and np.array_equal(got, np.asarray(img))
    assert seen_small >= 3 and seen_large >= 3


def test_packer_refusals(tmp_path, capsys):
    from ldmae_amd import pack_images as pk
    root = str(tmp_path / "tree")
    write_folder(root, n=3)
    os.makedirs(tmp_path / "empty")
    for argv, word in ((["--data_path", str(tmp_path / "empty"), "--out", str(tmp_path / "o1"), "--short_side", "64"], "no image files"),
                       (["--data_path", root, "--out", str(tmp_path / "o2"), "--short_side", "7"], "below 8")):
        with pytest.raises(SystemExit) as e:
            pk.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
        assert not os.path.exists(argv[3])
    out = str(tmp_path / "o3")
    assert pk.main(["--data_path", root, "--out", out, "--short_side", "64"]) == 3
    with pytest.raises(SystemExit) as e:
        pk.main(["--data_path", root, "--out", out, "--short_side", "64"])
    assert e.value.code == 2 and "already holds a pack" in capsys.readouterr().err


def test_crop_tables_are_box_plus_flip_under_the_same_generator():
    from ldmae_amd.datasets.packed_images import batch_seed, draw_table
    from ldmae_amd.vmae_pretrain import RandomResizedCropFlip
    sizes = np.array([(96, 128), (40, 56), (200, 96), (96, 96), (64, 333)], dtype=np.int32)        # the last one falls back to the central crop sometimes
    seed = batch_seed(3, 1, 2, 5)
    assert seed == batch_seed(3, 1, 2, 5) and 0 <= seed < 2 ** 63
    assert len({batch_seed(3, 1, 2, 5), batch_seed(4, 1, 2, 5), batch_seed(3, 0, 2, 5), batch_seed(3, 1, 3, 5), batch_seed(3, 1, 2, 6)}) == 5
    geom = draw_table(sizes, 32, (0.75, 1.0), (3 / 4, 4 / 3), torch.Generator().manual_seed(seed))
    g = torch.Generator().manual_seed(seed)
    tr = RandomResizedCropFlip(32)
    for b, (h, w) in enumerate(sizes):
        top, left, ch, cw = tr._box(int(w), int(h), generator=g)
        flip = int(bool(torch.rand(1, generator=g) < 0.5))
        assert geom[b].tolist() == [h, w, top, left, ch, cw, flip, 0]
        assert 0 <= top and top + ch <= h and 0 <= left and left + cw <= w and ch >= 1 and cw >= 1
    assert geom.dtype == torch.int32 and len(set(geom[:, 6].tolist())) <= 2
    # the generator argument defaults to the global RNG: today's draws are unchanged
    torch.manual_seed(11)
    a = [tr._box(200, 150) for _ in range(5)]
    torch.manual_seed(11)
    assert a == [tr._box(200, 150, generator=None) for _ in range(5)]
    g2 = torch.Generator().manual_seed(11)
    assert a == [tr._box(200, 150, generator=g2) for _ in range(5)]      # torch.manual_seed(11) seeds the default generator the same way


def test_box_draws_are_the_ones_of_the_form_without_a_generator():
    """_box as it stood before it took a generator (a fresh one-element tensor per draw, the global RNG), restated: the same boxes from the same seed."""
    import math
    from ldmae_amd.vmae_pretrain import RandomResizedCropFlip

    def before(w, h, scale=(0.75, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
        area, lr = w * h, (math.log(ratio[0]), math.log(ratio[1]))
        for _ in range(10):
            ta = area * float(torch.empty(1).uniform_(scale[0], scale[1]))
            ar = math.exp(float(torch.empty(1).uniform_(lr[0], lr[1])))
            cw, ch = int(round(math.sqrt(ta * ar))), int(round(math.sqrt(ta / ar)))
            if 0 < cw <= w and 0 < ch <= h:
                return int(torch.randint(0, h - ch + 1, (1,))), int(torch.randint(0, w - cw + 1, (1,))), ch, cw
        r = w / h
        if r < ratio[0]:
            cw, ch = w, int(round(w / ratio[0]))
        elif r > ratio[1]:
            ch, cw = h, int(round(h * ratio[1]))
        else:
            cw, ch = w, h
        return (h - ch) // 2, (w - cw) // 2, ch, cw
    tr = RandomResizedCropFlip(32)
    sizes = [(200, 150), (96, 96), (333, 64), (40, 56), (64, 333)]
    torch.manual_seed(21)
    want = [before(w, h) for w, h in sizes * 8]
    torch.manual_seed(21)
    assert [tr._box(w, h) for w, h in sizes * 8] == want
    assert any(b == ((h - b[2]) // 2, (w - b[3]) // 2, b[2], b[3]) and (b[2], b[3]) != (h, w) for b, (w, h) in zip(want, sizes * 8))     # the fall-back was reached


def test_table_check_names_the_sample():
    from ldmae_amd import ops
    off = torch.tensor([0, 304], dtype=torch.int64)
    good = torch.tensor([[10, 10, 0, 0, 10, 10, 0, 0], [8, 12, 1, 2, 7, 10, 1, 0]], dtype=torch.int32)
    ops.check_crop_table(off, good, 304 + 288)
    for row, total, word in (([8, 12, 2, 2, 7, 10, 0, 0], 592, "leaves the image"), ([8, 12, 0, 3, 8, 10, 0, 0], 592, "leaves the image"),
                             ([8, 12, 0, 0, 0, 5, 0, 0], 592, "empty crop"), ([8, 12, 1, 2, 7, 10, 0, 0], 591, "past the blob")):
        bad = good.clone()
        bad[1] = torch.tensor(row, dtype=torch.int32)
        with pytest.raises(ValueError, match="sample 1") as e:
            ops.check_crop_table(off, bad, total)
        assert word in str(e.value)
    with pytest.raises(ValueError, match=r"\[B, 8\]"):
        ops.check_crop_table(off, good[:, :7], 592)


def test_driver_flags(tmp_path, capsys):
    from ldmae_amd import pack_images as pk
    from ldmae_amd import vmae_pretrain as vp
    root = str(tmp_path / "tree")
    write_folder(root, n=3)
    out = str(tmp_path / "pack")
    pk.main(["--data_path", root, "--out", out, "--short_side", "64"])
    capsys.readouterr()
    args = vp.parse_args(["--packed_data", out, "--input_size", "64"])                      # --data_path is not needed
    assert args.packed_data == out and not args.data_path and not args.synthetic
    assert vp.parse_args(["--packed_data", out, "--data_path", root, "--input_size", "32"]).data_path == root
    for argv, words in ((["--packed_data", out, "--synthetic"], ("exclude",)),
                        (["--packed_data", out, "--input_size", "128"], ("re-pack", "--short_side 64")),
                        (["--packed_data", str(tmp_path / "nothing")], ("not a pack",)),
                        ([], ("--packed_data",))):
        with pytest.raises(SystemExit) as e:
            vp.parse_args(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w_ in err for w_ in words), err
    sh = open(os.path.join(ROOT, "ldmae_amd", "train_ae.sh")).read()
    assert 'stage1+=(--packed_data "$PACKED_DATA_128")' in sh and 'stage3+=(--packed_data "$PACKED_DATA_256")' in sh


def test_loader_refuses_a_host_device(tmp_path):
    from ldmae_amd import pack_images as pk
    from ldmae_amd.datasets.packed_images import PackedBatchLoader, PackedImages
    root = str(tmp_path / "tree")
    write_folder(root, n=3)
    pk.main(["--data_path", root, "--out", str(tmp_path / "pack"), "--short_side", "64"])
    ds = PackedImages(str(tmp_path / "pack"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PackedBatchLoader(ds, torch.utils.data.SequentialSampler(ds), 2, 32, 0, "cpu")


def test_abi_header_binding_and_library():
    from ldmae_amd import _lib
    name = "ldmae_crop_resize_flip_u8"
    header = open(os.path.join(ROOT, "include", "ldmae_hip.h")).read()
    m = re.search(r"\bint " + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in include/ldmae_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 11 and params[0] == "const unsigned char* blob" and params[1] == "long blob_bytes" and params[-1] == "void* stream"
    res, argt = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and len(argt) == 11
    assert argt[1] is ctypes.c_long and argt[5:8] == [ctypes.c_int] * 3 and argt[8:10] == [ctypes.c_float] * 2
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert "augment.hip" in open(os.path.join(ROOT, "ldmae_amd", "csrc", "Makefile")).read()
    lib = _lib.load()
    # LDMAE_ERR_INVALID (-1): every refusal of the contract is made before anything touches a device
    one = ctypes.c_void_p(16)
    for args in ((None, 64, one, one, one, 0, 1, 8, 0.5, 0.5, None), (one, 64, None, one, one, 0, 1, 8, 0.5, 0.5, None),
                 (one, 64, one, None, one, 0, 1, 8, 0.5, 0.5, None), (one, 64, one, one, None, 0, 1, 8, 0.5, 0.5, None),
                 (one, 64, one, one, one, 0, 0, 8, 0.5, 0.5, None), (one, 64, one, one, one, 0, 1, 0, 0.5, 0.5, None),
                 (one, 64, one, one, one, 0, 1, 8, 0.5, 0.0, None)):
        assert lib.ldmae_crop_resize_flip_u8(*args) == -1 and b"crop_resize_flip_u8" in lib.ldmae_last_error()
