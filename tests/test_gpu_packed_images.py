"""ldmae_crop_resize_flip_u8 on the device -- through the C ABI and through ops.crop_resize_flip -- against the f64 restatement within the
checker's derived bound (tests/augment_check.py), its exact cases, what may and may not influence a sample, and the packed loader and the
`vmae_pretrain --packed_data` driver on a generated folder.  Shapes beyond the issue's five geometries (EXTRA) are there for the code's own paths:
S that is no multiple of 4 / 8 (element-wise stores instead of 16-byte ones), a last column tile of 8, more than one chunk of source rows."""
import numpy as np
import pytest
import torch

import augment_check as ac

pytestmark = pytest.mark.gpu

# (h, w, top, left, ch, cw, S)
EXTRA = [
    (23, 19, 2, 3, 17, 13, 7),         # odd S: element-wise stores, f32 and bf16
    (23, 19, 2, 3, 17, 13, 10),
    (40, 33, 1, 2, 38, 30, 12),        # 16-byte f32 stores, element-wise bf16 ones
    (100, 90, 5, 4, 90, 80, 72),       # two column tiles, the second 8 wide; five row bands, the last 8 high
    (300, 20, 0, 0, 300, 20, 4),       # 75 x down: 300 taps per output row, ten chunks of source rows
    (160, 200, 3, 5, 150, 190, 200),   # 200 = 3 x 64 + 8 columns, a mixed up / down scale
]


def _launch(blob, offsets, geom, S, bf16=False, mean=0.5, std=0.5):
    """The C ABI itself: host arrays -> device, one launch -> [B, 3, S, S] tensor on the device."""
    from ldmae_amd import _lib
    b = torch.from_numpy(np.ascontiguousarray(blob)).cuda()
    o = torch.as_tensor(np.asarray(offsets), dtype=torch.int64).cuda()
    g = torch.as_tensor(np.asarray(geom), dtype=torch.int32).reshape(-1, 8).cuda()
    out = torch.full((g.shape[0], 3, S, S), float("nan"), dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
    _lib.call("ldmae_crop_resize_flip_u8", _lib.ptr(b), b.numel(), _lib.ptr(o), _lib.ptr(g), _lib.ptr(out), 1 if bf16 else 0, g.shape[0], S,
              float(mean), float(std), _lib.stream())
    torch.cuda.synchronize()
    return out


def _blob_of(images, first=3, gap=5):
    """Images back to back at ODD byte offsets, with a few bytes of 0xAA between them -> (blob, offsets)."""
    parts, offsets, pos = [np.full(first, 0xAA, np.uint8)], [], first
    for im in images:
        offsets.append(pos)
        parts += [np.ascontiguousarray(im).reshape(-1), np.full(gap, 0xAA, np.uint8)]
        pos += im.size + gap
        if pos % 2 == 0:
            parts.append(np.full(1, 0xAA, np.uint8))
            pos += 1
    return np.concatenate(parts), offsets


def _check(name, got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err / bound[None]).max())
    print(f"{name}: worst error {err.max():.3e}, worst error / bound {ratio:.4f} (bound up to {bound.max():.3e})")
    assert np.isfinite(got).all() and ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("geom", ac.GEOMS + EXTRA, ids=lambda g: "x".join(map(str, g)))
def test_kernel_against_the_restatement(geom, flip):
    from ldmae_amd import ops
    h, w, top, left, ch, cw, S = geom
    img = ac.make_image(w, h, "noise", seed=5)
    blob, off = _blob_of([img])
    row = [h, w, top, left, ch, cw, flip, 0]
    ref, bound = ac.restate(img, top, left, ch, cw, S, flip), ac.bound_f32(ch, cw, S, flip)
    abi = _launch(blob, off, [row], S)
    _check(f"abi {geom} flip {flip}", abi[0].cpu().numpy(), ref, bound)
    via_ops = ops.crop_resize_flip(torch.from_numpy(blob).cuda(), torch.tensor(off, dtype=torch.int64), torch.tensor([row], dtype=torch.int32), S)
    assert via_ops.dtype == torch.float32 and torch.equal(via_ops, abi)
    # bf16 output is the f32 output rounded to nearest even, bit for bit -- through both doors
    abi16 = _launch(blob, off, [row], S, bf16=True)
    assert torch.equal(abi16.view(torch.int16), abi.to(torch.bfloat16).view(torch.int16))
    ops16 = ops.crop_resize_flip(torch.from_numpy(blob).cuda(), torch.tensor(off, dtype=torch.int64), torch.tensor([row], dtype=torch.int32), S,
                                 out_dtype=torch.bfloat16)
    assert torch.equal(ops16.view(torch.int16), abi16.view(torch.int16))
    # other normalisation constants, into a caller's buffer
    out = torch.empty(1, 3, S, S, device="cuda")
    assert ops.crop_resize_flip(torch.from_numpy(blob).cuda(), torch.tensor(off, dtype=torch.int64), torch.tensor([row], dtype=torch.int32), S,
                                mean=0.45, std=0.25, out=out) is out
    _check(f"ops mean 0.45 std 0.25 {geom}", out[0].cpu().numpy(), ac.restate(img, top, left, ch, cw, S, flip, 0.45, 0.25),
           ac.bound_f32(ch, cw, S, flip, 0.45, 0.25))


def test_exact_cases():
    img = ac.make_image(21, 18, "noise", seed=6)
    blob, off = _blob_of([img])
    # a 1 x 1 crop: every output is that pixel
    got = _launch(blob, off, [[18, 21, 7, 9, 1, 1, 0, 0]], 8)[0].cpu()
    px = torch.from_numpy(img[7, 9].astype(np.float32))
    assert torch.equal(got, ((px / 255 - 0.5) / 0.5)[:, None, None].expand(3, 8, 8))
    # an S x S crop to S: the weights are exactly 0, 1, 0, 0 -- (p / 255 - 0.5) / 0.5 bit for bit, flipped or not
    for S in (8, 13):
        want = ((torch.from_numpy(img[2:2 + S, 5:5 + S].astype(np.float32)) / 255 - 0.5) / 0.5).permute(2, 0, 1)
        assert torch.equal(_launch(blob, off, [[18, 21, 2, 5, S, S, 0, 0]], S)[0].cpu(), want)
        assert torch.equal(_launch(blob, off, [[18, 21, 2, 5, S, S, 1, 0]], S)[0].cpu(), want.flip(-1))
    # a 0 / 255 checkerboard upscaled: the cubic overshoots, both clamps hold it inside [-1, 1]
    chk = ac.make_image(6, 6, "checker")
    cb, co = _blob_of([chk])
    out = _launch(cb, co, [[6, 6, 0, 0, 6, 6, 0, 0]], 32)[0].cpu().numpy()
    assert out.min() == -1.0 and out.max() == 1.0
    _check("checkerboard 6 -> 32", out, ac.restate(chk, 0, 0, 6, 6, 32), ac.bound_f32(6, 6, 32))
    unclamped = np.einsum("jy,yic->jic", ac.axis_matrix(6, 32), np.einsum("ix,yxc->yic", ac.axis_matrix(6, 32), chk.astype(np.float64)))
    assert unclamped.max() > 260 and unclamped.min() < -5          # there was something to clamp


def test_only_the_crop_box_influences_a_sample():
    """One batch of five with odd byte offsets.  Inverting EVERY byte of the blob outside sample b's crop box -- the rest of its own image, the
    neighbouring images, the bytes between them -- leaves output b bitwise equal; changing one pixel inside the box does not."""
    geoms = [ac.GEOMS[0], ac.GEOMS[2], ac.GEOMS[3], EXTRA[0], ac.GEOMS[6]]
    S = 16
    images = [ac.make_image(g[1], g[0], "noise", seed=10 + i) for i, g in enumerate(geoms)]
    blob, off = _blob_of(images)
    assert all(o % 2 == 1 for o in off)
    table = [[g[0], g[1], g[2], g[3], g[4], g[5], i % 2, 0] for i, g in enumerate(geoms)]
    base = _launch(blob, off, table, S)
    assert torch.equal(base, _launch(blob, off, table, S))                                 # two launches: the same bits
    for b, (g, im) in enumerate(zip(geoms, images)):
        _check(f"batch sample {b}", base[b].cpu().numpy(), ac.restate(im, g[2], g[3], g[4], g[5], S, b % 2), ac.bound_f32(g[4], g[5], S, b % 2))
        inside = np.zeros(blob.shape, dtype=bool)
        view = inside[off[b]:off[b] + im.size].reshape(im.shape)
        view[g[2]:g[2] + g[4], g[3]:g[3] + g[5]] = True
        other = np.where(inside, blob, blob ^ 0xFF).astype(np.uint8)
        got = _launch(other, off, table, S)
        assert torch.equal(got[b], base[b]), b
        assert all(not torch.equal(got[k], base[k]) for k in range(len(geoms)) if k != b)
        poked = blob.copy()
        pos = off[b] + ((g[2] + g[4] // 2) * g[1] + g[3] + g[5] // 2) * 3 + 1
        assert inside[pos]
        poked[pos] ^= 0x80
        got = _launch(poked, off, table, S)
        assert not torch.equal(got[b], base[b]), b
        assert all(torch.equal(got[k], base[k]) for k in range(len(geoms)) if k != b)


def test_ops_refuses_bad_tables():
    from ldmae_amd import ops
    img = ac.make_image(12, 8, "noise")
    blob = torch.from_numpy(img.reshape(-1).copy()).cuda()
    off = torch.zeros(1, dtype=torch.int64)
    ok = ops.crop_resize_flip(blob, off, torch.tensor([[8, 12, 1, 2, 7, 10, 0, 0]], dtype=torch.int32), 8)
    assert ok.shape == (1, 3, 8, 8)
    with pytest.raises(ValueError, match="sample 0 has a crop box that leaves the image"):
        ops.crop_resize_flip(blob, off, torch.tensor([[8, 12, 2, 2, 7, 10, 0, 0]], dtype=torch.int32), 8)
    with pytest.raises(ValueError, match="sample 0 has an image that ends past the blob"):
        ops.crop_resize_flip(blob, torch.ones(1, dtype=torch.int64), torch.tensor([[8, 12, 1, 2, 7, 10, 0, 0]], dtype=torch.int32), 8)
    with pytest.raises(ValueError, match=r"\[B, 8\]"):
        ops.crop_resize_flip(blob, off, torch.tensor([[8, 12, 1, 2, 7, 10, 0]], dtype=torch.int32), 8)
    with pytest.raises(ValueError, match="out_dtype"):
        ops.crop_resize_flip(blob, off, torch.tensor([[8, 12, 1, 2, 7, 10, 0, 0]], dtype=torch.int32), 8, out_dtype=torch.float16)


# ----------------------------------------------------------------------------- the loader and the driver, on one generated pack
@pytest.fixture(scope="module")
def pack(tmp_path_factory):
    from ldmae_amd import pack_images as pk
    from test_packed_images_cpu import write_folder
    root = tmp_path_factory.mktemp("packed")
    write_folder(str(root / "imagenet_like"), imagenet=True)
    pk.main(["--data_path", str(root / "imagenet_like"), "--out", str(root / "pack"), "--short_side", "96", "--shard_bytes", "150000"])
    return str(root / "pack")


def _epoch(ds, prefetch, epoch=0, seed=7):
    from ldmae_amd.datasets.packed_images import PackedBatchLoader
    sampler = torch.utils.data.DistributedSampler(ds, num_replicas=1, rank=0, shuffle=True, seed=0)
    sampler.set_epoch(epoch)
    loader = PackedBatchLoader(ds, sampler, 4, 32, seed, "cuda", prefetch=prefetch)
    assert len(loader) == 3
    got = []
    for images, labels in loader:
        t = loader.last_table
        got.append((images.clone(), labels.clone(), {k: (v.clone() if torch.is_tensor(v) else v) for k, v in t.items()}))
    return got, list(sampler)


def test_loader_batches(pack):
    from ldmae_amd.datasets.packed_images import PackedImages
    ds = PackedImages(pack)
    got, order = _epoch(ds, prefetch=2)
    assert len(got) == 3 and len(order) == 12
    seen = []
    for k, (images, labels, table) in enumerate(got):
        assert images.shape == (4, 3, 32, 32) and images.dtype == torch.float32 and images.is_cuda and table["batch"] == k and table["epoch"] == 0
        idx = table["index"].tolist()
        assert idx == order[4 * k:4 * k + 4] and labels.tolist() == ds.labels[idx].tolist()
        seen += idx
        for b, i in enumerate(idx):
            h, w, top, left, ch, cw, flip, _ = table["geom"][b].tolist()
            assert (h, w) == tuple(ds.sizes[i]) and int(table["offset"][b]) % 16 == 0
            _check(f"loader batch {k} sample {b}", images[b].cpu().numpy(), ac.restate(ds.image(i), top, left, ch, cw, 32, flip), ac.bound_f32(ch, cw, 32, flip))
    assert sorted(seen) == list(range(12))                                      # every index of the epoch, once
    # a sample is a function of (pack, seed, rank, epoch, position): the same bits whatever the prefetch depth
    for prefetch in (1, 3):
        again, _ = _epoch(ds, prefetch=prefetch)
        for (a, la, ta), (b, lb, tb) in zip(got, again):
            assert torch.equal(a, b) and torch.equal(la, lb) and torch.equal(ta["geom"], tb["geom"]) and torch.equal(ta["index"], tb["index"])
    # another epoch: another order and other boxes
    other, order1 = _epoch(ds, prefetch=2, epoch=1)
    assert order1 != order and sorted(order1) == list(range(12))
    boxes0 = {int(i): g.tolist() for _, _, t in got for i, g in zip(t["index"], t["geom"])}
    boxes1 = {int(i): g.tolist() for _, _, t in other for i, g in zip(t["index"], t["geom"])}
    assert sum(boxes0[i] != boxes1[i] for i in range(12)) >= 10
    # and another seed
    reseeded, _ = _epoch(ds, prefetch=2, seed=8)
    assert not torch.equal(reseeded[0][2]["geom"], got[0][2]["geom"])


def test_loader_keeps_its_buffers_and_interleaves_with_other_work(pack):
    """The staging slots are the loader's, made once: a second epoch reuses the same pinned and device buffers.  Batches stay right while the
    consumer's stream is busy allocating, filling and freeing tensors of the blobs' size between them (what a training step does)."""
    from ldmae_amd.datasets.packed_images import PackedBatchLoader, PackedImages
    ds = PackedImages(pack)
    sampler = torch.utils.data.DistributedSampler(ds, num_replicas=1, rank=0, shuffle=True, seed=0)
    loader = PackedBatchLoader(ds, sampler, 4, 32, 7, "cuda", prefetch=3)
    ptrs = []
    for epoch in range(2):
        sampler.set_epoch(epoch)
        want, _ = _epoch(ds, prefetch=1, epoch=epoch)
        it = iter(loader)
        for k, (images, labels) in enumerate(it):
            if k == 0:
                with pytest.raises(RuntimeError, match="one iteration at a time"):
                    next(iter(loader))
            for _ in range(8):                                     # churn on the consumer's stream, freed at once
                junk = torch.full((300_000,), 0x5A, dtype=torch.uint8, device="cuda")
                del junk
            assert torch.equal(images, want[k][0]) and torch.equal(labels, want[k][1])
        ptrs.append([(id(s_), s_.geom_h.data_ptr(), s_.geom_d.data_ptr(), s_.offsets_d.data_ptr()) for s_ in loader._slots])
    assert len(ptrs[0]) == 3 and ptrs[0] == ptrs[1]            # (the byte buffers may grow with a larger batch; the slots and their tables stay)


def test_pretrain_driver_on_a_pack(pack, tmp_path, capsys):
    import re
    from ldmae_amd import vmae_pretrain as vp
    from ldmae_amd.tokenizer import models_mae
    model, opt = vp.main(["--packed_data", pack, "--input_size", "64", "--batch_size", "6", "--epochs", "1", "--print_freq", "1", "--warmup_epochs", "0",
                          "--blr", "1e-2", "--output_dir", str(tmp_path / "out")])
    log = capsys.readouterr().out
    losses = [float(v) for v in re.findall(r" loss: ([0-9.eE+-]+|nan|inf)", log)]
    assert len(losses) == 2 and all(np.isfinite(losses)), log                  # 12 images, batches of 6: two steps
    assert "12 images; 2 iterations per epoch and rank" in log and opt.step_count == 2
    torch.manual_seed(0)
    start = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=False, no_cls=True, kl_loss_weight=1e-6, smooth_output=True, norm_pix_loss=False, img_size=64,
                                                fixed_std=None).state_dict()
    now = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    assert all(torch.isfinite(v).all() for v in now.values())
    for k in ("patch_embed.proj.weight", "blocks.0.attn.qkv.weight", "decoder_blocks.3.mlp.fc1.weight"):
        assert start[k].shape == now[k].shape and not torch.equal(start[k], now[k]), k
