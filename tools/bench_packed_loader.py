"""Feeding VMAE pre-training from real images on one MI355X host: today's image-folder DataLoader against the packed shards + the device-side
transform (ldmae_amd/pack_images.py, datasets/packed_images.py, ldmae_crop_resize_flip_u8).  Everything is generated here: a folder of synthetic
JPEGs of ImageNet-like sizes (PIL, seeded), packed at --short_side 160 and 320.  Reported:
  (a) images/s of the folder DataLoader (ImageFolder + RandomResizedCropFlip, forkserver workers) at --num_workers 8 and 16, in steady state;
  (b) images/s of PackedBatchLoader alone (thread + upload + kernel, nothing consuming the batches);
  (c) the kernel alone on a staged batch, 200 launches per round over 8 separate copies of blob and output taken in turn (more bytes than the
      last-level cache holds): ms per batch (device events, median over rounds with min .. max) and GB/s = (crop-box bytes read + output bytes
      written) / time, at input_size 128 and 256, batch 256, f32 and bf16 output;
  (d) the vmae_pretrain step (train_one_epoch on the shipped model, bf16 autocast) fed by the packed loader against the device-resident
      --synthetic batches, at 128 px with --mask_ratio 0.75 (the default) and 0.25 (stage 1) and at 256 px with 0.75, ALTERNATING round by round in one process: median step time with (min .. max) of each, so that the difference can be
      read against the spread.

    python tools/bench_packed_loader.py [--images 2048] [--batch 256] [--steps 20] [--rounds 4] [--out profiles/packed_loader_bench.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = [(500, 375), (375, 500), (500, 333), (333, 500), (640, 480), (500, 500), (400, 300), (256, 341)]     # (w, h)


_BASE = {}


def make_jpeg(args):
    """One seeded JPEG: a smooth pattern per size (made once), shifted per image, plus byte noise -- about as compressible as a photograph."""
    path, w, h, seed = args
    from PIL import Image
    rng = np.random.default_rng(seed)
    if (w, h) not in _BASE:
        yy, xx = np.mgrid[0:h, 0:w]
        _BASE[(w, h)] = np.stack([127 + 90 * np.sin(xx / (9.0 + 7 * c)) * np.cos(yy / (13.0 + 5 * c)) for c in range(3)], axis=2).astype(np.int16)
    img = np.roll(_BASE[(w, h)], (int(rng.integers(h)), int(rng.integers(w))), axis=(0, 1)) + rng.integers(-40, 41, (h, w, 3), dtype=np.int16)
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(path, quality=90)
    return os.path.getsize(path)


def make_folder(root, n):
    from multiprocessing.pool import ThreadPool
    jobs = []
    for i in range(n):
        d = os.path.join(root, "train", f"class{i % 16:02d}")
        os.makedirs(d, exist_ok=True)
        w, h = SIZES[i % len(SIZES)]
        jobs.append((os.path.join(d, f"{i:06d}.JPEG"), w, h, i))
    with ThreadPool(16) as pool:
        sizes = pool.map(make_jpeg, jobs)
    return sum(sizes) / n


def spread(ts, scale=1e3):
    return f"{statistics.median(ts) * scale:.3f} ({min(ts) * scale:.3f} .. {max(ts) * scale:.3f})"


def folder_rate(root, size, workers, batch=64, batches=96):
    """Steady-state images/s: the second half of `batches` batches (the first half outlasts worker start-up and the 2 x workers prefetched batches)."""
    from ldmae_amd import vmae_pretrain as vp
    from ldmae_amd.datasets.image_folder import ImageFolder
    ds = ImageFolder(os.path.join(root, "train"), transform=vp.RandomResizedCropFlip(size))
    sampler = torch.utils.data.RandomSampler(ds, replacement=True, num_samples=batch * batches, generator=torch.Generator().manual_seed(0))
    loader = torch.utils.data.DataLoader(ds, batch_size=batch, sampler=sampler, num_workers=workers, pin_memory=True, drop_last=True,
                                         multiprocessing_context="forkserver")
    assert batches // 2 > 2 * workers
    n, t0 = 0, None
    for k, (x, _) in enumerate(loader):
        x = x.cuda(non_blocking=True)
        if k + 1 == batches // 2:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        elif t0 is not None:
            n += x.shape[0]
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def packed_rate(ds, size, batch, epochs, dtype):
    from ldmae_amd.datasets.packed_images import PackedBatchLoader
    sampler = torch.utils.data.RandomSampler(ds, replacement=True, num_samples=batch * (len(ds) // batch) * epochs, generator=torch.Generator().manual_seed(0))
    loader = PackedBatchLoader(ds, sampler, batch, size, 0, "cuda", out_dtype=dtype)
    n, t0 = 0, None
    for x, _ in loader:
        if t0 is None:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        else:
            n += x.shape[0]
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def kernel_time(ds, size, batch, dtype, iters, rounds, copies=8):
    """`copies` separate (blob, output) pairs taken in turn, so that consecutive launches do not find their bytes in the last-level cache
    (8 x 72 MB at 128 px, 8 x 289 MB at 256 px against 256 MiB)."""
    from ldmae_amd import ops
    from ldmae_amd.datasets.packed_images import draw_table
    idx = np.arange(batch) % len(ds)
    parts, starts, pos = [], [], 0
    for i in idx:                               # the loader's staging layout: images back to back, every start on 16 bytes
        raw = ds.raw(int(i))
        starts.append(pos)
        parts += [raw, np.zeros(-len(raw) % 16, np.uint8)]
        pos += len(raw) + (-len(raw) % 16)
    geom_h = draw_table(ds.sizes[idx], size, (0.75, 1.0), (3 / 4, 4 / 3), torch.Generator().manual_seed(0))
    off_h = torch.tensor(starts, dtype=torch.int64)
    ops.check_crop_table(off_h, geom_h, pos)
    blob, off, geom = torch.from_numpy(np.concatenate(parts)).cuda(), off_h.cuda(), geom_h.cuda()
    blobs = [blob] + [blob.clone() for _ in range(copies - 1)]
    outs = [torch.empty(batch, 3, size, size, dtype=dtype, device="cuda") for _ in range(copies)]
    out = outs[0]
    read = int((3 * geom_h[:, 4].long() * geom_h[:, 5].long()).sum())
    written = out.numel() * out.element_size()
    ts = []
    for r in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            ops.crop_resize_flip(blobs[i % copies], off, geom, size, out_dtype=dtype, out=outs[i % copies])
        e1.record()
        torch.cuda.synchronize()
        if r:                                   # round 0 warms up
            ts.append(e0.elapsed_time(e1) * 1e-3 / iters)
    return ts, read, written, blob.numel()


def step_times(ds, size, batch, steps, rounds, mask_ratio):
    from ldmae_amd import vmae_pretrain as vp
    from ldmae_amd.datasets.packed_images import PackedBatchLoader
    from ldmae_amd.tokenizer import models_mae
    args = vp.parse_args(["--synthetic", "--batch_size", str(batch), "--input_size", str(size), "--print_freq", "100000", "--epochs", "1000",
                          "--warmup_epochs", "1", "--lr", "1e-4", "--mask_ratio", str(mask_ratio)])
    torch.manual_seed(0)
    model = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=False, no_cls=True, kl_loss_weight=args.kl_loss_weight, smooth_output=True, img_size=size).cuda()
    opt = vp.build_optimizer(model, args.lr, args.weight_decay)
    scaler = vp.LossScaler(enabled=True)
    sampler = torch.utils.data.RandomSampler(ds, replacement=True, num_samples=batch * steps, generator=torch.Generator().manual_seed(1))
    feeds = {"synthetic": vp._SyntheticLoader(steps, batch, size, 0), "packed": PackedBatchLoader(ds, sampler, batch, size, 0, "cuda")}
    out = {k: [] for k in feeds}
    for r in range(rounds + 1):
        for k, loader in feeds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vp.train_one_epoch(model, loader, opt, r, args, log=lambda *a: None, scaler=scaler)      # ends with a host read of the loss
            torch.cuda.synchronize()
            if r:
                out[k].append((time.perf_counter() - t0) / steps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--workers", default="8,16")
    ap.add_argument("--skip_folder", action="store_true", help="leave (a) out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_loader_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from ldmae_amd import pack_images as pk
    from ldmae_amd.datasets.packed_images import PackedImages
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "imagenet_synth")
        t0 = time.perf_counter()
        mean_bytes = make_folder(root, a.images)
        say(f"{a.images} synthetic JPEGs, sizes {SIZES} (w, h), {mean_bytes / 1e3:.1f} KB each on average; generated in {time.perf_counter() - t0:.1f} s")
        packs = {}
        for size, short in ((128, 160), (256, 320)):
            t0 = time.perf_counter()
            out = os.path.join(tmp, f"pack{short}")
            pk.pack(root, out, short, num_workers=16, log=lambda s: None)
            packs[size] = PackedImages(out)
            say(f"packed at --short_side {short}: {sum(packs[size].shard_bytes) / 2 ** 20:.1f} MiB, {a.images / (time.perf_counter() - t0):.0f} images/s with 16 threads")
        say(f"device: {torch.cuda.get_device_name(0)}; batch {a.batch}; os.cpu_count() {os.cpu_count()}, usable {len(os.sched_getaffinity(0))}")
        if not a.skip_folder:
            say("(a) folder DataLoader (ImageFolder + RandomResizedCropFlip, forkserver workers), images/s:")
            for size in (128, 256):
                for wk in (int(v) for v in a.workers.split(",")):
                    say(f"    input_size {size}  num_workers {wk:2d}: {folder_rate(root, size, wk):8.0f}")
        say("(b) PackedBatchLoader alone, images/s:")
        for size in (128, 256):
            for dtype in (torch.float32, torch.bfloat16):
                say(f"    input_size {size}  {str(dtype)[6:]:8s}: {packed_rate(packs[size], size, a.batch, 4, dtype):8.0f}")
        say(f"(c) ldmae_crop_resize_flip_u8 alone, {a.iters} launches per round over 8 copies of one staged batch: ms per batch, median (min .. max); "
            "GB/s = (crop bytes read + output bytes written) / median")
        for size in (128, 256):
            for dtype in (torch.float32, torch.bfloat16):
                ts, read, written, staged = kernel_time(packs[size], size, a.batch, dtype, a.iters, a.rounds)
                say(f"    input_size {size}  {str(dtype)[6:]:8s}: {spread(ts)} ms; reads {read / 1e6:.1f} MB of a {staged / 1e6:.1f} MB blob, writes {written / 1e6:.1f} MB; "
                    f"{(read + written) / statistics.median(ts) / 1e9:.0f} GB/s")
        for size, mask_ratio in ((128, 0.75), (128, 0.25), (256, 0.75)):         # the driver's default mask ratio, stage 1 of train_ae.sh, DESIGN section 9 item 4
            say(f"(d) vmae_pretrain step, batch {a.batch}, input_size {size}, mask_ratio {mask_ratio}, bf16 autocast, {a.steps} steps per round, {a.rounds} alternating "
                "rounds: ms per step, median (min .. max)")
            st = step_times(packs[size], size, a.batch, a.steps, a.rounds, mask_ratio)
            for k, ts in st.items():
                say(f"    {k:10s}: {spread(ts)}   rounds: {', '.join(f'{t * 1e3:.2f}' for t in ts)}")
            d = statistics.median(st["packed"]) - statistics.median(st["synthetic"])
            s = max(max(ts) - min(ts) for ts in st.values())
            say(f"    packed - synthetic = {d * 1e3:+.3f} ms per step; largest min .. max spread of one feed {s * 1e3:.3f} ms")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
