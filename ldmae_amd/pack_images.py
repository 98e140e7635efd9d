#!/usr/bin/env python3
"""Pack an image folder into raw uint8 shards for the device-side training transform (datasets/packed_images.py):
decode ONCE, offline, instead of in DataLoader workers on every epoch.

    python -m ldmae_amd.pack_images --data_path /data/imagenet --out /data/imagenet_160 --short_side 160
    python ldmae_amd/vmae_pretrain.py --packed_data /data/imagenet_160 --input_size 128 ...

The folder is walked exactly as vmae_pretrain.get_dataset walks it: ImageFolder(<data_path>/train) class and sample order when 'imagenet' is in the
path (labels = class indices), FlatImageTree order otherwise (no classes: every label is 0).  Every image is decoded with PIL, converted to RGB and,
if its short side exceeds --short_side, resized ONCE with PIL BICUBIC so that the short side equals it (aspect kept, the long side rounded); a
smaller image is stored as it is -- never upscaled.

Files written into --out (format version 1):
    shard-00000.bin, shard-00001.bin, ...   images back to back as HWC uint8, rows of 3 w bytes without padding; every image starts at a multiple
                                            of 16 bytes and every shard's length is a multiple of 16 (zero padding); an image never spans two
                                            shards; a shard is closed when the next image would take it past --shard_bytes.  numpy.memmap reads them.
    index.safetensors                       shard i32 [N], offset i64 [N] (bytes from the start of the shard), size i32 [N, 2] = (h, w), label i64 [N]
    pack.json                               {"format": "ldmae-packed-images", "version": 1, "short_side", "count", "shards": [byte lengths], "classes"}
index.safetensors is written last: a directory that has one is a finished pack, and packing into it again is refused (exit code 2), as are an empty
folder and a --short_side below 8."""
import argparse
import json
import os

import numpy as np

FORMAT, VERSION, ALIGN = "ldmae-packed-images", 1, 16
INDEX, META = "index.safetensors", "pack.json"


def list_samples(data_path):
    """-> ([(path, label)], classes) in the order vmae_pretrain.get_dataset iterates the folder."""
    from ldmae_amd.datasets.image_folder import IMG_EXTENSIONS, ImageFolder
    if "imagenet" in data_path:
        ds = ImageFolder(os.path.join(data_path, "train"))
        return list(ds.samples), list(ds.classes)
    paths = sorted(os.path.join(d, f) for d, _, fs in os.walk(data_path, followlinks=True) for f in fs if f.lower().endswith(IMG_EXTENSIONS))
    return [(p, 0) for p in paths], []


def load_image(path, short_side):
    """-> [h, w, 3] uint8: RGB, short side reduced to `short_side` by one BICUBIC resize if it is larger (never enlarged)."""
    from PIL import Image
    with open(path, "rb") as f:
        img = Image.open(f).convert("RGB")
    w, h = img.size
    if min(w, h) > short_side:
        if w <= h:
            w, h = short_side, max(short_side, int(round(h * short_side / w)))
        else:
            w, h = max(short_side, int(round(w * short_side / h))), short_side
        img = img.resize((w, h), Image.BICUBIC)
    return np.ascontiguousarray(np.asarray(img, dtype=np.uint8))


def pack(data_path, out, short_side, shard_bytes=1 << 30, num_workers=8, log=print):
    """-> the number of images packed.  FileNotFoundError when the folder has no image (nothing is written then)."""
    from multiprocessing.pool import ThreadPool                      # PIL releases the GIL while it decodes and resizes
    from safetensors.numpy import save_file
    samples, classes = list_samples(data_path)
    if not samples:
        raise FileNotFoundError(f"no image files under {data_path}")
    os.makedirs(out, exist_ok=True)
    n = len(samples)
    shard, offset, size = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros((n, 2), np.int32)
    label = np.asarray([t for _, t in samples], dtype=np.int64)
    lengths, cur, f = [], 0, None

    def close():
        nonlocal f, cur
        pad = -cur % ALIGN
        f.write(b"\0" * pad)
        f.close()
        lengths.append(cur + pad)
        f, cur = None, 0
    with ThreadPool(max(1, num_workers)) as pool:
        for i, arr in enumerate(pool.imap(lambda s: load_image(s[0], short_side), samples, chunksize=4)):
            nb = arr.size
            if f is not None and cur + (-cur % ALIGN) + nb > shard_bytes:
                close()
            if f is None:
                f = open(os.path.join(out, f"shard-{len(lengths):05d}.bin"), "wb")
            pad = -cur % ALIGN
            f.write(b"\0" * pad)
            cur += pad
            shard[i], offset[i], size[i] = len(lengths), cur, arr.shape[:2]
            f.write(arr.tobytes())
            cur += nb
            if (i + 1) % 10000 == 0:
                log(f"packed {i + 1} / {n} images")
    close()
    with open(os.path.join(out, META), "w") as mf:
        json.dump({"format": FORMAT, "version": VERSION, "short_side": int(short_side), "count": n, "shards": lengths, "classes": classes}, mf)
    save_file({"shard": shard, "offset": offset, "size": size, "label": label}, os.path.join(out, INDEX),
              metadata={"format": FORMAT, "version": str(VERSION)})
    log(f"packed {n} images into {len(lengths)} shard(s), {sum(lengths) / 2 ** 20:.1f} MiB, short side <= {short_side}: {out}")
    return n


def _parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--data_path", required=True, help="'imagenet' in the path: <path>/train/<class>/<image>; otherwise any tree of images")
    ap.add_argument("--out", required=True)
    ap.add_argument("--short_side", type=int, required=True, help="images whose short side is larger are reduced to it (160 for --input_size 128, 320 for 256)")
    ap.add_argument("--shard_bytes", type=int, default=1 << 30)
    ap.add_argument("--num_workers", type=int, default=8, help="decode threads")
    return ap


def main(argv=None):
    ap = _parser()
    args = ap.parse_args(argv)
    if args.short_side < 8:
        ap.error(f"--short_side {args.short_side} is below 8")
    if args.shard_bytes < ALIGN:
        ap.error(f"--shard_bytes {args.shard_bytes} is below {ALIGN}")
    if os.path.exists(os.path.join(args.out, INDEX)):
        ap.error(f"{args.out} already holds a pack ({INDEX}); choose another --out")
    try:
        return pack(args.data_path, args.out, args.short_side, args.shard_bytes, args.num_workers)
    except FileNotFoundError as ex:                # an empty folder: exit code 2, like the other refusals
        ap.error(str(ex))


if __name__ == "__main__":
    main()
