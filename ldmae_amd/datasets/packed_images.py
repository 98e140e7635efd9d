"""Packed image shards (written by `python -m ldmae_amd.pack_images`) and the batch loader that does the VMAE training transform on the device.

PackedImages(dir) reads the index and memory-maps the shards.  PackedBatchLoader replaces DataLoader + RandomResizedCropFlip for such a pack: per
batch a background THREAD (a GPU process must not fork workers: DESIGN.md section 8a) copies the batch's images out of the memory map into a pinned
staging buffer, draws the crop boxes and flips on the host by RandomResizedCropFlip's own algorithm, and uploads bytes and tables on a side stream;
the consumer's stream then runs ONE kernel (ops.crop_resize_flip) that crops, resamples (PIL's antialiased bicubic), flips and normalises the batch.
A sample is a function of (pack, seed, rank, epoch, position in the epoch): the draws of batch k come from a torch.Generator seeded from
(seed, rank, epoch, k), so `prefetch` changes only how far the thread runs ahead."""
import hashlib
import json
import os
import queue
import threading

import numpy as np
import torch

ALIGN = 16


class PackedImages(torch.utils.data.Dataset):
    """A pack directory (format: ldmae_amd/pack_images.py).  len(); labels i64 [N]; sizes i32 [N, 2] = (h, w); classes; short_side;
    image(i) -> [h, w, 3] uint8 view of the memory map; ds[i] -> (that view, label)."""

    def __init__(self, root):
        from safetensors.numpy import load_file
        from ldmae_amd.pack_images import FORMAT, INDEX, META, VERSION
        self.root = root
        if not os.path.exists(os.path.join(root, INDEX)) or not os.path.exists(os.path.join(root, META)):
            raise FileNotFoundError(f"{root} is not a pack: no {INDEX} / {META} (write one with `python -m ldmae_amd.pack_images`)")
        with open(os.path.join(root, META)) as f:
            meta = json.load(f)
        if meta.get("format") != FORMAT or int(meta.get("version", -1)) != VERSION:
            raise ValueError(f"{root}: format {meta.get('format')!r} version {meta.get('version')!r}, this reader takes {FORMAT!r} version {VERSION}")
        idx = load_file(os.path.join(root, INDEX))
        self.shard, self.offset, self.sizes, self.labels = idx["shard"], idx["offset"], idx["size"], idx["label"]
        self.classes, self.short_side, self.shard_bytes = list(meta["classes"]), int(meta["short_side"]), [int(n) for n in meta["shards"]]
        if not (len(self.shard) == len(self.offset) == len(self.sizes) == len(self.labels) == int(meta["count"])):
            raise ValueError(f"{root}: the index has {len(self.shard)} rows, {META} counts {meta['count']}")
        self.nbytes = 3 * self.sizes[:, 0].astype(np.int64) * self.sizes[:, 1].astype(np.int64)
        self._maps = [np.memmap(os.path.join(root, f"shard-{k:05d}.bin"), dtype=np.uint8, mode="r") for k in range(len(self.shard_bytes))]
        for k, m in enumerate(self._maps):
            if m.shape[0] != self.shard_bytes[k]:
                raise ValueError(f"{root}: shard {k} has {m.shape[0]} bytes, {META} says {self.shard_bytes[k]}")
        ends = self.offset + self.nbytes
        if len(self) and (int(self.offset.min()) < 0 or bool((ends > np.asarray(self.shard_bytes, dtype=np.int64)[self.shard]).any())):
            raise ValueError(f"{root}: an index row points outside its shard")

    def __len__(self):
        return len(self.shard)

    def raw(self, i):
        """The 3 h w bytes of image i (a view of the memory map)."""
        o = int(self.offset[i])
        return self._maps[int(self.shard[i])][o:o + int(self.nbytes[i])]

    def image(self, i):
        h, w = self.sizes[i]
        return self.raw(i).reshape(int(h), int(w), 3)

    def __getitem__(self, i):
        return self.image(i), int(self.labels[i])


def batch_seed(seed, rank, epoch, batch):
    """63-bit generator seed of one batch: a hash of the four numbers, so neighbouring batches / epochs / ranks share nothing."""
    return int.from_bytes(hashlib.sha256(f"ldmae-packed:{seed}:{rank}:{epoch}:{batch}".encode()).digest()[:8], "little") >> 1


def draw_table(sizes, input_size, scale, ratio, generator):
    """Crop boxes and flips of one batch: per sample RandomResizedCropFlip._box(w, h) followed by one flip draw, all from `generator`.
    sizes [B, 2] = (h, w) -> geom i32 [B, 8] = (h, w, top, left, ch, cw, flip, 0)."""
    from ldmae_amd.vmae_pretrain import RandomResizedCropFlip
    tr = RandomResizedCropFlip(input_size, scale=scale, ratio=ratio)
    rows = []
    for h, w in np.asarray(sizes).tolist():
        top, left, ch, cw = tr._box(w, h, generator=generator)
        flip = bool(torch.rand(1, generator=generator) < 0.5)
        rows.append([h, w, top, left, ch, cw, int(flip), 0])
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 8)


def center_table(sizes):
    """The same table without a draw: the centre square of the short side (top = (h - s) // 2, left = (w - s) // 2, s = min(h, w)), no flip --
    the evaluation transform of the linear probe (resized to the input size by the same kernel)."""
    rows = []
    for h, w in np.asarray(sizes).tolist():
        s = min(h, w)
        rows.append([h, w, (h - s) // 2, (w - s) // 2, s, s, 0, 0])
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 8)


class _Slot:
    """One batch in flight: pinned staging + tables, their device copies, and the two events that guard their reuse.  Every DEVICE buffer is
    allocated with the loader's side stream current, so it comes from that stream's pool of the caching allocator: a block the training loop has
    just freed (and whose last kernels may still be queued on its stream) is never handed to a side-stream copy.  The consumer's stream reads the
    buffers only between the `uploaded` wait and the `consumed` record, and a buffer is reused or freed only after `consumed` has completed."""

    def __init__(self, batch_size, device, side):
        self.device, self.side = device, side
        self.stage = self.blob = None
        self.offsets_h = torch.empty(batch_size, dtype=torch.int64).pin_memory()
        self.geom_h = torch.empty(batch_size, 8, dtype=torch.int32).pin_memory()
        with torch.cuda.stream(side):
            self.offsets_d = torch.empty(batch_size, dtype=torch.int64, device=device)
            self.geom_d = torch.empty(batch_size, 8, dtype=torch.int32, device=device)
        self.uploaded = torch.cuda.Event()         # recorded on the side stream after the copies
        self.consumed = torch.cuda.Event()         # recorded on the consumer's stream after the kernel
        self.used = False

    def reserve(self, nbytes):
        if self.stage is None or self.stage.numel() < nbytes:
            cap = (nbytes + nbytes // 4 + 4095) // 4096 * 4096
            self.stage = torch.empty(cap, dtype=torch.uint8).pin_memory()
            with torch.cuda.stream(self.side):             # the old blob (its last reader finished: `consumed`) goes back to the side stream's pool
                self.blob = torch.empty(cap, dtype=torch.uint8, device=self.device)


class PackedBatchLoader:
    """Iterates (images [B, 3, S, S] on `device`, labels i64 [B] on the host) over `sampler`'s indices, dropping the last partial batch unless
    drop_last=False (then it is yielded with its own, smaller B).  center=True: no draw -- every sample is the centre square of its short side,
    unflipped (center_table).
    The epoch is `sampler.epoch` (DistributedSampler.set_epoch) unless set_epoch() is called here; the rank is `sampler.rank` unless given.
    `last_table` describes the batch last yielded: {"index" i64 [B], "offset" i64 [B], "geom" i32 [B, 8], "epoch", "batch"} (host tensors)."""

    def __init__(self, dataset, sampler, batch_size, input_size, seed, device, scale=(0.75, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), prefetch=2,
                 out_dtype=torch.float32, mean=0.5, std=0.5, rank=None, center=False, drop_last=True):
        self.dataset, self.sampler, self.batch_size, self.input_size, self.seed = dataset, sampler, int(batch_size), int(input_size), int(seed)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"PackedBatchLoader runs its transform on a HIP device (no CPU fallback); got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.scale, self.ratio, self.prefetch, self.out_dtype, self.mean, self.std = scale, ratio, max(1, int(prefetch)), out_dtype, mean, std
        self.rank = int(rank if rank is not None else getattr(sampler, "rank", 0))
        self.epoch, self.last_table = None, None
        self.center, self.drop_last = bool(center), bool(drop_last)
        self._side, self._slots, self._active = None, None, False        # made on the first iteration, kept for the loader's life

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.sampler) // self.batch_size if self.drop_last else -(-len(self.sampler) // self.batch_size)

    # ---- producer: everything that needs no kernel, for batch k into slot k % prefetch
    def _fill(self, slot, idx, epoch, k):
        ds = self.dataset
        nbytes = ds.nbytes[idx]
        starts = np.zeros(len(idx), dtype=np.int64)
        pos = 0
        for b, n in enumerate(nbytes):
            starts[b] = pos
            pos += (int(n) + ALIGN - 1) // ALIGN * ALIGN
        slot.reserve(pos)
        stage = slot.stage.numpy()
        for b, i in enumerate(idx):
            stage[starts[b]:starts[b] + nbytes[b]] = ds.raw(int(i))
        g = torch.Generator().manual_seed(batch_seed(self.seed, self.rank, epoch, k))
        geom = center_table(ds.sizes[idx]) if self.center else draw_table(ds.sizes[idx], self.input_size, self.scale, self.ratio, g)
        offsets = torch.from_numpy(starts)
        from ldmae_amd import ops
        ops.check_crop_table(offsets, geom, pos)              # the kernel trusts the device copy of these
        slot.offsets_h[:len(idx)].copy_(offsets)
        slot.geom_h[:len(idx)].copy_(geom)
        slot.nbytes, slot.rows = pos, len(idx)
        return {"index": torch.from_numpy(np.asarray(idx, dtype=np.int64)), "offset": offsets, "geom": geom, "epoch": epoch, "batch": k}

    def _produce(self, batches, epoch, free_q, ready_q, stop):
        try:
            torch.cuda.set_device(self.device)
            side = self._side
            for k, idx in enumerate(batches):
                slot = free_q.get()
                if stop.is_set() or slot is None:
                    return
                if slot.used:
                    slot.consumed.synchronize()            # the kernel that read this slot's device buffers is done: staging and buffers are free
                table = self._fill(slot, idx, epoch, k)
                with torch.cuda.stream(side):
                    slot.blob[:slot.nbytes].copy_(slot.stage[:slot.nbytes], non_blocking=True)
                    slot.offsets_d.copy_(slot.offsets_h, non_blocking=True)
                    slot.geom_d.copy_(slot.geom_h, non_blocking=True)
                    slot.uploaded.record(side)
                labels = torch.from_numpy(self.dataset.labels[idx].astype(np.int64))
                ready_q.put((slot, table, labels))
            ready_q.put(None)
        except BaseException as ex:                            # handed to the consumer, which re-raises it
            ready_q.put(ex)

    def __iter__(self):
        from ldmae_amd import ops
        epoch = self.epoch if self.epoch is not None else int(getattr(self.sampler, "epoch", 0))
        order = np.fromiter(iter(self.sampler), dtype=np.int64)
        nb = len(order) // self.batch_size if self.drop_last else -(-len(order) // self.batch_size)
        batches = [order[k * self.batch_size:(k + 1) * self.batch_size] for k in range(nb)]
        if self._active:
            raise RuntimeError("PackedBatchLoader: one iteration at a time (the staging slots belong to the loader)")
        if self._slots is None:                    # once per loader: pinned staging and device buffers are not reallocated every epoch
            self._side = torch.cuda.Stream(self.device)
            self._slots = [_Slot(self.batch_size, self.device, self._side) for _ in range(self.prefetch)]
        free_q, ready_q, stop = queue.Queue(), queue.Queue(), threading.Event()
        for slot in self._slots:
            free_q.put(slot)
        self._active = True
        th = threading.Thread(target=self._produce, args=(batches, epoch, free_q, ready_q, stop), daemon=True, name="packed-batch-loader")
        th.start()
        try:
            while True:
                item = ready_q.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                slot, table, labels = item
                with torch.cuda.device(self.device):
                    cur = torch.cuda.current_stream()
                    cur.wait_event(slot.uploaded)
                    out = ops.crop_resize_flip(slot.blob[:slot.nbytes], slot.offsets_d[:slot.rows], slot.geom_d[:slot.rows], self.input_size, self.mean, self.std, self.out_dtype)
                    slot.consumed.record(cur)
                    for t in (slot.blob, slot.offsets_d, slot.geom_d):      # side-stream memory read on this stream: should the loader be dropped with the
                        t.record_stream(cur)                                # kernel still queued, the allocator holds the blocks back until it has run
                slot.used = True
                free_q.put(slot)
                self.last_table = table
                yield out, labels
        finally:
            stop.set()
            free_q.put(None)
            th.join()
            self._active = False
