#!/usr/bin/env python3
"""Linear-probe and k-NN evaluation of the VMAE tokenizer's features on the HIP kernels: what do the latents REPRESENT?

    python -m ldmae_amd.linear_probe --config_path configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml --ckpt vmae.pth \\
        --packed_data /data/imagenet_320 --packed_val /data/imagenet_val_320 --output_dir ./probe
    python -m ldmae_amd.linear_probe --config_path <cfg> --synthetic 256 --output_dir ./probe        # seeded stand-in data, no checkpoint

The encoder is frozen.  Features (--features latent: the posterior mean the DiT is trained on, what the reference's
MaskedAutoencoderViT.linear_probe pools; encoder: the tokens after the closing LayerNorm) are pooled (--pool mean: the reference's global pool;
flatten: the whole grid) and feed MAE's probe head, BatchNorm1d(affine=False, eps=1e-6) -> Linear, trained with LARS (the reference's
util/lars.py) under MAE's schedule (util/lr_sched.py: linear warm-up, half cosine, per iteration).  --aug rrc recomputes the features of
RandomResizedCrop(0.08 - 1) + flip views every epoch; --aug center extracts the centre-crop features once, keeps them on the device and
trains the head from them (epochs take seconds: use it for sweeps).  Validation is always the centre square of the short side over every
image.  --knn adds DINO's weighted k-NN classifier on the L2-normalised pooled features (bank: centre-crop training features).

The packs are the format of ldmae_amd/pack_images.py (labels and classes inside).  One process, one GPU: a data-parallel probe is out of
scope.  There is no CPU path.  Kernels: csrc/linprobe.hip; contracts and bounds: DESIGN.md section 23."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import yaml

_HERE = os.path.dirname(os.path.abspath(__file__))
for p in (_HERE, os.path.dirname(_HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

FEATURES, POOLS, AUGS, HEAD_NORMS = ("encoder", "latent"), ("mean", "flatten"), ("rrc", "center"), ("bn", "none")
JSON_KEYS = ("top1", "top5", "knn_top1", "knn_top5", "features", "pool", "epochs", "images")
BN_EPS, BN_MOMENTUM, HEAD_STD = 1e-6, 0.1, 0.01
RRC_SCALE = (0.08, 1.0)
KNN_QUERY_CHUNK, KNN_BANK_CHUNK = 4096, 8192
SYNTHETIC_CLASSES = 4


def log(msg):
    print(f"\033[34m[Linear probe]\033[0m {msg}", flush=True)


# ---------------------------------------------------------------------------------------------------- arguments and schedule
def build_parser():
    ap = argparse.ArgumentParser(description="Linear probe (MAE's recipe: BatchNorm + Linear, LARS) and weighted k-NN on frozen VMAE tokenizer features, "
                                             "on the HIP kernels.  Runs in ONE process on ONE GPU: a data-parallel probe is out of scope.")
    ap.add_argument("--config_path", type=str, default="configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml")
    ap.add_argument("--ckpt", type=str, default=None, help="vmae_pretrain checkpoint (default: vae.weight_path of the config)")
    ap.add_argument("--packed_data", type=str, default=None, help="training pack (python -m ldmae_amd.pack_images)")
    ap.add_argument("--packed_val", type=str, default=None, help="validation pack")
    ap.add_argument("--output_dir", type=str, default="./linear_probe")
    ap.add_argument("--synthetic", type=int, default=0, help="N seeded training images of 4 classes (and N / 2 validation images) written as packs "
                                                              "under --output_dir instead of --packed_data / --packed_val; random tokenizer weights allowed")
    ap.add_argument("--features", default="latent", choices=FEATURES)
    ap.add_argument("--pool", default="mean", choices=POOLS)
    ap.add_argument("--head_norm", default="bn", choices=HEAD_NORMS, help="bn: BatchNorm1d(affine=False, eps=1e-6) before the Linear (MAE); none: drop it")
    ap.add_argument("--aug", default="rrc", choices=AUGS)
    ap.add_argument("--batch_size", type=int, default=1024)
    ap.add_argument("--accum_iter", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=90)
    ap.add_argument("--warmup_epochs", type=int, default=10)
    ap.add_argument("--blr", type=float, default=0.1, help="lr = blr * batch_size * accum_iter / 256")
    ap.add_argument("--min_lr", type=float, default=0.0)
    ap.add_argument("--weight_decay", type=float, default=0.0)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--trust", type=float, default=0.001, help="LARS trust coefficient")
    ap.add_argument("--knn", dest="knn", action="store_true", default=True)
    ap.add_argument("--no-knn", dest="knn", action="store_false")
    ap.add_argument("--knn_k", type=int, default=20)
    ap.add_argument("--knn_T", type=float, default=0.07)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"], help="arithmetic of the frozen encoder")
    ap.add_argument("--resume", type=str, default=None, help="head.pt to continue from")
    ap.add_argument("--eval", action="store_true", help="only evaluate the head of --resume (default: <output_dir>/head.pt)")
    ap.add_argument("--seed", type=int, default=0)
    return ap


def check_args(args):
    """The refusals that need no device (argparse's `choices` cover the command line; this covers callers that build the namespace)."""
    from ldmae_amd import ops
    if args.features not in FEATURES:
        raise ValueError(f"--features {args.features!r}: one of {FEATURES}")
    if args.pool not in POOLS:
        raise ValueError(f"--pool {args.pool!r}: one of {POOLS}")
    if args.aug not in AUGS or args.head_norm not in HEAD_NORMS:
        raise ValueError(f"--aug {args.aug!r} (one of {AUGS}), --head_norm {args.head_norm!r} (one of {HEAD_NORMS})")
    if args.knn and not 1 <= args.knn_k <= ops.TOPK_MAX_K:
        raise ValueError(f"--knn_k {args.knn_k}: the top-k merge kernel keeps 1 .. TOPK_MAX_K = {ops.TOPK_MAX_K} neighbours")
    if args.knn and not args.knn_T > 0:
        raise ValueError(f"--knn_T {args.knn_T} must be positive")
    if args.batch_size < 2 or args.accum_iter < 1 or args.epochs < 0 or args.warmup_epochs < 0:
        raise ValueError(f"--batch_size {args.batch_size} (>= 2: BatchNorm), --accum_iter {args.accum_iter} (>= 1), --epochs {args.epochs}, "
                         f"--warmup_epochs {args.warmup_epochs} (>= 0)")


def scaled_lr(blr, batch_size, accum_iter=1):
    """MAE's main_linprobe.py: lr = blr * effective batch / 256."""
    return blr * batch_size * accum_iter / 256.0


def lr_at(it, iters_per_epoch, lr, min_lr, epochs, warmup_epochs):
    """util/lr_sched.py at iteration `it` (0-based, epoch = it / iters_per_epoch as a real number): linear warm-up from 0 over warmup_epochs,
    then min_lr + (lr - min_lr) * (1 + cos(pi (epoch - warmup) / (epochs - warmup))) / 2."""
    epoch = it / iters_per_epoch
    if epoch < warmup_epochs:
        return lr * epoch / warmup_epochs
    return min_lr + (lr - min_lr) * 0.5 * (1.0 + math.cos(math.pi * (epoch - warmup_epochs) / (epochs - warmup_epochs)))


# ---------------------------------------------------------------------------------------------------- synthetic packs
def synthetic_image(i, label, rng):
    """One learnable stand-in image: the class fixes the colour and the spatial frequency of a horizontal grating; size, phase and noise vary."""
    h, w = [(40, 56), (56, 40), (48, 48)][i % 3]                       # wide, tall and square: every branch of the centre crop
    colour = np.array([[230, 60, 60], [60, 230, 60], [60, 60, 230], [220, 220, 60]][label], dtype=np.float64)
    freq = (1, 2, 4, 8)[label]
    xs = np.arange(w)[None, :, None] / w
    wave = 0.5 + 0.5 * np.sin(2 * np.pi * (freq * xs + rng.uniform()))
    img = colour[None, None, :] * (0.55 + 0.45 * wave) + rng.normal(0.0, 6.0, (h, w, 3))
    return np.ascontiguousarray(np.clip(np.rint(np.broadcast_to(img, (h, w, 3))), 0, 255).astype(np.uint8))


def write_synthetic_pack(out, n, seed):
    """n seeded images of SYNTHETIC_CLASSES classes (label = i % classes) as a pack directory (format: ldmae_amd/pack_images.py)."""
    from safetensors.numpy import save_file
    from ldmae_amd.pack_images import ALIGN, FORMAT, INDEX, META, VERSION
    os.makedirs(out, exist_ok=True)
    rng = np.random.default_rng(seed)
    shard, offset, size = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros((n, 2), np.int32)
    label = (np.arange(n) % SYNTHETIC_CLASSES).astype(np.int64)
    cur = 0
    with open(os.path.join(out, "shard-00000.bin"), "wb") as f:
        for i in range(n):
            arr = synthetic_image(i, int(label[i]), rng)
            pad = -cur % ALIGN
            f.write(b"\0" * pad)
            cur += pad
            offset[i], size[i] = cur, arr.shape[:2]
            f.write(arr.tobytes())
            cur += arr.size
        pad = -cur % ALIGN
        f.write(b"\0" * pad)
        cur += pad
    with open(os.path.join(out, META), "w") as mf:
        json.dump({"format": FORMAT, "version": VERSION, "short_side": 40, "count": n, "shards": [cur],
                   "classes": [f"synthetic{c}" for c in range(SYNTHETIC_CLASSES)]}, mf)
    save_file({"shard": shard, "offset": offset, "size": size, "label": label}, os.path.join(out, INDEX), metadata={"format": FORMAT, "version": str(VERSION)})
    return out


# ---------------------------------------------------------------------------------------------------- features
class EpochSampler:
    """Indices 0 .. n - 1 in order, or (shuffle) in a permutation seeded by (seed, epoch): what PackedBatchLoader asks of a sampler."""
    rank = 0

    def __init__(self, n, shuffle, seed=0):
        self.n, self.shuffle, self.seed, self.epoch = int(n), shuffle, int(seed), 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return self.n

    def __iter__(self):
        if not self.shuffle:
            return iter(range(self.n))
        return iter(torch.randperm(self.n, generator=torch.Generator().manual_seed(self.seed * 1000003 + self.epoch)).tolist())


def pool_features(model, images, features, pool):
    """images [B, 3, S, S] -> f32 [B, D]: encode_features, then the token mean (ldmae_token_mean) or the flattened grid."""
    from ldmae_amd import ops
    if pool not in POOLS:
        raise ValueError(f"pool {pool!r}: one of {POOLS}")
    t = model.encode_features(images, features)
    if pool == "mean":
        return ops.token_mean(t)
    return t.float().reshape(t.shape[0], -1).contiguous()


def feature_width(model, features, pool):
    d = model.latent_dim if features == "latent" else model.pos_embed.shape[-1]
    return d if pool == "mean" else d * model.patch_embed.num_patches


def center_loader(ds, batch_size, input_size, device):
    from ldmae_amd.datasets.packed_images import PackedBatchLoader
    return PackedBatchLoader(ds, EpochSampler(len(ds), False), batch_size, input_size, 0, device, center=True, drop_last=False)


def extract_center(model, ds, args, input_size, device, what):
    """Centre-crop features of EVERY image of a pack, in pack order -> (f32 [n, D] on the device, labels i64 [n] on the host)."""
    n, d = len(ds), feature_width(model, args.features, args.pool)
    free = torch.cuda.mem_get_info(device)[0]
    if n * d * 4 > 0.8 * free:
        raise RuntimeError(f"the {what} features [{n}, {d}] f32 ({n * d * 4 / 2 ** 30:.1f} GiB) do not fit on the device ({free / 2 ** 30:.1f} GiB "
                           f"free): use --pool mean" + (", --aug rrc or --no-knn" if what == "training" else ""))
    out = torch.empty(n, d, dtype=torch.float32, device=device)
    done = 0
    for images, _ in center_loader(ds, min(args.batch_size, max(n, 1)), input_size, device):
        f = pool_features(model, images, args.features, args.pool)
        out[done:done + f.shape[0]].copy_(f)
        done += f.shape[0]
    assert done == n, (done, n)
    return out, torch.from_numpy(np.asarray(ds.labels, dtype=np.int64))


# ---------------------------------------------------------------------------------------------------- the head
class ProbeHead:
    """BatchNorm1d(affine=False) -> Linear on the kernels of csrc/linprobe.hip and the f32 GEMMs.  The master weight is kept PADDED to a
    multiple of 16 rows once (zero rows that stay zero: their gradient is zero), so no step re-pads it; everything is f32."""

    def __init__(self, width, num_classes, device, head_norm="bn", seed=0):
        if width % 16:
            raise ValueError(f"feature width {width}: the f32 GEMM of the head takes multiples of 16")
        self.D, self.C, self.Cp, self.device, self.head_norm = int(width), int(num_classes), -(-int(num_classes) // 16) * 16, device, head_norm
        w = torch.zeros(self.Cp, self.D)
        torch.nn.init.trunc_normal_(w[:self.C], std=HEAD_STD, generator=torch.Generator().manual_seed(seed))
        self.weight, self.bias = w.to(device), torch.zeros(self.Cp, device=device)
        self.run_mean, self.run_var = torch.zeros(self.D, device=device), torch.ones(self.D, device=device)
        self.mu_weight, self.mu_bias = torch.zeros_like(self.weight), torch.zeros_like(self.bias)
        self.grad_weight, self.grad_bias = torch.zeros_like(self.weight), torch.zeros_like(self.bias)
        self.norms = torch.empty(2, device=device)
        self._dlogits = {}

    def _norm(self, x, training):
        from ldmae_amd import ops
        if self.head_norm == "none":
            return x
        return ops.bn1d_fwd(x, self.run_mean, self.run_var, training=training, eps=BN_EPS, momentum=BN_MOMENTUM)

    def logits(self, x, training=False):
        """x [B, D] -> (xhat, logits [B, Cp]; the first C columns count)."""
        from ldmae_amd import ops
        xh = self._norm(x, training)
        if ops.thin_ok(self.Cp, self.D):
            return xh, ops.thin_nt(xh, self.weight, self.bias)
        return xh, ops.gemm_nt(xh, self.weight, self.bias)

    def accumulate(self, x, labels, grad_scale, first):
        """Forward + backward of one micro-batch; gradients accumulate over micro-batches (first: they are overwritten).  -> (loss [B], rank [B])."""
        from ldmae_amd import ops
        B = x.shape[0]
        xh, lg = self.logits(x, training=True)
        dl = self._dlogits.get(B)
        if dl is None:                                             # the padded columns are zero once and never written
            dl = self._dlogits[B] = torch.zeros(B, self.Cp, dtype=torch.float32, device=self.device)
        loss, rank, _ = ops.softmax_xent(lg, labels, self.C, grad_scale=grad_scale, dlogits=dl)
        if first and ops.thin_ok(self.Cp, self.D):
            gw, gb = ops.thin_tn(dl, xh, with_bias=True)
            self.grad_weight, self.grad_bias = gw, gb
        else:
            ops.gemm_tn(dl, xh, out=self.grad_weight, beta=0.0 if first else 1.0)
            ops.colsum(dl, out=self.grad_bias, beta=0.0 if first else 1.0)
        return loss, rank

    def step(self, lr, weight_decay, momentum, trust):
        from ldmae_amd import ops
        ops.lars_norms(self.weight, self.grad_weight, weight_decay, out=self.norms)
        ops.lars_step(self.weight, self.grad_weight, self.mu_weight, lr, self.norms, weight_decay, momentum, trust)
        ops.lars_step(self.bias, self.grad_bias, self.mu_bias, lr, None, weight_decay, momentum, trust)

    def state_dict(self, epoch):
        c = self.C
        return {"weight": self.weight[:c].cpu(), "bias": self.bias[:c].cpu(), "run_mean": self.run_mean.cpu(), "run_var": self.run_var.cpu(),
                "mu_weight": self.mu_weight[:c].cpu(), "mu_bias": self.mu_bias[:c].cpu(), "epoch": int(epoch), "head_norm": self.head_norm}

    def load_state_dict(self, sd):
        c = self.C
        if tuple(sd["weight"].shape) != (c, self.D) or sd.get("head_norm", self.head_norm) != self.head_norm:
            raise ValueError(f"head.pt holds a {tuple(sd['weight'].shape)} head (head_norm {sd.get('head_norm')!r}); this run needs ({c}, {self.D}), "
                             f"{self.head_norm!r}")
        for name in ("weight", "bias", "mu_weight", "mu_bias"):
            getattr(self, name).zero_()
            getattr(self, name)[:c].copy_(sd[name])
        self.run_mean.copy_(sd["run_mean"])
        self.run_var.copy_(sd["run_var"])
        return int(sd["epoch"])


def evaluate_head(head, feats, labels_dev, batch_size):
    """Validation on cached centre-crop features -> (top-1 count, top-5 count, loss sum) as device scalars."""
    from ldmae_amd import ops
    t1 = torch.zeros((), dtype=torch.int64, device=feats.device)
    t5, ls = torch.zeros_like(t1), torch.zeros((), dtype=torch.float64, device=feats.device)
    for s in range(0, feats.shape[0], batch_size):
        _, lg = head.logits(feats[s:s + batch_size], training=False)
        loss, rank, _ = ops.softmax_xent(lg, labels_dev[s:s + batch_size], head.C)
        t1 += (rank == 0).sum()
        t5 += (rank < 5).sum()
        ls += loss.double().sum()
    return t1, t5, ls


def knn_eval(bank, bank_labels, queries, query_labels, num_classes, k, temperature):
    """DINO's weighted k-NN on L2-normalised features: similarities by chunks of bank rows (ops.pairwise_logits), merged into per-query
    top-k lists (ops.topk_merge), then the vote (ops.knn_vote).  -> (top-1 fraction, top-5 fraction)."""
    from ldmae_amd import ops
    dev = bank.device
    if num_classes > ops.KNN_VOTE_MAX_C:
        raise ValueError(f"--knn with {num_classes} classes: the vote kernel holds a query's class scores in LDS, KNN_VOTE_MAX_C = {ops.KNN_VOTE_MAX_C} fit")
    bank, queries = ops.l2_normalize(bank), ops.l2_normalize(queries)
    bl, ql = ops.check_labels(bank_labels, num_classes, dev, "bank labels"), ops.check_labels(query_labels, num_classes, dev, "query labels")
    t1 = torch.zeros((), dtype=torch.int64, device=dev)
    t5 = torch.zeros_like(t1)
    for q0 in range(0, queries.shape[0], KNN_QUERY_CHUNK):
        q = queries[q0:q0 + KNN_QUERY_CHUNK]
        vals, idx = ops.topk_empty(q.shape[0], k, dev)
        for b0 in range(0, bank.shape[0], KNN_BANK_CHUNK):
            ops.topk_merge(ops.pairwise_logits(q, bank[b0:b0 + KNN_BANK_CHUNK]), b0, vals, idx)
        rank = ops.knn_vote(vals, idx, bl, ql[q0:q0 + KNN_QUERY_CHUNK], num_classes, temperature)
        t1 += (rank == 0).sum()
        t5 += ((rank >= 0) & (rank < 5)).sum()
    n = queries.shape[0]
    return int(t1) / n, int(t5) / n


# ---------------------------------------------------------------------------------------------------- the driver
def load_tokenizer(args, cfg, device):
    """The tokenizer as evaluate_tokenizer.py builds and loads it; random weights only with --synthetic."""
    from ldmae_amd.tokenizer import models_mae
    torch.manual_seed(args.seed)
    model = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, kl_loss_weight=True, smooth_output=True,
                                                img_size=cfg["data"].get("image_size", 256))
    chkpt = args.ckpt or cfg["vae"].get("weight_path")
    if chkpt and os.path.exists(chkpt):
        log(str(model.load_state_dict(torch.load(chkpt, map_location="cpu")["model"], strict=False)))
    elif not args.synthetic:
        raise FileNotFoundError(f"tokenizer checkpoint {chkpt!r} not found (--ckpt, or vae.weight_path of the config)")
    model = model.to(device).eval()
    if args.precision == "bf16":
        model.set_precision(torch.bfloat16)
    return model


def linear_probe(args, cfg, model=None):
    check_args(args)
    if not torch.cuda.is_available():
        raise RuntimeError("linear_probe needs a GPU: there is no CPU path in this package")
    from ldmae_amd import ops
    from ldmae_amd.datasets.packed_images import PackedBatchLoader, PackedImages
    device = torch.device("cuda", int(os.environ.get("LDMAE_DEVICE", 0)))
    torch.cuda.set_device(device)
    os.makedirs(args.output_dir, exist_ok=True)
    if args.synthetic:
        packs = []
        for name, n, seed in (("synthetic_train", args.synthetic, args.seed), ("synthetic_val", max(args.synthetic // 2, SYNTHETIC_CLASSES), args.seed + 1)):
            root = os.path.join(args.output_dir, name)
            packs.append(root if os.path.exists(os.path.join(root, "index.safetensors")) else write_synthetic_pack(root, n, seed))
        train_root, val_root = packs
    else:
        train_root, val_root = args.packed_data, args.packed_val
        if not val_root or not (train_root or (args.eval and not args.knn)):
            raise ValueError("--packed_val and --packed_data are needed (or --synthetic N); --eval --no-knn needs only --packed_val")
    val = PackedImages(val_root)
    train = PackedImages(train_root) if train_root else None
    classes = (train or val).classes
    num_classes = len(classes) if classes else int(max((train or val).labels.max(), val.labels.max())) + 1
    if model is None:
        model = load_tokenizer(args, cfg, device)
    input_size = model.img_size if hasattr(model, "img_size") else cfg["data"].get("image_size", 256)
    head = ProbeHead(feature_width(model, args.features, args.pool), num_classes, device, args.head_norm, args.seed)
    start_epoch = 0
    resume = args.resume or (os.path.join(args.output_dir, "head.pt") if args.eval else None)
    if resume:
        start_epoch = head.load_state_dict(torch.load(resume, map_location="cpu"))
        log(f"resumed {resume} at epoch {start_epoch}")

    with torch.no_grad():
        val_feats, val_labels = extract_center(model, val, args, input_size, device, "validation")
        val_labels_dev = ops.check_labels(val_labels, num_classes, device, "validation labels")
        need_bank = train is not None and (args.knn or (args.aug == "center" and not args.eval))
        bank, bank_labels = extract_center(model, train, args, input_size, device, "training") if need_bank else (None, None)

        def validate():
            t1, t5, ls = evaluate_head(head, val_feats, val_labels_dev, args.batch_size)
            return int(t1) / len(val), int(t5) / len(val), float(ls) / len(val)

        top1, top5, _ = validate() if (args.eval or start_epoch >= args.epochs) else (None, None, None)
        if not args.eval and start_epoch < args.epochs:
            lr = scaled_lr(args.blr, args.batch_size, args.accum_iter)
            if args.aug == "rrc":
                sampler = EpochSampler(len(train), True, args.seed)
                loader = PackedBatchLoader(train, sampler, args.batch_size, input_size, args.seed, device, scale=RRC_SCALE)
                micro = len(loader)
            else:
                bank_labels_dev = ops.check_labels(bank_labels, num_classes, device, "training labels")
                micro = len(train) // args.batch_size
            steps = micro // args.accum_iter                              # optimizer steps per epoch; a trailing partial group is dropped
            if steps < 1:
                raise ValueError(f"{len(train)} training images give no step of {args.batch_size} x {args.accum_iter}")
            grad_scale = 1.0 / (args.batch_size * args.accum_iter)
            for epoch in range(start_epoch, args.epochs):
                loss_sum = torch.zeros((), dtype=torch.float64, device=device)
                if args.aug == "rrc":
                    sampler.set_epoch(epoch)
                    batches = ((pool_features(model, images, args.features, args.pool), labels) for images, labels in loader)
                else:
                    perm = torch.randperm(len(train), generator=torch.Generator().manual_seed(args.seed * 1000003 + epoch)).to(device)
                    batches = ((ops.gather_rows(bank[None], perm[None, j * args.batch_size:(j + 1) * args.batch_size])[0],
                                bank_labels_dev[perm[j * args.batch_size:(j + 1) * args.batch_size]]) for j in range(micro))
                for j, (x, labels) in enumerate(batches):
                    if j >= steps * args.accum_iter:
                        break
                    loss, _ = head.accumulate(x, labels, grad_scale, first=j % args.accum_iter == 0)
                    loss_sum += loss.double().sum()
                    if (j + 1) % args.accum_iter == 0:
                        it = epoch * steps + j // args.accum_iter
                        head.step(lr_at(it, steps, lr, args.min_lr, args.epochs, args.warmup_epochs), args.weight_decay, args.momentum, args.trust)
                train_loss = float(loss_sum) / (steps * args.accum_iter * args.batch_size)
                top1, top5, val_loss = validate()
                log(f"epoch {epoch + 1}/{args.epochs}: train loss {train_loss:.4f}  val loss {val_loss:.4f}  val top-1 {top1:.4f}  top-5 {top5:.4f}")
                print(json.dumps({"metric": "linear_probe_epoch", "epoch": epoch + 1, "train_loss": train_loss, "val_loss": val_loss, "top1": top1,
                                  "top5": top5}), flush=True)
                torch.save(head.state_dict(epoch + 1), os.path.join(args.output_dir, "head.pt"))
        knn1 = knn5 = None
        if args.knn and bank is not None:
            knn1, knn5 = knn_eval(bank, bank_labels, val_feats, val_labels, num_classes, args.knn_k, args.knn_T)
            log(f"k-NN (k = {args.knn_k}, T = {args.knn_T}): top-1 {knn1:.4f}  top-5 {knn5:.4f}")
    res = {"top1": top1, "top5": top5, "knn_top1": knn1, "knn_top5": knn5, "features": args.features, "pool": args.pool,
           "epochs": max(start_epoch, args.epochs) if not args.eval else start_epoch, "images": len(val)}
    print(json.dumps({"metric": "linear_probe", **res}), flush=True)
    return res


def main(argv=None):
    args = build_parser().parse_args(argv)
    with open(args.config_path) as f:
        cfg = yaml.safe_load(f)
    from ldmae_amd.evaluate_tokenizer import model_type_of
    model_type_of(cfg)                  # refuse an SD-VAE config before touching the GPU
    return linear_probe(args, cfg)


if __name__ == "__main__":
    main()
