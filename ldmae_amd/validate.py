#!/usr/bin/env python3
"""Held-out validation of the DiT: `python -m ldmae_amd.validate --config CFG --ckpt CKPT --data DIR` (or `--synthetic N`).

The flow-matching loss mean_flat((model(xt, t, y) - ut) ** 2) on latents the model has not seen, with the noise and the time of validation
sample i a function of (seed, i) alone: t_i is a low-discrepancy sequence in i, the posterior draw and x0 are the named Philox draws
normal(seed, 2 i) and normal(seed, 2 i + 1), generated inside the kernel that builds (xt, ut) (ops.fm_valid_plan; the loss is ops.row_mse).
Two checkpoints are therefore compared on the same question, whatever the batch size, the number of ranks or the state of any other random
stream.  Prints the uniform-in-t mean with its standard error, the mean per time bin, under transport.use_lognorm the importance-weighted
mean that estimates the expected TRAINING loss, and one JSON line.  With --snapshots / --sigma_rels it rebuilds one EMA per width from
post-hoc EMA snapshots (posthoc_ema.reconstruct) and validates each.  Only the MSE term is reported, as the training log reports it.
The latents are normalised with the statistics of the TRAINING set (--stats, default <training latent directory>/latents_stats.pt); they
are never computed here.  Nothing is downloaded: a checkpoint or a directory that is not on disk is an error."""
import argparse
import json
import math
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for p in (_HERE, os.path.dirname(_HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = 0.6180339887498949           # frac of the golden ratio: i -> frac(0.5 + i GOLDEN) is low-discrepancy over every prefix
WEIGHTS = ("model", "ema", "both")
VALID_KEYS = {"every", "num", "batch", "seed", "bins", "weights"}


# ----------------------------------------------------------------------------- host arithmetic (no device, tested on the CPU)
def sample_times(indices, interval=(0.0, 1.0)):
    """t_i = lo + (hi - lo) frac(0.5 + i GOLDEN) in f64, rounded to f32: a function of i (and the interval) only."""
    lo, hi = float(interval[0]), float(interval[1])
    u = 0.5 + np.asarray(indices, dtype=np.float64) * GOLDEN
    return (lo + (hi - lo) * (u - np.floor(u))).astype(np.float32)


def check_interval(interval):
    lo, hi = float(interval[0]), float(interval[1])
    if not (0.0 <= lo < hi <= 1.0):
        raise ValueError(f"interval ({lo}, {hi}): needs 0 <= lo < hi <= 1")
    return lo, hi


def lognorm_weights(t):
    """Density of the logit-normal(0, 1) time the training objective draws (transport.sample_logit_normal), phi(logit t) / (t (1 - t)), in
    f64; 0 at t = 0 and t = 1 (its limit there)."""
    t = np.asarray(t, dtype=np.float64)
    w = np.zeros_like(t)
    ok = (t > 0) & (t < 1)
    tt = t[ok]
    z = np.log(tt) - np.log1p(-tt)
    w[ok] = np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) / (tt * (1.0 - tt))
    return w


def bin_edges(bins, interval=(0.0, 1.0)):
    lo, hi = float(interval[0]), float(interval[1])
    return lo + (hi - lo) * np.arange(bins + 1, dtype=np.float64) / bins


def bin_index(t, bins, interval=(0.0, 1.0)):
    """Equal-width bins over the interval: bin k holds edges[k] <= t < edges[k + 1], the last one its right end too."""
    lo, hi = float(interval[0]), float(interval[1])
    k = np.floor((np.asarray(t, dtype=np.float64) - lo) / (hi - lo) * bins).astype(np.int64)
    return np.clip(k, 0, bins - 1)


def _mean_sem(x):
    n = x.size
    if n == 0:
        return None, None
    return float(x.mean()), (float(x.std(ddof=1) / math.sqrt(n)) if n > 1 else None)


def report(losses, t, bins=10, interval=(0.0, 1.0), use_lognorm=False):
    """The figures of one evaluation from the per-sample losses (f64, ordered by index) and their times."""
    losses, t = np.asarray(losses, dtype=np.float64), np.asarray(t, dtype=np.float64)
    mean, sem = _mean_sem(losses)
    edges, k = bin_edges(bins, interval), bin_index(t, bins, interval)
    rows = []
    for b in range(bins):
        m, s = _mean_sem(losses[k == b])
        rows.append({"lo": float(edges[b]), "hi": float(edges[b + 1]), "count": int((k == b).sum()), "mean": m, "sem": s})
    out = {"num": int(losses.size), "loss": mean, "sem": sem, "bins": rows}
    if use_lognorm:
        w = lognorm_weights(t)
        sw = float(w.sum())
        if sw > 0:
            wm = float((w * losses).sum() / sw)
            out["loss_train_weighted"] = wm
            out["sem_train_weighted"] = float(math.sqrt(float((w * w * (losses - wm) ** 2).sum())) / sw) if losses.size > 1 else None
        else:
            out["loss_train_weighted"] = out["sem_train_weighted"] = None
    return out


def rank_indices(num, rank, world):
    """The validation indices of one rank: i % world == rank."""
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} of {world}")
    return np.arange(rank, num, world, dtype=np.int64)


def merge_by_index(parts, num):
    """[(indices, losses)] of every rank -> the f64 losses ordered by index; every index 0 .. num - 1 must come exactly once."""
    out = np.full(num, np.nan, dtype=np.float64)
    seen = np.zeros(num, dtype=np.int64)
    for idx, loss in parts:
        idx, loss = np.asarray(idx, dtype=np.int64), np.asarray(loss, dtype=np.float64)
        if idx.shape != loss.shape or (idx.size and (idx.min() < 0 or idx.max() >= num)):
            raise ValueError("merge_by_index: indices and losses of a rank do not match, or an index is outside 0 .. num - 1")
        np.add.at(seen, idx, 1)
        out[idx] = loss
    if (seen != 1).any():
        raise ValueError(f"merge_by_index: {int((seen == 0).sum())} indices missing and {int((seen > 1).sum())} repeated of {num}")
    return out


def format_report(name, rep):
    se = lambda s: "n/a" if s is None else f"{s:.5f}"          # noqa: E731
    lines = [f"{name}: {rep['num']} samples, loss {rep['loss']:.5f} +- {se(rep['sem'])} (uniform in t)"]
    if rep.get("loss_train_weighted") is not None:
        lines.append(f"{name}: expected training loss (logit-normal t, importance-weighted) {rep['loss_train_weighted']:.5f} +- "
                     f"{se(rep['sem_train_weighted'])}")
    for r in rep["bins"]:
        m = "     n/a" if r["mean"] is None else f"{r['mean']:8.5f}"
        lines.append(f"  t in [{r['lo']:.3f}, {r['hi']:.3f}{']' if r is rep['bins'][-1] else ')'}  n {r['count']:6d}  loss {m} +- {se(r['sem'])}")
    return "\n".join(lines)


def training_latent_dir(data_cfg):
    """The directory training reads its latents (and their statistics) from: train_accum.make_loader's rule."""
    return data_cfg["data_path"] + ("_sample" if "sample" in data_cfg else "")


def valid_config(cfg, per_gpu=None):
    """The opt-in ``train.valid: {every, num, batch, seed, bins, weights}`` (not a reference key) with its defaults filled in, or None when the
    key is absent.  It needs data.valid_path."""
    tr = cfg["train"]
    v = tr.get("valid")
    if v is None:
        return None
    if not isinstance(v, dict) or set(v) - VALID_KEYS:
        raise ValueError(f"train.valid must be a mapping with keys out of {sorted(VALID_KEYS)}; got {v!r}")
    if "valid_path" not in cfg["data"]:
        raise ValueError("train.valid needs data.valid_path: the directory of held-out latent shards")
    out = {"every": v.get("every", tr.get("ckpt_every")), "num": v.get("num", 10000), "batch": v.get("batch", per_gpu), "seed": v.get("seed", 0),
           "bins": v.get("bins", 10), "weights": v.get("weights", "both")}
    for k in ("every", "num", "batch", "bins"):
        if not isinstance(out[k], int) or isinstance(out[k], bool) or out[k] < 1:
            raise ValueError(f"train.valid.{k} must be a positive integer; got {out[k]!r}")
    if not isinstance(out["seed"], int) or isinstance(out["seed"], bool) or out["seed"] < 0:
        raise ValueError(f"train.valid.seed must be a non-negative integer; got {out['seed']!r}")
    if out["weights"] not in WEIGHTS:
        raise ValueError(f"train.valid.weights must be one of {', '.join(WEIGHTS)}; got {out['weights']!r}")
    return out


def training_plan(cfg, per_gpu=None):
    """What the train driver does about validation: (settings or None, the line it logs or None)."""
    v = valid_config(cfg, per_gpu)
    if v is not None:
        return v, (f"Validation every {v['every']} steps: {v['num']} samples of {cfg['data']['valid_path']!r}, batch {v['batch']}, seed {v['seed']}, "
                   f"weights {v['weights']}")
    if "valid_path" in cfg["data"]:
        # train_accum.py:148-163,288-297 builds a validation loader and calls an `evaluate` that the reference never defines (NameError at the
        # first checkpoint step); no shipped config sets the key.  Said once instead of dying after ckpt_every steps.
        return None, f"data.valid_path={cfg['data']['valid_path']!r} is ignored: the reference's validation pass calls an undefined evaluate()"
    return None, None


# ----------------------------------------------------------------------------- sources
class ShardSource:
    """Latent shards in the ImgLatentDataset format, read with ds._read (never __getitem__: its flip pick draws from numpy's global stream,
    which the training objective shares).  The unflipped copy; normalisation with the statistics handed in, never the directory's own."""

    def __init__(self, data_dir, data_cfg, stats_path=None):
        import torch
        from ldmae_amd.datasets.img_latent_dataset import ImgLatentDataset
        self.ds = ImgLatentDataset(data_dir=data_dir, latent_norm=False, latent_multiplier=data_cfg.get("latent_multiplier", 0.18215),
                                   sample=data_cfg.get("sample", False), raw=True)
        if len(self.ds) == 0:
            raise SystemExit(f"{data_dir!r} holds no *.safetensors shard")
        self.sample, self.multiplier, self.name = bool(self.ds.sample), float(self.ds.latent_multiplier), data_dir
        self.mean = self.std = None
        if data_cfg.get("latent_norm", False):
            stats_path = stats_path or os.path.join(training_latent_dir(data_cfg), "latents_stats.pt")
            if not os.path.isfile(stats_path):
                raise SystemExit(f"data.latent_norm is on, but the statistics file {stats_path!r} does not exist: give the TRAINING set's "
                                 f"latents_stats.pt with --stats (statistics are never computed here)")
            st = torch.load(stats_path, map_location="cpu")
            self.mean, self.std = st["mean"].float().reshape(-1), st["std"].float().reshape(-1)

    def __len__(self):
        return len(self.ds)

    def read(self, indices):
        import torch
        xs, ys = [], []
        for idx in indices:
            f, i = self.ds.index[int(idx)]
            xs.append(self.ds._read(f, i, "latents").float())
            ys.append(self.ds._read(f, i, "labels").reshape(1))
        return torch.cat(xs), torch.cat(ys).long()


class SyntheticSource:
    """N(0, 1) latents with uniform labels, item i a function of (seed, i) (SyntheticLatentDataset): smoke runs."""

    def __init__(self, n, cfg, seed):
        from ldmae_amd.datasets.img_latent_dataset import SyntheticLatentDataset
        d = cfg["data"]
        self.ds = SyntheticLatentDataset(length=n, channels=cfg["model"].get("in_chans", 4), size=d["image_size"] // cfg["vae"].get("downsample_ratio", 16),
                                         num_classes=d["num_classes"], seed=seed)
        self.sample, self.multiplier, self.mean, self.std, self.name = False, 1.0, None, None, f"synthetic:{n}"

    def __len__(self):
        return len(self.ds)

    def read(self, indices):
        import torch
        items = [self.ds[int(i)] for i in indices]
        return torch.stack([x for x, _ in items]), torch.stack([y for _, y in items]).long()


# ----------------------------------------------------------------------------- the evaluation
def evaluate_model(model, source, indices, *, seed=0, batch=256, precision="bf16", interval=(0.0, 1.0), device=None):
    """Per-sample losses (f64 numpy, in the order of `indices`) of `model` as it stands.  model.eval() (the label embedder drops nothing),
    no_grad, bf16 autocast unless precision is fp32; the losses stay on the device until the end and come to the host once."""
    import torch
    from ldmae_amd import ops
    device = device or next(model.parameters()).device
    indices = np.asarray(indices, dtype=np.int64)
    was_training = model.training
    model.eval()
    mean, std = (s.to(device) if s is not None else None for s in (source.mean, source.std))
    losses = torch.empty(max(indices.size, 1), dtype=torch.float32, device=device)
    try:
        with torch.no_grad():
            for lo in range(0, indices.size, batch):
                idx = indices[lo:lo + batch]
                stored, y = source.read(idx)
                t = torch.from_numpy(sample_times(idx, interval)).to(device)
                xt, ut = ops.fm_valid_plan(stored.to(device), torch.from_numpy(idx).to(device), t, mean, std, source.multiplier, source.sample, seed)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=precision == "bf16"):
                    out = model(xt, t, y=y.to(device))
                assert out.size() == xt.size()
                ops.row_mse(out, ut, out=losses[lo:lo + idx.size])
    finally:
        model.train(was_training)
    return losses[:indices.size].double().cpu().numpy()


def gather_losses(idx, loss, num, rank, world):
    """The losses of every rank, merged by index on rank 0 (None elsewhere)."""
    if world == 1:
        return merge_by_index([(idx, loss)], num)
    import torch.distributed as dist
    parts = [None] * world
    dist.all_gather_object(parts, (idx, loss))
    return merge_by_index(parts, num) if rank == 0 else None


def evaluate(model, source, *, num=None, seed=0, batch=256, bins=10, precision="bf16", interval=(0.0, 1.0), use_lognorm=False, rank=0, world=1,
             device=None):
    """One evaluation of the model as it stands over samples 0 .. num - 1 of the source, split over the ranks: the report on rank 0, None elsewhere."""
    num = len(source) if num is None else min(int(num), len(source))
    idx = rank_indices(num, rank, world)
    losses = gather_losses(idx, evaluate_model(model, source, idx, seed=seed, batch=batch, precision=precision, interval=interval, device=device),
                           num, rank, world)
    if losses is None:
        return None
    return report(losses, sample_times(np.arange(num), interval), bins, interval, use_lognorm)


class TrainValidator:
    """The in-training hook of train_accum.do_train (train.valid): validates the live weights, then the EMA through opt.swap_in_ema() (swap,
    validate, swap back), logs one line and appends one JSON line to <exp_dir>/validation.jsonl.  It draws from no random stream of training."""

    def __init__(self, cfg, settings, exp_dir, precision, rank, world, device, use_lognorm):
        self.s, self.precision, self.rank, self.world, self.device, self.use_lognorm = settings, precision, rank, world, device, use_lognorm
        self.source = ShardSource(cfg["data"]["valid_path"], cfg["data"])
        self.path = os.path.join(exp_dir, "validation.jsonl")

    def due(self, step):
        return step > 0 and step % self.s["every"] == 0

    def run(self, model, opt, step, logger):
        kw = dict(num=self.s["num"], seed=self.s["seed"], batch=self.s["batch"], bins=self.s["bins"], precision=self.precision,
                  use_lognorm=self.use_lognorm, rank=self.rank, world=self.world, device=self.device)
        reps = {}
        if self.s["weights"] in ("model", "both"):
            reps["model"] = evaluate(model, self.source, **kw)
        if self.s["weights"] in ("ema", "both"):
            opt.swap_in_ema()
            try:
                reps["ema"] = evaluate(model, self.source, **kw)
            finally:
                opt.swap_in_ema()
        model.train()
        if self.rank == 0:
            f = lambda k: f"{reps[k]['loss']:.4f}" if k in reps else "-"          # noqa: E731
            logger.info(f"(step={step:07d}) Validation Loss (model / ema): {f('model')} / {f('ema')} ({reps[next(iter(reps))]['num']} samples)")
            with open(self.path, "a") as fh:
                fh.write(json.dumps({"step": step, "seed": self.s["seed"], **reps}) + "\n")
        return reps


# ----------------------------------------------------------------------------- command line
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m ldmae_amd.validate", description=__doc__.split("\n\n")[1])
    ap.add_argument("--config", required=True, help="the training YAML of the model")
    ap.add_argument("--ckpt", default=None, help="checkpoint with 'model' and 'ema' state dicts (or one plain state dict); required with --data")
    ap.add_argument("--data", default=None, help="directory of held-out latent shards (*.safetensors as extract_features writes them)")
    ap.add_argument("--synthetic", type=int, default=None, metavar="N", help="N latents drawn N(0, I) with uniform labels instead of --data")
    ap.add_argument("--num", type=int, default=None, help="validate the first N samples (default: all)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0, help="seed of the named draws (posterior sample and x0 of every validation sample)")
    ap.add_argument("--bins", type=int, default=10, help="equal-width time bins of the report")
    ap.add_argument("--weights", choices=WEIGHTS, default=None, help="which weights of the checkpoint (default: ema when it has them)")
    ap.add_argument("--interval", type=float, nargs=2, default=(0.0, 1.0), metavar=("LO", "HI"), help="the times cover [LO, HI]")
    ap.add_argument("--stats", default=None, help="latents_stats.pt of the TRAINING set (default: <training latent directory>/latents_stats.pt)")
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="bf16")
    ap.add_argument("--snapshots", default=None, help="post-hoc EMA snapshot directory: validate one reconstructed EMA per --sigma_rels width")
    ap.add_argument("--sigma_rels", default=None, help="comma-separated relative widths, e.g. 0.03,0.05,0.075,0.1 (needs --snapshots)")
    ap.add_argument("--step", type=int, default=None, help="the step the reconstructed averages end at (default: the last snapshot)")
    a = ap.parse_args(argv)
    if (a.data is None) == (a.synthetic is None):
        ap.error("give exactly one of --data DIR and --synthetic N")
    if a.synthetic is not None and a.synthetic < 1:
        ap.error("--synthetic N needs N >= 1")
    if a.batch < 1 or a.bins < 1 or a.seed < 0 or (a.num is not None and a.num < 1):
        ap.error("--batch, --bins and --num must be positive, --seed non-negative")
    for what, path in (("--ckpt", a.ckpt), ("--data", a.data), ("--config", a.config), ("--stats", a.stats), ("--snapshots", a.snapshots)):
        if path is not None and "://" in path:
            ap.error(f"{what} {path!r}: this tool downloads nothing; give a path on disk")
    if (a.sigma_rels is None) != (a.snapshots is None):
        ap.error("--sigma_rels and --snapshots go together: the widths to rebuild and the snapshot directory to rebuild them from")
    if a.step is not None and a.snapshots is None:
        ap.error("--step needs --snapshots")
    if a.sigma_rels is not None:
        try:
            from ldmae_amd.posthoc_ema import check_sigma_rel
            a.sigma_rels = [check_sigma_rel(float(s)) for s in a.sigma_rels.split(",")]
        except ValueError as e:
            ap.error(f"--sigma_rels: {e}")
        if a.weights is not None:
            ap.error("--weights does not apply to --sigma_rels: every row is a reconstructed EMA")
    if a.data is not None and a.ckpt is None and a.snapshots is None:
        ap.error("--data needs --ckpt (or --snapshots): the loss of real latents under untrained weights says nothing")
    if a.ckpt is not None and not os.path.isfile(a.ckpt):
        ap.error(f"--ckpt {a.ckpt!r} does not exist")
    if a.data is not None and not os.path.isdir(a.data):
        ap.error(f"--data {a.data!r} is not a directory")
    if a.snapshots is not None and not os.path.isdir(a.snapshots):
        ap.error(f"--snapshots {a.snapshots!r} is not a directory")
    if a.stats is not None and not os.path.isfile(a.stats):
        ap.error(f"--stats {a.stats!r} does not exist")
    if not os.path.isfile(a.config):
        ap.error(f"--config {a.config!r} does not exist")
    try:
        a.interval = check_interval(a.interval)
    except ValueError as e:
        ap.error(f"--interval: {e}")
    return a


def _load_into(model, sd):
    from ldmae_amd import ops
    model.load_state_dict({k.replace("module.", ""): v for k, v in sd.items()})
    ops.invalidate_weight_cache()


def run(a):
    import torch
    import yaml
    from ldmae_amd.train_accum import build_model
    from ldmae_amd.transport import create_transport
    if not torch.cuda.is_available():
        raise SystemExit("ldmae_amd.validate: needs a HIP device (the model and the objective are HIP kernels; no CPU fallback)")
    with open(a.config) as f:
        cfg = yaml.safe_load(f)
    rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
    local = int(os.environ.get("LDMAE_DEVICE", local))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            backend = os.environ.get("LDMAE_DIST_BACKEND", "nccl")
            dist.init_process_group(backend, **({"device_id": device} if backend == "nccl" else {}))
    t = cfg["transport"]
    # the refusals of everything but the linear path with velocity prediction are create_transport's
    tr = create_transport(t["path_type"], t["prediction"], t["loss_weight"], t["train_eps"], t["sample_eps"],
                          use_cosine_loss=t.get("use_cosine_loss", False), use_lognorm=t.get("use_lognorm", False))
    source = SyntheticSource(a.synthetic, cfg, a.seed) if a.synthetic is not None else ShardSource(a.data, cfg["data"], a.stats)
    model = build_model(cfg).to(device).eval().requires_grad_(False)
    kw = dict(num=a.num, seed=a.seed, batch=a.batch, bins=a.bins, precision=a.precision, interval=a.interval, use_lognorm=tr.use_lognorm,
              rank=rank, world=world, device=device)
    res = {"source": source.name, "seed": a.seed, "batch": a.batch, "precision": a.precision, "interval": list(a.interval),
           "weights_file": a.ckpt or "initial (no --ckpt)"}
    if a.snapshots is not None:
        from ldmae_amd import posthoc_ema
        base = model.state_dict()                     # buffers (entries that are no parameters) stay as the model builds them
        if a.ckpt is not None:
            ck = torch.load(a.ckpt, map_location="cpu")
            base.update({k.replace("module.", ""): v for k, v in (ck["ema"] if "ema" in ck else ck.get("model", ck)).items()})
        rows = []
        for s in a.sigma_rels:
            sd, rec = posthoc_ema.reconstruct(a.snapshots, s, a.step, device=device)
            _load_into(model, dict(base, **sd))
            rep = evaluate(model, source, **kw)
            if rep is not None:
                rows.append({"sigma_rel": s, "step": rec["step"], "residual_rel": rec["residual_rel"], **rep})
        if rank == 0:
            best = min(range(len(rows)), key=lambda i: rows[i]["loss"])
            print(f"EMA width sweep at step {rows[0]['step']} from {a.snapshots} ({rows[0]['num']} samples, uniform in t):")
            for i, r in enumerate(rows):
                sem = "n/a" if r["sem"] is None else f"{r['sem']:.5f}"
                print(f"  sigma_rel {r['sigma_rel']:g} -> {r['loss']:.5f} +- {sem}{'   <- minimum' if i == best else ''}")
            res.update(snapshots=a.snapshots, sweep=rows, best_sigma_rel=rows[best]["sigma_rel"])
        return res if rank == 0 else None
    ck = torch.load(a.ckpt, map_location="cpu") if a.ckpt is not None else None
    which = a.weights or ("ema" if ck is not None and "ema" in ck else "model")
    names = ("model", "ema") if which == "both" else (which,)
    if ck is not None and any(n not in ck for n in names) and not (names == ("model",) and "ema" not in ck):
        raise SystemExit(f"--weights {which}: {a.ckpt!r} has no {' / '.join(repr(n) for n in names if n not in ck)} entry")
    res["weights"] = {}
    for n in names:
        if ck is not None:
            _load_into(model, ck[n] if n in ck else ck)
        rep = evaluate(model, source, **kw)
        if rep is not None:
            print(format_report(n, rep))
            res["weights"][n] = rep
    return res if rank == 0 else None


def main(argv=None):
    res = run(parse_args(argv))
    if res is not None:
        print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
