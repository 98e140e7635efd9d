#!/usr/bin/env python3
"""Likelihood evaluation: `python -m ldmae_amd.likelihood --config CFG --ckpt CKPT --data DIR` (or `--synthetic N`).

Integrates the probability-flow ODE from each latent to noise with Hutchinson's trace estimator (transport.Sampler.sample_ode_likelihood) and
prints the class-conditional log-likelihood in bits per dimension OF THE LATENT SPACE, -log2 p(x | y) / (C h w): mean and standard error over
the images, the solver's nfe / accepted / rejected of the last batch, and one JSON line at the end.  The latents are read as training reads
them (ImgLatentDataset on the shards extract_features writes: posterior sample, channel normalisation, multiplier, the unflipped copy) or
drawn N(0, I) with uniform labels (--synthetic).  Nothing is downloaded: a checkpoint or a directory that is not on disk is an error."""
import argparse
import json
import math
import os
import sys

import torch
import yaml

_HERE = os.path.dirname(os.path.abspath(__file__))
for p in (_HERE, os.path.dirname(_HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m ldmae_amd.likelihood", description=__doc__.split("\n\n")[1])
    ap.add_argument("--config", required=True, help="the training / sampling YAML of the model")
    ap.add_argument("--ckpt", default=None, help="checkpoint with an 'ema' (or plain) state dict; required with --data")
    ap.add_argument("--data", default=None, help="directory of latent shards (*.safetensors as extract_features writes them)")
    ap.add_argument("--synthetic", type=int, default=None, metavar="N", help="N latents drawn N(0, I) with uniform labels instead of --data")
    ap.add_argument("--num-images", type=int, default=None, help="evaluate the first K images of --data (default: all)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--method", default="dopri5", help="dopri5 / euler / heun / midpoint")
    ap.add_argument("--num-steps", type=int, default=50)
    ap.add_argument("--atol", type=float, default=1e-6)
    ap.add_argument("--rtol", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0, help="seed of the Rademacher probe (and of --synthetic)")
    a = ap.parse_args(argv)
    if (a.data is None) == (a.synthetic is None):
        ap.error("give exactly one of --data DIR and --synthetic N")
    if a.synthetic is not None and a.synthetic < 1:
        ap.error("--synthetic N needs N >= 1")
    if a.batch < 1 or (a.num_images is not None and a.num_images < 1):
        ap.error("--batch and --num-images must be positive")
    for what, path in (("--ckpt", a.ckpt), ("--data", a.data), ("--config", a.config)):
        if path is not None and "://" in path:
            ap.error(f"{what} {path!r}: this tool downloads nothing; give a path on disk")
    if a.data is not None and a.ckpt is None:
        ap.error("--data needs --ckpt: the likelihood of real latents under untrained weights says nothing")
    if a.ckpt is not None and not os.path.isfile(a.ckpt):
        ap.error(f"--ckpt {a.ckpt!r} does not exist")
    if a.data is not None and not os.path.isdir(a.data):
        ap.error(f"--data {a.data!r} is not a directory")
    if not os.path.isfile(a.config):
        ap.error(f"--config {a.config!r} does not exist")
    return a


def _batches(a, cfg, model):
    """Yields (x [b, C, h, w] f32, y [b] i64) on the host."""
    if a.synthetic is not None:
        g = torch.Generator().manual_seed(a.seed)
        size = model.x_embedder.img_size[0]
        for lo in range(0, a.synthetic, a.batch):
            b = min(a.batch, a.synthetic - lo)
            yield torch.randn(b, model.in_channels, size, size, generator=g), torch.randint(0, cfg["data"]["num_classes"], (b,), generator=g)
        return
    from ldmae_amd.datasets.img_latent_dataset import DiagonalGaussianDistribution, ImgLatentDataset
    d = cfg["data"]
    ds = ImgLatentDataset(data_dir=a.data, latent_norm=d.get("latent_norm", False), latent_multiplier=d.get("latent_multiplier", 0.18215),
                          sample=d.get("sample", False), raw=True)
    if len(ds) == 0:
        raise SystemExit(f"--data {a.data!r} holds no *.safetensors shard")
    n = len(ds) if a.num_images is None else min(a.num_images, len(ds))
    for lo in range(0, n, a.batch):
        xs, ys = [], []
        for idx in range(lo, min(lo + a.batch, n)):
            f, i = ds.index[idx]
            x = ds._read(f, i, "latents")
            if ds.sample:
                x = DiagonalGaussianDistribution(x).sample()
            if ds.latent_norm:
                x = (x - ds._latent_mean) / ds._latent_std
            xs.append((x * ds.latent_multiplier).float())
            ys.append(ds._read(f, i, "labels").reshape(1))
        yield torch.cat(xs), torch.cat(ys).long()


def evaluate(a):
    from ldmae_amd.train_accum import build_model
    from ldmae_amd.transport import Sampler, create_transport
    if not torch.cuda.is_available():
        raise SystemExit("ldmae_amd.likelihood: needs a HIP device (the model, the probe and the solver are HIP kernels; no CPU fallback)")
    cfg = yaml.safe_load(open(a.config))
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    torch.manual_seed(a.seed)
    model = build_model(cfg, learn_sigma=cfg["model"].get("learn_sigma", False))
    if a.ckpt is not None:
        ck = torch.load(a.ckpt, map_location="cpu")
        model.load_state_dict(ck["ema"] if "ema" in ck else ck)
    model = model.to(device).eval().requires_grad_(False)
    t = cfg["transport"]
    tr = create_transport(t["path_type"], t["prediction"], t["loss_weight"], t["train_eps"], t["sample_eps"])
    fn = Sampler(tr).sample_ode_likelihood(sampling_method=a.method, num_steps=a.num_steps, atol=a.atol, rtol=a.rtol, seed=a.seed)
    bpd = []
    for x, y in _batches(a, cfg, model):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=a.precision == "bf16"):
            logp, _ = fn(x.to(device), model.forward, y=y.to(device))
        bpd.append(-logp.double().cpu() / (x[0].numel() * math.log(2.0)))
    bpd = torch.cat(bpd)
    n = bpd.numel()
    mean = float(bpd.mean())
    sem = float(bpd.std(unbiased=True) / math.sqrt(n)) if n > 1 else float("nan")
    o = fn.ode
    print(f"{n} images: {mean:.4f} +- {sem:.4f} bits / latent dim ({a.method}, atol {a.atol:g}, rtol {a.rtol:g}, {a.precision}); "
          f"last batch: nfe {o.nfe}, accepted {o.accepted}, rejected {o.rejected}")
    return {"images": n, "bits_per_dim": mean, "bits_per_dim_sem": sem if n > 1 else None, "nfe": o.nfe, "accepted": o.accepted,
            "rejected": o.rejected, "method": a.method, "atol": a.atol, "rtol": a.rtol, "precision": a.precision, "seed": a.seed,
            "weights": a.ckpt or "initial (no --ckpt)", "source": a.data or f"synthetic:{a.synthetic}"}


def main(argv=None):
    res = evaluate(parse_args(argv))
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
