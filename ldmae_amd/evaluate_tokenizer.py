#!/usr/bin/env python3
"""Tokenizer evaluation on the HIP kernels -- counterpart of the reference's ``evaluate_tokenizer.py``: encode images with the VMAE
tokenizer, optionally perturb the latent (``--epsilon``, the LDMAE robustness experiment), decode, and report rFID, PSNR, LPIPS and SSIM.

    torchrun --nproc_per_node N -m ldmae_amd.evaluate_tokenizer --config_path configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml \\
        --data_path /data/dataset/imagenet/1K_dataset/val --output_path ./rfid --epsilon 0.1 --lpips_vgg vgg16-397923af.pth --lpips_lin vgg.pth
    python -m ldmae_amd.evaluate_tokenizer --config_path <cfg> --synthetic 64          # no image folder: seeded random images

Same as the reference: DistributedSampler(shuffle=False) shares; ToTensor -> Resize(256) -> CenterCrop(256) -> Normalize(0.5, 0.5); the
latent is the posterior mode plus ``epsilon * randn * latent_std`` (latents_stats.pt under data.data_path, + "_sample" when data.sample is
set); PNGs ``ref_images/ref_image_rank_{r}_{i}.png`` (skipped when 50 000 exist) and ``{model_type}_{epsilon}/decoded_images/
decoded_image_rank_{r}_{i}.png``; LPIPS and SSIM are per-batch means averaged over batches, then over ranks; PSNR is the mean over all images;
rFID = calculate_fid_given_paths([ref, decoded], 50, dims=2048) on rank 0.

Different on purpose:
  - the noise comes from a generator seeded with ``seed + rank`` (the reference parses --seed and never uses it, so its noise is unseeded);
  - reconstruction and metrics always run (the reference skips them once 50 000 decoded PNGs exist and then averages empty lists);
  - PSNR comes from the exact integer squared error of the uint8 images the PNGs hold, computed while quantising (PNG is lossless, so this
    is the reference's calculate_psnr_between_folders without reading the files back; it rounds each mean to f32, this does not);
  - LPIPS, SSIM and the quantisation run on this package's kernels; weights are the user's files (--lpips_vgg, --lpips_lin, --fid_weights)
    and are never downloaded;
  - only the VMAE tokenizer is built here; the SD-VAE model types (ae, dae, vae, sdv3) are refused.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import torch
import torch.distributed as dist
import torch.nn.functional as F
import yaml
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.distributed import DistributedSampler

_HERE = os.path.dirname(os.path.abspath(__file__))
for p in (_HERE, os.path.dirname(_HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

IMAGE_SIZE = 256
REF_SKIP_AT = 50000                 # evaluate_tokenizer.py: reference PNGs are rewritten unless this many exist
SDVAE_TYPES = ("ae", "dae", "vae", "sdv3")
PNG_THREADS = 16


def print_with_prefix(content, prefix="Tokenizer Evaluation", rank=0):
    if rank == 0:
        print(f"\033[34m[{prefix}]\033[0m {content}", flush=True)


# ---------------------------------------------------------------------------------------------------- pre-processing
def resized_size(h, w, size=IMAGE_SIZE):
    """torchvision Resize(size) for an int size: the short side becomes `size`, the long side int(size * long / short)."""
    short, long = (h, w) if h <= w else (w, h)
    new_short, new_long = size, int(size * long / short)
    return (new_short, new_long) if h <= w else (new_long, new_short)


def crop_offsets(h, w, size=IMAGE_SIZE):
    """torchvision CenterCrop(size): (top, left) = (int(round((h - size) / 2)), int(round((w - size) / 2)))."""
    return int(round((h - size) / 2.0)), int(round((w - size) / 2.0))


class EvalTransform:
    """ToTensor -> Resize(256, bilinear, antialias) -> CenterCrop(256) -> Normalize(0.5, 0.5), torchvision's tensor path without torchvision."""

    def __init__(self, size=IMAGE_SIZE):
        self.size = size

    def __call__(self, pil_image):
        import numpy as np
        x = torch.from_numpy(np.array(pil_image.convert("RGB"), dtype=np.uint8)).permute(2, 0, 1).float().div_(255.0)
        return self.tensor(x)

    def tensor(self, x):
        """The same on a CHW float tensor in [0, 1] (ToTensor's output)."""
        h, w = x.shape[-2:]
        oh, ow = resized_size(h, w, self.size)
        if (oh, ow) != (h, w):
            x = F.interpolate(x[None], size=(oh, ow), mode="bilinear", align_corners=False, antialias=True)[0]
        if oh < self.size or ow < self.size:
            raise ValueError(f"image {h}x{w} resized to {oh}x{ow} is smaller than the {self.size} crop")
        top, left = crop_offsets(oh, ow, self.size)
        x = x[:, top:top + self.size, left:left + self.size]
        return ((x - 0.5) / 0.5).contiguous()


class SyntheticImages(Dataset):
    """N seeded random images in [-1, 1] (already transformed), label 0: the driver without an image folder."""

    def __init__(self, n, size=IMAGE_SIZE):
        self.n, self.size = n, size

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(i)
        return torch.rand(3, self.size, self.size, generator=g) * 2 - 1, 0


# ---------------------------------------------------------------------------------------------------- layout and aggregation
def output_dirs(output_path, model_type, epsilon):
    """(decoded_images dir, ref_images dir) in the reference's layout."""
    return os.path.join(output_path, f"{model_type}_{epsilon}", "decoded_images"), os.path.join(output_path, "ref_images")


def ref_name(rank, i):
    return f"ref_image_rank_{rank}_{i}.png"


def decoded_name(rank, i):
    return f"decoded_image_rank_{rank}_{i}.png"


def latent_stats_path(cfg):
    data_path = cfg["data"]["data_path"] + ("_sample" if "sample" in cfg["data"] else "")      # key presence, as the reference tests it
    return os.path.join(data_path, "latents_stats.pt")


def aggregate(lpips_batches, ssim_batches, psnr_sum, psnr_count, world=1):
    """The reference's arithmetic: LPIPS / SSIM = mean over batches of the per-batch means, averaged elementwise over ranks first (all-reduce
    AVG of the per-batch vectors, equal lengths under DistributedSampler); PSNR = sum over all images / their count.  Inputs are this rank's
    values; with world > 1 the reductions run over the default process group."""
    dev = lpips_batches.device
    lp, ss = lpips_batches.double().clone(), ssim_batches.double().clone()
    ps = torch.tensor([float(psnr_sum), float(psnr_count)], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(lp)
        dist.all_reduce(ss)
        dist.all_reduce(ps)
        lp, ss = lp / world, ss / world
    return {"lpips": float(lp.mean()), "ssim": float(ss.mean()), "psnr": float(ps[0] / ps[1])}


def _save_png(arr, path):
    from PIL import Image
    Image.fromarray(arr).save(path)


# ---------------------------------------------------------------------------------------------------- the driver
def build_parser():
    ap = argparse.ArgumentParser(description="rFID, PSNR, LPIPS and SSIM of VMAE reconstructions on the HIP kernels")
    ap.add_argument("--config_path", type=str, default="configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml")
    ap.add_argument("--model_type", type=str, default="vmae", help="accepted; the type comes from vae.model_name, as in the reference")
    ap.add_argument("--data_path", type=str, default="/data/dataset/imagenet/1K_dataset/val")
    ap.add_argument("--output_path", type=str, default="./rfid")
    ap.add_argument("--seed", type=int, default=42, help="latent noise generator seed (+ rank)")
    ap.add_argument("--epsilon", type=float, default=0, help="Noise pertubation ratio for latent robustness experiment.")
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--num_workers", type=int, default=4)
    ap.add_argument("--lpips_vgg", type=str, default=None, help="torchvision vgg16-397923af.pth (default: $LDMAE_LPIPS_VGG, torch.hub)")
    ap.add_argument("--lpips_lin", type=str, default=None, help="taming's LPIPS vgg.pth (default: $LDMAE_LPIPS_LIN, the reference's path)")
    ap.add_argument("--lpips_precision", default=None, choices=["f32", "fp16"],
                    help="arithmetic of the LPIPS network: f32 (default, exact) or fp16 (fp16 VGG, f32 accumulation; models/lpips.py).  When given, "
                         "the JSON line names it")
    ap.add_argument("--fid_weights", type=str, default=None, help="pt_inception-2015-12-05-6726825d.pth (default: $LDMAE_FID_WEIGHTS, torch.hub)")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--synthetic", type=int, default=0, help="N seeded random images instead of an image folder")
    return ap


def model_type_of(cfg):
    """vae.model_name's prefix; SD-VAE types are named and refused, anything else but vmae too."""
    mt = cfg["vae"]["model_name"].split("_")[0]
    if mt in SDVAE_TYPES:
        raise NotImplementedError(f"tokenizer '{mt}': the SD-VAE model types {SDVAE_TYPES} are not built here; only vmae is")
    if mt != "vmae":
        raise NotImplementedError(f"tokenizer '{mt}': only the vmae tokenizer is supported")
    return mt


def evaluate_tokenizer(args, cfg, log=print_with_prefix):
    if not torch.cuda.is_available():
        raise RuntimeError("evaluate_tokenizer needs a GPU: there is no CPU path in this package")
    model_type = model_type_of(cfg)
    from ldmae_amd import fid, ops
    from ldmae_amd.metrics import psnr_from_sse, ssim
    from ldmae_amd.models.lpips import LPIPS
    from ldmae_amd.tokenizer import models_mae

    distributed = "RANK" in os.environ and not (dist.is_available() and dist.is_initialized())
    if distributed:
        dist.init_process_group("nccl" if os.environ.get("LDMAE_DIST_BACKEND", "nccl") == "nccl" else "gloo")
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    device = torch.device("cuda", int(os.environ.get("LDMAE_DEVICE", os.environ.get("LOCAL_RANK", rank % torch.cuda.device_count()))))
    torch.cuda.set_device(device)
    log(f"Loading model... {model_type.upper()} {args.epsilon}", rank=rank)
    # weights first: a missing file fails before any image is written
    lpips_precision = getattr(args, "lpips_precision", None)
    lpips = LPIPS(args.lpips_vgg, args.lpips_lin, device=device, precision=lpips_precision or "f32")
    if args.fid_weights:
        os.environ[fid.WEIGHTS_ENV] = args.fid_weights
    fid.resolve_weights()
    torch.manual_seed(args.seed)                # the same initial weights on every rank when no checkpoint is loaded (--synthetic)
    model = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, kl_loss_weight=True, smooth_output=True,
                                                img_size=cfg["data"].get("image_size", IMAGE_SIZE))
    chkpt = cfg["vae"].get("weight_path")
    if chkpt and os.path.exists(chkpt):
        msg = model.load_state_dict(torch.load(chkpt, map_location="cpu")["model"], strict=False)
        log(str(msg), rank=rank)
    elif not args.synthetic:
        raise FileNotFoundError(f"vae.weight_path {chkpt!r} not found")
    model = model.to(device).eval()
    if args.precision == "bf16":
        model.set_precision(torch.bfloat16)
    stats_file = latent_stats_path(cfg)
    if os.path.exists(stats_file):
        latent_std = torch.load(stats_file, map_location="cpu")["std"].float().to(device)
    elif args.epsilon != 0:
        raise FileNotFoundError(f"latents_stats.pt not found at {stats_file}: --epsilon {args.epsilon} scales its noise by the latent std")
    else:
        latent_std = None

    dataset = SyntheticImages(args.synthetic) if args.synthetic else _image_folder(args.data_path)
    res, save_dir, ref_path = reconstruct_and_score(args, model_type, lambda images: model.encode(images).latent_dist.mode(),
                                                    lambda latents: model.decode(latents).sample, dataset, latent_std, lpips, device, rank, world, log,
                                                    extra={"lpips_precision": lpips_precision} if lpips_precision else None)
    if distributed:
        dist.destroy_process_group()
    return res, save_dir, ref_path


def reconstruct_and_score(args, model_type, encode, decode, dataset, latent_std, lpips, device, rank=0, world=1, log=print_with_prefix,
                          extra=None):
    """The evaluation loop for any tokenizer: encode(images [B, 3, H, W] in [-1, 1]) -> latents, + epsilon * randn * latent_std, decode(latents)
    -> images; PNGs, LPIPS / SSIM / PSNR, rFID on rank 0 and the JSON line.  Returns (metrics, decoded dir, reference dir)."""
    from ldmae_amd import fid, ops
    from ldmae_amd.metrics import psnr_from_sse, ssim
    sampler = DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=False)
    loader = DataLoader(dataset, batch_size=args.batch_size, shuffle=False, sampler=sampler, num_workers=args.num_workers,
                        pin_memory=True, multiprocessing_context="forkserver" if args.num_workers > 0 else None)
    save_dir, ref_path = output_dirs(args.output_path, model_type, args.epsilon)
    os.makedirs(save_dir, exist_ok=True)
    os.makedirs(ref_path, exist_ok=True)
    log(f"Output dir: {save_dir}", rank=rank)
    log(f"Reference dir: {ref_path}", rank=rank)
    write_refs = len([f for f in os.listdir(ref_path) if f.endswith(".png")]) < REF_SKIP_AT
    if world > 1:
        dist.barrier()                              # every rank has counted the reference PNGs before any writes one

    gen = torch.Generator(device=device).manual_seed(args.seed + rank)
    lpips_vals, ssim_vals, psnr_all = [], [], []
    n_done, pending = 0, []
    log("Generating reconstructions...", rank=rank)
    with torch.no_grad(), ThreadPoolExecutor(max_workers=PNG_THREADS) as pool:
        for images, _ in loader:
            images = images.to(device, non_blocking=True).float().contiguous()
            latents = encode(images).to(torch.float32)
            if args.epsilon != 0:
                noise = torch.randn(latents.shape, generator=gen, device=device, dtype=torch.float32)
                latents = latents + args.epsilon * noise * latent_std
            decoded = decode(latents).float().contiguous()
            lpips_vals.append(lpips(decoded, images).mean())
            ssim_vals.append(ssim(decoded, images, data_range=(-1.0, 1.0)))
            dec8, ref8, sse = ops.recon_quantize_sse(decoded, images)
            psnr_all.append(psnr_from_sse(sse, decoded[0].numel()))
            dec_h = dec8.cpu().numpy()
            ref_h = ref8.cpu().numpy() if write_refs else None
            for j in range(dec_h.shape[0]):
                pending.append(pool.submit(_save_png, dec_h[j], os.path.join(save_dir, decoded_name(rank, n_done + j))))
                if write_refs:
                    pending.append(pool.submit(_save_png, ref_h[j], os.path.join(ref_path, ref_name(rank, n_done + j))))
            n_done += dec_h.shape[0]
            if rank == 0 and n_done % 800 < args.batch_size:
                log(f"Rank {rank}, Processed {n_done} images", rank=rank)
            if len(pending) > 4 * PNG_THREADS * max(1, args.batch_size):
                for fut in pending:
                    fut.result()
                pending = []
        for fut in pending:
            fut.result()
    if n_done == 0:
        raise RuntimeError("no images to evaluate")
    psnr = torch.cat(psnr_all)
    if world > 1:
        dist.barrier()
    res = aggregate(torch.stack(lpips_vals), torch.stack(ssim_vals), psnr.sum(), psnr.numel(), world)
    res.update({"epsilon": args.epsilon, "images": len(dataset), "world": world})
    res.update(extra or {})             # fields a caller adds to the JSON line (evaluate_conv_tokenizer: the precision)
    if rank == 0:
        log("Computing rFID...")
        res["rfid"] = fid.calculate_fid_given_paths([ref_path, save_dir], batch_size=50, device=device, dims=2048, num_workers=16)
        log("Computing PSNR...")
        log("Final Metrics:")
        log(f"rFID: {res['rfid']:.3f}")
        log(f"PSNR: {res['psnr']:.3f}")
        log(f"LPIPS: {res['lpips']:.3f}")
        log(f"SSIM: {res['ssim']:.3f}")
        print(json.dumps({"metric": "tokenizer_eval", "model_type": model_type, **res}), flush=True)
    if world > 1:
        dist.barrier()
    return res, save_dir, ref_path


def _image_folder(root):
    from ldmae_amd.datasets.image_folder import ImageFolder
    return ImageFolder(root, transform=EvalTransform())


def main(argv=None):
    args = build_parser().parse_args(argv)
    with open(args.config_path) as f:
        cfg = yaml.safe_load(f)
    model_type_of(cfg)                  # refuse an SD-VAE config before touching the GPU
    return evaluate_tokenizer(args, cfg)[0]


if __name__ == "__main__":
    main()
