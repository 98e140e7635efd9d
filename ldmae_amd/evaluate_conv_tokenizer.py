#!/usr/bin/env python3
"""rFID, PSNR, LPIPS and SSIM of the convolutional KL-VAE tokenizers (tokenizer/sdvae.py, vavae.py, marvae.py) on the HIP kernels: the
baselines the VMAE tokenizer is compared with, through the loop and the metric code of ``evaluate_tokenizer.py``.

    python -m ldmae_amd.evaluate_conv_tokenizer --family sdvae --weights sdv3_f8d16.pt --data_path /data/imagenet/val --output_path ./rfid \\
        --epsilon 0.1 --latent_stats latents_stats.pt --lpips_vgg vgg16-397923af.pth --lpips_lin vgg.pth --fid_weights pt_inception.pth
    python -m ldmae_amd.evaluate_conv_tokenizer --family sdvae --synthetic 64          # no image folder, seeded random weights

``--family sdvae`` builds ``Diffusers_AutoencoderKL`` with the keyword set of the reference's drivers (block widths, latent channels and
depth can be changed by flag) and loads ``checkpoint['model']``; ``vavae`` reads ``model.params.embed_dim`` from ``--config_path`` and loads
``checkpoint['state_dict']``; ``marvae`` loads ``checkpoint['model']``.  The latent is the posterior mode; ``--epsilon`` adds
``epsilon * randn * std`` with the std of ``--latent_stats`` (a latents_stats.pt).  Output layout and the JSON line are those of
``evaluate_tokenizer.py`` with the family as model type and the ``--precision`` of the run.  Weights are the user's files; nothing is downloaded.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch
import torch.distributed as dist

_HERE = os.path.dirname(os.path.abspath(__file__))
for p in (_HERE, os.path.dirname(_HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from ldmae_amd import evaluate_tokenizer as et  # noqa: E402

FAMILIES = ("sdvae", "vavae", "marvae")


def build_parser():
    ap = argparse.ArgumentParser(description="rFID, PSNR, LPIPS and SSIM of the convolutional KL-VAE tokenizers on the HIP kernels")
    ap.add_argument("--family", required=True, choices=FAMILIES)
    ap.add_argument("--weights", type=str, default=None, help="checkpoint of the tokenizer (required unless --synthetic)")
    ap.add_argument("--config_path", type=str, default=None, help="vavae: the YAML holding model.params.embed_dim")
    ap.add_argument("--data_path", type=str, default="/data/dataset/imagenet/1K_dataset/val")
    ap.add_argument("--output_path", type=str, default="./rfid")
    ap.add_argument("--seed", type=int, default=42, help="latent noise generator seed (+ rank)")
    ap.add_argument("--epsilon", type=float, default=0, help="Noise pertubation ratio for latent robustness experiment.")
    ap.add_argument("--latent_stats", type=str, default=None, help="latents_stats.pt whose 'std' scales the --epsilon noise")
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--num_workers", type=int, default=4)
    ap.add_argument("--image_size", type=int, default=et.IMAGE_SIZE)
    ap.add_argument("--block_out_channels", type=str, default="128,256,512,512", help="sdvae: widths per level")
    ap.add_argument("--latent_channels", type=int, default=16, help="sdvae")
    ap.add_argument("--layers_per_block", type=int, default=2, help="sdvae")
    ap.add_argument("--lpips_vgg", type=str, default=None, help="torchvision vgg16-397923af.pth (default: $LDMAE_LPIPS_VGG, torch.hub)")
    ap.add_argument("--lpips_lin", type=str, default=None, help="taming's LPIPS vgg.pth (default: $LDMAE_LPIPS_LIN, the reference's path)")
    ap.add_argument("--fid_weights", type=str, default=None, help="pt_inception-2015-12-05-6726825d.pth (default: $LDMAE_FID_WEIGHTS, torch.hub)")
    ap.add_argument("--synthetic", type=int, default=0, help="N seeded random images instead of an image folder")
    ap.add_argument("--precision", choices=("f32", "tf32"), default="f32",
                    help="tf32: the 3x3 convolutions round both operands once to fp16 and accumulate in f32 (what the reference computes under allow_tf32)")
    return ap


def build_tokenizer(args, device):
    """(encode, decode): images -> posterior mode, latents -> images, for the chosen family."""
    if args.weights is None and not args.synthetic:
        raise FileNotFoundError("--weights is required (only --synthetic runs on seeded random weights)")
    if args.weights is not None and not os.path.isfile(args.weights):
        raise FileNotFoundError(f"--weights {args.weights!r} not found")
    if args.family == "sdvae":
        from ldmae_amd.tokenizer.sdvae import DECODER_BLOCK, ENCODER_BLOCK, Diffusers_AutoencoderKL
        boc = tuple(int(c) for c in args.block_out_channels.split(","))
        vae = Diffusers_AutoencoderKL(img_size=args.image_size, sample_size=128, in_channels=3, out_channels=3, layers_per_block=args.layers_per_block,
                                      latent_channels=args.latent_channels, norm_num_groups=32, act_fn="silu", block_out_channels=boc,
                                      force_upcast=False, use_quant_conv=False, use_post_quant_conv=False,
                                      down_block_types=(ENCODER_BLOCK,) * len(boc), up_block_types=(DECODER_BLOCK,) * len(boc))
        if args.weights is not None:
            vae.load_state_dict(torch.load(args.weights, map_location="cpu")["model"], strict=False)
        vae = vae.to(device).eval().set_precision(args.precision)
        return (lambda x: vae.encode(x, return_dict=False)[0].mode()), (lambda z: vae.decode(z, return_dict=False)[0])
    from ldmae_amd.tokenizer.autoencoder import AutoencoderKL
    if args.family == "vavae":
        import yaml
        if args.config_path is None:
            raise FileNotFoundError("--family vavae needs --config_path (the YAML holding model.params.embed_dim)")
        with open(args.config_path) as f:
            embed_dim = yaml.safe_load(f)["model"]["params"]["embed_dim"]
        model = AutoencoderKL(embed_dim=embed_dim, ch_mult=(1, 1, 2, 2, 4), ckpt_path=args.weights)
    else:
        model = AutoencoderKL(embed_dim=16, ch_mult=(1, 1, 2, 2, 4), ckpt_path=args.weights, model_type="marvae")
    model = model.to(device).eval().set_precision(args.precision)
    return (lambda x: model.encode(x).mode()), model.decode


def evaluate_conv_tokenizer(args, log=et.print_with_prefix):
    if not torch.cuda.is_available():
        raise RuntimeError("evaluate_conv_tokenizer needs a GPU: there is no CPU path in this package")
    from ldmae_amd import fid
    from ldmae_amd.models.lpips import LPIPS
    distributed = "RANK" in os.environ and not (dist.is_available() and dist.is_initialized())
    if distributed:
        dist.init_process_group("nccl" if os.environ.get("LDMAE_DIST_BACKEND", "nccl") == "nccl" else "gloo")
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    device = torch.device("cuda", int(os.environ.get("LDMAE_DEVICE", os.environ.get("LOCAL_RANK", rank % torch.cuda.device_count()))))
    torch.cuda.set_device(device)
    log(f"Loading model... {args.family.upper()} {args.epsilon}", rank=rank)
    lpips = LPIPS(args.lpips_vgg, args.lpips_lin, device=device)          # weights first: a missing file fails before any image is written
    if args.fid_weights:
        os.environ[fid.WEIGHTS_ENV] = args.fid_weights
    fid.resolve_weights()
    torch.manual_seed(args.seed)                # the same initial weights on every rank when no checkpoint is loaded (--synthetic)
    encode, decode = build_tokenizer(args, device)
    if args.latent_stats is not None:
        latent_std = torch.load(args.latent_stats, map_location="cpu")["std"].float().to(device)
    elif args.epsilon != 0:
        raise FileNotFoundError(f"--epsilon {args.epsilon} scales its noise by the latent std: pass --latent_stats latents_stats.pt")
    else:
        latent_std = None
    if args.synthetic:
        dataset = et.SyntheticImages(args.synthetic, args.image_size)
    else:
        from ldmae_amd.datasets.image_folder import ImageFolder
        dataset = ImageFolder(args.data_path, transform=et.EvalTransform(args.image_size))
    out = et.reconstruct_and_score(args, args.family, encode, decode, dataset, latent_std, lpips, device, rank, world, log,
                                   extra={"precision": args.precision})
    if distributed:
        dist.destroy_process_group()
    return out


def main(argv=None):
    return evaluate_conv_tokenizer(build_parser().parse_args(argv))[0]


if __name__ == "__main__":
    main()
