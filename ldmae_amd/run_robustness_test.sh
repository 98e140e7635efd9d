#!/bin/bash
# Counterpart of the reference's run_robustness_test.sh: the LDMAE latent-robustness sweep, rFID / PSNR / LPIPS / SSIM of VMAE
# reconstructions with latent noise epsilon = 0, 0.01, 0.05, 0.1, 0.2, 0.3 (body: _launch.sh, one process per GPU).
#   run_robustness_test.sh [config.yaml] [driver flags ...]     e.g. --data_path .../val --lpips_vgg vgg16-397923af.pth --lpips_lin vgg.pth
# The first run writes output_path/ref_images; the later ones find them there and reuse them.  The first point passes no --epsilon, as the
# reference's first call does (its folder is vmae_0).
config=${1:-configs/imagenet/lightningdit_b_vmae_f8d16_cfg.yaml}
shift
here="$(cd "$(dirname "$0")" && pwd)"
for eps in "" 0.01 0.05 0.1 0.2 0.3; do
  (DRIVER=evaluate_tokenizer.py DEFAULT_PORT=1241 source "$here/_launch.sh" "$config" ${eps:+--epsilon $eps} "$@") || exit 1
done
