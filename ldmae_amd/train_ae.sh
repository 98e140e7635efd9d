#!/bin/bash
# Counterpart of the reference's VMAE/train_ae.sh (the tokenizer recipe), for the stages this package builds:
#   Stage 1  VMAE pre-training at 128 x 128 (main_pretrain.py -> vmae_pretrain.py; one process per GPU, RCCL all-reduce)
#   Stage 2  position-embedding reset to the 256 x 256 grid (pe_reset.py)
#   Stage 3  decoder tuning at 256 x 256 with the LPIPS loss (main_pretrain.py --tune_decoder -> vmae_pretrain.py; LPIPS and its backward on this
#            package's kernels, from the user's weight files: LPIPS_VGG / LPIPS_LIN, or $LDMAE_LPIPS_VGG / $LDMAE_LPIPS_LIN, or the default places)
# Stage 1's flags are the reference script's (train_ae.sh:26-46) minus --perceptual_loss_ratio (the LPIPS term inside the masked pre-training loss; vmae_pretrain.py
# refuses it by name rather than train a different objective silently); stage 3's are the reference's (train_ae.sh:84-106) as they stand -- with its
# --mask_ratio 0.0 the reference freezes nothing, and neither does this.  torch.distributed.run replaces the deprecated torch.distributed.launch; fp16 = the
# reference's torch.amp.autocast('cuda').
GPUS_PER_NODE=${GPUS_PER_NODE:-8}
DATA_PATH=${DATA_PATH:-/data/dataset/imagenet/1K_dataset}
OUT=${OUT:-./work_dir/vmae_before_decoder_finetuning}
export HSA_ENABLE_IPC_MODE_LEGACY=${HSA_ENABLE_IPC_MODE_LEGACY:-0}     # dmabuf IPC: RCCL needs it on this driver
cd "$(dirname "$0")" || exit 1

stage1=(--batch_size 128 --no_cls --accum_iter 2 --num_workers 12 --smooth_output --fixed_std 1e-3 --model mae_for_ldmae_f8d16_prev --input_size 128
        --mask_ratio 0.25 --visible_loss_ratio 0.75 --epochs 400 --warmup_epochs 10 --blr 1.0e-4 --weight_decay 0.05 --kl_loss_weight 1e-6 --precision fp16
        --data_path "$DATA_PATH" --output_dir "$OUT" --log_dir "$OUT")
# PACKED_DATA_128 / PACKED_DATA_256: packs of DATA_PATH written by `python -m ldmae_amd.pack_images` (--short_side 160 / 320: README) -- the
# training transform then runs on the device (vmae_pretrain.py --packed_data) instead of in DataLoader workers; unset = the image folder as before
[ -n "$PACKED_DATA_128" ] && stage1+=(--packed_data "$PACKED_DATA_128")
echo "Stage 1: VMAE pre-training (128 x 128, mask ratio 0.25)"
python -m torch.distributed.run --nproc-per-node "$GPUS_PER_NODE" --nnodes 1 --node-rank 0 --master-addr 127.0.0.1 vmae_pretrain.py "${stage1[@]}" "$@" || exit 1

echo "Stage 2: position embeddings of epoch 90's checkpoint -> the 256 x 256 grid"
python pe_reset.py --model_name mae_for_ldmae_f8d16_prev --ckpt_dir "$OUT/checkpoint-90.pth" || exit 1

OUT3=${OUT3:-./work_dir/vmae}
stage3=(--no_cls --tune_decoder --perceptual_loss_ratio 10.0 --batch_size 16 --accum_iter 16 --smooth_output --num_workers 12 --model mae_for_ldmae_f8d16_prev
        --input_size 256 --mask_ratio 0.0 --visible_loss_ratio 0.5 --epochs 10 --save_epochs 1 --warmup_epochs 0 --blr 1.0e-5 --weight_decay 0.05 --kl_loss_weight 0.0
        --precision fp16 --data_path "$DATA_PATH" --output_dir "$OUT3" --log_dir "$OUT3" --resume "$OUT/checkpoint-90.pth")
[ -n "$PACKED_DATA_256" ] && stage3+=(--packed_data "$PACKED_DATA_256")
[ -n "$LPIPS_VGG" ] && stage3+=(--lpips_vgg "$LPIPS_VGG")
[ -n "$LPIPS_LIN" ] && stage3+=(--lpips_lin "$LPIPS_LIN")
# LPIPS_PRECISION=fp16: the VGG in 16 bits (fp16 forward, bf16 data gradient; models/lpips.py); default f32 = exact
stage3+=(--lpips_precision "${LPIPS_PRECISION:-f32}")
echo "Stage 3: decoder tuning (256 x 256, LPIPS ratio 10.0)"
python -m torch.distributed.run --nproc-per-node "$GPUS_PER_NODE" --nnodes 1 --node-rank 0 --master-addr 127.0.0.1 vmae_pretrain.py "${stage3[@]}" "$@" || exit 1
