"""Pack a folder of samples into the .npz the ADM evaluator reads (the reference's tools/save_npz.py:11-41).

    python -m ldmae_amd.save_npz config.yaml [--num 50000]

writes {sample_dir}.npz with arr_0 = uint8 [N, H, W, 3], sample_dir = <train.output_dir>/<train.exp_name>/<inference.sample_folder_name>,
the folder inference.py samples into.  The first N PNG files are taken in SORTED file-name order, where the reference takes os.listdir's
order (arbitrary, file-system dependent).  The order matters to the Inception Score, whose splits are runs of consecutive images.
The array is written one image at a time into the zip member (np.savez's layout: stored, arr_0.npy), so 50 000 images at 256 x 256 never
sit in memory together.
"""
from __future__ import annotations

import argparse
import os
import zipfile

import numpy as np


def sample_dir_of(cfg):
    from .inference import sample_folder_name
    return os.path.join(cfg['train']['output_dir'], cfg['train']['exp_name'], sample_folder_name(cfg, cfg['ckpt_path']))


def png_files(sample_dir, num):
    files = sorted(f for f in os.listdir(sample_dir) if f.lower().endswith(".png"))
    if len(files) < num:
        raise ValueError(f"{sample_dir} holds {len(files)} PNG files, fewer than the {num} asked for")
    return [os.path.join(sample_dir, f) for f in files[:num]]


def create_npz_from_sample_folder(sample_dir, num=50_000):
    """Write {sample_dir}.npz with arr_0 = the first `num` PNGs (sorted names) as uint8 [num, H, W, 3]; returns its path."""
    from .fid import _decode
    files = png_files(sample_dir, num)
    first = _decode(files[0])
    if first.ndim != 3 or first.shape[2] != 3:
        raise ValueError(f"{files[0]}: expected an RGB image, got shape {first.shape}")
    shape = (num, *first.shape)
    npz_path = f"{sample_dir.rstrip(os.sep)}.npz"
    tmp = npz_path + ".tmp"
    try:
        with zipfile.ZipFile(tmp, "w", zipfile.ZIP_STORED, allowZip64=True) as z:
            with z.open("arr_0.npy", "w", force_zip64=True) as f:
                header = {"descr": np.lib.format.dtype_to_descr(np.dtype(np.uint8)), "fortran_order": False, "shape": shape}
                np.lib.format.write_array_header_2_0(f, header) if len(repr(header)) > 65000 else np.lib.format.write_array_header_1_0(f, header)
                for i, path in enumerate(files):
                    img = first if i == 0 else _decode(path)
                    if img.shape != first.shape:
                        raise ValueError(f"{path}: shape {img.shape}, expected {first.shape} like {files[0]}")
                    f.write(np.ascontiguousarray(img, dtype=np.uint8).tobytes())
        os.replace(tmp, npz_path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    print(f"Saved .npz file to {npz_path} [shape={shape}].")
    return npz_path


def main(argv=None):
    import yaml
    ap = argparse.ArgumentParser(description="Pack the samples of a config's sample folder into {sample_dir}.npz (arr_0, uint8 NHWC)")
    ap.add_argument("config", type=str)
    ap.add_argument("--num", type=int, default=50_000, help="number of PNG files to pack (sorted names)")
    a = ap.parse_args(argv)
    with open(a.config) as f:
        cfg = yaml.safe_load(f)
    return create_npz_from_sample_folder(sample_dir_of(cfg), a.num)


if __name__ == "__main__":
    main()
