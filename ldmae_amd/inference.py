#!/usr/bin/env python3
"""Sampling driver -- counterpart of the reference's LDMAE/inference.py (`run_inference.sh`): EMA checkpoint -> shifted-grid
ODE (sample.sampling_method: euler / heun / midpoint / dopri5), or with sample.mode SDE the Euler-Maruyama / Heun SDE, with classifier-free guidance (CFG on the first three channels, interval
gate) -> latent de-normalisation -> VMAE ``decode_to_images`` -> PNGs.  Ranks are independent replicas (seed = global_seed * world + rank, inference.py:87)."""
import argparse
import math
import os
import sys

import torch
import yaml

_HERE = os.path.dirname(os.path.abspath(__file__))
for p in (_HERE, os.path.dirname(_HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from ldmae_amd.guidance import Guidance                      # noqa: E402
from ldmae_amd.models.lightningdit import _act_dtype        # noqa: E402
from ldmae_amd.tokenizer import models_mae                  # noqa: E402
from ldmae_amd.train_accum import build_model               # noqa: E402
from ldmae_amd.transport import Sampler, create_transport   # noqa: E402


def build_sampler(cfg):
    t, s = cfg['transport'], cfg['sample']
    tr = create_transport(t['path_type'], t['prediction'], t['loss_weight'], t['train_eps'], t['sample_eps'],
                          use_cosine_loss=t.get('use_cosine_loss', False), use_lognorm=t.get('use_lognorm', False))
    if s['mode'] == "SDE":
        return build_sde_sampler(cfg, tr)
    if s['mode'] != "ODE":
        raise NotImplementedError(f"Sampling mode {s['mode']} is not supported.")
    return Sampler(tr).sample_ode(sampling_method=s['sampling_method'], num_steps=s['num_sampling_steps'], atol=s['atol'], rtol=s['rtol'],
                                  reverse=s['reverse'], timestep_shift=s.get('timestep_shift', 0))


SDE_DEFAULTS = dict(diffusion_form="sigma", diffusion_norm=1.0, last_step="Mean", last_step_size=0.04)
SDE_METHOD_NAMES = {"euler": "Euler", "heun": "Heun"}


def sde_options(cfg):
    """The keyword arguments of Sampler.sample_sde from the YAML's sample.* keys: sampling_method (the ODE's key; 'euler' / 'heun' in any case),
    num_sampling_steps, and the optional diffusion_form (default 'sigma': finite at t0 = 0, unlike the sampler's own default SBDM),
    diffusion_norm, last_step ('None' / null for no last step), last_step_size."""
    s = cfg['sample']
    method = SDE_METHOD_NAMES.get(str(s['sampling_method']).lower())
    if method is None:
        raise NotImplementedError(f"sample.mode SDE: sampling_method {s['sampling_method']!r} is not supported: 'euler' or 'heun'")
    kw = {k: s.get(k, d) for k, d in SDE_DEFAULTS.items()}
    if kw['last_step'] in ("None", "none"):
        kw['last_step'] = None
    return dict(kw, sampling_method=method, num_steps=s['num_sampling_steps'])


def build_sde_sampler(cfg, tr):
    """sample.mode SDE.  create_transport forces sample_eps = 0 for the velocity model; the SBDM diffusion needs t0 = sample_eps > 0, so for that
    form the transport takes the YAML's transport.sample_eps (null or 0: Sampler.sample_sde refuses, saying why).  Every rank draws its own
    noise: seed = global_seed * world + rank, the rule of torch.manual_seed in do_sample."""
    kw = sde_options(cfg)
    if kw['diffusion_form'] == "SBDM":
        tr.sample_eps = cfg['transport'].get('sample_eps') or 0
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    seed = (cfg.get('train') or {}).get('global_seed', 0) * world + rank
    return Sampler(tr).sample_sde(seed=seed, keep_trajectory=False, **kw)


@torch.no_grad()
def sample_latents(model, sample_fn, n, cfg_scale, cfg_interval_start, device, num_classes=1000, generator=None, truncation=None,
                   labels=None, cfg_interval=True, guidance=None):
    """inference.py:264-292: z ~ N(0,I); CFG on a doubled batch with the null class; Euler; drop the null half.
    `truncation`: the resampling loop of :266-272 (|z| > bound redrawn, at most 100 rounds).  `labels` / `cfg_interval=False`: the demo
    branch (:219-232), fixed classes and guidance on every step.
    `guidance`: a function of ldmae_amd.guidance.Guidance.model_fn (the YAML key sample.guidance).  It replaces the cfg_scale branch: the state
    is NOT doubled (the function runs the negative forward itself, inside its interval), so dopri5's error norm runs over the n kept samples --
    a stated departure from the reference's doubled-batch norm.  cfg_scale / cfg_interval_start / cfg_interval are not read then."""
    if guidance is not None:
        guidance.guidance.check_sampler(sample_fn)          # a momentum under a solver with several evaluations per step: refused before the draw
    latent = model.x_embedder.img_size[0]
    z = torch.randn(n, model.in_channels, latent, latent, device=device, generator=generator)
    if truncation is not None:
        for _ in range(100):
            bad = z.abs() > truncation
            if not bool(bad.any()):
                break
            z[bad] = torch.randn(int(bad.sum()), device=device, generator=generator)
    if labels is None:
        y = torch.randint(0, num_classes, (n,), device=device, generator=generator)
    else:
        y = torch.as_tensor(labels, device=device, dtype=torch.long)
    if guidance is not None:
        guidance.reset()                     # the APG momentum belongs to one trajectory
        out = sample_fn(z, guidance, y=y)[-1]
    elif cfg_scale > 1.0:
        z = torch.cat([z, z], 0)
        y = torch.cat([y, torch.full((n,), num_classes, device=device)], 0)
        # dopri5's error norm runs over the whole doubled batch, as the reference's does: it gets forward_with_cfg at every evaluation
        fixed_step = getattr(getattr(sample_fn, "__self__", None), "sampler_type", "euler") != "dopri5"

        def cfg_forward(x, t, y, cfg_scale, cfg_interval=None, cfg_interval_start=None):
            # Below the interval start forward_with_cfg applies NO guidance (lightningdit.py:436-439): the conditional half gets its own
            # output, and the unconditional half's output is never used for the samples that are kept -- every step rebuilds the doubled
            # batch from the first half of the state (:423-424) and only that half is returned (inference.py:288).  So those steps run the
            # conditional half alone (the model is bitwise independent of the batch: tests/test_gpu_dit.py); 27 % of the 250 steps of the
            # shipped configuration (interval start 0.10, timestep shift 0.3).  The gate reads t[0] on the host, as the reference's does.
            # Valid ONLY for a fixed-step, per-sample-independent integrator (the shipped Euler / Heun grid): the second half returned here is
            # the conditional output again, which an adaptive solver's error norm would see.  And only while the half batch takes the same
            # adaLN path as the doubled one (the batched bf16 adaLN GEMM needs a batch that is a multiple of 8; an n of 4, 12, 20 ... would put
            # the half on the per-block f32 path and the guided steps on the batched bf16 one: not bit-for-bit the doubled batch any more).
            same_path = _act_dtype(getattr(model, "precision", None)) != torch.bfloat16 or (len(x) // 2) % 8 == 0 or len(x) % 8 != 0
            if fixed_step and cfg_interval is True and cfg_interval_start and float(t[0]) < cfg_interval_start and same_path:
                half = len(x) // 2
                out = model.forward(x[:half], t[:half], y[:half])
                return torch.cat([out, out], dim=0)
            return model.forward_with_cfg(x, t, y, cfg_scale, cfg_interval, cfg_interval_start)
        out = sample_fn(z, cfg_forward, y=y, cfg_scale=cfg_scale, cfg_interval=cfg_interval, cfg_interval_start=cfg_interval_start)[-1]
        out, _ = out.chunk(2, dim=0)
    else:
        out = sample_fn(z, model.forward, y=y)[-1]
    return out, y[:n]


class PngWriter:
    """PNG encoding on a host thread: the reference writes each image synchronously inside the sampling loop (inference.py:293-297),
    so the GPU sits idle while 256 PNGs are compressed; here the loop hands the uint8 batch over and goes on enqueueing the next
    batch's Euler steps.  Bounded queue (2 batches) so host memory stays flat; `close()` drains it and re-raises a writer error."""

    def __init__(self, depth=2):
        import queue
        import threading
        self.q, self.err = queue.Queue(maxsize=depth), None
        self.th = threading.Thread(target=self._run, daemon=True)
        self.th.start()

    def _run(self):
        from PIL import Image
        while True:
            item = self.q.get()
            if item is None:
                return
            try:
                imgs, paths = item
                for im, path in zip(imgs, paths):
                    Image.fromarray(im).save(path)
            except Exception as e:          # surfaced by close()
                self.err = e

    def put(self, imgs, paths):
        if self.err is not None:
            raise self.err
        self.q.put((imgs, paths))

    def close(self):
        self.q.put(None)
        self.th.join()
        if self.err is not None:
            raise self.err


DEMO_LABELS = [975, 3, 207, 387, 388, 88, 979, 279]          # inference.py:223


def sample_folder_name(cfg, ckpt_path, cfg_scale=None):
    """The directory name rule of inference.py:45-52 (the FID tooling downstream finds the PNGs by it).  With the key sample.guidance the name
    gains Guidance.folder_suffix(): the rule, the source, k and every parameter, so two settings never share a folder."""
    s = cfg['sample']
    method = ("sde-" if s.get('mode') == "SDE" else "") + s['sampling_method']          # the SDE's euler is not the ODE's: its own folder
    name = f"{cfg['model']['model_type'].replace('/', '-')}-ckpt-{ckpt_path.split('/')[-1].split('.')[0]}-{method}-{s['num_sampling_steps']}".lower()
    cfg_scale = s['cfg_scale'] if cfg_scale is None else cfg_scale
    if cfg_scale > 1.0:
        name += f"-interval{s.get('cfg_interval_start', 0):.2f}" + f"-cfg{cfg_scale:.2f}" + f"-shift{s.get('timestep_shift', 0):.2f}"
    if s.get('guidance') is not None:
        name += Guidance.from_config(cfg).folder_suffix()
    return name


def build_vae(cfg, device):
    """inference.py:129-136.  The reference's other branch (`ae/dae/vae/sdv3` -> a diffusers AutoencoderKL, :137-167) is a different tokenizer
    family, outside this package: refused by name."""
    kind = cfg['vae']['model_name'].split("_")[0]
    if kind != 'vmae':
        raise NotImplementedError(f"vae.model_name {cfg['vae']['model_name']!r}: only the VMAE tokenizer ('vmae_*') is built here; "
                                  "the reference's diffusers AutoencoderKL branch is out of scope")
    vae = models_mae.mae_for_ldmae_f8d16_prev(ldmae_mode=True, no_cls=True, kl_loss_weight=True, smooth_output=True,
                                              img_size=cfg['data']['image_size'])
    vck = torch.load(cfg['vae']['weight_path'], map_location='cpu')
    vae.load_state_dict(vck['model'], strict=False)
    return vae.to(device).eval()


def latent_stats(cfg, device):
    """inference.py:203-217: the statistics come through the latent dataset -- the cached latents_stats.pt when it is there (downloaded with the
    checkpoint), otherwise computed from the shards of data_path and cached, exactly as the reference's ImgLatentDataset.get_latent_stats does."""
    data_dir = cfg['data']['data_path'] + ('_sample' if 'sample' in cfg['data'] else '')
    cache = os.path.join(data_dir, "latents_stats.pt")
    if os.path.exists(cache):
        stats = torch.load(cache)
        mean, std = stats['mean'], stats['std']
    else:
        from ldmae_amd.datasets.img_latent_dataset import ImgLatentDataset
        mean, std = ImgLatentDataset(data_dir, latent_norm=cfg['data'].get('latent_norm', False), latent_multiplier=cfg['data'].get('latent_multiplier', 0.18215),
                                     sample=cfg['data'].get('sample', False)).get_latent_stats()
    return mean.to(device), std.to(device)


GEMM_PRECISIONS = (None, "mxfp8")
MX8_NOTICE = ("gemm_precision=mxfp8: the four GEMMs of every DiT block run in MXFP8 (block-scaled OCP e4m3, one E8M0 scale per 32 along K); "
              "the mode's effect on FID has not been measured")


def resolve_gemm_precision(cfg, flag=None):
    """The block-GEMM arithmetic of the sampler: the --gemm_precision flag when given, else the YAML key sample.gemm_precision, else None (the
    activation type's own GEMMs, as before the key existed)."""
    mode = flag if flag is not None else (cfg.get('sample') or {}).get('gemm_precision')
    if mode in ("", "none", "None"):
        mode = None
    if mode not in GEMM_PRECISIONS:
        raise SystemExit(f"gemm_precision={mode!r}: 'mxfp8', or absent for the activation type's own GEMMs")
    return mode


GUIDANCE_NOTICE = "sample.guidance: the effect of the guidance rules (all-channel CFG, rescale, APG, autoguidance) on FID has not been measured"


def build_guidance(cfg, model, device, gemm_precision=None):
    """The guided model function of sample.guidance for `model`.  source auto: the guide is built from the same YAML with
    guidance.guide_model_type, loaded from guidance.guide_ckpt as the main model is (guide_weights ema: the checkpoint's "ema" entry, or the
    file itself when it is a bare state dict such as a post-hoc EMA reconstruction; model: its "model" entry), at the same gemm_precision."""
    g = Guidance.from_config(cfg)
    guide = None
    if g.source == "auto":
        gcfg = dict(cfg, model=dict(cfg['model'], model_type=g.guide_model_type))
        guide = build_model(gcfg, learn_sigma=cfg['model'].get('learn_sigma', False))
        ck = torch.load(g.guide_ckpt, map_location='cpu')
        if g.guide_weights == "model":
            if "model" not in ck:
                raise KeyError(f"sample.guidance.guide_weights model: {g.guide_ckpt} has no 'model' entry")
            ck = {k.replace('module.', ''): v for k, v in ck["model"].items()}
        elif "ema" in ck:
            ck = ck["ema"]
        guide.load_state_dict(ck)
        guide = guide.to(device).eval()
        if gemm_precision is not None:
            guide.set_gemm_precision(gemm_precision)
    return g.model_fn(model, guide)


def do_sample(cfg, ckpt_path, out_dir=None, num_samples=None, precision="bf16", cfg_scale=None, demo=False, gemm_precision=None):
    """inference.py:40-300.  `out_dir=None` -> <train.output_dir>/<train.exp_name>/<sample_folder_name> as the reference; a folder that already
    holds more than `fid_num` PNGs is left alone (:69-77).  `demo=True`: the eight fixed classes, guidance on every step, unshifted grid, one
    2 x 4 sheet under ./demo_images (:54-57, :219-262) written by rank 0; returns None as the reference does."""
    rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
    s = cfg['sample']
    if s.get('guidance') is not None:                        # every refusal of the key happens here, before anything is loaded
        if demo:
            raise NotImplementedError("sample.guidance with --demo: the demo sheet is the reference's CFG; remove the key or --demo")
        Guidance.from_config(cfg)
    cfg_scale = s['cfg_scale'] if cfg_scale is None else cfg_scale
    if out_dir is None:
        out_dir = os.path.join(cfg['train']['output_dir'], cfg['train']['exp_name'], sample_folder_name(cfg, ckpt_path, cfg_scale))
    want = num_samples or s['fid_num']
    if not demo and os.path.isdir(out_dir) and sum(f.endswith('.png') for f in os.listdir(out_dir)) > want:
        if rank == 0:
            print(f"Found more than {want} PNG files in {out_dir}, skip sampling.")
        return out_dir
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    torch.manual_seed(cfg['train']['global_seed'] * world + rank)
    model = build_model(cfg, learn_sigma=cfg['model'].get('learn_sigma', False))        # inference.py:336-348
    ck = torch.load(ckpt_path, map_location='cpu')
    model.load_state_dict(ck["ema"] if "ema" in ck else ck)
    model = model.to(device).eval()
    if gemm_precision is None:
        gemm_precision = resolve_gemm_precision(cfg)
    if gemm_precision is not None:
        model.set_gemm_precision(gemm_precision)
        if rank == 0:
            print(MX8_NOTICE)
    guided = None
    if s.get('guidance') is not None:                        # opt-in: absent, nothing below differs from before the key existed
        guided = build_guidance(cfg, model, device, gemm_precision)
        if rank == 0:
            print(GUIDANCE_NOTICE)
    if demo:                                                  # :54-57 -- the demo sheet is drawn with guidance on every step of the unshifted grid
        cfg = dict(cfg, sample=dict(s, cfg_interval_start=0, timestep_shift=0))
        s = cfg['sample']
    sample_fn = build_sampler(cfg)
    vae = build_vae(cfg, device)
    mean, std = latent_stats(cfg, device)
    mult = cfg['data'].get('latent_multiplier', 0.18215)

    def decode(lat):
        # inference.py:79 of the reference sets allow_tf32: the f32 decode runs TF32-class (fp16 operands = TF32's mantissa, f32
        # accumulation: the LDMAE_F16 kernel family); LDMAE_TF32=0 keeps the exact-f32 kernels
        with models_mae.reference_tf32():
            return vae.decode_to_images(lat * std / mult + mean)                      # uint8 NHWC on the host (inference.py:290-292)

    if demo:
        if rank != 0:
            return None
        import numpy as np
        from PIL import Image
        sheet = []
        for label in (DEMO_LABELS if cfg_scale > 1.0 else [0] * 8):                    # one image per call, as :224-245 (the noise stream depends on it)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=precision == "bf16"):
                lat, _ = sample_latents(model, sample_fn, 1, cfg_scale, 0, device, cfg['data']['num_classes'], labels=[label], cfg_interval=False)
            sheet.append(decode(lat)[0])
        h, w = sheet[0].shape[:2]
        grid = np.zeros((2 * h, 4 * w, 3), np.uint8)
        for k, im in enumerate(sheet):
            i, j = divmod(k, 4)
            grid[i * h:(i + 1) * h, j * w:(j + 1) * w] = im
        os.makedirs('demo_images', exist_ok=True)
        ckpt_iter = ckpt_path.split("/")[-1][:-3]
        Image.fromarray(grid).save(f"demo_images/{cfg['train']['exp_name']}_cfg{cfg_scale}_{ckpt_iter}_demo_samples.png")
        return None

    n = s['per_proc_batch_size']
    total = int(math.ceil(want / (n * world)) * n * world)
    # :266-272 -- the reference looks the switch up under the key 'trunaction' (sic) and the bound under 'truncation'; a config written for it
    # behaves the same here
    trunc = s['truncation'] if 'trunaction' in s else None
    os.makedirs(out_dir, exist_ok=True)
    done = 0
    writer = PngWriter()
    try:
        for it in range(total // (n * world)):
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=precision == "bf16"):
                lat, _ = sample_latents(model, sample_fn, n, cfg_scale, s.get('cfg_interval_start', 0), device, cfg['data']['num_classes'], truncation=trunc,
                                        **({} if guided is None else {"guidance": guided}))
            solver = getattr(sample_fn, "__self__", None)
            if it == 0 and rank == 0 and getattr(solver, "sampler_type", None) == "dopri5":
                print(f"dopri5 (atol {solver.atol:g}, rtol {solver.rtol:g}): nfe {solver.nfe}, accepted {solver.accepted}, rejected {solver.rejected}")
            if it == 0 and rank == 0 and hasattr(sample_fn, "model_calls"):
                print(f"SDE ({sample_fn.sde.sampler_type}, {len(sample_fn.sde.t)} steps): {sample_fn.model_calls} model calls per batch")
            imgs = decode(lat)
            writer.put(imgs, [f"{out_dir}/{i * world + rank + done:06d}.png" for i in range(len(imgs))])   # index rule: inference.py:294
            done += n * world
    finally:
        writer.close()
    return out_dir


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', type=str, default='configs/lightningdit_b_ldmvae_f16d16.yaml')           # inference.py:318
    ap.add_argument('--demo', action='store_true', default=False)                                          # inference.py:319
    ap.add_argument('--ckpt', type=str, default=None, help="default: the config's ckpt_path (inference.py:324-327)")
    ap.add_argument('--out', type=str, default=None, help="default: <output_dir>/<exp_name>/<the reference's folder name>")
    ap.add_argument('--gemm_precision', type=str, default=None, choices=['mxfp8', 'none'],
                    help="block-GEMM arithmetic of the DiT (overrides the YAML key sample.gemm_precision); mxfp8: MX block-scaled fp8, forward-only bf16")
    ap.add_argument('--guidance_rule', type=str, default=None, choices=['cfg', 'rescale', 'apg'], help="overrides the YAML key sample.guidance.rule")
    ap.add_argument('--guidance_source', type=str, default=None, choices=['null_class', 'auto'], help="overrides sample.guidance.source")
    ap.add_argument('--guidance_channels', type=str, default=None, help="overrides sample.guidance.channels: 'all' or an integer")
    ap.add_argument('--guide_ckpt', type=str, default=None, help="overrides sample.guidance.guide_ckpt (the guiding model of source auto)")
    ap.add_argument('--mode', type=str, default=None, choices=['ODE', 'SDE'],
                    help="overrides the YAML key sample.mode; SDE: Euler-Maruyama / Heun with the optional keys sample.diffusion_form (default "
                         "sigma), diffusion_norm, last_step, last_step_size")
    return ap


def apply_guidance_flags(c, a):
    """The --guidance_* / --guide_ckpt flags over the YAML's sample.guidance, the way --mode overrides sample.mode; no flag: c itself."""
    over = {k: v for k, v in (("rule", a.guidance_rule), ("source", a.guidance_source), ("channels", a.guidance_channels),
                              ("guide_ckpt", a.guide_ckpt)) if v is not None}
    if not over:
        return c
    if "channels" in over and over["channels"] != "all":
        try:
            over["channels"] = int(over["channels"])
        except ValueError:
            raise SystemExit(f"--guidance_channels {over['channels']!r}: 'all' or an integer")
    return dict(c, sample=dict(c['sample'], guidance=dict(c['sample'].get('guidance') or {}, **over)))


def main(argv=None):
    a = build_parser().parse_args(argv)
    c = yaml.safe_load(open(a.config))
    if a.mode is not None:
        c = dict(c, sample=dict(c['sample'], mode=a.mode))
    c = apply_guidance_flags(c, a)
    if a.ckpt is None:
        assert 'ckpt_path' in c, "ckpt_path must be specified in config"
    # run_inference.sh passes --mixed_precision $PRECISION (default bf16) to the launcher, which exports ACCELERATE_MIXED_PRECISION; the
    # reference's sampler never prepares the model, so there the flag is inert and it samples in f32 with TF32 matmuls -- here it selects the
    # activation type (bf16 = BASELINE config 5; PRECISION=fp32 / no -> the exact-f32 kernels)
    precision = os.environ.get("PRECISION") or os.environ.get("ACCELERATE_MIXED_PRECISION") or "bf16"
    precision = {"no": "fp32"}.get(precision, precision)
    if precision not in ("bf16", "fp32"):
        raise SystemExit(f"PRECISION={precision!r}: the sampler runs in bf16 or fp32")
    gemm_precision = resolve_gemm_precision(c, a.gemm_precision)
    if a.gemm_precision == "none":            # the flag overrides the YAML in both directions
        c = dict(c, sample={k: v for k, v in c['sample'].items() if k != 'gemm_precision'})
    folder = do_sample(c, a.ckpt or c['ckpt_path'], a.out, demo=a.demo, precision=precision, gemm_precision=gemm_precision)
    if not a.demo and int(os.environ.get("RANK", 0)) == 0:
        # inference.py:352-367: an Inception FID of the samples against data.fid_reference_file (tools/calculate_fid.py -> ldmae_amd.fid), run
        # when that file exists (a relative path is taken from the working directory) and the user's Inception weights resolve
        from . import fid as fid_mod
        ref = c['data'].get('fid_reference_file')
        missing = []
        if not ref or not os.path.exists(ref):
            missing.append(f"data.fid_reference_file {ref!r} does not exist")
        try:
            fid_mod.resolve_weights()
        except FileNotFoundError as e:
            missing.append(str(e))
        if missing:
            print(f"samples written to {folder}; FID (tools/calculate_fid.py in the reference) is not part of this package")
            print("FID skipped: " + "; ".join(missing))
        else:
            print(f"Calculating FID with {c['sample']['fid_num']} number of samples")
            fid = fid_mod.calculate_fid_given_paths([ref, folder], batch_size=50, device='cuda', dims=2048, num_workers=8,
                                                    sp_len=c['sample']['fid_num'])
            print('fid=', fid)
    return folder


if __name__ == "__main__":
    main()
