#!/usr/bin/env python3
"""Post-hoc EMA: power-function EMA profiles, the snapshot directory, and the reconstruction of any EMA width after training.

Karras et al. 2024, "Analyzing and Improving the Training Dynamics of Diffusion Models", section 3.  THE CONTRACT (also restated at the
kernel, csrc/pointwise.hip):

Power-function EMA.  Step t counts optimizer steps from 1.  With exponent gamma:
    beta(t) = (1 - 1/t)^(gamma+1)
    e(t)    = beta e(t-1) + (1 - beta) theta(t)        theta(t): the parameter AFTER the AdamW update of step t
    beta(1) = 0, so e(1) = theta(1) whatever the slab held before.
    The weight of theta(tau) in e(t) is w_tau = (1 - beta(tau)) (tau/t)^(gamma+1); the weights sum to exactly 1 over tau = 1..t.
    Their continuous form is p_{t,gamma}(tau) = (gamma+1) tau^gamma / t^(gamma+1) on [0, t].
Width.  sigma_rel = (gamma+1)^(1/2) (gamma+2)^(-1) (gamma+3)^(-1/2): the standard deviation of the profile relative to t.  gamma is the
    largest real root of  g^3 + 7 g^2 + (16 - sigma_rel^-2) g + (12 - sigma_rel^-2) = 0;  0 < sigma_rel < 12^(-1/2) ~ 0.2887.
Reconstruction.  For two profiles a = (t_a, gamma_a), b = (t_b, gamma_b):
    <a, b> = (gamma_a+1)(gamma_b+1) / (gamma_a+gamma_b+1) * min(t_a,t_b)^(gamma_a+gamma_b+1) / (t_a^(gamma_a+1) t_b^(gamma_b+1))
    evaluated in logs, in f64.  Given stored snapshots i and a target r = (t_r, gamma_r): solve A x = b, A_ij = <i, j>, b_i = <i, r>, by
    least squares in f64 on the host, scale x to sum to 1; the reconstructed parameters are sum_i x_i snapshot_i (f64 accumulator on the GPU).

Command line:
    python -m ldmae_amd.posthoc_ema --snapshots <dir> --sigma_rel 0.075 [--step T] --out ema_0075.pt [--base <ckpt.pt>]
    python -m ldmae_amd.posthoc_ema --snapshots <dir> --list
The output is a checkpoint whose "ema" entry is the reconstructed state dict (with --base: plus that checkpoint's "model" and "config", and
its non-parameter "ema" entries), which inference.py / run_inference.sh load unchanged.

The mathematics here needs numpy only; torch and the HIP library are imported where the slabs are combined.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

FORMAT, VERSION, INDEX = "ldmae-posthoc-ema-snapshots", 1, "snapshots.json"
SIGMA_REL_MAX = 12.0 ** -0.5
MAX_TRACKS = 4


# ----------------------------------------------------------------------------- profiles
def check_sigma_rel(sigma_rel) -> float:
    s = float(sigma_rel)
    if not (0.0 < s < SIGMA_REL_MAX):
        raise ValueError(f"posthoc_ema: sigma_rel {sigma_rel!r} is outside (0, 12^-1/2 = {SIGMA_REL_MAX:.4f}): no power-function profile has "
                         f"that relative width")
    return s


def sigma_rel_to_gamma(sigma_rel) -> float:
    """The exponent of the profile of relative width sigma_rel: the largest real root of the cubic above (then polished by Newton steps on
    the cubic, in f64)."""
    s = check_sigma_rel(sigma_rel)
    t = s ** -2
    roots = np.roots([1.0, 7.0, 16.0 - t, 12.0 - t])
    g = float(max(r.real for r in roots if abs(r.imag) <= 1e-9 * max(1.0, abs(r.real))))
    for _ in range(3):
        f, df = ((g + 7.0) * g + (16.0 - t)) * g + (12.0 - t), (3.0 * g + 14.0) * g + (16.0 - t)
        if df == 0.0:
            break
        g -= f / df
    return g


def gamma_to_sigma_rel(gamma) -> float:
    g = float(gamma)
    return math.sqrt(g + 1.0) / ((g + 2.0) * math.sqrt(g + 3.0))


def track_coef(gamma, t) -> float:
    """c = 1 - beta(t) = -expm1((gamma+1) log1p(-1/t)) in f64; 1 at t = 1."""
    t = int(t)
    if t < 1:
        raise ValueError(f"posthoc_ema: step {t} (steps count from 1)")
    return 1.0 if t == 1 else -math.expm1((float(gamma) + 1.0) * math.log1p(-1.0 / t))


def discrete_weights(t, gamma, lo=1, hi=None) -> np.ndarray:
    """w_tau for tau = lo..hi (default 1..t) of the profile (t, gamma), f64; zero for tau > t."""
    t, hi = int(t), int(t if hi is None else hi)
    tau = np.arange(lo, hi + 1, dtype=np.float64)
    w = np.zeros_like(tau)
    m = tau <= t
    tm = tau[m]
    with np.errstate(divide="ignore"):
        c = -np.expm1((gamma + 1.0) * np.log1p(-1.0 / tm))          # tau = 1: log1p(-1) = -inf, expm1(-inf) = -1, c = 1
    w[m] = c * np.exp((gamma + 1.0) * np.log(tm / t))
    return w


def log_inner(ta, ga, tb, gb):
    """log <a, b> of two continuous profiles, f64 (broadcasts)."""
    ta, ga, tb, gb = (np.asarray(v, dtype=np.float64) for v in (ta, ga, tb, gb))
    return (np.log(ga + 1.0) + np.log(gb + 1.0) - np.log(ga + gb + 1.0) + (ga + gb + 1.0) * np.log(np.minimum(ta, tb))
            - (ga + 1.0) * np.log(ta) - (gb + 1.0) * np.log(tb))


def inner(ta, ga, tb, gb):
    return np.exp(log_inner(ta, ga, tb, gb))


def solve_coefficients(steps, gammas, t_r, gamma_r):
    """x (summing to 1) such that sum_i x_i profile(steps[i], gammas[i]) is the least-squares fit of profile(t_r, gamma_r); also the
    condition number of A.  steps / gammas list one entry per stored snapshot."""
    steps, gammas = np.asarray(steps, dtype=np.float64), np.asarray(gammas, dtype=np.float64)
    if steps.size < 2:
        raise ValueError(f"posthoc_ema: {steps.size} snapshot(s); a reconstruction needs at least 2")
    A = inner(steps[:, None], gammas[:, None], steps[None, :], gammas[None, :])
    b = inner(steps, gammas, float(t_r), float(gamma_r))
    x = np.linalg.lstsq(A, b, rcond=None)[0]
    x = x / x.sum()
    return x, float(np.linalg.cond(A))


def profile_residual(steps, gammas, x, t_r, gamma_r, chunk=1 << 16):
    """(||x . W - w_r||_2, ||w_r||_2) over tau = 1..max step, on the DISCRETE weights w_tau (what the slabs really hold), in chunks of tau."""
    top = int(max(max(steps), t_r))
    num = den = 0.0
    for lo in range(1, top + 1, chunk):
        hi = min(top, lo + chunk - 1)
        fit = np.zeros(hi - lo + 1)
        for s, g, xi in zip(steps, gammas, x):
            if s >= lo:
                fit += xi * discrete_weights(s, g, lo, hi)
        w = discrete_weights(t_r, gamma_r, lo, hi)
        num += float(((fit - w) ** 2).sum())
        den += float((w ** 2).sum())
    return math.sqrt(num), math.sqrt(den)


# ----------------------------------------------------------------------------- the snapshot directory
def snapshot_file(step, track) -> str:
    return f"step{int(step):09d}_track{int(track)}.f32"


def new_index(layout, numel, sigma_rels) -> dict:
    """layout: (name, offset, shape) of every parameter in the slab of `numel` f32 elements."""
    sig = [check_sigma_rel(s) for s in sigma_rels]
    return {"format": FORMAT, "version": VERSION, "dtype": "float32", "numel": int(numel),
            "layout": [[str(n), int(o), [int(d) for d in shape]] for n, o, shape in layout],
            "sigma_rels": sig, "gammas": [sigma_rel_to_gamma(s) for s in sig], "steps": []}


def write_index(directory, index) -> None:
    """Atomically: a reader sees the old index or the new one, never a partial file."""
    tmp = os.path.join(directory, INDEX + ".tmp")
    with open(tmp, "w") as f:
        json.dump(index, f, indent=1)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, os.path.join(directory, INDEX))


def read_index(directory, verify=True) -> dict:
    """The index of a snapshot directory, refused by name when it is not one, is of another version, or (verify) lists a snapshot whose file
    is missing or has another size than the layout says (an unfinished or mismatched directory)."""
    path = os.path.join(directory, INDEX)
    if not os.path.exists(path):
        raise RuntimeError(f"posthoc_ema: {directory} has no {INDEX}: not a snapshot directory")
    with open(path) as f:
        ix = json.load(f)
    if ix.get("format") != FORMAT or ix.get("version") != VERSION:
        raise RuntimeError(f"posthoc_ema: {path} is format {ix.get('format')!r} version {ix.get('version')!r}; this reader understands "
                           f"{FORMAT!r} version {VERSION}")
    need = ("numel", "layout", "sigma_rels", "gammas", "steps")
    if any(k not in ix for k in need) or len(ix["sigma_rels"]) != len(ix["gammas"]) or not 1 <= len(ix["gammas"]) <= MAX_TRACKS:
        raise RuntimeError(f"posthoc_ema: {path} is incomplete (needs {', '.join(need)}; 1..{MAX_TRACKS} tracks)")
    for n, o, shape in ix["layout"]:
        if o < 0 or o + int(np.prod(shape, dtype=np.int64)) > ix["numel"]:
            raise RuntimeError(f"posthoc_ema: {path}: parameter {n} at offset {o} with shape {shape} does not fit a slab of {ix['numel']} elements "
                               f"(mismatched layout)")
    if ix["steps"] != sorted(set(int(s) for s in ix["steps"])):
        raise RuntimeError(f"posthoc_ema: {path}: the steps are not strictly ascending integers")
    if verify:
        for s in ix["steps"]:
            for k in range(len(ix["gammas"])):
                p = os.path.join(directory, snapshot_file(s, k))
                if not os.path.exists(p) or os.path.getsize(p) != 4 * ix["numel"]:
                    raise RuntimeError(f"posthoc_ema: {p} is missing or is not {4 * ix['numel']} bytes (unfinished snapshot or mismatched layout)")
    return ix


def same_run(ix, layout, numel, sigma_rels) -> bool:
    fresh = new_index(layout, numel, sigma_rels)
    return all(ix[k] == fresh[k] for k in ("numel", "layout", "sigma_rels"))


def write_snapshot_files(directory, index, step, slabs) -> None:
    """One raw f32 file per track (host numpy arrays of index['numel'] elements), each renamed into place, THEN the index."""
    step = int(step)
    if index["steps"] and step <= index["steps"][-1]:
        if step in index["steps"]:
            index = dict(index, steps=[s for s in index["steps"] if s < step])        # a resumed run rewrites what it repeats
        else:
            raise RuntimeError(f"posthoc_ema: snapshot of step {step} after step {index['steps'][-1]}: steps must ascend")
    for k, a in enumerate(slabs):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.size != index["numel"]:
            raise RuntimeError(f"posthoc_ema: track {k} has {a.size} elements, the layout says {index['numel']}")
        tmp = os.path.join(directory, snapshot_file(step, k) + ".tmp")
        a.tofile(tmp)
        os.replace(tmp, os.path.join(directory, snapshot_file(step, k)))
    index["steps"] = [s for s in index["steps"] if s < step] + [step]
    write_index(directory, index)


# ----------------------------------------------------------------------------- reconstruction
def plan(index, sigma_rel, step=None):
    """Which snapshots with which coefficients: (entries [(step, track, x)], report dict).  Uses every snapshot up to the target step."""
    gamma_r = sigma_rel_to_gamma(sigma_rel)
    steps = [int(s) for s in index["steps"]]
    if not steps:
        raise RuntimeError("posthoc_ema: the directory holds no snapshot")
    t_r = steps[-1] if step is None else int(step)
    if t_r > steps[-1]:
        raise RuntimeError(f"posthoc_ema: --step {t_r} is past the last snapshot (step {steps[-1]}): an average cannot reach past what was stored")
    if t_r < 1:
        raise RuntimeError(f"posthoc_ema: --step {t_r} (steps count from 1)")
    use = [(s, k) for s in steps if s <= t_r for k in range(len(index["gammas"]))]
    if len(use) < 2:
        raise RuntimeError(f"posthoc_ema: {len(use)} snapshot(s) at or before step {t_r}; a reconstruction needs at least 2")
    st, gm = [s for s, _ in use], [index["gammas"][k] for _, k in use]
    x, cond = solve_coefficients(st, gm, t_r, gamma_r)
    num, den = profile_residual(st, gm, x, t_r, gamma_r)
    report = {"sigma_rel": float(sigma_rel), "gamma": gamma_r, "step": t_r, "snapshots": len(use), "coef_min": float(x.min()),
              "coef_max": float(x.max()), "condition": cond, "residual_abs": num, "residual_rel": num / den}
    return [(s, k, float(xi)) for (s, k), xi in zip(use, x)], report


def combine(directory, index, entries, device="cuda", chunk=1 << 24):
    """sum_i x_i snapshot_i as one f32 slab on the host: the files are memory-mapped, streamed through two pinned chunks into the f64
    accumulator on the GPU (ldmae_snapshot_accumulate), rounded once (ldmae_snapshot_finish)."""
    import torch
    from . import ops
    n = int(index["numel"])
    out = np.empty(n, dtype=np.float32)
    maps = [(np.memmap(os.path.join(directory, snapshot_file(s, k)), dtype=np.float32, mode="r", shape=(n,)), x) for s, k, x in entries]
    chunk = min(chunk, n)
    pins = [torch.empty(chunk, dtype=torch.float32).pin_memory() for _ in range(2)]
    free = [torch.cuda.Event() for _ in range(2)]           # recorded when the copy out of that pinned chunk has run
    used = [False, False]
    dev = [torch.empty(chunk, dtype=torch.float32, device=device) for _ in range(2)]
    acc = torch.empty(chunk, dtype=torch.float64, device=device)
    res = torch.empty(chunk, dtype=torch.float32, device=device)
    turn = 0
    for lo in range(0, n, chunk):
        k = min(chunk, n - lo)
        acc.zero_()
        for mm, x in maps:
            b = turn & 1
            turn += 1
            if used[b]:
                free[b].synchronize()
            pins[b][:k].numpy()[:] = mm[lo:lo + k]
            dev[b][:k].copy_(pins[b][:k], non_blocking=True)
            free[b].record()
            used[b] = True
            ops.snapshot_accumulate(acc[:k], dev[b][:k], x)
        ops.snapshot_finish(acc[:k], res[:k])
        out[lo:lo + k] = res[:k].cpu().numpy()
    return out


def state_dict_from_slab(index, slab):
    import torch
    sd = {}
    for n, o, shape in index["layout"]:
        k = int(np.prod(shape, dtype=np.int64))
        sd[n] = torch.from_numpy(slab[o:o + k].reshape(shape).copy())
    return sd


def reconstruct(directory, sigma_rel, step=None, device="cuda"):
    """(state dict, report) of the EMA of relative width sigma_rel at `step` (default: the last snapshot)."""
    index = read_index(directory)
    entries, report = plan(index, sigma_rel, step)
    return state_dict_from_slab(index, combine(directory, index, entries, device)), report


def describe(index) -> str:
    st = index["steps"]
    lines = [f"{FORMAT} v{index['version']}: {len(index['layout'])} parameters, {index['numel']} f32 elements per snapshot "
             f"({4 * index['numel'] / 2 ** 20:.1f} MiB)"]
    for k, (s, g) in enumerate(zip(index["sigma_rels"], index["gammas"])):
        lines.append(f"  track {k}: sigma_rel {s:g}, gamma {g:.4f}")
    lines.append(f"  {len(st)} snapshot step(s)" + (f": {st[0]} .. {st[-1]}" if st else ""))
    if st:
        lines.append("  steps: " + " ".join(map(str, st)))
    return "\n".join(lines)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="Reconstruct an EMA of any width from power-function EMA snapshots (post-hoc EMA).")
    ap.add_argument("--snapshots", required=True, help="directory written during training (train.posthoc_ema)")
    ap.add_argument("--sigma_rel", type=float, help=f"relative width of the wanted EMA profile, in (0, {SIGMA_REL_MAX:.4f})")
    ap.add_argument("--step", type=int, default=None, help="the step the average ends at (default: the last snapshot)")
    ap.add_argument("--out", help="checkpoint to write")
    ap.add_argument("--base", help="checkpoint whose 'model' and 'config' are copied into the output")
    ap.add_argument("--list", action="store_true", help="print what the directory holds")
    a = ap.parse_args(argv)
    try:
        if a.list:
            print(describe(read_index(a.snapshots)))
            return 0
        if a.sigma_rel is None or not a.out:
            raise RuntimeError("posthoc_ema: --sigma_rel and --out are needed (or --list)")
        check_sigma_rel(a.sigma_rel)
        import torch
        sd, rep = reconstruct(a.snapshots, a.sigma_rel, a.step)
        ck = {"ema": sd, "posthoc_ema": rep}
        if a.base:
            base = torch.load(a.base, map_location="cpu")
            for k in ("model", "config"):
                if k in base:
                    ck[k] = base[k]
            for k, v in base.get("ema", {}).items():          # buffers: entries of the state dict that are no parameters
                ck["ema"].setdefault(k, v)
            missing = set(base.get("ema", sd)) ^ set(ck["ema"])
            if missing:
                raise RuntimeError(f"posthoc_ema: --base holds another model: keys differ ({sorted(missing)[:4]} ...)")
        torch.save(ck, a.out)
    except (RuntimeError, ValueError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    print(f"sigma_rel {rep['sigma_rel']:g} (gamma {rep['gamma']:.4f}) at step {rep['step']} from {rep['snapshots']} snapshots")
    print(f"coefficients {rep['coef_min']:+.4f} .. {rep['coef_max']:+.4f}; condition number {rep['condition']:.3e}")
    print(f"relative L2 residual of the profile fit (discrete weights): {rep['residual_rel']:.3e}")
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
