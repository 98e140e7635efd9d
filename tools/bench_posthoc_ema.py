#!/usr/bin/env python3
"""Cost of the post-hoc EMA on one MI355X at the DiT-B/1 slab size: the optimizer launch with tracks off (ldmae_adamw_ema, the entry every
run without train.posthoc_ema uses) against 2 tracks (ldmae_adamw_ema_tracks), in alternating rounds; one snapshot write; one 64-snapshot
reconstruction.  Writes profiles/posthoc_ema_bench.txt (or --out).      python tools/bench_posthoc_ema.py [--numel N] [--rounds R]

By the bytes: the AdamW + EMA pass streams p, g, m, v, ema once = 9 slab passes (5 reads, 4 writes); a track adds a read and a write, so 2
tracks make 13.  The snapshot files of the reconstruction are 64 hard links to two written files, so the reads come from the page cache:
the figure is the time of the pipeline (memory map -> pinned chunk -> device -> f64 accumulator), not of a disk."""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ldmae_amd import ops, posthoc_ema as ph      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--numel", type=int, default=131_000_000, help="slab length in f32 elements (DiT-B/1: 131 M, 524 MB per pass)")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posthoc_ema_bench.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
n = a.numel // 64 * 64
g = torch.Generator(device="cuda").manual_seed(0)
p, grad, m, v = (torch.randn(n, device="cuda", generator=g) * s for s in (1.0, 0.1, 0.01, 1.0))
v = v.square() * 1e-4
ema = p.clone()
tracks = [p.clone(), p.clone()]
gammas = [ph.sigma_rel_to_gamma(s) for s in (0.05, 0.10)]
hyp = (2e-4, 0.9, 0.95, 1e-8, 0.0, 0.9999)
step = [1000]


def off():
    step[0] += 1
    ops.adamw_ema(p, grad, m, v, ema, step[0], *hyp)


def on():
    step[0] += 1
    ops.adamw_ema_tracks(p, grad, m, v, ema, tracks, [ph.track_coef(gm, step[0]) for gm in gammas], step[0], *hyp)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(a.iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / a.iters


for fn in (off, on):
    for _ in range(3):
        fn()
torch.cuda.synchronize()
t_off, t_on = [], []
for _ in range(a.rounds):          # alternating: drift of the clocks or of a neighbour's load hits both alike
    t_off.append(timed(off))
    t_on.append(timed(on))
lines = [f"post-hoc EMA on {torch.cuda.get_device_name(0)}: slab of {n} f32 elements ({4 * n / 1e6:.0f} MB per pass); "
         f"{a.rounds} alternating rounds of {a.iters} launches, device events"]
for name, ts, passes in (("tracks off (ldmae_adamw_ema)       ", t_off, 9), ("2 tracks  (ldmae_adamw_ema_tracks)", t_on, 13)):
    med = statistics.median(ts)
    lines.append(f"  {name}: median {med:.3f} ms (min {min(ts):.3f} .. max {max(ts):.3f}); {passes} passes = {passes * 4 * n / 1e9:.2f} GB -> "
                 f"{passes * 4 * n / med / 1e9:.2f} TB/s")
d = statistics.median(t_on) - statistics.median(t_off)
lines.append(f"  2 tracks cost {d:+.3f} ms per step = {d / 2:+.3f} ms per track (4 extra passes = {16 * n / 1e9:.2f} GB)")

tmp = tempfile.mkdtemp(prefix="posthoc_bench_")
try:
    index = ph.new_index([("slab", 0, (n,))], n, (0.05, 0.10))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ph.write_snapshot_files(tmp, index, 8, [t.cpu().numpy() for t in tracks])
    lines.append(f"  snapshot write (2 tracks, {8 * n / 1e6:.0f} MB, device -> host -> file, index rewritten): {time.perf_counter() - t0:.2f} s")
    for s in range(16, 32 * 8 + 1, 8):
        for k in (0, 1):
            os.link(os.path.join(tmp, ph.snapshot_file(8, k)), os.path.join(tmp, ph.snapshot_file(s, k)))
    index["steps"] = list(range(8, 32 * 8 + 1, 8))
    ph.write_index(tmp, index)
    del p, grad, m, v, ema, tracks
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    ix = ph.read_index(tmp)
    entries, rep = ph.plan(ix, 0.075)
    t1 = time.perf_counter()
    slab = ph.combine(tmp, ix, entries)
    t2 = time.perf_counter()
    assert slab.shape == (n,) and np.isfinite(slab[:1024]).all()
    lines.append(f"  reconstruction from {rep['snapshots']} snapshots ({rep['snapshots'] * 4 * n / 1e9:.1f} GB read through the page cache): solve + residual "
                 f"{t1 - t0:.2f} s, combine {t2 - t1:.2f} s ({rep['snapshots'] * 4 * n / (t2 - t1) / 1e9:.2f} GB/s)")
finally:
    shutil.rmtree(tmp, ignore_errors=True)
lines.append("  not measured: the effect of the EMA width on FID (needs a trained run)")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
