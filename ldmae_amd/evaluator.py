"""The ADM / guided-diffusion evaluator (the reference's tools/evaluator.py) without TensorFlow: Inception Score, FID, sFID, precision and
recall of a sample batch against a reference batch, on the HIP kernels of csrc/inception.hip and csrc/adm_eval.hip.

Features are those of the TF graph classify_image_graph_def.pb, computed with the same 2015-12-05 Inception weights in their PyTorch port
(pt_inception-2015-12-05, see fid.py): the graph's pre-processing (TF1 ResizeBilinear to 299 x 299, then (x - 128) / 128), pool_3
(2048 values) and mixed_6/conv[..., :7] (Mixed_6d's branch1x1, 17 x 17 x 7 = 2023 values, NHWC order).  The Inception Score uses
fc.weight of the same state dict without its bias, as the graph's softmax/logits/MatMul does.  Distances for precision / recall are exact
f32 (ADM's own fallback when its f16 distances are not finite).

    python -m ldmae_amd.evaluator REF SAMPLE [--batch-size 64] [--weights P] [--device cuda]
        [--kid [--kid-subsets 100] [--kid-subset-size 1000] [--kid-seed 2020]] [--density-coverage [--nearest-k 5]]

--kid adds one line, `KID: <mean> +- <std>` (Binkowski et al. 2018: the unbiased MMD^2 with the cubic polynomial kernel over random
subsets of the pool features); --density-coverage adds `Density:` and `Coverage:` (Naeem et al. 2020).  Neither writes anything into the
.npz caches, and without the flags the output is what it was.  Agreement with torch-fidelity's KID and with the prdc package has NOT been
checked (neither was available); the tests compare with f64 restatements of the papers' formulas.

REF and SAMPLE are .npz files with arr_0 = uint8 [N, H, W, 3] (read a batch at a time), or folders of images (fid.list_images order).
Like the reference, an .npz that lacks act / act_s gets act, act_s, mu, mu_s, sigma, sigma_s added (written to a temporary file, then
renamed over it) and a later run reads them instead of running the network; stored mu / sigma win over recomputed ones.  A folder is
never written to.
"""
from __future__ import annotations

import argparse
import os
import shutil
import tempfile
import zipfile
from contextlib import contextmanager

import numpy as np
import torch

from . import fid

CACHE_KEYS = ("act", "act_s", "mu", "mu_s", "sigma", "sigma_s")
SPATIAL_DIM = 17 * 17 * 7


class FIDStatistics:
    """mu / sigma of one feature set (evaluator.py:104-150)."""

    def __init__(self, mu, sigma):
        self.mu = mu
        self.sigma = sigma

    def frechet_distance(self, other, eps=1e-6):
        return fid.calculate_frechet_distance(self.mu, self.sigma, other.mu, other.sigma, eps)


# ---------------------------------------------------------------------------------------------------- .npz streaming (evaluator.py:448-586)
class NpzArrayReader:
    """Batches of the first axis of one .npy member of an .npz, read from the zip stream (stored or deflated: zipfile decompresses as it
    reads, so neither form is loaded whole).  An array numpy's header readers cannot stream (format 3.0, Fortran order, object dtype) is
    loaded whole instead (MemoryNpzArrayReader of the reference)."""

    def __init__(self, fp=None, shape=None, dtype=None, arr=None):
        self.fp, self.arr = fp, arr
        self.shape = tuple(arr.shape) if arr is not None else tuple(shape)
        self.dtype = arr.dtype if arr is not None else dtype
        self.idx = 0

    def remaining(self):
        return max(0, self.shape[0] - self.idx)

    def read_batch(self, batch_size):
        bs = min(batch_size, self.remaining())
        if bs <= 0:
            return None
        i0, self.idx = self.idx, self.idx + bs
        if self.arr is not None:
            return self.arr[i0:i0 + bs]
        out = np.empty((bs, *self.shape[1:]), dtype=self.dtype)
        buf = memoryview(out.reshape(-1).view(np.uint8))
        got = 0
        while got < len(buf):
            r = self.fp.readinto(buf[got:])
            if not r:
                raise ValueError(f"EOF: reading array data, expected {len(buf)} bytes got {got}")
            got += r
        return out

    def read_batches(self, batch_size):
        while True:
            b = self.read_batch(batch_size)
            if b is None:
                return
            yield b


@contextmanager
def open_npz_array(path, arr_name="arr_0"):
    with open(path, "rb") as f, zipfile.ZipFile(f, "r") as z:
        member = f"{arr_name}.npy"
        if member not in z.namelist():
            raise ValueError(f"missing {arr_name} in npz file {path}")
        with z.open(member, "r") as af:
            version = np.lib.format.read_magic(af)
            header = None
            if version == (1, 0):
                header = np.lib.format.read_array_header_1_0(af)
            elif version == (2, 0):
                header = np.lib.format.read_array_header_2_0(af)
            if header is None or header[1] or header[2].hasobject:
                with np.load(path) as full:
                    yield NpzArrayReader(arr=full[arr_name])
                return
            shape, _, dtype = header
            yield NpzArrayReader(af, shape, dtype)


def _npz_keys(path):
    with zipfile.ZipFile(path, "r") as z:
        return [n[:-4] for n in z.namelist() if n.endswith(".npy")]


def write_npz_cache(path, arrays):
    """Add `arrays` (name -> ndarray) to the .npz at `path`, replacing members of the same name: the other members are copied stream to
    stream (arr_0 is never loaded), the result goes to a temporary file in the same folder and is renamed over `path`."""
    d = os.path.dirname(os.path.abspath(path))
    fd, tmp = tempfile.mkstemp(prefix=".evaluator-", suffix=".npz", dir=d)
    os.close(fd)
    try:
        with zipfile.ZipFile(path, "r") as zin, zipfile.ZipFile(tmp, "w", allowZip64=True) as zout:
            for info in zin.infolist():
                if info.filename[:-4] in arrays:
                    continue
                out = zipfile.ZipInfo(info.filename, date_time=info.date_time)
                out.compress_type = info.compress_type
                with zin.open(info, "r") as src, zout.open(out, "w", force_zip64=True) as dst:
                    shutil.copyfileobj(src, dst, 1 << 24)
            comp = zin.infolist()[0].compress_type if zin.infolist() else zipfile.ZIP_STORED
            for name, arr in arrays.items():
                info = zipfile.ZipInfo(f"{name}.npy", date_time=(1980, 1, 1, 0, 0, 0))
                info.compress_type = comp
                with zout.open(info, "w", force_zip64=True) as dst:
                    np.lib.format.write_array(dst, np.asarray(arr), allow_pickle=False)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


# ---------------------------------------------------------------------------------------------------- Inception Score (evaluator.py:194-207)
def inception_score_from_sums(h, S, n_rows, split_size=5000):
    """IS = mean_s exp((sum_{i in s} h_i - sum_c S_sc log(S_sc / n_s)) / n_s), h_i = sum_c p_ic log p_ic and S_sc = sum_{i in s} p_ic:
    the reference's mean over splits of exp(mean_i KL(p_i || mean of the split)), with 0 log 0 = 0.  The last split may be short."""
    h, S = np.asarray(h, np.float64), np.asarray(S, np.float64)
    scores = []
    for s in range(S.shape[0]):
        i0 = s * split_size
        n = min(split_size, n_rows - i0)
        Ss = S[s]
        pos = Ss > 0
        t = np.zeros_like(Ss)
        t[pos] = Ss[pos] * np.log(Ss[pos] / n)
        scores.append(np.exp((h[i0:i0 + n].sum() - t.sum()) / n))
    return float(np.mean(scores))


# ---------------------------------------------------------------------------------------------------- KID (Binkowski et al. 2018)
def kid_subset_indices(n1, n2, num_subsets, subset_size, seed):
    """(idx1 [S, m], idx2 [S, m]) int32: numpy.random.RandomState(seed); per subset choice(n1, m, replace=False) and THEN
    choice(n2, m, replace=False) -- the order torch-fidelity documents for its KID.  Agreement with torch-fidelity's draws has NOT been
    checked: that package was not available when this was written."""
    n1, n2, S, m = int(n1), int(n2), int(num_subsets), int(subset_size)
    if S < 1 or m < 2:
        raise ValueError(f"kid_subset_indices: {S} subsets of {m} rows (at least 1 subset of at least 2 rows)")
    if m > min(n1, n2):
        raise ValueError(f"kid_subset_indices: subset_size {m} is above the smaller feature set ({min(n1, n2)} rows): "
                         f"pass a subset_size of at most {min(n1, n2)}")
    rng = np.random.RandomState(seed)
    idx1, idx2 = np.empty((S, m), np.int32), np.empty((S, m), np.int32)
    for s in range(S):
        idx1[s] = rng.choice(n1, m, replace=False)
        idx2[s] = rng.choice(n2, m, replace=False)
    return idx1, idx2


def kid_from_sums(sums, m):
    """sums [S, 3] = (sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{i, j} k(x_i, y_j)) per subset of m rows ->
    (mean, std) over the subsets of the unbiased mmd^2 = aa / (m (m - 1)) + bb / (m (m - 1)) - 2 ab / m^2, in host f64; std is numpy.std
    (the population form)."""
    s = np.asarray(sums, np.float64)
    m = int(m)
    if s.ndim != 2 or s.shape[1] != 3 or s.shape[0] < 1 or m < 2:
        raise ValueError(f"kid_from_sums: sums {s.shape} must be [S, 3] with S >= 1, and m = {m} at least 2")
    mmd2 = s[:, 0] / (m * (m - 1)) + s[:, 1] / (m * (m - 1)) - 2.0 * s[:, 2] / (m * m)
    return float(np.mean(mmd2)), float(np.std(mmd2))


def _check_nearest_k(nearest_k):
    k = int(nearest_k)
    if not 1 <= k <= 7:
        raise ValueError(f"density_coverage: nearest_k {nearest_k} outside 1..7 (the k-NN kernel keeps the 8 smallest distances of a row, "
                         "the self-distance among them)")
    return k


def _features_2d(x, what):
    """A [N, D] f32 array (numpy or torch) checked finite on the host side of the call, before any kernel."""
    if isinstance(x, torch.Tensor):
        if x.dim() != 2:
            raise ValueError(f"{what}: need [N, D] features, got {tuple(x.shape)}")
        if not bool(torch.isfinite(x).all()):
            raise ValueError(f"{what}: features hold non-finite values")
        return x
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError(f"{what}: need [N, D] features, got {x.shape}")
    if not np.isfinite(x).all():
        raise ValueError(f"{what}: features hold non-finite values")
    return x


class ManifoldEstimator:
    """k-NN manifold estimate of a feature set (evaluator.py:210-406) on the pairwise kernels: squared distances
    max(|u|^2 - 2 u.v + |v|^2, 0) in exact f32.  nsplit: column splits of each pass (default ops.default_col_splits; results are the same
    for every value).  evaluate() / realism scores are not provided."""

    def __init__(self, nhood_sizes=(3,), clamp_to_percentile=None, eps=1e-5, device="cuda", nsplit=None):
        self.nhood_sizes = tuple(int(k) for k in nhood_sizes)
        if not self.nhood_sizes or len(self.nhood_sizes) > 8 or min(self.nhood_sizes) < 0 or max(self.nhood_sizes) > 7:
            raise ValueError(f"nhood_sizes {nhood_sizes}: 1..8 sizes, each in [0, 7]")
        self.num_nhoods = len(self.nhood_sizes)
        self.clamp_to_percentile = clamp_to_percentile
        self.eps = eps
        self.device = torch.device(device)
        self.nsplit = nsplit

    def _dev(self, x):
        if isinstance(x, torch.Tensor):
            return x.to(self.device, torch.float32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)

    def manifold_radii(self, features):
        """[N, D] -> f32 [N, len(nhood_sizes)]: the value at sorted index k of each row's distances to all rows (itself included), as
        np.partition(d, seq)[:, k] over the full row; clamped at the percentile when clamp_to_percentile is set."""
        from . import ops
        features = _features_2d(features, "manifold_radii")
        if features.shape[0] <= max(self.nhood_sizes):
            raise ValueError(f"manifold_radii: {features.shape[0]} feature rows hold no neighbour at sorted index {max(self.nhood_sizes)}")
        radii = ops.knn_radii(self._dev(features), self.nhood_sizes, nsplit=self.nsplit).cpu().numpy()
        if self.clamp_to_percentile is not None:
            max_distances = np.percentile(radii, self.clamp_to_percentile, axis=0)
            radii[radii > max_distances] = 0
        return radii

    def evaluate_pr(self, features_1, radii_1, features_2, radii_2):
        """(precision [K], recall [K]): precision = the fraction of features_2 inside some ball of features_1 (radius radii_1), recall = the
        fraction of features_1 inside some ball of features_2 (evaluator.py:340-375)."""
        from . import ops
        features_1 = _features_2d(features_1, "evaluate_pr features_1")
        features_2 = _features_2d(features_2, "evaluate_pr features_2")
        r1, r2 = np.asarray(radii_1, np.float32), np.asarray(radii_2, np.float32)
        if r1.ndim != 2 or r2.ndim != 2 or r1.shape != (features_1.shape[0], r2.shape[1]) or r2.shape[0] != features_2.shape[0]:
            raise ValueError(f"evaluate_pr: radii {r1.shape} / {r2.shape} do not match {features_1.shape[0]} / {features_2.shape[0]} rows "
                             "with one column count")
        if features_1.shape[1] != features_2.shape[1]:
            raise ValueError(f"evaluate_pr: feature widths {features_1.shape[1]} and {features_2.shape[1]} differ")
        in1, in2 = ops.pr_flags(self._dev(features_1), self._dev(r1), self._dev(features_2), self._dev(r2), nsplit=self.nsplit)
        # exact counts over n, as np.mean of the boolean flags gives them
        return (in2.sum(0).cpu().numpy().astype(np.float64) / in2.shape[0], in1.sum(0).cpu().numpy().astype(np.float64) / in1.shape[0])

    def density_coverage(self, features_real, features_fake, nearest_k=5):
        """(density, coverage) of Naeem et al. 2020: with r_i the squared distance of real row i to its nearest_k-th neighbour (sorted index
        nearest_k of its distances to all real rows, the self-distance at index 0 -- manifold_radii with nhood_sizes=(nearest_k,), no
        percentile clamp) and counts[i] = #{ fake j : d(i, j) < r_i }: density = sum_i counts[i] / (nearest_k N_fake), coverage = the
        fraction of real rows with counts[i] > 0 (a real row's nearest fake lies inside its ball exactly when some fake does)."""
        from . import ops
        k = _check_nearest_k(nearest_k)
        features_real = _features_2d(features_real, "density_coverage features_real")
        features_fake = _features_2d(features_fake, "density_coverage features_fake")
        if features_real.shape[1] != features_fake.shape[1]:
            raise ValueError(f"density_coverage: feature widths {features_real.shape[1]} and {features_fake.shape[1]} differ")
        real = self._dev(features_real)
        radii = ManifoldEstimator((k,), None, self.eps, self.device, self.nsplit).manifold_radii(real)
        counts = ops.ball_counts(real, self._dev(radii[:, 0]), self._dev(features_fake), nsplit=self.nsplit).cpu().numpy().astype(np.int64)
        return float(counts.sum() / (k * features_fake.shape[0])), float(np.mean(counts > 0))


class Evaluator:
    """The reference's Evaluator (evaluator.py:153-224) on the HIP Inception-v3.  The network is loaded on first use (weights through
    fid.resolve_weights: the argument, $LDMAE_FID_WEIGHTS, torch.hub's checkpoints; never downloaded); state_dict= gives one directly.
    softmax_batch_size is accepted for the reference's signature: the softmax runs over all rows in one pass."""

    def __init__(self, weights=None, device="cuda", batch_size=64, softmax_batch_size=512, state_dict=None, nsplit=None):
        self.weights, self.state_dict = weights, state_dict
        self.device = torch.device(device)
        self.batch_size = batch_size
        self.softmax_batch_size = softmax_batch_size
        self.manifold_estimator = ManifoldEstimator(device=device, nsplit=nsplit)
        self._model = None

    @property
    def model(self):
        if self._model is None:
            m = fid.InceptionFID(None if self.state_dict is not None else fid.resolve_weights(self.weights), 2048, self.device,
                                 state_dict=self.state_dict)
            m.adm_logits_weight()            # the Inception Score needs fc.weight: refuse a state dict without it before any image is read
            self._model = m
        return self._model

    def read_activations(self, path):
        """(pool [N, 2048], spatial [N, 2023]) of an .npz's arr_0 (streamed) or of a folder of images."""
        path = str(path)
        if os.path.isdir(path):
            files = fid.list_images(path)
            if not files:
                raise ValueError(f"no images in {path}")
            return self.compute_activations(fid._batches(files, self.batch_size, fid.MAX_DECODE_THREADS))
        with open_npz_array(path, "arr_0") as reader:
            return self.compute_activations(reader.read_batches(self.batch_size))

    def compute_activations(self, batches):
        """NHWC batches with values 0..255 -> (pool f32 [N, 2048], spatial f32 [N, 2023]) as numpy arrays."""
        pools, spatials = [], []
        for batch in batches:
            batch = np.asarray(batch)
            if batch.dtype != np.uint8:
                if not (np.all(batch == np.round(batch)) and batch.min(initial=0) >= 0 and batch.max(initial=0) <= 255):
                    raise ValueError("compute_activations: images must hold integers in [0, 255]")
                batch = batch.astype(np.uint8)
            pool, spatial = self.model.adm_features(batch)
            pools.append(pool.cpu().numpy())
            spatials.append(spatial.cpu().numpy())
        if not pools:
            raise ValueError("compute_activations: no images")
        return np.concatenate(pools, 0), np.concatenate(spatials, 0)

    def read_statistics(self, npz_path, activations):
        """Stored mu / sigma / mu_s / sigma_s of an .npz win (evaluator.py:179-187); otherwise computed from the activations."""
        p = str(npz_path)
        if not os.path.isdir(p) and "mu" in _npz_keys(p):
            with np.load(p) as obj:
                return FIDStatistics(obj["mu"], obj["sigma"]), FIDStatistics(obj["mu_s"], obj["sigma_s"])
        return tuple(self.compute_statistics(x) for x in activations)

    def compute_statistics(self, activations):
        """mu = mean, sigma = np.cov(rowvar=False), accumulated in f64 on the device (fid.FeatureStats)."""
        acts = _features_2d(activations, "compute_statistics")
        stats = fid.FeatureStats(acts.shape[1], self.device)
        for i in range(0, acts.shape[0], 4096):
            stats.update(torch.from_numpy(np.ascontiguousarray(acts[i:i + 4096], dtype=np.float32)).to(self.device))
        mu, sigma = stats.finalize()
        return FIDStatistics(mu, sigma)

    def compute_inception_score(self, activations, split_size=5000):
        """exp(E KL(p(y|x) || p(y))) per split of split_size rows, averaged (evaluator.py:194-207); p = softmax(pool . fc.weight^T)."""
        from . import ops
        acts = _features_2d(activations, "compute_inception_score")
        x = torch.from_numpy(np.ascontiguousarray(acts, dtype=np.float32)).to(self.device)
        logits = ops.pairwise_logits(x, self.model.adm_logits_weight())
        h, S = ops.adm_softmax_is(logits, split_size)
        return inception_score_from_sums(h.cpu().numpy(), S.cpu().numpy(), acts.shape[0], split_size)

    def compute_prec_recall(self, activations_ref, activations_sample):
        radii_1 = self.manifold_estimator.manifold_radii(activations_ref)
        radii_2 = self.manifold_estimator.manifold_radii(activations_sample)
        pr = self.manifold_estimator.evaluate_pr(activations_ref, radii_1, activations_sample, radii_2)
        return float(pr[0][0]), float(pr[1][0])

    def compute_kid(self, act_ref, act_sample, num_subsets=100, subset_size=1000, seed=2020, gamma=None, coef0=1.0):
        """(mean, std) over num_subsets subsets of the unbiased MMD^2 between subset_size rows of each feature set, with the cubic
        polynomial kernel (gamma x.y + coef0)^3; gamma=None is 1 / D.  The subsets are kid_subset_indices(...); all of them run in one
        launch (ops.kid_sums), the estimator itself in host f64 (kid_from_sums)."""
        from . import ops
        ref, sample = _features_2d(act_ref, "compute_kid act_ref"), _features_2d(act_sample, "compute_kid act_sample")
        if ref.shape[1] != sample.shape[1]:
            raise ValueError(f"compute_kid: feature widths {ref.shape[1]} and {sample.shape[1]} differ")
        n = min(ref.shape[0], sample.shape[0])
        if int(subset_size) > n:
            raise ValueError(f"compute_kid: subset_size {subset_size} is above the smaller feature set ({n} rows): pass subset_size={n} or less")
        idx1, idx2 = kid_subset_indices(ref.shape[0], sample.shape[0], num_subsets, subset_size, seed)
        g = 1.0 / ref.shape[1] if gamma is None else float(gamma)
        dev = self.manifold_estimator._dev
        sums = ops.kid_sums(dev(ref), dev(sample), idx1, idx2, g, coef0, nsplit=self.manifold_estimator.nsplit)
        return kid_from_sums(sums.cpu().numpy(), subset_size)

    def compute_density_coverage(self, act_ref, act_sample, nearest_k=5):
        return self.manifold_estimator.density_coverage(act_ref, act_sample, nearest_k)


def activations_and_statistics(evaluator, path):
    """((pool, spatial), (stats, spatial stats)) of an input, with the reference's caching (evaluator.py:44-69): an .npz's act / act_s are
    used when present; otherwise the activations are computed and act, act_s, mu, mu_s, sigma, sigma_s written back into it.  A folder
    is computed every time and never written."""
    path = str(path)
    if os.path.isdir(path):
        acts = evaluator.read_activations(path)
        return acts, tuple(evaluator.compute_statistics(x) for x in acts)
    keys = _npz_keys(path)
    if "act" in keys or "act_s" in keys:
        with np.load(path) as z:
            acts = (z["act"], z["act_s"])
    else:
        acts = evaluator.read_activations(path)
    stats = evaluator.read_statistics(path, acts)
    if "act" not in keys or "act_s" not in keys:
        write_npz_cache(path, {"act": acts[0], "act_s": acts[1], "mu": stats[0].mu, "mu_s": stats[1].mu, "sigma": stats[0].sigma,
                               "sigma_s": stats[1].sigma})
    return acts, stats


def build_parser():
    ap = argparse.ArgumentParser(description="Inception Score, FID, sFID, precision and recall (the ADM evaluator) on the HIP Inception-v3; "
                                             "optionally KID and density / coverage")
    ap.add_argument("ref_batch", help="reference batch: .npz with arr_0 uint8 [N, H, W, 3], or a folder of images")
    ap.add_argument("sample_batch", help="sample batch: .npz with arr_0 uint8 [N, H, W, 3], or a folder of images")
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--weights", default=None, help=f"{fid.WEIGHTS_NAME} (default: ${fid.WEIGHTS_ENV}, then torch.hub's checkpoints)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--kid", action="store_true", help="also print the Kernel Inception Distance (mean +- std over subsets) of the pool features")
    ap.add_argument("--kid-subsets", type=int, default=100)
    ap.add_argument("--kid-subset-size", type=int, default=1000)
    ap.add_argument("--kid-seed", type=int, default=2020)
    ap.add_argument("--density-coverage", action="store_true", help="also print density and coverage (Naeem et al. 2020) of the pool features")
    ap.add_argument("--nearest-k", type=int, default=5)
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    for p in (a.ref_batch, a.sample_batch):
        if not os.path.exists(p):
            raise SystemExit(f"no such file or folder: {p}")
    evaluator = Evaluator(a.weights, a.device, a.batch_size)
    print("computing reference batch activations...")
    ref_acts, (ref_stats, ref_stats_spatial) = activations_and_statistics(evaluator, a.ref_batch)
    print("computing sample batch activations...")
    sample_acts, (sample_stats, sample_stats_spatial) = activations_and_statistics(evaluator, a.sample_batch)
    print("Computing evaluations...")
    out = {"is": evaluator.compute_inception_score(sample_acts[0]),
           "fid": sample_stats.frechet_distance(ref_stats),
           "sfid": sample_stats_spatial.frechet_distance(ref_stats_spatial)}
    print("Inception Score:", out["is"])
    print("FID:", out["fid"])
    print("sFID:", out["sfid"])
    out["precision"], out["recall"] = evaluator.compute_prec_recall(ref_acts[0], sample_acts[0])
    print("Precision:", out["precision"])
    print("Recall:", out["recall"])
    if a.kid:
        out["kid_mean"], out["kid_std"] = evaluator.compute_kid(ref_acts[0], sample_acts[0], a.kid_subsets, a.kid_subset_size, a.kid_seed)
        print("KID:", out["kid_mean"], "+-", out["kid_std"])
    if a.density_coverage:
        out["density"], out["coverage"] = evaluator.compute_density_coverage(ref_acts[0], sample_acts[0], a.nearest_k)
        print("Density:", out["density"])
        print("Coverage:", out["coverage"])
    return out


if __name__ == "__main__":
    main()
