"""Set metrics on Inception features next to FID (fid.py): KID and improved precision / recall, density / coverage.

    feature_gram(z)                                         — device fp64 Gram matrix Z Z^T of fp32 feature rows
    kid_from_features(f1, f2, subsets=100, subset_size=None, seed=0, gamma=None, coef0=1.0)
    prdc_from_features(reference, generated, k=3)
    kid_between / prdc_between(a, b, model, dims=2048, ...) — sides as fid.fid_between takes them (frames, a scene, a directory)
    get_kid_score(generated_path, gt_path, ...)             — the call shape of fid.get_fid_score

KID (Bińkowski et al. 2018) is the unbiased MMD^2 estimator under the polynomial kernel k(x, y) = (gamma x.y + coef0)^3,
gamma = 1 / d, coef0 = 1, averaged over `subsets` random subsets of `subset_size` rows per side (100 subsets of
min(N1, N2, 1000): the defaults of the common implementations, written from the paper — the reference has no KID to pin them
to).  Precision / recall (Kynkäänniemi et al. 2019) and density / coverage (Naeem et al. 2020) use k-th-neighbour balls, k = 3.

All of them are read off one object, the Gram matrix G of the stacked rows [first set; second set]: k(x, y) from G_ij, squared
distances as (G_ii + G_jj) - 2 G_ij.  G is formed in fp64 on the device by sgam_feature_gram_f64 (csrc/feature_metrics.hip);
subset choice, kernel sums, radii and membership counts stay there too, and only the per-subset values or the four counts cross
to the host.  There is no CPU path."""
import torch

from . import _lib
from ._lib import SgamHipError, check
from ._opscore import _p, _stream

MAX_ROWS = 16384            # rows of one Gram matrix (a 2 GiB fp64 array): the limit of every entry point of feature_metrics.hip
MAX_K = 32
DEFAULT_SUBSET_SIZE = 1000


def _shapes(f1, f2, what):
    """shape rules of a pair of feature sets (checked before anything touches the device) -> (N1, N2, d)"""
    for f in (f1, f2):
        if not isinstance(f, torch.Tensor) or f.dim() != 2 or f.shape[0] < 1:
            raise ValueError(f"{what}: (N, d) feature tensors expected, not {tuple(f.shape) if isinstance(f, torch.Tensor) else type(f)}")
    if f1.shape[1] != f2.shape[1]:
        raise ValueError(f"{what}: the two sets have {f1.shape[1]} and {f2.shape[1]} feature dimensions")
    if f1.shape[1] % 4 != 0:
        raise ValueError(f"{what}: the feature dimension must be a multiple of 4 (64 / 192 / 768 / 2048 are), not {f1.shape[1]}")
    if f1.shape[0] + f2.shape[0] > MAX_ROWS:
        raise ValueError(f"{what}: {f1.shape[0]} + {f2.shape[0]} rows; one Gram matrix holds at most {MAX_ROWS} rows (2 GiB of fp64)")
    return int(f1.shape[0]), int(f2.shape[0]), int(f1.shape[1])


def _stacked(f1, f2, what):
    if not (f1.is_cuda and f2.is_cuda):
        raise SgamHipError(f"{what}: features must be tensors on the GPU (there is no CPU fallback)")
    return torch.cat([f1.float(), f2.float().to(f1.device)])


def feature_gram(z):
    """(N, d) fp32 rows on the device (any row pitch) -> (N, N) fp64 Gram matrix Z Z^T on the device: run-to-run identical,
    symmetric bit for bit, equal rows give equal entries"""
    if not (isinstance(z, torch.Tensor) and z.is_cuda):
        raise SgamHipError("feature_gram: features must be a tensor on the GPU (there is no CPU fallback)")
    if z.dim() != 2 or z.dtype != torch.float32 or z.shape[0] < 1 or z.shape[1] % 4 != 0:
        raise ValueError(f"feature_gram: (N, d) fp32 rows with d a multiple of 4 expected, not {tuple(z.shape)} {z.dtype}")
    if z.shape[0] > MAX_ROWS:
        raise ValueError(f"feature_gram: {z.shape[0]} rows; one Gram matrix holds at most {MAX_ROWS} rows (2 GiB of fp64)")
    if z.stride(1) != 1 or (z.shape[0] > 1 and z.stride(0) < z.shape[1]):
        z = z.contiguous()
    n, d = z.shape
    G = torch.empty((n, n), device=z.device, dtype=torch.float64)
    check(_lib.load().sgam_feature_gram_f64(_p(z), n, d, z.stride(0) if n > 1 else d, _p(G), _stream()), "sgam_feature_gram_f64")
    return G


def kid_subsets(n1, n2, subset_size, subsets, seed=0, device="cuda"):
    """-> (subsets, 2, subset_size) int32 on the device: the rows of each set that subset s takes, ascending (the rule of
    sgam_kid_subsets_u32: the subset_size smallest Philox keys of counter (row, s, side, 0) under `seed`)"""
    idx = torch.empty((subsets, 2, subset_size), device=device, dtype=torch.int32)
    nb = 2 * subsets * max(n1, n2)
    ws = torch.empty((nb,), device=device, dtype=torch.uint8)
    check(_lib.load().sgam_kid_subsets_u32(n1, n2, subset_size, subsets, int(seed) & 0xFFFFFFFFFFFFFFFF, _p(ws), nb, _p(idx), _stream()),
          "sgam_kid_subsets_u32")
    return idx


def kid_from_features(f1, f2, subsets=100, subset_size=None, seed=0, gamma=None, coef0=1.0):
    """Kernel inception distance of two feature sets (N1, d), (N2, d) on the device -> {"kid": mean of the per-subset MMD^2,
    "kid_std": their population standard deviation, "values": (S,) fp64 device tensor, "subsets": S, "subset_size": m}.
    subset_size None: min(N1, N2, 1000).  With m == N1 == N2 every subset is the whole of both sets: one is evaluated."""
    n1, n2, d = _shapes(f1, f2, "kid_from_features")
    m = min(n1, n2, DEFAULT_SUBSET_SIZE) if subset_size is None else int(subset_size)
    if m > min(n1, n2):
        raise ValueError(f"kid_from_features: subset_size {m} exceeds the smaller set ({min(n1, n2)} rows)")
    if m < 2:
        raise ValueError(f"kid_from_features: subset_size {m}; the unbiased estimator needs at least 2 rows per subset")
    S = int(subsets)
    if S < 1:
        raise ValueError(f"kid_from_features: subsets {subsets}")
    if m == n1 == n2:
        S = 1
    g = 1.0 / d if gamma is None else float(gamma)
    z = _stacked(f1, f2, "kid_from_features")
    G = feature_gram(z)
    idx = kid_subsets(n1, n2, m, S, seed, z.device)
    values = torch.empty((S,), device=z.device, dtype=torch.float64)
    nb = 24 * S * m
    ws = torch.empty((nb // 8,), device=z.device, dtype=torch.float64)
    check(_lib.load().sgam_kid_mmd_f64(_p(G), n1, n2, _p(idx), m, S, g, float(coef0), _p(ws), nb, _p(values), _stream()),
          "sgam_kid_mmd_f64")
    v = values.cpu().numpy()
    return {"kid": float(v.mean()), "kid_std": float(v.std()) if S > 1 else 0.0, "values": values, "subsets": S, "subset_size": m}


def prdc_counts(G, n_reference, n_generated, k):
    """the Gram of [reference; generated] -> (counts (4,) int64, radius2 (N,) fp64) on the device (sgam_feature_prdc_f64)"""
    counts = torch.empty((4,), device=G.device, dtype=torch.int64)
    radius2 = torch.empty((n_reference + n_generated,), device=G.device, dtype=torch.float64)
    check(_lib.load().sgam_feature_prdc_f64(_p(G), n_reference, n_generated, k, _p(radius2), _p(counts), _stream()),
          "sgam_feature_prdc_f64")
    return counts, radius2


def prdc_from_features(reference, generated, k=3):
    """Improved precision / recall and density / coverage of `generated` (N_f, d) against `reference` (N_r, d), balls of the
    k-th neighbour inside each set -> {"precision", "recall", "density", "coverage"} as floats, and "k"."""
    k = int(k)
    nr, nf, _ = _shapes(reference, generated, "prdc_from_features")
    if not 1 <= k <= MAX_K:
        raise ValueError(f"prdc_from_features: k between 1 and {MAX_K}, not {k}")
    if k + 1 > min(nr, nf):
        raise ValueError(f"prdc_from_features: k = {k} needs at least {k + 1} rows in each set, not {nr} and {nf}")
    counts, _ = prdc_counts(feature_gram(_stacked(reference, generated, "prdc_from_features")), nr, nf, k)
    c = [int(v) for v in counts.cpu().tolist()]
    return {"precision": c[0] / nf, "recall": c[1] / nr, "density": c[2] / (k * nf), "coverage": c[3] / nr, "k": k}


# ---- sides: frames, a scene, a directory --------------------------------------------------------------------------------------
def _side_features(s, model, dims, batch_size, device, num_workers, what):
    from . import fid
    if hasattr(s, "frames") and hasattr(s, "_stored_coords"):          # a scene: its stored frames, where the store keeps them
        s = torch.stack([s.frames[c]["rgb_u8"] for c in s._stored_coords(None, what)])
    s = fid._side(s)
    if isinstance(s, str):
        raise ValueError(f"{what}: {s} holds only statistics (mu, sigma); this metric needs the features themselves — pass the "
                         "frames or the directory of images")
    return fid._side_features(s, model, batch_size, dims, device, num_workers)


def kid_between(a, b, model, dims=2048, subsets=100, subset_size=None, seed=0, gamma=None, coef0=1.0, batch_size=50, device="cuda",
                num_workers=1):
    """KID between two sides, each a (N,H,W,3) tensor of frames, a scene or a directory of images (kid_from_features of their
    `dims`-dimensional Inception features)"""
    fa = _side_features(a, model, dims, batch_size, device, num_workers, "kid")
    fb = _side_features(b, model, dims, batch_size, device, num_workers, "kid")
    return kid_from_features(fa, fb, subsets=subsets, subset_size=subset_size, seed=seed, gamma=gamma, coef0=coef0)


def prdc_between(a, b, model, dims=2048, k=3, batch_size=50, device="cuda", num_workers=1):
    """precision / recall / density / coverage of side `b` (generated) against side `a` (reference); sides as in kid_between"""
    fa = _side_features(a, model, dims, batch_size, device, num_workers, "prdc")
    fb = _side_features(b, model, dims, batch_size, device, num_workers, "prdc")
    return prdc_from_features(fa, fb, k=k)


def get_kid_score(generated_path, gt_path, batch_size=64, num_workers=0, device="cuda:0", dims=2048, model=None, **kid_options):
    """KID of two directories of images, called like fid.get_fid_score; `kid_options`: subsets, subset_size, seed, gamma, coef0.
    Returns the dict of kid_from_features (first set = generated_path)."""
    import os
    from . import fid
    device = torch.device("cuda" if device is None else device)
    if num_workers is None:
        num_workers = min(len(os.sched_getaffinity(0)), 8)
    for p in (generated_path, gt_path):
        if not os.path.exists(p):
            raise RuntimeError(f"Invalid path: {p}")
    if model is None:
        model = fid.InceptionV3([fid.InceptionV3.BLOCK_INDEX_BY_DIM[dims]]).to(device)
    return kid_between(generated_path, gt_path, model, dims=dims, batch_size=batch_size, device=device, num_workers=num_workers,
                       **kid_options)


__all__ = ["MAX_ROWS", "feature_gram", "kid_subsets", "kid_from_features", "prdc_counts", "prdc_from_features", "kid_between",
           "prdc_between", "get_kid_score"]
