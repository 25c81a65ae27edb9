"""CPU restatement of the feature-set metrics (include/sgam_hip.h: sgam_feature_gram_f64, sgam_kid_subsets_u32, sgam_kid_mmd_f64,
sgam_feature_prdc_f64) in numpy fp64; Philox from sampler_oracle.  Test infrastructure only — the product path never imports it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
from sampler_oracle import philox4x32_10  # noqa: E402

MASK32 = 0xFFFFFFFF


def gram(z):
    z = np.asarray(z, np.float64)
    return z @ z.T


def gram_majorant(z):
    """(|Z| |Z|^T): what the rounding bounds of the Gram are stated against"""
    a = np.abs(np.asarray(z, np.float64))
    return a @ a.T


def kid_subsets(n1, n2, m, subsets, seed):
    """(subsets, 2, m) int32: per subset and side the m indices with the smallest pairs (Philox word 0 of counter
    (i, s, side, 0), i), ascending"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    out = np.empty((subsets, 2, m), np.int32)
    for s in range(subsets):
        for side, n in enumerate((n1, n2)):
            i = np.arange(n, dtype=np.uint64)
            key = philox4x32_10((i, s, side, 0), (seed & MASK32, seed >> 32))[0]
            order = np.lexsort((i, key))                    # by key, an equal key to the lower index
            out[s, side] = np.sort(order[:m])
    return out


def kid_values(G, n1, idx, gamma, coef0, majorant=False):
    """per-subset MMD^2 from the Gram of [first set; second set]; with majorant=True the three sums are added instead (G is then
    the majorant Gram): the scale the tolerance is stated against"""
    G = np.asarray(G, np.float64)
    out = np.empty((idx.shape[0],))
    m = idx.shape[2]
    t = gamma * G + coef0
    K = (t * t) * t
    for s in range(idx.shape[0]):
        a, b = idx[s, 0].astype(np.int64), idx[s, 1].astype(np.int64) + n1
        kaa, kbb, kab = K[np.ix_(a, a)], K[np.ix_(b, b)], K[np.ix_(a, b)]
        saa = kaa.sum() - np.trace(kaa)
        sbb = kbb.sum() - np.trace(kbb)
        sab = kab.sum()
        if majorant:
            out[s] = saa / (m * (m - 1)) + sbb / (m * (m - 1)) + 2 * sab / (m * m)
        else:
            out[s] = saa / (m * (m - 1)) + sbb / (m * (m - 1)) - 2 * sab / (m * m)
    return out


def kid(f1, f2, subsets=100, subset_size=None, seed=0, gamma=None, coef0=1.0):
    f1, f2 = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    n1, n2 = len(f1), len(f2)
    m = min(n1, n2, 1000) if subset_size is None else subset_size
    if m == n1 == n2:
        subsets = 1
    gamma = 1.0 / f1.shape[1] if gamma is None else gamma
    idx = kid_subsets(n1, n2, m, subsets, seed)
    v = kid_values(gram(np.concatenate([f1, f2])), n1, idx, gamma, coef0)
    return {"kid": float(v.mean()), "kid_std": float(v.std()), "values": v, "subsets": subsets, "subset_size": m, "idx": idx}


def squared_distances(G):
    """d2(i, j) = (G_ii + G_jj) - 2 G_ij, in this order"""
    g = np.diag(G)
    return (g[:, None] + g[None, :]) - 2.0 * G


def prdc(G, nr, nf, k):
    """counts and margins from the Gram of [reference; generated].  radius2[i]: the k-th smallest d2 to another row (by index)
    of i's own set.  Returns dict(counts (4,) int64 [precision, recall, density, coverage numerators], radius2, margin: the
    smallest |d2 - radius2| over every comparison the four counts make, gap: the smallest distance between the k-th neighbour
    distance and the (k - 1)-th / (k + 1)-th of the same row)."""
    d2 = squared_distances(np.asarray(G, np.float64))
    n = nr + nf
    radius2 = np.empty((n,))
    gap = np.inf
    for lo, hi in ((0, nr), (nr, n)):
        block = d2[lo:hi, lo:hi].copy()
        block[np.arange(hi - lo), np.arange(hi - lo)] = np.inf          # exclusion by index
        srt = np.sort(block, axis=1)
        radius2[lo:hi] = srt[:, k - 1]
        if k >= 2:
            gap = min(gap, float((srt[:, k - 1] - srt[:, k - 2]).min()))
        if k < hi - lo - 1:
            gap = min(gap, float((srt[:, k] - srt[:, k - 1]).min()))
    cross = d2[:nr, nr:]                                                # (reference i, generated j)
    in_ref_ball = cross <= radius2[:nr, None]
    in_gen_ball = cross <= radius2[None, nr:]
    nearest = cross.min(axis=1)
    counts = np.array([in_ref_ball.any(axis=0).sum(), in_gen_ball.any(axis=1).sum(), in_ref_ball.sum(),
                       (nearest <= radius2[:nr]).sum()], np.int64)
    margin = min(float(np.abs(cross - radius2[:nr, None]).min()), float(np.abs(cross - radius2[None, nr:]).min()))
    return {"counts": counts, "radius2": radius2, "margin": margin, "gap": gap}


def prdc_values(counts, nr, nf, k):
    return {"precision": counts[0] / nf, "recall": counts[1] / nr, "density": counts[2] / (k * nf), "coverage": counts[3] / nr}
