"""numpy restatement of the segmentation kernels (csrc/point_segment.hip) for tests, on sampler_oracle (Philox4x32-10) and
cloud_oracle (the Jacobi loop): the fixed-radius neighbour relation with the kernel's fp32 d2, DBSCAN's core / cluster / border /
noise rules with clusters numbered in ascending root order, the plane RANSAC's draw rule, float64 hypothesis, fp32 inlier test,
selection and peel, the least-squares refit with the kernel's block-sum fold order, and the cluster boxes.  Nothing here comes
from another project.  Test infrastructure only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import cloud_oracle as CO  # noqa: E402
import sampler_oracle as SO  # noqa: E402

f32 = np.float32
MAX_DRAWS = 16                    # csrc/point_segment.hip: PLANE_MAX_DRAWS
SWEEPS = 6                        # csrc/jacobi3.h: JACOBI_SWEEPS
FIT_CHUNK = 4096                  # points per workgroup of the refit's sums


def max_d2_of(eps):
    e = f32(eps)
    return f32(e * e)


def finite3(points):
    return np.isfinite(np.asarray(points, dtype=f32)).all(axis=1)


def pair_d2(points):
    """(N,N) fp32: d2[i][j] = (dx * dx + dy * dy) + dz * dz, dx = p_j.x - p_i.x, one fp32 operation per operator; NaN where either
    is not a point"""
    p = np.asarray(points, dtype=f32)
    with np.errstate(all="ignore"):
        d = p[None, :, :] - p[:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    ok = finite3(p)
    d2[~ok, :] = np.nan
    d2[:, ~ok] = np.nan
    return d2


def neighbours(points, eps):
    """(N,N) bool: j is a neighbour of i (i itself included), and the d2 matrix"""
    d2 = pair_d2(points)
    with np.errstate(invalid="ignore"):
        return d2 <= max_d2_of(eps), d2


def radius_count(points, eps):
    return neighbours(points, eps)[0].sum(axis=1).astype(np.int32)


def dbscan(points, eps, min_points):
    """-> {"labels", "core", "count", "n_clusters", "sizes"} by the rules of include/sgam_hip.h"""
    p = np.asarray(points, dtype=f32)
    n = len(p)
    nb, d2 = neighbours(p, eps)
    count = nb.sum(axis=1).astype(np.int32)
    core = count >= int(min_points)
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in np.argwhere(np.triu(nb & core[:, None] & core[None, :], 1)):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)                 # the root of a cluster is its least core index
    root = np.full(n, -1, dtype=np.int64)
    for i in np.flatnonzero(core):
        root[i] = find(i)
    # border: the core neighbour of least (d2 bits, index); argmin takes the first of equal minima, the lower index
    cand = nb & core[None, :]
    for i in np.flatnonzero(~core & cand.any(axis=1)):
        root[i] = root[int(np.argmin(np.where(cand[i], d2[i], np.inf)))]
    roots = np.flatnonzero(root == np.arange(n))          # ascending: the numbering
    rank = np.full(n, -1, dtype=np.int64)
    rank[roots] = np.arange(len(roots))
    labels = np.where(root >= 0, rank[np.maximum(root, 0)], -1).astype(np.int32)
    sizes = np.zeros(n, dtype=np.int32)
    sizes[:len(roots)] = np.bincount(labels[labels >= 0], minlength=len(roots))[:len(roots)] if len(roots) else 0
    return {"labels": labels, "core": core, "count": count, "n_clusters": np.int32(len(roots)), "sizes": sizes}


# ---------------------------------------------------------------- planes
def draw(H, n_active, rnd, seed):
    """(H,3) picks (-1: a failed draw): slot by slot, word 0 of Philox at counter (h, draw, round, 0) under the seed's two words,
    pick = (word * n_active) >> 32, a duplicate of an earlier slot drawn again, at most MAX_DRAWS draws per hypothesis"""
    h = np.arange(H, dtype=np.uint64)
    picks = np.full((H, 3), -1, dtype=np.int64)
    if n_active < 3:
        return picks
    draws = np.zeros(H, dtype=np.uint64)
    key = (int(seed) & SO.MASK32, int(seed) >> 32)
    ok = np.ones(H, dtype=bool)
    for s in range(3):
        got = np.full(H, -1, dtype=np.int64)
        for _ in range(MAX_DRAWS):
            need = ok & (got < 0) & (draws < MAX_DRAWS)
            if not need.any():
                break
            w = SO.philox4x32_10((h, draws, int(rnd), 0), key)[0]
            cand = ((w * np.uint64(n_active)) >> np.uint64(32)).astype(np.int64)
            draws = draws + need.astype(np.uint64)
            dup = (picks[:, :s] == cand[:, None]).any(axis=1)
            got = np.where(need & ~dup, cand, got)
        picks[:, s] = got
        ok = ok & (got >= 0)
    return picks


def hypotheses(points, active_list, H, rnd, seed):
    """(H,4) fp32 planes, NaN where the hypothesis is not valid"""
    p = np.asarray(points, dtype=f32).astype(np.float64)
    planes = np.full((H, 4), np.nan, dtype=f32)
    picks = draw(H, len(active_list), rnd, seed)
    ok = (picks >= 0).all(axis=1)
    if not ok.any():
        return planes
    idx = np.asarray(active_list)[np.where(ok[:, None], picks, 0)]
    p0, p1, p2 = p[idx[:, 0]], p[idx[:, 1]], p[idx[:, 2]]
    u, v = p1 - p0, p2 - p0
    with np.errstate(all="ignore"):
        nx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        ny = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        nz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        nn = (nx * nx + ny * ny) + nz * nz
        ok = ok & (nn > 0) & np.isfinite(nn)
        inv = 1.0 / np.sqrt(nn)
        nx, ny, nz = nx * inv, ny * inv, nz * inv
        d = -((nx * p0[:, 0] + ny * p0[:, 1]) + nz * p0[:, 2])
        out = np.stack([nx, ny, nz, d], axis=1).astype(f32)
    planes[ok] = out[ok]
    return planes


def inlier(planes, points, threshold):
    """(H,N) bool: fabsf(((a * x + b * y) + c * z) + d) <= fp32(threshold), one fp32 operation per operator; NaN fails"""
    pl = np.asarray(planes, dtype=f32).reshape(-1, 4)
    p = np.asarray(points, dtype=f32)
    with np.errstate(all="ignore"):
        e = ((pl[:, 0:1] * p[None, :, 0] + pl[:, 1:2] * p[None, :, 1]) + pl[:, 2:3] * p[None, :, 2]) + pl[:, 3:4]
        return np.abs(e) <= f32(threshold)


def score(points, active, planes, threshold):
    """(H,) int32 inlier counts over the active points"""
    return (inlier(planes, points, threshold) & np.asarray(active)[None, :]).sum(axis=1).astype(np.int32)


def select(planes, counts, min_inliers):
    """(winner h or -1, its count or 0): the valid hypothesis of the greatest count, a tie to the lowest h"""
    valid = np.isfinite(planes).all(axis=1)
    if not valid.any():
        return -1, 0
    c = np.where(valid, counts.astype(np.int64), -1)
    h = int(np.argmax(c))                                  # the first of equal maxima
    if c[h] < max(int(min_inliers), 3):
        return -1, 0
    return h, int(c[h])


def wave_sum(v):
    """the DPP wave sum of 64 doubles: a balanced tree over adjacent lanes"""
    v = np.asarray(v, dtype=np.float64)
    while len(v) > 1:
        v = v[0::2] + v[1::2]
    return v[0]


def block_sums(values, select_mask):
    """values (N,C) float64, summed over the selected rows the way plane_fit_sums_kernel + the fold do: per block of FIT_CHUNK rows a
    lane takes base + c * 256 + lane in ascending c, the wave sum, the four waves as ((w0 + w1) + w2) + w3; the blocks in order"""
    values = np.asarray(values, dtype=np.float64)
    n, C = values.shape
    total = np.zeros(C)
    for base in range(0, n, FIT_CHUNK):
        lanes = np.zeros((256, C))
        for c in range(FIT_CHUNK // 256):
            lo = base + c * 256
            if lo >= n:
                break
            m = min(256, n - lo)
            lanes[:m] = lanes[:m] + np.where(select_mask[lo:lo + m, None], values[lo:lo + m], 0.0)
        w = [np.array([wave_sum(lanes[k * 64:(k + 1) * 64, j]) for j in range(C)]) for k in range(4)]
        total = total + (((w[0] + w[1]) + w[2]) + w[3])
    return total


def refit(points, mask, ransac_plane):
    """the least-squares plane through points[mask] as four fp32, and the same in float64"""
    p = np.where(mask[:, None], np.asarray(points, dtype=f32), 0).astype(np.float64)
    nanp = np.full(4, np.nan)
    s = block_sums(np.concatenate([p, np.ones((len(p), 1))], axis=1), mask)
    if not s[3] >= 3 or not np.isfinite(ransac_plane[:3]).all():
        return nanp.astype(f32), nanp
    cen = s[:3] / s[3]
    e = p - cen
    m = block_sums(np.stack([e[:, 0] * e[:, 0], e[:, 0] * e[:, 1], e[:, 0] * e[:, 2], e[:, 1] * e[:, 1], e[:, 1] * e[:, 2],
                             e[:, 2] * e[:, 2]], axis=1), mask)
    A = np.array([[m[0], m[1], m[2]], [m[1], m[3], m[4]], [m[2], m[4], m[5]]])
    w, V, _ = CO.jacobi_eigh(A[None], SWEEPS)
    w, V = w[0], V[0]
    s1 = w[1] < w[0]
    s2 = w[2] < (w[1] if s1 else w[0])
    n = V[:, 2 if s2 else (1 if s1 else 0)].copy()
    n = n * (1.0 / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))
    r = np.asarray(ransac_plane, dtype=f32).astype(np.float64)
    if (n[0] * r[0] + n[1] * r[1]) + n[2] * r[2] < 0:
        n = -n
    d = -((n[0] * cen[0] + n[1] * cen[1]) + n[2] * cen[2])
    out = np.array([n[0], n[1], n[2], d])
    return out.astype(f32), out


def segment_planes(points, threshold, max_planes, min_inliers=3, num_iterations=1000, seed=0):
    """-> {"labels" (N,) int32, "planes", "ransac_planes" (max_planes,4) fp32, "counts" (max_planes,) int32, "planes64"}"""
    p = np.asarray(points, dtype=f32)
    n = len(p)
    labels = np.full(n, -1, dtype=np.int32)
    planes = np.full((max_planes, 4), np.nan, dtype=f32)
    planes64 = np.full((max_planes, 4), np.nan)
    ransac = np.full((max_planes, 4), np.nan, dtype=f32)
    counts = np.zeros(max_planes, dtype=np.int32)
    ok = finite3(p)
    for r in range(max_planes):
        active = ok & (labels < 0)
        hyp = hypotheses(p, np.flatnonzero(active), num_iterations, r, seed)
        h, c = select(hyp, score(p, active, hyp, threshold), min_inliers)
        if h < 0:
            continue
        ransac[r], counts[r] = hyp[h], c
        took = active & inlier(hyp[h], p, threshold)[0]
        labels[took] = r
        planes[r], planes64[r] = refit(p, took, hyp[h])
    return {"labels": labels, "planes": planes, "ransac_planes": ransac, "counts": counts, "planes64": planes64}


def cluster_boxes(points, labels, n_clusters):
    p = np.asarray(points, dtype=f32)
    ok = finite3(p) & (labels >= 0) & (labels < n_clusters)
    count = np.bincount(labels[ok], minlength=n_clusters).astype(np.int32)
    lo = np.full((n_clusters, 3), np.inf, dtype=f32)
    hi = np.full((n_clusters, 3), -np.inf, dtype=f32)
    for c in range(n_clusters):
        m = ok & (labels == c)
        if m.any():
            lo[c], hi[c] = p[m].min(axis=0), p[m].max(axis=0)
    return {"count": count, "lo": lo, "hi": hi}
