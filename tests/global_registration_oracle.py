"""numpy restatement of the global registration kernels (csrc/point_global.hip) for tests, on cloud_oracle (k-NN, normals),
icp_oracle (transform, accumulate, update, the ICP loop, the test surface) and sampler_oracle (Philox4x32-10): the FPFH pair
features, bins, counts and combine in float64 with the kernel's expressions operation for operation; the nearest feature with the
fp32 sum in ascending j; the RANSAC draw rule, checks and Horn's closed form with the kernel's cyclic Jacobi loop; the fp32 scoring,
the packed best, the inliers and the refit; and register_ransac / register_global as loops over them.  Test infrastructure only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import cloud_oracle as CO  # noqa: E402
import icp_oracle as IO  # noqa: E402
import sampler_oracle as SO  # noqa: E402

f32 = np.float32
INF = f32(np.inf)
FPFH_DIM, FPFH_ROW = 33, 34
MAX_DRAWS = 16                    # csrc/point_global.hip: RANSAC_MAX_DRAWS
SWEEPS = 8                        # RANSAC_SWEEPS
PAIRS4 = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
# the bin edges of theta, (cos, sin)(-pi + 2 pi b / 11) for b = 1..10: the literals of csrc/point_global.hip
EDGES = ((-0.8412535328311811, -0.5406408174555978), (-0.4154150130018863, -0.9096319953545184),
         (0.14231483827328512, -0.9898214418809327), (0.6548607339452851, -0.7557495743542583),
         (0.9594929736144975, -0.2817325568414295), (0.9594929736144975, 0.2817325568414295),
         (0.6548607339452851, 0.7557495743542583), (0.14231483827328512, 0.9898214418809327),
         (-0.41541501300188616, 0.9096319953545186), (-0.8412535328311813, 0.5406408174555974))


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


# ---------------------------------------------------------------- FPFH
def theta_bin(x, y):
    """the bin of atan2(y, x) among 11 over [-pi, pi] without the arctangent: half-plane tests against the ten edge directions"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    past = [(c * y - s * x >= 0.0).astype(np.int64) for c, s in EDGES]
    lower = ((past[0] + past[1]) + past[2]) + past[3] + past[4]
    upper = 5 + (((past[5] + past[6]) + past[7]) + past[8] + past[9])
    out = np.where(y < 0.0, lower, upper)
    return np.where((x == 0.0) & (y == 0.0), 5, out)


def theta_bin_arctan(x, y):
    """the formula the rule replaces: floor(11 (theta + pi) / 2 pi), clamped"""
    t = np.floor(11.0 * (np.arctan2(y, x) + np.pi) / (2.0 * np.pi))
    return np.clip(t, 0, 10).astype(np.int64)


def unit_bin(f):
    t = np.floor((11.0 * (np.asarray(f, dtype=np.float64) + 1.0)) * 0.5)
    return np.clip(t, 0, 10).astype(np.int64)


def pair_features(p1, n1, p2, n2):
    """(ok, theta bin, f1 bin, f2 bin) of the pairs (p1, n1) -> (p2, n2), float64 rows: the kernel's expressions"""
    with np.errstate(all="ignore"):
        dp = p2 - p1
        d = np.sqrt(dot3(dp, dp))
        ok = d != 0.0
        a1, a2 = dot3(n1, dp) / d, dot3(n2, dp) / d
        swap = np.abs(a1) < np.abs(a2)
        m1 = np.where(swap[:, None], n2, n1)
        m2 = np.where(swap[:, None], n1, n2)
        f2 = np.where(swap, -a2, a1)
        dp = np.where(swap[:, None], -dp, dp)
        v = cross3(dp, m1)
        vn = np.sqrt(dot3(v, v))
        ok &= vn != 0.0
        v = v / vn[:, None]
        w = cross3(m1, v)
        f1 = dot3(v, m2)
        x, y = dot3(m1, m2), dot3(w, m2)
        ok &= np.isfinite(vn) & np.isfinite(d)
        return ok, theta_bin(np.where(ok, x, 1.0), np.where(ok, y, 0.0)), unit_bin(np.where(ok, f1, 0.0)), unit_bin(np.where(ok, f2, 0.0))


def fpfh_counts(points, normals, knn_index):
    """(N, 34) int32: the 33 counts and the number of pairs counted"""
    p32, n32 = np.asarray(points, dtype=f32).reshape(-1, 3), np.asarray(normals, dtype=f32).reshape(-1, 3)
    idx = np.asarray(knn_index)
    N = len(p32)
    fine = np.isfinite(p32).all(1) & np.isfinite(n32).all(1)
    p, n = p32.astype(np.float64), n32.astype(np.float64)
    counts = np.zeros((N, FPFH_ROW), dtype=np.int32)
    rows = np.arange(N)
    for c in range(idx.shape[1]):
        j = idx[:, c]
        ok = fine & (j >= 0) & (j < N) & (j != rows)
        jj = np.where(ok, j, 0)
        ok &= fine[jj]
        good, tb, b1, b2 = pair_features(p, n, p[jj], n[jj])
        ok &= good
        r = rows[ok]
        np.add.at(counts, (r, tb[ok]), 1)
        np.add.at(counts, (r, 11 + b1[ok]), 1)
        np.add.at(counts, (r, 22 + b2[ok]), 1)
        counts[r, 33] += 1
    return counts


def fpfh_combine(counts, points, normals, knn_index, knn_d2):
    """(N, 33) fp32"""
    p32, n32 = np.asarray(points, dtype=f32).reshape(-1, 3), np.asarray(normals, dtype=f32).reshape(-1, 3)
    idx, d2 = np.asarray(knn_index), np.asarray(knn_d2, dtype=f32)
    counts = np.asarray(counts)
    N = len(p32)
    m = counts[:, 33]
    A = np.zeros((N, FPFH_DIM))
    with np.errstate(all="ignore"):
        for c in range(1, idx.shape[1]):
            j = idx[:, c]
            ok = (j >= 0) & (j < N) & (d2[:, c] > 0) & np.isfinite(d2[:, c])
            jj = np.where(ok, j, 0)
            ok &= m[jj] > 0
            scale = 100.0 / np.where(ok, m[jj], 1).astype(np.float64)
            dd = np.where(ok, d2[:, c], 1).astype(np.float64)
            term = (counts[jj, :FPFH_DIM].astype(np.float64) * scale[:, None]) / dd[:, None]
            A = A + np.where(ok[:, None], term, 0.0)
        own = counts[:, :FPFH_DIM].astype(np.float64) * np.where(m > 0, 100.0 / np.where(m > 0, m, 1).astype(np.float64), 0.0)[:, None]
        out = np.zeros((N, FPFH_DIM))
        for f in range(3):
            S = A[:, f * 11].copy()
            for b in range(1, 11):
                S = S + A[:, f * 11 + b]
            blk = slice(f * 11, f * 11 + 11)
            safe = np.where(S == 0.0, 1.0, S)[:, None]
            out[:, blk] = np.where((S == 0.0)[:, None], own[:, blk], (100.0 * A[:, blk]) / safe + own[:, blk])
    out = out.astype(f32)
    out[~(np.isfinite(p32).all(1) & np.isfinite(n32).all(1))] = np.nan
    return out


def fpfh(points, normals, k=32, radius=None):
    """-> (features (N,33) fp32, counts (N,34) int32): the neighbourhood is cloud_oracle's exact k-NN with the radius"""
    d2, idx = CO.knn_brute(points, points, k, CO.max_d2_of(radius))
    counts = fpfh_counts(points, normals, idx)
    return fpfh_combine(counts, points, normals, idx, d2), counts


# ---------------------------------------------------------------- nearest feature
def match(source, target, chunk=128):
    """-> (d2 (Ns,) fp32, index (Ns,) int32): the target row of least (d2 bits, index), d2 summed in fp32 in ascending j"""
    a, b = np.asarray(source, dtype=f32), np.asarray(target, dtype=f32)
    d2_out, idx_out = np.full(len(a), INF, dtype=f32), np.full(len(a), -1, dtype=np.int32)
    with np.errstate(all="ignore"):
        for s in range(0, len(a), chunk):
            q = a[s:s + chunk]
            d = q[:, None, 0] - b[None, :, 0]
            acc = d * d
            for j in range(1, a.shape[1]):
                d = q[:, None, j] - b[None, :, j]
                acc = acc + d * d
            assert acc.dtype == f32
            acc = np.where(acc < INF, acc, INF)                            # (a NaN never compares)
            best = np.argmin(acc, axis=1)                                  # (the first of equal values: the lowest index)
            got = acc[np.arange(len(q)), best]
            d2_out[s:s + chunk] = got
            idx_out[s:s + chunk] = np.where(got < INF, best, -1)
    return d2_out, idx_out


def match_mutual(source, target):
    """-> the set of (i, j) with j nearest to i and i nearest to j"""
    _, fwd = match(source, target)
    _, back = match(target, source)
    return {(i, int(j)) for i, j in enumerate(fwd) if j >= 0 and back[j] == i}


def correspondences_of(index):
    rows = np.flatnonzero(np.asarray(index) >= 0)
    return np.stack([rows, np.asarray(index)[rows]], axis=1).astype(np.int32)


# ---------------------------------------------------------------- RANSAC
def draw(H, C, n, seed):
    """(H,4) int32 picks of hypotheses 0..H-1 (-1: past n, or a failed draw): slot by slot, word 0 of Philox at counter
    (h, draw, 0, 0) under the seed's two words, pick = (word * C) >> 32, a duplicate of an earlier slot drawn again, at most
    MAX_DRAWS draws per hypothesis"""
    h = np.arange(H, dtype=np.uint64)
    picks = np.full((H, 4), -1, dtype=np.int64)
    draws = np.zeros(H, dtype=np.uint64)
    key = (int(seed) & SO.MASK32, int(seed) >> 32)
    for s in range(n):
        got = np.full(H, -1, dtype=np.int64)
        for _ in range(MAX_DRAWS):
            need = (got < 0) & (draws < MAX_DRAWS)
            if not need.any():
                break
            w = SO.philox4x32_10((h, draws, 0, 0), key)[0]
            cand = ((w * np.uint64(C)) >> np.uint64(32)).astype(np.int64)
            draws = draws + need.astype(np.uint64)
            dup = (picks[:, :s] == cand[:, None]).any(axis=1)
            got = np.where(need & ~dup, cand, got)
        picks[:, s] = got
    return picks.astype(np.int32)


def jacobi4(A):
    """the kernel's eigen-solver on a batch of symmetric 4x4 matrices: SWEEPS cyclic sweeps over PAIRS4 -> (diagonal (H,4),
    eigenvector columns (H,4,4))"""
    A = np.array(A, dtype=np.float64)
    V = np.broadcast_to(np.eye(4), A.shape).copy()
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q in PAIRS4:
                apq = A[:, p, q].copy()
                live = apq != 0
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * np.where(live, apq, 1.0))
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(live, t, 0.0)                                 # (t = 0: c = 1, s = 0, nothing moves)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                A[:, p, p], A[:, q, q] = A[:, p, p] - t * apq, A[:, q, q] + t * apq
                A[:, p, q] = A[:, q, p] = np.where(live, 0.0, apq)
                for r in range(4):
                    if r in (p, q):
                        continue
                    pr, qr = A[:, p, r].copy(), A[:, q, r].copy()
                    A[:, p, r] = A[:, r, p] = np.where(live, c * pr - s * qr, pr)
                    A[:, q, r] = A[:, r, q] = np.where(live, s * pr + c * qr, qr)
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = np.where(live[:, None], c[:, None] * vp - s[:, None] * vq, vp)
                V[:, :, q] = np.where(live[:, None], s[:, None] * vp + c[:, None] * vq, vq)
    return np.stack([A[:, e, e] for e in range(4)], axis=1), V


def horn(p, q):
    """(H,n,3) float64 source and target samples -> (H,3,4) poses [R | t] by Horn's closed form, the kernel's expressions"""
    n = p.shape[1]
    with np.errstate(all="ignore"):
        cs, ct = p[:, 0] + p[:, 1], q[:, 0] + q[:, 1]
        for s in range(2, n):
            cs, ct = cs + p[:, s], ct + q[:, s]
        cs, ct = cs / float(n), ct / float(n)
        S = np.zeros((len(p), 3, 3))
        for a in range(3):
            for b in range(3):
                u = (p[:, 0, a] - cs[:, a]) * (q[:, 0, b] - ct[:, b])
                for s in range(1, n):
                    u = u + (p[:, s, a] - cs[:, a]) * (q[:, s, b] - ct[:, b])
                S[:, a, b] = u
        A = np.zeros((len(p), 4, 4))
        A[:, 0, 0] = (S[:, 0, 0] + S[:, 1, 1]) + S[:, 2, 2]
        A[:, 0, 1], A[:, 0, 2], A[:, 0, 3] = S[:, 1, 2] - S[:, 2, 1], S[:, 2, 0] - S[:, 0, 2], S[:, 0, 1] - S[:, 1, 0]
        A[:, 1, 1] = (S[:, 0, 0] - S[:, 1, 1]) - S[:, 2, 2]
        A[:, 1, 2], A[:, 1, 3] = S[:, 0, 1] + S[:, 1, 0], S[:, 2, 0] + S[:, 0, 2]
        A[:, 2, 2] = (S[:, 1, 1] - S[:, 0, 0]) - S[:, 2, 2]
        A[:, 2, 3] = S[:, 1, 2] + S[:, 2, 1]
        A[:, 3, 3] = (S[:, 2, 2] - S[:, 0, 0]) - S[:, 1, 1]
        for a in range(4):
            for b in range(a):
                A[:, a, b] = A[:, b, a]
        w, V = jacobi4(A)
        big, e = w[:, 0].copy(), np.zeros(len(p), dtype=np.int64)
        for k in range(1, 4):                                             # the largest, the lowest index on a tie
            better = w[:, k] > big
            big, e = np.where(better, w[:, k], big), np.where(better, k, e)
        quat = V[np.arange(len(p)), :, e]
        qn = np.sqrt(((quat[:, 0] * quat[:, 0] + quat[:, 1] * quat[:, 1]) + quat[:, 2] * quat[:, 2]) + quat[:, 3] * quat[:, 3])
        qw, qx, qy, qz = (quat[:, k] / qn for k in range(4))
        T = np.zeros((len(p), 3, 4))
        T[:, 0, 0], T[:, 0, 1], T[:, 0, 2] = 1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)
        T[:, 1, 0], T[:, 1, 1], T[:, 1, 2] = 2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)
        T[:, 2, 0], T[:, 2, 1], T[:, 2, 2] = 2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)
        for r in range(3):
            T[:, r, 3] = ct[:, r] - ((T[:, r, 0] * cs[:, 0] + T[:, r, 1] * cs[:, 1]) + T[:, r, 2] * cs[:, 2])
    return T


def kabsch(p, q):
    """(n,3) -> 3x4 [R | t] of least squares by numpy.linalg.svd: the outside reference of horn()"""
    cs, ct = p.mean(0), q.mean(0)
    U, _, Vt = np.linalg.svd((p - cs).T @ (q - ct))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return np.concatenate([R, (ct - R @ cs)[:, None]], axis=1)


def hypotheses(source, target, corr, H, n, similarity, max_distance, seed):
    """-> (samples (H,4) int32, valid (H,) int32, poses (H,12) float64: zeros where not valid)"""
    src, tgt = np.asarray(source, dtype=f32).reshape(-1, 3), np.asarray(target, dtype=f32).reshape(-1, 3)
    corr = np.asarray(corr).reshape(-1, 2)
    picks = draw(H, len(corr), n, seed)
    ok = (picks[:, :n] >= 0).all(axis=1)
    rows = corr[np.where(picks[:, :n] >= 0, picks[:, :n], 0)]                 # (H,n,2)
    si, ti = rows[:, :, 0], rows[:, :, 1]
    ok &= ((si >= 0) & (si < len(src)) & (ti >= 0) & (ti < len(tgt))).all(axis=1)
    p32, q32 = src[np.clip(si, 0, len(src) - 1)], tgt[np.clip(ti, 0, len(tgt) - 1)]
    ok &= np.isfinite(p32).all(axis=(1, 2)) & np.isfinite(q32).all(axis=(1, 2))
    p = np.where(ok[:, None, None], p32, 0).astype(np.float64)
    q = np.where(ok[:, None, None], q32, 0).astype(np.float64)
    with np.errstate(all="ignore"):
        for b in range(1, n):
            for a in range(b):
                ea, eb = p[:, a] - p[:, b], q[:, a] - q[:, b]
                la, lb = np.sqrt(dot3(ea, ea)), np.sqrt(dot3(eb, eb))
                ok &= (la >= similarity * lb) & (lb >= similarity * la)
        T = horn(p, q)
        ok &= np.isfinite(T).all(axis=(1, 2))
        limit = max_distance * max_distance
        for s in range(n):
            e = np.stack([(((T[:, r, 0] * p[:, s, 0] + T[:, r, 1] * p[:, s, 1]) + T[:, r, 2] * p[:, s, 2]) + T[:, r, 3]) - q[:, s, r]
                          for r in range(3)], axis=1)
            ok &= dot3(e, e) <= limit
    poses = np.where(ok[:, None], T.reshape(H, 12), 0.0)
    return picks, ok.astype(np.int32), poses


def pairs_of(source, target, corr):
    """(C,3) fp32 source and target points of the correspondences, NaN where a row names no pair of points"""
    src, tgt = np.asarray(source, dtype=f32).reshape(-1, 3), np.asarray(target, dtype=f32).reshape(-1, 3)
    corr = np.asarray(corr).reshape(-1, 2)
    ok = (corr[:, 0] >= 0) & (corr[:, 0] < len(src)) & (corr[:, 1] >= 0) & (corr[:, 1] < len(tgt))
    s, t = src[np.where(ok, corr[:, 0], 0)].copy(), tgt[np.where(ok, corr[:, 1], 0)].copy()
    s[~ok], t[~ok] = np.nan, np.nan
    return s, t


def inlier_mask(pose, s, t, max_distance):
    """(C,) bool: the score's rule for one pose (12 float64): fp32 transform, fp32 d2 <= fp32(distance)^2"""
    T = np.zeros(16)
    T[:12] = np.asarray(pose, dtype=np.float64).reshape(12)
    moved = IO.transform(s, T)
    with np.errstate(all="ignore"):
        dx, dy, dz = moved[:, 0] - t[:, 0], moved[:, 1] - t[:, 1], moved[:, 2] - t[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == f32
        return d2 <= CO.max_d2_of(max_distance)


def score(source, target, corr, poses, valid, max_distance):
    """-> (counts (H,) int32: -1 where not valid, best: the packed integer, 0 without a valid hypothesis)"""
    s, t = pairs_of(source, target, corr)
    counts = np.full(len(poses), -1, dtype=np.int32)
    best = 0
    for h in np.flatnonzero(np.asarray(valid) != 0):
        counts[h] = int(inlier_mask(poses[h], s, t, max_distance).sum())
        best = max(best, (int(counts[h]) << 32) | (0xFFFFFFFF - int(h)))
    return counts, best


def unpack(best):
    """(hypothesis, count) of a packed best; (-1, 0) for 0"""
    return (-1, 0) if best == 0 else (0xFFFFFFFF - (best & 0xFFFFFFFF), best >> 32)


def inliers(source, target, corr, poses, best, max_distance):
    """-> (mask (C,) uint8, index (Ns,) int32, T 4x4 or None, (hypothesis, count))"""
    corr = np.asarray(corr).reshape(-1, 2)
    ns = len(np.asarray(source).reshape(-1, 3))
    h, count = unpack(int(best))
    mask, index = np.zeros(len(corr), dtype=np.uint8), np.full(ns, -1, dtype=np.int32)
    if h < 0:
        return mask, index, None, (h, count)
    s, t = pairs_of(source, target, corr)
    mask = inlier_mask(poses[h], s, t, max_distance).astype(np.uint8)
    np.maximum.at(index, corr[mask != 0, 0], corr[mask != 0, 1])
    T = np.eye(4)
    T[:3] = np.asarray(poses[h]).reshape(3, 4)
    return mask, index, T, (h, count)


def refit(source, target, index, T, iterations):
    """`iterations` point-to-point Gauss-Newton steps on the fixed correspondences `index`: icp_oracle's accumulate and update with
    criteria 0 (no stop rule) and d2 = 0"""
    state = IO.new_state(T)
    zeros = np.zeros(len(index), dtype=f32)
    for it in range(iterations):
        moved = IO.transform(source, state[:16])
        state, _ = IO.update(IO.accumulate(moved, target, None, index, zeros)[0], it, 0.0, 0.0, state)
    return state[:16].reshape(4, 4).copy()


def register_ransac(source, target, corr, max_distance, max_iterations=100_000, ransac_n=3, edge_length_similarity=0.9, seed=0,
                    refit_iterations=4):
    picks, valid, poses = hypotheses(source, target, corr, max_iterations, ransac_n, edge_length_similarity, max_distance, seed)
    counts, best = score(source, target, corr, poses, valid, max_distance)
    mask, index, T, (h, count) = inliers(source, target, corr, poses, best, max_distance)
    out = {"hypothesis": h, "inliers": {"count": count, "mask": mask != 0}, "valid_hypotheses": int(valid.sum()), "status": 0 if h >= 0 else 2,
           "samples": picks, "valid": valid, "poses": poses, "counts": counts, "best": best}
    T = np.eye(4) if T is None else refit(source, target, index, T, refit_iterations)
    out.update(transformation=T, **{k: v for k, v in IO.evaluate(source, target, max_distance, T).items() if k != "correspondences"})
    return out


def register_global(source, source_normals, target, target_normals, max_distance, feature_k=32, feature_radius=None, mutual=False,
                    refine=True, **ransac):
    """features, matching, RANSAC and (refine) point-to-plane ICP from its pose, on the clouds and normals as given"""
    fs, _ = fpfh(source, source_normals, feature_k, feature_radius)
    ft, _ = fpfh(target, target_normals, feature_k, feature_radius)
    if mutual:
        corr = np.array(sorted(match_mutual(fs, ft)), dtype=np.int32).reshape(-1, 2)
    else:
        corr = correspondences_of(match(fs, ft)[1])
    coarse = register_ransac(source, target, corr, max_distance, **ransac)
    out = {"ransac": coarse, "icp": None, "correspondences": corr, "transformation": coarse["transformation"]}
    if refine:
        out["icp"] = IO.register_icp(source, target, max_distance, init=coarse["transformation"], normals=target_normals)
        out["transformation"] = out["icp"]["transformation"]
    return out


# ---------------------------------------------------------------- the test case: two clouds that share no frame
def far_motion():
    """the 140 degree motion of the recovery tests: far outside what ICP converges from"""
    return IO.rigid(140.0, [1.0, -2.0, 1.5], [0.6, -0.7, 0.9])


def moved_normals(normals, T):
    return (np.asarray(normals, dtype=f32).astype(np.float64) @ T[:3, :3].T).astype(f32)
