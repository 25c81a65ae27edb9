"""numpy restatement of the cloud clean-up kernels (csrc/point_nn.hip: the k-NN kernels; csrc/point_cloud.hip) for tests: k nearest
neighbours over all pairs with the exact fp32 d2 expression and the (d2 bits, index) order, uniform voxel sampling with the fp32
voxel and centre arithmetic spelled out, the statistical outlier rule in float64, normals from a float64 covariance and
numpy.linalg.eigh — and, for the sweep count of the kernel's eigen-solver, the kernel's cyclic Jacobi loop itself (jacobi_eigh)."""
import numpy as np

f32 = np.float32
INF = f32(np.inf)
KNN_MAX_K = 32


def max_d2_of(max_distance):
    if max_distance is None:
        return INF
    m = f32(max_distance)
    return f32(m * m)


def _valid(points):
    return np.isfinite(np.asarray(points, dtype=f32).reshape(-1, 3)).all(axis=1)


def knn_brute(query, ref, k, max_d2=INF, exclude_self=False, chunk=256):
    """query (Nq,3), ref (Nr,3) fp32 -> (d2 (Nq,k) fp32, index (Nq,k) int32): per query the k least (d2 bits, index) among the
    reference points with d2 <= max_d2 and d2 < +inf (a NaN never compares), ascending; the tail of a short row: -1 / +inf"""
    query, ref = np.asarray(query, dtype=f32).reshape(-1, 3), np.asarray(ref, dtype=f32).reshape(-1, 3)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"k is in 1..{KNN_MAX_K}, not {k}")
    if exclude_self and len(query) != len(ref):
        raise ValueError("exclude_self: query and ref are the same cloud")
    max_d2 = f32(max_d2)
    nq, nr = len(query), len(ref)
    d2_out = np.full((nq, k), INF, dtype=f32)
    idx_out = np.full((nq, k), -1, dtype=np.int32)
    rx, ry, rz = ref[None, :, 0], ref[None, :, 1], ref[None, :, 2]
    ids = np.broadcast_to(np.arange(nr), (chunk, nr))
    with np.errstate(all="ignore"):
        for s in range(0, nq, chunk):
            q = query[s:s + chunk]
            dx, dy, dz = rx - q[:, 0:1], ry - q[:, 1:2], rz - q[:, 2:3]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == f32
            ok = (d2 <= max_d2) & (d2 < INF)
            if exclude_self:
                ok &= np.arange(nr)[None, :] != np.arange(s, s + len(q))[:, None]
            d2 = np.where(ok, d2, INF)
            bits = d2.view(np.uint32)                                    # (d2 >= 0: the bits order like the values)
            order = np.lexsort((ids[:len(q)], bits), axis=1)[:, :k]      # least (d2 bits, index) first
            rows = np.arange(len(q))[:, None]
            got, good = d2[rows, order], ok[rows, order]
            kk = order.shape[1]
            d2_out[s:s + chunk, :kk] = np.where(good, got, INF)
            idx_out[s:s + chunk, :kk] = np.where(good, order, -1)
    return d2_out, idx_out


def box_of(points):
    """fp32 minimum and maximum corner of the valid points"""
    p = np.asarray(points, dtype=f32).reshape(-1, 3)
    p = p[_valid(p)]
    return p.min(axis=0), p.max(axis=0)


def voxel_sample(points, voxel_size, origin=None):
    """-> (index (M,) int32 ascending, count (M,) int32).  Per axis in fp32: v = floor((p - o) / voxel), c = o + (v + 0.5) * voxel;
    the kept point of a voxel is its member of least (d2(p, c) bits, index); o defaults to the minimum corner of the valid points"""
    p = np.asarray(points, dtype=f32).reshape(-1, 3)
    ok = _valid(p)
    if not ok.any():
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    o = box_of(p)[0] if origin is None else np.asarray(origin, dtype=f32).reshape(3)
    h = f32(voxel_size)
    ids = np.flatnonzero(ok)
    q = p[ids]
    with np.errstate(all="ignore"):
        v = np.floor((q - o) / h)
        c = o + (v + f32(0.5)) * h
        d = q - c
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert v.dtype == c.dtype == d2.dtype == f32
    _, voxel = np.unique(v.astype(np.int64), axis=0, return_inverse=True)
    voxel = voxel.reshape(-1)
    order = np.lexsort((ids, d2.view(np.uint32), voxel))                 # by voxel, then (d2 bits, index)
    first = np.r_[True, voxel[order][1:] != voxel[order][:-1]]
    kept = ids[order[first]]
    counts = np.bincount(voxel)[voxel[order[first]]]
    back = np.argsort(kept)
    return kept[back].astype(np.int32), counts[back].astype(np.int32)


def mean_distance(d2, index):
    """(N,) float64: the mean of sqrt(d2) over the valid entries of every k-NN row in ascending column order; none: NaN"""
    d2, index = np.asarray(d2, dtype=f32), np.asarray(index)
    s, m = np.zeros(len(d2)), np.zeros(len(d2))
    for c in range(d2.shape[1]):
        ok = index[:, c] >= 0
        s = s + np.where(ok, np.sqrt(np.where(ok, d2[:, c], 0).astype(np.float64)), 0.0)
        m = m + ok
    with np.errstate(all="ignore"):
        return np.where(m > 0, s / m, np.nan)


def statistical_outliers(points, nb_neighbors=20, std_ratio=2.0):
    """-> dict(keep (N,) bool, mean_distance (N,) float64, mean, std, threshold): Open3D's documented rule, the point itself among
    its neighbours, mean and std (divisor n - 1) over the points that are points"""
    md = mean_distance(*knn_brute(points, points, nb_neighbors))
    v = md[np.isfinite(md)]
    mean = float(v.sum() / len(v)) if len(v) else float("nan")
    std = float(np.sqrt(((v - mean) ** 2).sum() / (len(v) - 1))) if len(v) > 1 else 0.0
    thr = mean + float(std_ratio) * std
    with np.errstate(invalid="ignore"):
        return dict(keep=md <= thr, mean_distance=md, mean=mean, std=std, threshold=thr)


def covariances(points, knn_index):
    """(N,3,3) float64 covariance of every neighbourhood (centroid first, then the centred products: the textbook two passes) and
    (N,) the number of valid neighbours"""
    p = np.asarray(points, dtype=f32).reshape(-1, 3).astype(np.float64)
    idx = np.asarray(knn_index)
    ok = idx >= 0
    m = ok.sum(axis=1)
    nb = np.where(ok[:, :, None], p[np.where(ok, idx, 0)], 0.0)
    with np.errstate(all="ignore"):
        mean = nb.sum(axis=1) / m[:, None]
        e = np.where(ok[:, :, None], nb - mean[:, None, :], 0.0)
        C = np.einsum("nki,nkj->nij", e, e) / m[:, None, None]
    return C, m


def orient(n, points, viewpoints=None, view_of=None):
    n = n.copy()
    if viewpoints is not None:
        to_view = np.asarray(viewpoints, dtype=f32).astype(np.float64)[np.asarray(view_of)] - np.asarray(points, dtype=f32).astype(np.float64)
        flip = (n * to_view).sum(axis=1) < 0
    else:
        big = np.argmax(np.abs(n), axis=1)                                # the first of equal magnitudes: the lowest axis
        flip = n[np.arange(len(n)), big] < 0
    n[flip] *= -1
    return n


def normals(points, k=16, viewpoints=None, view_of=None, knn_index=None):
    """-> (normals (N,3) float64 (NaN with fewer than 3 neighbours), eigenvalues (N,3) ascending): eigh of the float64 covariance,
    the eigenvector of the least eigenvalue, oriented by the kernel's rule"""
    if knn_index is None:
        knn_index = knn_brute(points, points, k)[1]
    C, m = covariances(points, knn_index)
    good = m >= 3
    w = np.full((len(C), 3), np.nan)
    n = np.full((len(C), 3), np.nan)
    if good.any():
        ww, vv = np.linalg.eigh(C[good])
        w[good], n[good] = ww, vv[:, :, 0]
        n[good] = orient(n[good], np.asarray(points, dtype=f32).reshape(-1, 3)[good], viewpoints,
                         None if view_of is None else np.asarray(view_of)[good])
    return n, w


def jacobi_eigh(C, sweeps):
    """the kernel's eigen-solver on a batch of symmetric 3x3 float64 matrices: `sweeps` cyclic sweeps of Jacobi rotations over the
    pairs (0,1), (0,2), (1,2).  -> (diagonal (N,3), eigenvector columns (N,3,3), off-diagonal mass left / trace)"""
    A = np.array(C, dtype=np.float64)
    V = np.broadcast_to(np.eye(3), A.shape).copy()
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                apq = A[:, p, q]
                live = apq != 0
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * np.where(live, apq, 1.0))
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(live, t, 0.0)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                app, aqq = A[:, p, p] - t * apq, A[:, q, q] + t * apq
                apr, aqr = c * A[:, p, r] - s * A[:, q, r], s * A[:, p, r] + c * A[:, q, r]
                A[:, p, p], A[:, q, q] = app, aqq
                A[:, p, q] = A[:, q, p] = np.where(live, 0.0, apq)
                A[:, p, r] = A[:, r, p] = apr
                A[:, q, r] = A[:, r, q] = aqr
                vp, vq = c[:, None] * V[:, :, p] - s[:, None] * V[:, :, q], s[:, None] * V[:, :, p] + c[:, None] * V[:, :, q]
                V[:, :, p], V[:, :, q] = vp, vq
        off = np.sqrt(A[:, 0, 1] ** 2 + A[:, 0, 2] ** 2 + A[:, 1, 2] ** 2) / np.trace(A, axis1=1, axis2=2)
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], 1), V, off


def clean_pipeline(points, frame_pixels, centres, voxel_size=None, nb_neighbors=None, std_ratio=2.0, want_normals=False, normal_k=16):
    """merged_point_cloud's clean-up on the uncompacted cloud -> dict(index int32[, normals float64, eigenvalues])"""
    p = np.asarray(points, dtype=f32).reshape(-1, 3)
    index = np.flatnonzero(_valid(p))
    if voxel_size is not None and len(index):
        index = index[voxel_sample(p[index], voxel_size)[0]]
    if nb_neighbors is not None and len(index):
        index = index[statistical_outliers(p[index], nb_neighbors, std_ratio)["keep"]]
    out = {"index": index.astype(np.int32)}
    if want_normals:
        out["normals"], out["eigenvalues"] = normals(p[index], normal_k, centres, index // frame_pixels)
    return out
