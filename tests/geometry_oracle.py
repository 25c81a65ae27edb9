"""numpy restatement of the geometry kernels (csrc/point_nn.hip) for tests: the fp32 unprojection in its spelled order, the
brute-force nearest neighbour with the exact d2 expression, lowest-index ties, the NaN and max_d2 rules, and the reductions in
float64.  float32 arrays, one numpy operation per operator of the kernel's stated arithmetic.  The GPU outputs — of the
brute-force AND of the grid kernel — are compared with it bit for bit."""
import numpy as np

f32 = np.float32
INF = f32(np.inf)


def unproject(depths, Kinv, T_c2w, z_near, z_far):
    """(F*Hs*Ws, 3) fp32 world points, frame-major then row-major pixels.  depths: F arrays (Hs,Ws) fp32; Kinv fp32[9];
    T_c2w (F,3,4) fp32.  A depth that is not finite or outside [z_near, z_far] gives a NaN point."""
    Kinv = np.asarray(Kinv, dtype=f32).reshape(9)
    T_c2w = np.asarray(T_c2w, dtype=f32).reshape(len(depths), 12)
    z_near, z_far = f32(z_near), f32(z_far)
    Hs, Ws = depths[0].shape
    i, j = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing="ij")
    fi, fj = i.ravel().astype(f32), j.ravel().astype(f32)
    out = []
    with np.errstate(all="ignore"):
        a = (Kinv[0] * fj + Kinv[1] * fi) + Kinv[2]
        b = (Kinv[3] * fj + Kinv[4] * fi) + Kinv[5]
        c = (Kinv[6] * fj + Kinv[7] * fi) + Kinv[8]
        for f, depth in enumerate(depths):
            d = np.asarray(depth, dtype=f32).ravel()
            T = T_c2w[f]
            x, y, z = a * d, b * d, c * d
            X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3]
            Y = ((T[4] * x + T[5] * y) + T[6] * z) + T[7]
            Z = ((T[8] * x + T[9] * y) + T[10] * z) + T[11]
            assert X.dtype == Y.dtype == Z.dtype == f32
            ok = np.isfinite(d) & (z_near <= d) & (d <= z_far)
            p = np.stack([X, Y, Z], axis=1)
            p[~ok] = np.nan
            out.append(p)
    return np.concatenate(out)


def max_d2_of(max_distance):
    if max_distance is None:
        return INF
    m = f32(max_distance)
    return f32(m * m)


def nn_brute(query, ref, max_d2=INF, chunk=256):
    """query (Nq,3), ref (Nr,3) fp32 -> (d2 (Nq,) fp32, index (Nq,) int32): the least d2 = (dx*dx + dy*dy) + dz*dz among the
    reference points with d2 <= max_d2 and d2 < +inf (a NaN never compares), the lowest index among equal ones; none: -1, +inf"""
    query, ref = np.asarray(query, dtype=f32).reshape(-1, 3), np.asarray(ref, dtype=f32).reshape(-1, 3)
    max_d2 = f32(max_d2)
    d2_out = np.empty(len(query), dtype=f32)
    idx_out = np.empty(len(query), dtype=np.int32)
    rx, ry, rz = ref[None, :, 0], ref[None, :, 1], ref[None, :, 2]
    with np.errstate(all="ignore"):
        for s in range(0, len(query), chunk):
            q = query[s:s + chunk]
            dx, dy, dz = rx - q[:, 0:1], ry - q[:, 1:2], rz - q[:, 2:3]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == f32
            ok = (d2 <= max_d2) & (d2 < INF)
            d2 = np.where(ok, d2, INF)
            k = np.argmin(d2, axis=1)                    # the first of equal minima: the lowest index
            best = d2[np.arange(len(q)), k]
            d2_out[s:s + chunk] = best
            idx_out[s:s + chunk] = np.where(best < INF, k, -1)
    return d2_out, idx_out


def reduce(d2, threshold=0.0):
    """float64: (sum d2, sum sqrt(d2), number of finite entries, number of finite entries with d2 <= threshold^2)"""
    d = np.asarray(d2, dtype=f32).ravel()
    v = d[np.isfinite(d)].astype(np.float64)
    t = np.float64(f32(threshold))
    return float(v.sum()), float(np.sqrt(v).sum()), int(v.size), int((v <= t * t).sum())


def _mean(total, count):
    return total / count if count else float("nan")


def chamfer(x, y):
    """pytorch3d's default chamfer distance of two single clouds: the mean squared nearest-neighbour distance each way, summed"""
    sx, _, nx, _ = reduce(nn_brute(x, y)[0])
    sy, _, ny, _ = reduce(nn_brute(y, x)[0])
    return _mean(sx, nx) + _mean(sy, ny)


def cloud_metrics(pred, ref, threshold, max_distance=None):
    m = max_d2_of(max_distance)
    s2p, s1p, mp, hp = reduce(nn_brute(pred, ref, m)[0], threshold)
    s2r, s1r, mr, hr = reduce(nn_brute(ref, pred, m)[0], threshold)
    n_pred = int(np.isfinite(np.asarray(pred)).all(axis=1).sum())
    n_ref = int(np.isfinite(np.asarray(ref)).all(axis=1).sum())
    precision, recall = _mean(hp, n_pred), _mean(hr, n_ref)
    both = precision + recall
    return {"chamfer": _mean(s2p, mp) + _mean(s2r, mr), "accuracy": _mean(s1p, mp), "completeness": _mean(s1r, mr),
            "precision": precision, "recall": recall, "fscore": 2.0 * precision * recall / both if both > 0 else 0.0,
            "n_pred": n_pred, "n_ref": n_ref}
