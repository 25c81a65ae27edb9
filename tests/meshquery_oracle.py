"""CPU restatement of csrc/mesh_query.hip (include/sgam_hip.h, "Queries against a triangle mesh"): the point–triangle rule in
np.float32, one IEEE operation at a time and in the kernel's order, the (d2 bits, index) winner, twice-the-area, the integer
weights and their sums, and the area-uniform sampler on sampler_oracle.philox4x32_10 with Python integers for mulhi64.  Test
infrastructure only — the product path never imports it."""
import numpy as np

import sampler_oracle

f32 = np.float32
INF, NAN = f32(np.inf), f32(np.nan)                 # (region codes: 0 1 2 the vertices a b c, 3 4 5 the edges ab bc ca, 6 the face)


def _quiet(fn):
    def run(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    run.__doc__ = fn.__doc__
    return run


def dot3(u, v):
    """(u.x * v.x + u.y * v.y) + u.z * v.z on (...,3) float32 arrays"""
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def dist2(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


@_quiet
def normals(a, b, c):
    """n = ab x ac, each component a difference of two products; -> (n (...,3), dot(n, n))"""
    ab, ac = b - a, c - a
    n = np.stack([ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1], ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2],
                  ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]], -1)
    return n, dot3(n, n)


def corners(vertices, triangles):
    """(a, b, c (nt,3) float32, ok (nt,) bool: the triangle's three indices lie inside the mesh) — corners of a bad one are NaN"""
    v, t = np.asarray(vertices, dtype=f32).reshape(-1, 3), np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    ok = ((t >= 0) & (t < len(v))).all(1)
    safe = np.where(ok[:, None], t, 0)
    out = [np.where(ok[:, None], v[safe[:, k]], NAN).astype(f32) if len(v) else np.full((len(t), 3), NAN, f32) for k in range(3)]
    return out[0], out[1], out[2], ok


@_quiet
def candidates(a, b, c):
    fin = np.isfinite(a).all(-1) & np.isfinite(b).all(-1) & np.isfinite(c).all(-1)
    return fin & (normals(a, b, c)[1] > 0)


@_quiet
def point_triangle(a, b, c, q):
    """the closest point of triangles (a, b, c) to queries q (all (...,3) float32, broadcast against each other)
    -> (d2, closest (...,3), region code 0..6)"""
    a, b, c, q = np.broadcast_arrays(*(np.asarray(x, dtype=f32) for x in (a, b, c, q)))
    ab, ac, bc = b - a, c - a, c - b
    ap, bp, cp = q - a, q - b, q - c
    p1, p2 = dot3(ab, ap), dot3(ac, ap)
    p3, p4 = dot3(ab, bp), dot3(ac, bp)
    p5, p6 = dot3(ab, cp), dot3(ac, cp)
    vc = p1 * p4 - p3 * p2
    vb = p5 * p2 - p1 * p6
    va = p3 * p6 - p5 * p4
    e43, e56 = p4 - p3, p5 - p6
    tests = [((p1 <= 0) & (p2 <= 0), 0), ((p3 >= 0) & (p4 <= p3), 1), ((vc <= 0) & (p1 >= 0) & (p3 <= 0), 3), ((p6 >= 0) & (p5 <= p6), 2),
             ((vb <= 0) & (p2 >= 0) & (p6 <= 0), 5), ((va <= 0) & (e43 >= 0) & (e56 >= 0), 4)]
    region = np.full(p1.shape, 6, dtype=np.int32)
    for cond, code in reversed(tests):
        region = np.where(cond, np.int32(code), region)
    total = (va + vb) + vc
    zero, one = np.zeros_like(p1), np.ones_like(p1)
    n1 = np.select([region == 3, region == 5, region == 4, region == 6], [p1, p2, e43, vb], zero)
    m1 = np.select([region == 3, region == 5, region == 4, region == 6], [p1 - p3, p2 - p6, e43 + e56, total], one)
    n2, m2 = np.where(region == 6, vc, zero), np.where(region == 6, total, one)
    s1, s2 = (n1 / m1).astype(f32), (n2 / m2).astype(f32)
    from_b, from_c = ((region == 1) | (region == 4))[..., None], (region == 2)[..., None]
    base = np.where(from_b, b, np.where(from_c, c, a))
    e1 = np.where((region == 5)[..., None], ac, np.where((region == 4)[..., None], bc, ab))
    x = ((base + e1 * s1[..., None]) + ac * s2[..., None]).astype(f32)
    return dist2(x, q).astype(f32), x, region


def _bits(d2):
    return np.ascontiguousarray(d2, dtype=f32).view(np.uint32).astype(np.int64)


@_quiet
def mesh_distance(vertices, triangles, query, max_d2=np.inf, chunk=256):
    """every query against every candidate -> dict(d2 (Nq,) float32, triangle (Nq,) int32, closest (Nq,3) float32, region (Nq,) int32
    (-1 without a winner), bad_index: a triangle names a vertex outside the mesh)"""
    q = np.asarray(query, dtype=f32).reshape(-1, 3)
    a, b, c, ok = corners(vertices, triangles)
    cand = np.flatnonzero(candidates(a, b, c))
    nq = len(q)
    out = dict(d2=np.full(nq, INF, f32), triangle=np.full(nq, -1, np.int32), closest=np.full((nq, 3), NAN, f32),
               region=np.full(nq, -1, np.int32), bad_index=bool((~ok).any()))
    if not len(cand) or not nq:
        return out
    max_d2 = f32(max_d2)
    point = np.isfinite(q).all(1)
    for s in range(0, nq, chunk):
        qs = q[s:s + chunk]
        d2, x, region = point_triangle(a[cand][None], b[cand][None], c[cand][None], qs[:, None])
        usable = (d2 <= max_d2) & np.isfinite(d2) & point[s:s + chunk, None]
        key = np.where(usable, (_bits(d2) << 32) | cand[None], np.iinfo(np.int64).max)
        j = key.argmin(1)
        rows = np.arange(len(qs))
        won = usable[rows, j]
        out["d2"][s:s + chunk] = np.where(won, d2[rows, j], INF)
        out["triangle"][s:s + chunk] = np.where(won, cand[j], -1)
        out["closest"][s:s + chunk] = np.where(won[:, None], x[rows, j], NAN)
        out["region"][s:s + chunk] = np.where(won, region[rows, j], -1)
    return out


@_quiet
def area2(vertices, triangles):
    """(nt,) float32: sqrt(dot(n, n)), twice the area; 0 for what is not a triangle"""
    a, b, c, _ = corners(vertices, triangles)
    nn = normals(a, b, c)[1]
    return np.where(candidates(a, b, c), np.sqrt(nn.astype(f32)), f32(0)).astype(f32)


def weights(a2):
    """w[t] = floor(double(A2[t]) / double(max A2) * 2^32) as int64, and their inclusive sums"""
    a2 = np.asarray(a2, dtype=f32).astype(np.float64)
    top = a2.max() if len(a2) else 0.0
    if not top > 0:
        w = np.zeros(len(a2), dtype=np.int64)
    else:
        w = np.floor(a2 / top * 4294967296.0).astype(np.int64)
    return w, np.cumsum(w, dtype=np.int64)


def sample_words(seed, n):
    """the four Philox words of samples 0..n-1"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    i = np.arange(n, dtype=np.uint64)
    return sampler_oracle.philox4x32_10((i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), 0, 0), (seed & 0xFFFFFFFF, seed >> 32))


@_quiet
def sample(vertices, triangles, n, seed=0, colors=None, want_normals=False):
    """-> dict(points (n,3), triangle (n,) int32, weights (n,3): (wa, wb, wc), colors (n,3) | None, normals (n,3) | absent)"""
    v = np.asarray(vertices, dtype=f32).reshape(-1, 3)
    _, cdf = weights(area2(v, triangles))
    W = int(cdf[-1]) if len(cdf) else 0
    if n and W == 0:
        raise ValueError("sample: the mesh has no area")
    w0, w1, w2, w3 = sample_words(seed, n)
    target = np.array([(((int(x) << 32) | int(y)) * W) >> 64 for x, y in zip(w0, w1)], dtype=np.int64)
    tri = np.searchsorted(cdf, target, side="right").astype(np.int32)       # the first t with cdf[t] > target
    r1 = ((w2 >> np.uint64(8)).astype(f32) * f32(2.0 ** -24)).astype(f32)
    r2 = ((w3 >> np.uint64(8)).astype(f32) * f32(2.0 ** -24)).astype(f32)
    s = np.sqrt(r1).astype(f32)
    wa, wb, wc = f32(1) - s, s * (f32(1) - r2), s * r2
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)[tri]

    def mix(x):
        x = np.asarray(x, dtype=f32)
        return ((wa[:, None] * x[t[:, 0]] + wb[:, None] * x[t[:, 1]]) + wc[:, None] * x[t[:, 2]]).astype(f32)

    out = dict(points=mix(v), triangle=tri, weights=np.stack([wa, wb, wc], 1), colors=None if colors is None else mix(colors))
    if want_normals:
        nrm, nn = normals(v[t[:, 0]], v[t[:, 1]], v[t[:, 2]])
        out["normals"] = (nrm / np.sqrt(nn.astype(f32)).astype(f32)[:, None]).astype(f32)
    return out


def reduce_d2(d2, threshold):
    """geometry.reduce_d2 in float64: (sum d2, sum sqrt(d2), finite entries, those with d2 <= fp32(threshold)^2)"""
    d = np.asarray(d2, dtype=f32)
    d = d[np.isfinite(d)].astype(np.float64)
    tau = float(f32(threshold))
    return float(d.sum()), float(np.sqrt(d).sum()), len(d), int((d <= tau * tau).sum())


def _mean(total, count):
    return total / count if count else float("nan")


def surface_metrics(pred, ref, threshold, n_samples=None, seed=0, max_d2=np.inf, nearest=None):
    """meshops.surface_metrics restated: pred / ref are (vertices, triangles) tuples or (N,3) clouds; `nearest(query, cloud) -> d2` is
    needed only where a cloud is on the `to` side"""
    def points_of(g):
        return sample(g[0], g[1], n_samples, seed)["points"] if isinstance(g, tuple) else np.asarray(g, dtype=f32)

    def distance(p, g):
        return mesh_distance(g[0], g[1], p, max_d2)["d2"] if isinstance(g, tuple) else nearest(p, g)

    pp, rp = points_of(pred), points_of(ref)
    s2p, s1p, mp, hp = reduce_d2(distance(pp, ref), threshold)
    s2r, s1r, mr, hr = reduce_d2(distance(rp, pred), threshold)
    n_pred, n_ref = int(np.isfinite(pp).all(1).sum()), int(np.isfinite(rp).all(1).sum())
    precision, recall = _mean(hp, n_pred), _mean(hr, n_ref)
    both = precision + recall
    fscore = 2.0 * precision * recall / both if both > 0 else (0.0 if both == 0 else float("nan"))
    return {"chamfer": _mean(s2p, mp) + _mean(s2r, mr), "accuracy": _mean(s1p, mp), "completeness": _mean(s1r, mr),
            "precision": precision, "recall": recall, "fscore": fscore, "n_pred": n_pred, "n_ref": n_ref}
