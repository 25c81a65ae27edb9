"""numpy restatement of the mesh clean-up kernels (csrc/mesh_ops.hip, sgam_points_voxel_assign_f32 of csrc/point_cloud.hip) for tests:
connected components by min-label propagation, selection, incidence as CSR, vertex normals and the Taubin step in float64 with the
summation order spelled out (ascending CSR entries), vertex clustering with the fp32 voxel arithmetic of cloud_oracle.voxel_sample
and the triangle de-duplication by sorting.  A mesh is (vertices (nv,3) fp32, triangles (nt,3) int32[, colours (nv,3) fp32]);
nothing here imports the package."""
import numpy as np

f32 = np.float32


def _tris(triangles):
    return np.asarray(triangles, dtype=np.int64).reshape(-1, 3)


def components(triangles, nv):
    """-> dict(vertex_label (nv,) int32: the least vertex index of the vertex's component, triangle_label (nt,) int32: corner 0's,
    labels (C,) int32 ascending: the components with a triangle, n_triangles (C,) int32)"""
    t = _tris(triangles)
    lab = np.arange(nv, dtype=np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    while len(e):
        m = np.minimum(lab[e[:, 0]], lab[e[:, 1]])
        new = lab.copy()
        np.minimum.at(new, e[:, 0], m)
        np.minimum.at(new, e[:, 1], m)
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    tl = lab[t[:, 0]] if len(t) else np.zeros(0, np.int64)
    labels, counts = np.unique(tl, return_counts=True)
    return dict(vertex_label=lab.astype(np.int32), triangle_label=tl.astype(np.int32), labels=labels.astype(np.int32),
                n_triangles=counts.astype(np.int32))


def select_triangles(vertices, triangles, keep, colors=None):
    """-> dict(vertices, triangles, colors or None, vertex_index (new -> old) int32): kept triangles and the vertices they use, in order"""
    v, t = np.asarray(vertices, dtype=f32).reshape(-1, 3), _tris(triangles)
    keep = np.asarray(keep, dtype=bool).reshape(-1)
    kt = t[keep]
    used = np.zeros(len(v), dtype=bool)
    used[kt.reshape(-1)] = True
    index = np.flatnonzero(used)
    new = np.cumsum(used) - 1
    return dict(vertices=v[index], triangles=new[kt].astype(np.int32).reshape(-1, 3),
                colors=None if colors is None else np.asarray(colors, dtype=f32).reshape(-1, 3)[index], vertex_index=index.astype(np.int32))


def kept_components(comp, min_triangles=None, keep_largest=None):
    """the labels remove_small_components keeps: n_triangles >= min_triangles, and among the keep_largest largest (ties: lower label)"""
    labels, n = comp["labels"], comp["n_triangles"]
    ok = np.ones(len(labels), dtype=bool)
    if min_triangles is not None:
        ok &= n >= min_triangles
    if keep_largest is not None:
        order = np.lexsort((labels, -n.astype(np.int64)))[:max(int(keep_largest), 0)]
        top = np.zeros(len(labels), dtype=bool)
        top[order] = True
        ok &= top
    return labels[ok]


def remove_small_components(vertices, triangles, colors=None, min_triangles=None, keep_largest=None):
    comp = components(triangles, len(vertices))
    keep = np.isin(comp["triangle_label"], kept_components(comp, min_triangles, keep_largest))
    return select_triangles(vertices, triangles, keep, colors)


def incidence(triangles, nv, kind):
    """-> (offsets (nv+1,) int32, items int32): kind "triangles": the triangles using each vertex, ascending, each once; "vertices":
    the distinct other vertices sharing a triangle with it, ascending"""
    t = _tris(triangles)
    tid = np.arange(len(t), dtype=np.int64)
    if kind == "triangles":
        pairs = np.concatenate([np.stack([t[:, k], tid], 1) for k in range(3)])
    elif kind == "vertices":
        pairs = np.concatenate([np.stack([t[:, a], t[:, b]], 1) for a in range(3) for b in range(3) if a != b])
        pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    else:
        raise ValueError(f"kind 'triangles' or 'vertices', not {kind!r}")
    pairs = np.unique(pairs, axis=0) if len(pairs) else pairs.reshape(0, 2)          # sorted by (vertex, item), each once
    offsets = np.zeros(nv + 1, dtype=np.int64)
    np.add.at(offsets, pairs[:, 0] + 1, 1)
    return np.cumsum(offsets).astype(np.int32), pairs[:, 1].astype(np.int32)


def _by_rank(offsets):
    """for r = 0, 1, ...: (the vertices with more than r entries, the position of their r-th entry)"""
    offsets = np.asarray(offsets, dtype=np.int64)
    deg = np.diff(offsets)
    for r in range(int(deg.max()) if len(deg) else 0):
        who = np.flatnonzero(deg > r)
        yield who, offsets[who] + r


def vertex_normals(vertices, triangles):
    """(nv,3) fp32: per vertex the float64 sum, in ascending triangle id, of (v1 - v0) x (v2 - v0) of its triangles (from the fp32
    positions, differences of products), divided by sqrt((x * x + y * y) + z * z); a zero sum: zero; rounded to fp32 once"""
    v, t = np.asarray(vertices, dtype=f32).reshape(-1, 3).astype(np.float64), _tris(triangles)
    u, w = v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
    fn = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    offsets, items = incidence(t, len(v), "triangles")
    s = np.zeros_like(v)
    for who, at in _by_rank(offsets):
        s[who] = s[who] + fn[items[at]]
    ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    with np.errstate(all="ignore"):
        n = np.where(ln[:, None] > 0, s / ln[:, None], 0.0)
    return n.astype(f32)


def smooth_step(vertices, offsets, items, weight):
    """one step: p' = fp32(p + w (s / m - p)) in float64, s = the sum of the m neighbours in ascending index; m = 0: p stays"""
    p32 = np.asarray(vertices, dtype=f32).reshape(-1, 3)
    p = p32.astype(np.float64)
    s = np.zeros_like(p)
    for who, at in _by_rank(offsets):
        s[who] = s[who] + p[items[at]]
    m = np.diff(np.asarray(offsets, dtype=np.int64)).astype(np.float64)
    with np.errstate(all="ignore"):
        new = p + float(weight) * (s / m[:, None] - p)
    return np.where(m[:, None] > 0, new.astype(f32), p32)


def smooth_taubin(vertices, triangles, iterations=10, lambda_filter=0.5, mu=-0.53):
    v = np.asarray(vertices, dtype=f32).reshape(-1, 3).copy()
    offsets, items = incidence(triangles, len(v), "vertices")
    for _ in range(int(iterations)):
        v = smooth_step(v, offsets, items, lambda_filter)
        v = smooth_step(v, offsets, items, mu)
    return v


def voxel_assign(points, voxel_size, origin=None):
    """rep (N,) int32: the index of the kept point of each point's voxel under cloud_oracle.voxel_sample's rule (-1: not a point).
    Per axis in fp32: v = floor((p - o) / voxel), c = o + (v + 0.5) * voxel; kept: the member of least (d2(p, c) bits, index)"""
    p = np.asarray(points, dtype=f32).reshape(-1, 3)
    ok = np.isfinite(p).all(axis=1)
    rep = np.full(len(p), -1, dtype=np.int32)
    if not ok.any():
        return rep
    o = p[ok].min(axis=0) if origin is None else np.asarray(origin, dtype=f32).reshape(3)
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
    order = np.lexsort((ids, d2.view(np.uint32), voxel))
    first = np.r_[True, voxel[order][1:] != voxel[order][:-1]]
    winner = np.zeros(voxel.max() + 1, dtype=np.int64)
    winner[voxel[order[first]]] = ids[order[first]]
    rep[ids] = winner[voxel]
    return rep


def simplify_vertex_clustering(vertices, triangles, voxel_size, colors=None, origin=None):
    """-> dict(vertices, triangles, colors or None, vertex_index (new -> old) int32).  New vertices: the representatives, in ascending
    old index.  A triangle with two corners in one cluster (or a corner in none) is dropped; of the triangles with the same new
    triple after rotating the least index to the front (orientation kept) the one with the lowest old index survives; survivors stay
    in old order with their corners in the old order"""
    v, t = np.asarray(vertices, dtype=f32).reshape(-1, 3), _tris(triangles)
    rep = voxel_assign(v, voxel_size, origin)
    is_rep = rep == np.arange(len(v))
    index = np.flatnonzero(is_rep)
    new = np.cumsum(is_rep) - 1
    cluster = np.where(rep >= 0, new[np.maximum(rep, 0)], -1)
    nt = cluster[t]
    live = (nt >= 0).all(axis=1) & (nt[:, 0] != nt[:, 1]) & (nt[:, 1] != nt[:, 2]) & (nt[:, 0] != nt[:, 2])
    keep = np.zeros(len(t), dtype=bool)
    if live.any():
        ids = np.flatnonzero(live)
        c = nt[ids]
        shift = np.argmin(c, axis=1)
        rot = np.stack([c[np.arange(len(c)), (shift + k) % 3] for k in range(3)], 1)
        _, first = np.unique(rot, axis=0, return_index=True)                  # the first occurrence: the lowest old index
        keep[ids[first]] = True
    return dict(vertices=v[index], triangles=nt[keep].astype(np.int32).reshape(-1, 3),
                colors=None if colors is None else np.asarray(colors, dtype=f32).reshape(-1, 3)[index], vertex_index=index.astype(np.int32))


def clean(vertices, triangles, colors=None, min_triangles=None, keep_largest=None, smooth_iterations=0, voxel_size=None, normals=True):
    """rules 3 -> 6 -> 7 -> 5: dict(vertices, triangles, colors, vertex_index into the input, vertex_normals or None)"""
    v, t = np.asarray(vertices, dtype=f32).reshape(-1, 3), _tris(triangles).astype(np.int32)
    c = None if colors is None else np.asarray(colors, dtype=f32).reshape(-1, 3)
    index = np.arange(len(v), dtype=np.int32)
    if (min_triangles is not None or keep_largest is not None) and len(t):
        m = remove_small_components(v, t, c, min_triangles, keep_largest)
        v, t, c, index = m["vertices"], m["triangles"], m["colors"], index[m["vertex_index"]]
    if smooth_iterations and len(t):
        v = smooth_taubin(v, t, smooth_iterations)
    if voxel_size is not None and len(v):
        m = simplify_vertex_clustering(v, t, voxel_size, c)
        v, t, c, index = m["vertices"], m["triangles"], m["colors"], index[m["vertex_index"]]
    return dict(vertices=v, triangles=t, colors=c, vertex_index=index, vertex_normals=vertex_normals(v, t) if normals else None)
