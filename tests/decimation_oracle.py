"""numpy restatement of quadric-error decimation (csrc/mesh_simplify.hip, meshops.simplify_quadric_decimation; the rules 1 to 8 of
include/sgam_hip.h) for tests: float64 from the widened fp32 inputs in the kernels' operation order, sums over a
CSR segment rank by rank, minima and counts by whatever numpy offers (their result has no order).  A mesh is (vertices (nv,3)
fp32, triangles (nt,3) int32[, colours (nv,3) fp32]) whose triangles name vertices of the mesh; nothing here imports the package."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import meshops_oracle as MO  # noqa: E402

f32 = np.float32
F32_MAX = f32(3.4028234663852886e38)
PRIORITY_NONE = np.uint32(0xFFFFFFFF)
_M32 = np.uint64(0xFFFFFFFF)


def edge_priority(e):
    """the 32-bit bijection of the edge id: x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (mod 2^32)"""
    x = np.asarray(e).astype(np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & _M32
    return (x ^ (x >> np.uint64(16))).astype(np.uint32)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)


def plane_quadric(p, d, w):
    """(n,10): w [p; d][p; d]^T, entry (i, j) = (w * p_i) * p_j, in the order xx xy xz xw yy yz yw zz zw ww"""
    wx, wy, wz, wd = w * p[:, 0], w * p[:, 1], w * p[:, 2], w * d
    return np.stack([wx * p[:, 0], wx * p[:, 1], wx * p[:, 2], wx * d, wy * p[:, 1], wy * p[:, 2], wy * d, wz * p[:, 2], wz * d, wd * d], 1)


def _unit(m):
    """(unit vector, length, usable): usable where the length is positive and finite"""
    with np.errstate(all="ignore"):
        ln = np.sqrt(dot(m, m))
        ok = (ln > 0) & np.isfinite(ln)
        return m / ln[:, None], ln, ok


def _expand(offsets, owners):
    """every entry of the segments of `owners`: (the position in `owners` it belongs to, its position in the items)"""
    offsets = np.asarray(offsets, dtype=np.int64)
    owners = np.asarray(owners, dtype=np.int64)
    n = offsets[owners + 1] - offsets[owners]
    rep = np.repeat(np.arange(len(owners)), n)
    start = np.cumsum(n) - n
    return rep, offsets[owners][rep] + (np.arange(int(n.sum())) - start[rep])


class Shared:
    """shared(a, b): the number of triangles that name both a and b (a != b), a triangle counting once"""

    def __init__(self, t, nv):
        self.nv = nv
        tid = np.arange(len(t), dtype=np.int64)
        rows = np.concatenate([np.stack([tid, np.minimum(t[:, a], t[:, b]), np.maximum(t[:, a], t[:, b])], 1) for a, b in ((0, 1), (1, 2), (0, 2))])
        rows = np.unique(rows[rows[:, 1] != rows[:, 2]], axis=0) if len(rows) else rows.reshape(0, 3)
        self.keys, self.counts = np.unique(rows[:, 1] * nv + rows[:, 2], return_counts=True)

    def __call__(self, a, b):
        a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
        key = np.minimum(a, b) * self.nv + np.maximum(a, b)
        if len(self.keys) == 0:
            return np.zeros(key.shape, dtype=np.int64)
        at = np.minimum(np.searchsorted(self.keys, key), len(self.keys) - 1)
        return np.where(self.keys[at] == key, self.counts[at], 0)


# ---------------------------------------------------------------- rule 1
def vertex_quadrics(vertices, triangles, boundary_weight=1.0):
    """(nv,10) float64.  Per vertex, over its triangles in ascending id: first the plane of every triangle with area (unit normal n
    of (b - a) x (c - a), d = -n.a, weight A = half the cross product's length); then, again in ascending id and per triangle for
    k = 0, 1, 2, the plane through the edge (corner k, corner k + 1) when the vertex is an end of it and exactly one triangle names
    both ends: unit normal of (p[k + 1] - p[k]) x n, d = -u.p[k], weight boundary_weight * A"""
    v, t = np.asarray(vertices, dtype=f32).reshape(-1, 3).astype(np.float64), MO._tris(triangles)
    nv = len(v)
    Q = np.zeros((nv, 10))
    if len(t) == 0:
        return Q
    p = [v[t[:, k]] for k in range(3)]
    n, ln, ok = _unit(cross(p[1] - p[0], p[2] - p[0]))
    area = 0.5 * ln
    with np.errstate(all="ignore"):
        K = plane_quadric(n, -dot(n, p[0]), area)
    shared = Shared(t, nv)
    offsets, items = MO.incidence(t, nv, "triangles")
    for who, at in MO._by_rank(offsets):
        tt = items[at]
        m = ok[tt]
        Q[who[m]] = Q[who[m]] + K[tt[m]]
    for who, at in MO._by_rank(offsets):
        tt = items[at]
        for k in range(3):
            frm, to = t[tt, k], t[tt, (k + 1) % 3]
            m = ok[tt] & (frm != to) & ((frm == who) | (to == who))
            m &= shared(who, np.where(frm == who, to, frm)) == 1
            u, _, uok = _unit(cross(p[(k + 1) % 3][tt] - p[k][tt], n[tt]))
            m &= uok
            with np.errstate(all="ignore"):
                B = plane_quadric(u, -dot(u, p[k][tt]), float(boundary_weight) * area[tt])
            Q[who[m]] = Q[who[m]] + B[m]
    return Q


# ---------------------------------------------------------------- rule 2
def edges_of(triangles, nv):
    """(edges (ne,2) int32 ascending (lo, hi), offsets, items of the "vertices" CSR, edge_of_entry (n_items,) int32: the id of the
    edge at an entry whose item is above its owner, -1 elsewhere)"""
    offsets, items = MO.incidence(triangles, nv, "vertices")
    owner = np.repeat(np.arange(nv, dtype=np.int64), np.diff(offsets.astype(np.int64)))
    up = items > owner
    edge_of_entry = np.where(up, np.cumsum(up) - 1, -1).astype(np.int32)
    return np.stack([owner[up], items[up]], 1).astype(np.int32).reshape(-1, 2), offsets, items, edge_of_entry


# ---------------------------------------------------------------- rules 3 and 4
def quadric_value(Q, p):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    sq = (x * (Q[:, 0] * x) + y * (Q[:, 4] * y)) + z * (Q[:, 7] * z)
    mixed = (x * (Q[:, 1] * y) + x * (Q[:, 2] * z)) + y * (Q[:, 5] * z)
    lin = (Q[:, 3] * x + Q[:, 6] * y) + Q[:, 8] * z
    return (sq + 2.0 * mixed) + (2.0 * lin + Q[:, 9])


def clamped_cost(Q, p):
    c = quadric_value(Q, p)
    return np.where(c > 0, c, np.where(c <= 0, 0.0, c))


def contraction_target(Q, lo, hi):
    """(target (n,3), cost (n,)) of edges with Q = Q_lo + Q_hi and end positions lo, hi (float64)"""
    with np.errstate(all="ignore"):
        mid = (lo + hi) * 0.5
        c00, c01, c02 = Q[:, 4] * Q[:, 7] - Q[:, 5] * Q[:, 5], Q[:, 1] * Q[:, 7] - Q[:, 5] * Q[:, 2], Q[:, 1] * Q[:, 5] - Q[:, 4] * Q[:, 2]
        det = (Q[:, 0] * c00 - Q[:, 1] * c01) + Q[:, 2] * c02
        tr3 = ((Q[:, 0] + Q[:, 4]) + Q[:, 7]) / 3.0
        regular = np.abs(det) > 1e-8 * ((tr3 * tr3) * tr3)
        r0, r1, r2 = -Q[:, 3], -Q[:, 6], -Q[:, 8]
        dx = (r0 * c00 - Q[:, 1] * (r1 * Q[:, 7] - Q[:, 5] * r2)) + Q[:, 2] * (r1 * Q[:, 5] - Q[:, 4] * r2)
        dy = (Q[:, 0] * (r1 * Q[:, 7] - r2 * Q[:, 5]) - r0 * c01) + Q[:, 2] * (Q[:, 1] * r2 - r1 * Q[:, 2])
        dz = (Q[:, 0] * (Q[:, 4] * r2 - Q[:, 5] * r1) - Q[:, 1] * (Q[:, 1] * r2 - Q[:, 2] * r1)) + r0 * c02
        s = np.stack([dx / det, dy / det, dz / det], 1)
        off, edge = s - mid, hi - lo
        solved = regular & (dot(off, off) <= 4.0 * dot(edge, edge))
        cl, ch, cm = clamped_cost(Q, lo), clamped_cost(Q, hi), clamped_cost(Q, mid)
        take_lo = (cl <= ch) & (cl <= cm)
        take_hi = ~take_lo & (ch <= cm)
        target = np.where(take_lo[:, None], lo, np.where(take_hi[:, None], hi, mid))
        cost = np.where(take_lo, cl, np.where(take_hi, ch, cm))
        return np.where(solved[:, None], s, target), np.where(solved, clamped_cost(Q, s), cost)


def evaluate(vertices, colors, triangles, Q, edges):
    """-> dict(cost (ne,) fp32: +inf for an edge that is not legal, removed (ne,) int32, position (ne,3) fp32, color (ne,3) fp32 or
    None)"""
    v32, t = np.asarray(vertices, dtype=f32).reshape(-1, 3), MO._tris(triangles)
    v, nv, ne = v32.astype(np.float64), len(v32), len(edges)
    lo, hi = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    target, cost = contraction_target(Q[lo] + Q[hi], v[lo], v[hi])
    position = target.astype(f32)
    color = None
    if colors is not None:
        c = np.asarray(colors, dtype=f32).reshape(-1, 3).astype(np.float64)
        with np.errstate(all="ignore"):
            edge = v[hi] - v[lo]
            l2 = dot(edge, edge)
            w = np.where(l2 > 0, dot(target - v[lo], edge) / l2, 0.0)
            w = np.where(w >= 0, np.where(w <= 1, w, 1.0), 0.0)[:, None]
            color = ((1.0 - w) * c[lo] + w * c[hi]).astype(f32)
    shared = Shared(t, nv)
    removed = shared(lo, hi)
    # link, the vertices
    voff, vitems = MO.incidence(t, nv, "vertices")
    owner = np.repeat(np.arange(nv, dtype=np.int64), np.diff(voff.astype(np.int64)))
    adjacent = owner * nv + vitems                                          # ascending
    rep, at = _expand(voff, lo)
    x = vitems[at].astype(np.int64)
    key = hi[rep] * nv + x
    pos = np.minimum(np.searchsorted(adjacent, key), max(len(adjacent) - 1, 0))
    common = np.zeros(ne, dtype=np.int64)
    np.add.at(common, rep, adjacent[pos] == key)
    with np.errstate(all="ignore"):
        cost32 = cost.astype(f32)
    legal = (removed > 0) & (common == removed) & (cost32 <= F32_MAX)
    # link, the border: an edge with more than one triangle does not join two ends of edges with exactly one
    single = shared.keys[shared.counts == 1]
    border = np.zeros(nv, dtype=bool)
    border[single // nv] = True
    border[single % nv] = True
    legal &= ~((removed != 1) & border[lo] & border[hi])
    # link, the edges; and the flip test from either side
    toff, titems = MO.incidence(t, nv, "triangles")
    triples = np.sort(t, axis=1)
    known = np.unique((triples[:, 0] * nv + triples[:, 1]) * nv + triples[:, 2])
    assert nv < 2 ** 20
    moved = position.astype(np.float64)
    for end, other in ((lo, hi), (hi, lo)):
        rep, at = _expand(toff, end)
        tt = t[titems[at]]
        free = ~(tt == other[rep][:, None]).any(axis=1)
        rep, tt = rep[free], tt[free]
        if end is lo:
            swapped = np.sort(np.where(tt == lo[rep][:, None], hi[rep][:, None], tt), axis=1)
            k = (swapped[:, 0] * nv + swapped[:, 1]) * nv + swapped[:, 2]
            pos = np.minimum(np.searchsorted(known, k), len(known) - 1)
            np.logical_and.at(legal, rep, known[pos] != k)
        before = cross(v[tt[:, 1]] - v[tt[:, 0]], v[tt[:, 2]] - v[tt[:, 0]])
        q = [np.where((tt[:, c] == end[rep])[:, None], moved[rep], v[tt[:, c]]) for c in range(3)]
        with np.errstate(all="ignore"):
            after = cross(q[1] - q[0], q[2] - q[0])
            np.logical_and.at(legal, rep, dot(before, after) > 0)
    return dict(cost=np.where(legal, cost32, f32(np.inf)).astype(f32), removed=removed.astype(np.int32), position=position, color=color)


# ---------------------------------------------------------------- rules 5 to 7
def threshold(cost, nt, target, oversample, max_error):
    """tau (fp32) of rule 5, None without a legal edge: the ceil(oversample * need)-th smallest legal cost, need = ceil((nt -
    target) / 2), capped by the largest fp32 <= max_error"""
    legal = np.sort(cost[cost <= F32_MAX])
    if len(legal) == 0:
        return None
    need = (nt - target + 1) // 2
    tau = legal[min(max(int(math.ceil(float(oversample) * need)), 1), len(legal)) - 1]
    return min(tau, f32_at_most(max_error))


def f32_at_most(x):
    """the largest fp32 <= x (x >= 0, +inf: the largest finite one)"""
    with np.errstate(over="ignore"):
        c = f32(min(float(x), float(F32_MAX)))
    return c if float(c) <= float(x) else np.nextafter(c, f32(-np.inf))


def select(nv, offsets, items, edges, cost, tau):
    """(ne,) bool: rule 6"""
    ne = len(edges)
    lo, hi = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    cand = cost <= tau
    prio = edge_priority(np.arange(ne))
    p1 = np.full(nv, PRIORITY_NONE, dtype=np.uint32)
    np.minimum.at(p1, lo[cand], prio[cand])
    np.minimum.at(p1, hi[cand], prio[cand])
    p2 = p1.copy()
    owner = np.repeat(np.arange(nv, dtype=np.int64), np.diff(np.asarray(offsets, dtype=np.int64)))
    np.minimum.at(p2, owner, p1[items])
    return cand & (prio == p2[lo]) & (prio == p2[hi])


def budget(selected, cost, removed, nt, target):
    """the ids of the edges to apply, ascending: every selected one, or — when that would take nt below target — those of the prefix
    in ascending (cost bits, priority) before which the running triangle count is still > target"""
    ids = np.flatnonzero(selected)
    if nt - int(removed[ids].sum()) >= target:
        return ids
    order = ids[np.lexsort((edge_priority(ids), cost[ids].view(np.uint32)))]
    before = nt - (np.cumsum(removed[order]) - removed[order])
    return np.sort(order[before > target])


# ---------------------------------------------------------------- the rounds
def decimate(vertices, triangles, colors=None, target_triangles=None, target_ratio=None, max_error=math.inf, boundary_weight=1.0,
             oversample=2.0, max_rounds=256, trace=None):
    """-> dict(vertices, triangles, colors or None, vertex_index (new -> the input vertex its slot descends from) int32, rounds,
    max_cost, stopped).  trace: a list that receives, per round, dict(edges, selected (ids), chosen (ids), offsets, items)"""
    v = np.asarray(vertices, dtype=f32).reshape(-1, 3).copy()
    t = MO._tris(triangles).astype(np.int32)
    c = None if colors is None else np.asarray(colors, dtype=f32).reshape(-1, 3).copy()
    target = int(target_triangles) if target_triangles is not None else int(math.floor(float(target_ratio) * len(t)))
    index = np.arange(len(v), dtype=np.int32)
    rounds, max_cost = 0, 0.0
    if len(t) <= target:
        return dict(vertices=v, triangles=t, colors=c, vertex_index=index, rounds=0, max_cost=0.0, stopped="target")
    Q = vertex_quadrics(v, t, boundary_weight)
    while True:
        nv, nt = len(v), len(t)
        if nt <= target:
            stopped = "target"
            break
        if rounds == max_rounds:
            stopped = "max_rounds"
            break
        edges, offsets, items, _ = edges_of(t, nv)
        if len(edges) == 0:
            stopped = "no_candidates"
            break
        ev = evaluate(v, c, t, Q, edges)
        tau = threshold(ev["cost"], nt, target, oversample, max_error)
        selected = None if tau is None else select(nv, offsets, items, edges, ev["cost"], tau)
        if selected is None or not selected.any():
            stopped = "no_candidates"
            break
        chosen = budget(selected, ev["cost"], ev["removed"].astype(np.int64), nt, target)
        if trace is not None:
            trace.append(dict(edges=edges, selected=np.flatnonzero(selected), chosen=chosen, offsets=offsets, items=items))
        rounds += 1
        max_cost = max(max_cost, float(ev["cost"][chosen].max()))
        lo, hi = edges[chosen, 0].astype(np.int64), edges[chosen, 1].astype(np.int64)
        v[lo] = ev["position"][chosen]
        if c is not None:
            c[lo] = ev["color"][chosen]
        Q[lo] = Q[lo] + Q[hi]
        vkeep, merge = np.ones(nv, dtype=bool), np.arange(nv, dtype=np.int64)
        vkeep[hi], merge[hi] = False, lo
        tkeep = np.ones(nt, dtype=bool)
        toff, titems = MO.incidence(t, nv, "triangles")
        rep, at = _expand(toff, lo)
        tkeep[titems[at][(t[titems[at]] == hi[rep][:, None]).any(axis=1)]] = False
        vmap = (np.cumsum(vkeep) - 1)[merge]
        t = vmap[t[tkeep]].astype(np.int32).reshape(-1, 3)
        v, Q, index = v[vkeep], Q[vkeep], index[vkeep]
        c = None if c is None else c[vkeep]
    return dict(vertices=v, triangles=t, colors=c, vertex_index=index, rounds=rounds, max_cost=max_cost, stopped=stopped)
