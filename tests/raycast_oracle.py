"""CPU restatement of csrc/mesh_ray.hip (include/sgam_hip.h, "Rays against a triangle mesh"): the intersection rule with its guard in
np.float32, one IEEE operation at a time and in the kernel's order, the (t bits, index) winner, the any-hit answer, the pinhole
rays, the visibility rule with its projection, a reference walk through the triangle grid (the kernel's steps, boxes and stop
rule, so the rule can be exercised without a GPU) and a float64 restatement of the plain intersection as the independent
reference.  Test infrastructure only — the product path never imports it."""
import numpy as np

import meshquery_oracle as Q

f32 = np.float32
INF, NAN = f32(np.inf), f32(np.nan)
F32_MAX = np.finfo(f32).max
_quiet = Q._quiet


def cross(u, v):
    """each component a difference of two products"""
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def guard_of(vertices, triangles):
    """meshops' guard: 2^-15 of the largest |coordinate| of the candidates' corners; None without a candidate"""
    a, b, c, _ = Q.corners(vertices, triangles)
    cand = Q.candidates(a, b, c)
    if not cand.any():
        return None
    return f32(max(np.abs(x[cand]).max() for x in (a, b, c))) * f32(2.0 ** -15)


def is_ray(rays):
    r = np.asarray(rays, dtype=f32).reshape(-1, 6)
    return np.isfinite(r).all(1) & (r[:, 3:] != 0).any(1)


@_quiet
def ray_triangle(a, b, c, o, d, tnear, tfar, guard):
    """the rule on (...,3) float32 arrays broadcast against each other -> (hit, t, u, v)"""
    a, b, c, o, d = np.broadcast_arrays(*(np.asarray(x, dtype=f32) for x in (a, b, c, o, d)))
    tnear, tfar, guard = f32(tnear), f32(tfar), f32(guard)
    e1, e2 = b - a, c - a
    p = cross(d, e2)
    det = Q.dot3(e1, p)
    s = o - a
    u = (Q.dot3(s, p) / det).astype(f32)
    q = cross(s, e1)
    v = (Q.dot3(d, q) / det).astype(f32)
    t = ((Q.dot3(e2, q) / det).astype(f32) + f32(0)).astype(f32)
    hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= tnear) & (t <= tfar)
    P = (o + t[..., None] * d).astype(f32)
    lo = np.minimum(np.minimum(a, b), c) - guard
    hi = np.maximum(np.maximum(a, b), c) + guard
    return hit & ((P >= lo) & (P <= hi)).all(-1), t, u, v


def _bits(t):
    return np.ascontiguousarray(t, dtype=f32).view(np.uint32).astype(np.int64)


@_quiet
def unit_normals(a, b, c):
    n, nn = Q.normals(a, b, c)
    return (n / np.sqrt(nn.astype(f32)).astype(f32)[..., None]).astype(f32)


@_quiet
def cast_rays(vertices, triangles, rays, tnear=0.0, tfar=np.inf, guard=None, chunk=256):
    """every ray against every candidate -> dict(t, triangle, uv, normal, hit (the any-hit answer), bad_index)"""
    r = np.asarray(rays, dtype=f32).reshape(-1, 6)
    a, b, c, ok = Q.corners(vertices, triangles)
    cand = np.flatnonzero(Q.candidates(a, b, c))
    n = len(r)
    out = dict(t=np.full(n, INF, f32), triangle=np.full(n, -1, np.int32), uv=np.full((n, 2), NAN, f32), normal=np.full((n, 3), NAN, f32),
               hit=np.zeros(n, bool), bad_index=bool((~ok).any()))
    if not len(cand) or not n:
        return out
    guard = guard_of(vertices, triangles) if guard is None else f32(guard)
    real = is_ray(r)
    for s in range(0, n, chunk):
        rs = r[s:s + chunk]
        hit, t, u, v = ray_triangle(a[cand][None], b[cand][None], c[cand][None], rs[:, None, :3], rs[:, None, 3:], tnear, tfar, guard)
        hit &= real[s:s + chunk, None]
        key = np.where(hit, (_bits(t) << 32) | cand[None], np.iinfo(np.int64).max)
        j = key.argmin(1)
        rows = np.arange(len(rs))
        won = hit[rows, j]
        w = cand[j]
        out["hit"][s:s + chunk] = won
        out["t"][s:s + chunk] = np.where(won, t[rows, j], INF)
        out["triangle"][s:s + chunk] = np.where(won, w, -1)
        out["uv"][s:s + chunk] = np.where(won[:, None], np.stack([u[rows, j], v[rows, j]], 1), NAN)
        out["normal"][s:s + chunk] = np.where(won[:, None], unit_normals(a[w], b[w], c[w]), NAN)
    return out


def cast_rays_f64(vertices, triangles, rays, tnear=0.0, tfar=np.inf):
    """the independent reference: plain two-sided Moeller-Trumbore in float64 on the fp32 inputs, no guard -> dict(t, triangle,
    edge (n,): the least of u, v, 1 - u - v of the winner — how far inside its triangle the hit lies)"""
    r = np.asarray(rays, dtype=f32).reshape(-1, 6).astype(np.float64)
    a, b, c, _ = Q.corners(vertices, triangles)
    cand = np.flatnonzero(Q.candidates(a, b, c))
    a, b, c = (x[cand].astype(np.float64) for x in (a, b, c))
    n = len(r)
    out = dict(t=np.full(n, np.inf), triangle=np.full(n, -1, np.int64), edge=np.full(n, np.nan))
    e1, e2 = (b - a)[None], (c - a)[None]
    with np.errstate(all="ignore"):
        for s in range(0, n, 256):
            o, d = r[s:s + 256, None, :3], r[s:s + 256, None, 3:]
            p = np.cross(d, e2)
            det = (e1 * p).sum(-1)
            sv = o - a[None]
            u = (sv * p).sum(-1) / det
            q = np.cross(sv, e1)
            v = (d * q).sum(-1) / det
            t = (e2 * q).sum(-1) / det
            hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= tnear) & (t <= tfar)
            tt = np.where(hit, t, np.inf)
            j = tt.argmin(1)
            rows = np.arange(len(j))
            won = hit[rows, j]
            out["t"][s:s + 256] = np.where(won, t[rows, j], np.inf)
            out["triangle"][s:s + 256] = np.where(won, cand[j], -1)
            out["edge"][s:s + 256] = np.where(won, np.minimum(np.minimum(u, v), 1 - u - v)[rows, j], np.nan)
    return out


# ---------------------------------------------------------------- pinhole rays and visibility
def _centre(M):
    """c_k = -((R[0][k] * T[0] + R[1][k] * T[1]) + R[2][k] * T[2]) of (P,4,4) float32 poses -> (P,3)"""
    return (-((M[:, 0, :3] * M[:, 0, 3:4] + M[:, 1, :3] * M[:, 1, 3:4]) + M[:, 2, :3] * M[:, 2, 3:4])).astype(f32)


@_quiet
def rays_pinhole(poses_w2c, fx, fy, cx, cy, H, W):
    M = np.asarray(poses_w2c, dtype=f32).reshape(-1, 4, 4)
    fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
    i, j = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
    a, b = ((j - cx) / fx).astype(f32)[None, ..., None], ((i - cy) / fy).astype(f32)[None, ..., None]
    d = ((M[:, None, None, 0, :3] * a + M[:, None, None, 1, :3] * b) + M[:, None, None, 2, :3]).astype(f32)
    o = np.broadcast_to(_centre(M)[:, None, None], d.shape)
    return np.concatenate([o, d], -1).astype(f32)


@_quiet
def visibility_rays(points, poses_w2c, fx, fy, cx, cy, H, W, z_near, z_far):
    """-> (rays (P,N,6) from each camera centre to each point, in_frustum (P,N))"""
    x = np.asarray(points, dtype=f32).reshape(-1, 3)
    M = np.asarray(poses_w2c, dtype=f32).reshape(-1, 4, 4)
    fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
    X = [(((M[:, r, 0:1] * x[None, :, 0] + M[:, r, 1:2] * x[None, :, 1]) + M[:, r, 2:3] * x[None, :, 2]) + M[:, r, 3:4]).astype(f32) for r in range(3)]
    u = ((fx * X[0]) / X[2] + cx).astype(f32)
    v = ((fy * X[1]) / X[2] + cy).astype(f32)
    uf, vf = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
    inside = (f32(z_near) <= X[2]) & (X[2] <= f32(z_far)) & (uf >= 0) & (uf < f32(W)) & (vf >= 0) & (vf < f32(H))
    c = _centre(M)[:, None]
    d = (x[None] - c).astype(f32)
    return np.concatenate([np.broadcast_to(c, d.shape), d], -1).astype(f32), inside


def visibility(points, vertices, triangles, poses_w2c, fx, fy, cx, cy, H, W, z_near, z_far, tolerance=1e-3, guard=None):
    """-> count (N,) int32: the poses that see each point"""
    rays, inside = visibility_rays(points, poses_w2c, fx, fy, cx, cy, H, W, z_near, z_far)
    tfar = f32(1) - f32(tolerance)
    hit = cast_rays(vertices, triangles, rays.reshape(-1, 6), 0.0, tfar, guard)["hit"].reshape(inside.shape)
    return (inside & is_ray(rays.reshape(-1, 6)).reshape(inside.shape) & ~hit).sum(0).astype(np.int32)


# ---------------------------------------------------------------- the reference walk through the triangle grid
@_quiet
def cell_of(p, o, h, g):
    t = np.floor(((f32(p) - f32(o)) / f32(h)).astype(f32))
    return int(min(max(t, f32(0)), f32(g - 1)))


def margin_of(origin, h, dims):
    """make_grid's margin with MESH_MARGIN = 2^-14: float64, rounded to fp32 once"""
    o = np.asarray(origin, dtype=f32).astype(np.float64)
    far = o + np.asarray(dims, dtype=np.float64) * float(f32(h))
    corner = max(np.abs(o).max(), np.abs(far).max())
    edge = (np.asarray(dims, dtype=np.float64) * float(f32(h))).max()
    return f32((corner + edge) / 16384.0)


class Grid:
    """sgam_mesh_grid_build restated: every candidate into every cell of the block [cell(min), cell(max)] of its bounding box"""

    def __init__(self, vertices, triangles, origin, h, dims):
        self.origin, self.h, self.dims = np.asarray(origin, dtype=f32), f32(h), tuple(int(g) for g in dims)
        self.margin = margin_of(origin, h, dims)
        self.a, self.b, self.c, _ = Q.corners(vertices, triangles)
        self.cells = {}
        for t in np.flatnonzero(Q.candidates(self.a, self.b, self.c)):
            tri = np.stack([self.a[t], self.b[t], self.c[t]])
            lo = [cell_of(tri[:, k].min(), self.origin[k], self.h, self.dims[k]) for k in range(3)]
            hi = [cell_of(tri[:, k].max(), self.origin[k], self.h, self.dims[k]) for k in range(3)]
            for z in range(lo[2], hi[2] + 1):
                for y in range(lo[1], hi[1] + 1):
                    for x in range(lo[0], hi[0] + 1):
                        self.cells.setdefault((x, y, z), []).append(int(t))


def grid_for(vertices, triangles, h):
    """geometry.grid_for over the box of the candidates' vertices (origin = its minimum corner, g = floor(extent / h) + 1)"""
    a, b, c, _ = Q.corners(vertices, triangles)
    cand = Q.candidates(a, b, c)
    pts = np.concatenate([a[cand], b[cand], c[cand]])
    lo, hi = pts.min(0).astype(f32), pts.max(0).astype(f32)
    h = float(f32(h))
    dims = tuple(int(v) for v in np.floor((hi.astype(np.float64) - lo.astype(np.float64)) / h) + 1.0)
    return Grid(vertices, triangles, lo, h, dims)


@_quiet
def _along(o, d, t):
    return f32(f32(o) + f32(f32(t) * f32(d)))


@_quiet
def walk(G, ray, tnear=0.0, tfar=np.inf, guard=0.0, any_hit=False):
    """the kernel's walk for ONE ray -> (t, triangle, hit, cells visited, steps); (+inf, -1, False) without a hit"""
    r = np.asarray(ray, dtype=f32)
    tnear, tfar, guard = f32(tnear), f32(tfar), f32(guard)
    best, bi, visited, steps = INF, -1, [], 0
    if not is_ray(r)[0]:
        return best, bi, False, visited, steps
    o, d = r[:3], r[3:]
    ad = np.abs(d)
    m = 0 if (ad[0] >= ad[1] and ad[0] >= ad[2]) else (1 if ad[1] >= ad[2] else 2)
    W = G.margin
    W2, W3 = f32(f32(2) * W), f32(f32(3) * W)
    lo = [f32(G.origin[k] - W2) for k in range(3)]
    hi = [f32(f32(G.origin[k] + f32(f32(G.dims[k]) * G.h)) + W2) for k in range(3)]
    om, dm, Om, gm = o[m], d[m], G.origin[m], G.dims[m]
    fwd = dm > 0
    tend = min(tfar, F32_MAX)
    ta = tnear
    tc = f32(f32((f32(lo[m] - W2) if fwd else f32(hi[m] + W2)) - om) / dm)
    pm = _along(om, dm, tc)
    if tc > ta and (pm < lo[m] if fwd else pm > hi[m]):
        ta = tc
    if not ta <= tend:
        return best, bi, False, visited, steps
    k = cell_of(_along(om, dm, ta), Om, G.h, gm)
    prev = None

    def offer(cell):
        nonlocal best, bi
        visited.append(cell)
        for t_id in G.cells.get(cell, ()):
            hit, t, _, _ = ray_triangle(G.a[t_id], G.b[t_id], G.c[t_id], o, d, tnear, tfar, guard)
            if hit and (t < best or (t == best and t_id < bi)):
                best, bi = f32(t), t_id
            if any_hit and bi >= 0:
                return True
        return False

    for steps in range(1, gm + 2):
        last = k >= gm - 1 if fwd else k <= 0
        if not last:
            plane = f32(Om + f32(f32(k + 1 if fwd else k) * G.h))
            tb = f32(f32((f32(plane + W3) if fwd else f32(plane - W3)) - om) / dm)
        else:
            tb = f32(f32((f32(hi[m] + W2) if fwd else f32(lo[m] - W2)) - om) / dm)
        tb = min(max(tb, ta), tend)
        if last and tb < tend:
            pm = _along(om, dm, tb)
            if not (pm > hi[m] if fwd else pm < lo[m]):
                tb = tend
        p0 = [_along(o[j], d[j], ta) for j in range(3)]
        p1 = [_along(o[j], d[j], tb) for j in range(3)]
        mn, mx = [min(p0[j], p1[j]) for j in range(3)], [max(p0[j], p1[j]) for j in range(3)]
        if not any(mx[j] < lo[j] or mn[j] > hi[j] for j in range(3)):
            c0 = [cell_of(f32(mn[j] - W), G.origin[j], G.h, G.dims[j]) for j in range(3)]
            c1 = [cell_of(f32(mx[j] + W), G.origin[j], G.h, G.dims[j]) for j in range(3)]
            for z in range(c0[2], c1[2] + 1):
                for y in range(c0[1], c1[1] + 1):
                    for x in range(c0[0], c1[0] + 1):
                        if prev and all(prev[0][j] <= (x, y, z)[j] <= prev[1][j] for j in range(3)):
                            continue
                        if offer((x, y, z)):
                            return best, bi, True, visited, steps
            prev = (c0, c1)
        if (bi >= 0 if any_hit else best <= tb) or tb >= tend or last:
            break
        ta = tb
        k += 1 if fwd else -1
    return best, bi, bi >= 0, visited, steps
