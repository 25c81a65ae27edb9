"""numpy marching cubes over a dense fp32 grid (NaN = unobserved), the independent restatement of csrc/tsdf.hip's
tsdf_extract_mesh rule for tests: the same generated tables (sgam_neurips22_amd/mc_tables.py), the same fp32 expressions
for vertex positions and colours, the same vertex order (key order) and triangle order (cell key, table order)."""
import numpy as np

from sgam_neurips22_amd import mc_tables

MASK, NTRI, TRI, EDGE = mc_tables.table_arrays()
f32 = np.float32


def marching_cubes(grid, voxel, origin=(0, 0, 0), colors=None, key_fn=None):
    """grid (nz, ny, nx) fp32, grid[z, y, x] = TSDF at global lattice point origin + (x, y, z) (voxel centres at
    (i + 0.5) * voxel), NaN where unobserved; colors (nz, ny, nx, 3) fp32 0..255 or None.  key_fn(ix, iy, iz) -> int64 key of
    a global lattice point (vectorised; default: its linear index in the grid).  A vertex's key is key_fn(low end) * 3 + axis.
    Returns dict(vertices (n,3) f32, triangles (m,3) int32, keys (n,) int64[, vertex_colors (n,3) f32 0..255])."""
    g = np.asarray(grid, dtype=f32)
    nz, ny, nx = g.shape
    ox, oy, oz = (int(v) for v in origin)
    voxel = f32(voxel)
    if key_fn is None:
        def key_fn(ix, iy, iz):
            return ((iz - oz).astype(np.int64) * ny + (iy - oy)) * nx + (ix - ox)
    corners = []
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        corners.append(g[dz:dz + nz - 1, dy:dy + ny - 1, dx:dx + nx - 1])
    valid = np.ones(corners[0].shape, dtype=bool)
    case = np.zeros(corners[0].shape, dtype=np.int64)
    for c, v in enumerate(corners):
        valid &= ~np.isnan(v)
        case |= (np.nan_to_num(v, nan=1.0) < 0).astype(np.int64) << c
    sel = valid & (case != 0) & (case != 255)
    cz, cy, cx = np.nonzero(sel)
    gx, gy, gz = cx + ox, cy + oy, cz + oz
    ckey = key_fn(gx, gy, gz)
    order = np.argsort(ckey, kind="stable")
    cz, cy, cx, gx, gy, gz = cz[order], cy[order], cx[order], gx[order], gy[order], gz[order]
    cases = case[cz, cy, cx]
    tri = TRI[cases]                                  # (cells, 3 * max)
    used = tri >= 0
    e = tri[used]                                     # cell order, then table order
    cell = np.nonzero(used)[0]
    ax, ex, ey, ez = EDGE[e, 0], EDGE[e, 1], EDGE[e, 2], EDGE[e, 3]
    lx, ly, lz = gx[cell] + ex, gy[cell] + ey, gz[cell] + ez       # the edge's low end (global lattice)
    vkey = key_fn(lx, ly, lz) * 3 + ax
    keys, first = np.unique(vkey, return_index=True)
    triangles = np.searchsorted(keys, vkey).astype(np.int32).reshape(-1, 3)
    vx, vy, vz, va = lx[first], ly[first], lz[first], ax[first]
    f0 = g[vz - oz, vy - oy, vx - ox]
    f1 = g[vz - oz + (va == 2), vy - oy + (va == 1), vx - ox + (va == 0)]
    r0, r1 = np.abs(f0), np.abs(f1)
    den = r0 + r1
    p = np.stack([(vx.astype(f32) + f32(0.5)) * voxel, (vy.astype(f32) + f32(0.5)) * voxel, (vz.astype(f32) + f32(0.5)) * voxel], 1)
    pa = p[np.arange(len(va)), va]
    p[np.arange(len(va)), va] = (pa * r1 + (pa + voxel) * r0) / den
    out = {"vertices": p.astype(f32), "triangles": triangles, "keys": keys.astype(np.int64)}
    if colors is not None:
        col = np.asarray(colors, dtype=f32)
        c0 = col[vz - oz, vy - oy, vx - ox]
        c1 = col[vz - oz + (va == 2), vy - oy + (va == 1), vx - ox + (va == 0)]
        out["vertex_colors"] = ((c0 * r1[:, None] + c1 * r0[:, None]) / den[:, None]).astype(f32)
    return out


def euler_and_edges(triangles):
    """(V - E + F over the vertices the triangles use, undirected edge -> use count, directed edge count per edge)"""
    t = np.asarray(triangles, dtype=np.int64)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    und = np.sort(d, 1)
    uk, ucount = np.unique(und[:, 0] * (1 << 32) + und[:, 1], return_counts=True)
    dk, dcount = np.unique(d[:, 0] * (1 << 32) + d[:, 1], return_counts=True)
    V = len(np.unique(t))
    return V - len(uk) + len(t), (uk, ucount), (dk, dcount)


def area_and_volume(vertices, triangles):
    """surface area and enclosed volume (divergence theorem; positive when normals point outward) in float64"""
    v = np.asarray(vertices, dtype=np.float64)[np.asarray(triangles)]
    cr = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    return 0.5 * np.linalg.norm(cr, axis=1).sum(), (v[:, 0] * np.cross(v[:, 1], v[:, 2])).sum() / 6.0


def rasterise(vertices, triangles, w2c, K, H, W, z_near, z_far):
    """numpy restatement of csrc/mesh_raster.hip (same fp32 expressions, same 24.8 fixed-point coverage rule)"""
    fx, fy, cx, cy = f32(K[0, 0]), f32(K[1, 1]), f32(K[0, 2]), f32(K[1, 2])
    M = np.asarray(w2c, dtype=f32)
    zn, zf = f32(z_near), f32(z_far)
    zbuf = np.full((H, W), np.inf, dtype=f32)
    V = np.asarray(vertices, dtype=f32)
    cam = []
    for r in range(3):
        cam.append(((M[r, 0] * V[:, 0] + M[r, 1] * V[:, 1]) + M[r, 2] * V[:, 2]) + M[r, 3])
    cam = np.stack(cam, 1).astype(f32)
    for tri in np.asarray(triangles):
        P = [cam[i] for i in tri]
        for poly in _clip_near(P, zn):
            for k in range(1, len(poly) - 1):
                _raster_one([poly[0], poly[k], poly[k + 1]], fx, fy, cx, cy, H, W, zn, zf, zbuf)
    return np.where(np.isinf(zbuf), f32(0), zbuf)


def _lerp_near(a, b, zn):
    """the point of segment a (inside, z >= zn) -> b (outside) on the plane z = zn"""
    t = (zn - a[2]) / (b[2] - a[2])
    return np.array([a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), zn], dtype=f32)


def _clip_near(P, zn):
    inside = [p[2] >= zn for p in P]
    n_in = sum(inside)
    if n_in == 3:
        return [P]
    if n_in == 0:
        return []
    if n_in == 1:
        i = inside.index(True)
        a, b, c = P[i], P[(i + 1) % 3], P[(i + 2) % 3]
        return [[a, _lerp_near(a, b, zn), _lerp_near(a, c, zn)]]
    o = inside.index(False)
    c, a, b = P[o], P[(o + 1) % 3], P[(o + 2) % 3]        # a, b inside, c outside; polygon a, b, b->c, a->c
    return [[a, b, _lerp_near(b, c, zn), _lerp_near(a, c, zn)]]


LIM = f32(1 << 20)


def _raster_one(P, fx, fy, cx, cy, H, W, zn, zf, zbuf):
    X, Y, iz = [], [], []
    for p in P:
        xs = (fx * p[0]) / p[2] + cx
        ys = (fy * p[1]) / p[2] + cy
        if not (abs(xs) < LIM and abs(ys) < LIM):
            return
        X.append(int(np.rint(xs * f32(256))))
        Y.append(int(np.rint(ys * f32(256))))
        iz.append(f32(1) / p[2])
    area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    if area == 0:
        return
    if area < 0:
        X[1], X[2], Y[1], Y[2], iz[1], iz[2] = X[2], X[1], Y[2], Y[1], iz[2], iz[1]
        area = -area
    u0 = max(0, -((-min(X)) // 256))
    u1 = min(W - 1, max(X) // 256)
    v0 = max(0, -((-min(Y)) // 256))
    v1 = min(H - 1, max(Y) // 256)
    fa = f32(float(area))
    for v in range(v0, v1 + 1):
        for u in range(u0, u1 + 1):
            px, py = u * 256, v * 256
            E = []
            for i in range(3):
                a, b = i, (i + 1) % 3
                dx, dy = X[b] - X[a], Y[b] - Y[a]
                e = dx * (py - Y[a]) - dy * (px - X[a])
                own = dy < 0 or (dy == 0 and dx > 0)
                if e < 0 or (e == 0 and not own):
                    break
                E.append(e)
            else:
                # E[i] is the edge opposite vertex (i + 2) % 3
                w = ((f32(float(E[1])) * iz[0] + f32(float(E[2])) * iz[1]) + f32(float(E[0])) * iz[2]) / fa
                z = f32(1) / w
                if zn <= z <= zf and z < zbuf[v, u]:
                    zbuf[v, u] = z
