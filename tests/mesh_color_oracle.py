"""numpy restatement of the coloured rasteriser (csrc/mesh_raster.hip: sgam_mesh_render_rgbd_f32) for tests.  Transform, clipping,
coverage and depth are tests/mc_oracle.py's (its functions are called, or restated where the colour has to ride along); a
fragment replaces the kept one on z < zbuf, triangles in index order, so an exact z tie stays with the lower index; the colour is
the fp32 expression stated at the top of the kernel file."""
import numpy as np

import mc_oracle
from mc_oracle import LIM, f32


def _clip_near_colour(P, C, zn):
    """mc_oracle._clip_near with the vertices' colours: a new vertex takes Ca + t * (Cb - Ca) with the t of its position"""
    def lerp(i, j):
        a, b = P[i], P[j]
        t = (zn - a[2]) / (b[2] - a[2])
        return mc_oracle._lerp_near(a, b, zn), (C[i] + t * (C[j] - C[i])).astype(f32)

    inside = [p[2] >= zn for p in P]
    n_in = sum(inside)
    if n_in == 3:
        return [(P, C)]
    if n_in == 0:
        return []
    if n_in == 1:
        i = inside.index(True)
        (pb, cb), (pc, cc) = lerp(i, (i + 1) % 3), lerp(i, (i + 2) % 3)
        return [([P[i], pb, pc], [C[i], cb, cc])]
    o = inside.index(False)
    a, b = (o + 1) % 3, (o + 2) % 3
    (pbc, cbc), (pac, cac) = lerp(b, o), lerp(a, o)
    return [([P[a], P[b], pbc], [C[a], C[b], cbc]), ([P[a], pbc, pac], [C[a], cbc, cac])]


def _raster_one(P, C, frag, fx, fy, cx, cy, H, W, zn, zf, zbuf, rgb, win, perspective):
    X, Y, iz = [], [], []
    for p in P:
        xs = (fx * p[0]) / p[2] + cx
        ys = (fy * p[1]) / p[2] + cy
        if not (abs(xs) < LIM and abs(ys) < LIM):
            return
        X.append(int(np.rint(xs * f32(256))))
        Y.append(int(np.rint(ys * f32(256))))
        iz.append(f32(1) / p[2])
    C = list(C)
    area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    if area == 0:
        return
    if area < 0:
        X[1], X[2], Y[1], Y[2], iz[1], iz[2], C[1], C[2] = X[2], X[1], Y[2], Y[1], iz[2], iz[1], C[2], C[1]
        area = -area
    u0 = max(0, -((-min(X)) // 256))
    u1 = min(W - 1, max(X) // 256)
    v0 = max(0, -((-min(Y)) // 256))
    v1 = min(H - 1, max(Y) // 256)
    fa = f32(float(area))
    lo, hi = np.minimum(np.minimum(C[0], C[1]), C[2]), np.maximum(np.maximum(C[0], C[1]), C[2])
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
                a0, a1, a2 = f32(float(E[1])) * iz[0], f32(float(E[2])) * iz[1], f32(float(E[0])) * iz[2]
                z = f32(1) / (((a0 + a1) + a2) / fa)
                if zn <= z <= zf and z < zbuf[v, u]:
                    zbuf[v, u] = z
                    win[v, u] = frag
                    if not perspective:                     # screen-space (affine) weights: what the kernel must NOT compute
                        a0, a1, a2 = f32(float(E[1])), f32(float(E[2])), f32(float(E[0]))
                    x = ((a0 * C[0] + a1 * C[1]) + a2 * C[2]) / ((a0 + a1) + a2)
                    rgb[v, u] = np.minimum(np.maximum(x, lo), hi)


def rasterise_rgbd(vertices, colors, triangles, w2c, K, H, W, z_near, z_far, perspective=True):
    """(depth (H,W) f32, rgb (H,W,3) f32 0..255, fragment id (H,W) int64: 2 * triangle + sub, -1 where nothing is hit)"""
    fx, fy, cx, cy = f32(K[0, 0]), f32(K[1, 1]), f32(K[0, 2]), f32(K[1, 2])
    M = np.asarray(w2c, dtype=f32)
    zn, zf = f32(z_near), f32(z_far)
    zbuf = np.full((H, W), np.inf, dtype=f32)
    rgb = np.zeros((H, W, 3), dtype=f32)
    win = np.full((H, W), -1, dtype=np.int64)
    V = np.asarray(vertices, dtype=f32)
    col = np.asarray(colors, dtype=f32)
    cam = np.stack([((M[r, 0] * V[:, 0] + M[r, 1] * V[:, 1]) + M[r, 2] * V[:, 2]) + M[r, 3] for r in range(3)], 1).astype(f32)
    for t, tri in enumerate(np.asarray(triangles)):
        for sub, (P, C) in enumerate(_clip_near_colour([cam[i] for i in tri], [col[i] for i in tri], zn)):
            _raster_one(P, C, 2 * t + sub, fx, fy, cx, cy, H, W, zn, zf, zbuf, rgb, win, perspective)
    return np.where(np.isinf(zbuf), f32(0), zbuf), rgb, win
