"""numpy restatement of the coloured-ICP kernels (csrc/point_icp.hip: sgam_points_color_gradient_f32 and
sgam_points_icp_accumulate_colored) and of geometry.register_icp(estimation="colored") for tests: every expression in float64 on the
widened fp32 / uint8 inputs in the kernels' written order, scalar loops where the order of additions matters (the neighbours of a
point in column order; a correspondence's geometric row before its photometric one).  Search, update, Rodrigues and the pose error
are tests/icp_oracle.py's, the k nearest neighbours tests/cloud_oracle.py's.  Also the textured test surfaces of
tests/test_colored_icp_cpu.py and tests/test_gpu_colored_icp.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import cloud_oracle as CO  # noqa: E402
import icp_oracle as IO  # noqa: E402

f32 = np.float32
LAMBDA = 0.968                    # Open3D's lambda_geometric


def intensity(colors):
    """(N,) float64 of (N,3) uint8: (double)(r + g + b) / 765.0, the sum an integer"""
    c = np.asarray(colors)
    assert c.dtype == np.uint8
    return c.reshape(-1, 3).astype(np.int64).sum(1).astype(np.float64) / 765.0


def knn_rows(points, k):
    """the k-NN rows the gradient is taken over: the cloud against itself, the point excluded"""
    return CO.knn_brute(points, points, k, exclude_self=True)[1]


# ---------------------------------------------------------------- the gradient kernel
def gradient_system(points, normals, knn_index, I):
    """-> (A (N,3,3) symmetric, b (N,3), m (N,)): the normal equations of every point's gradient, the neighbours added one column
    after the other (the kernel's order), the tangent-plane constraint last"""
    p = np.asarray(points, dtype=f32).reshape(-1, 3).astype(np.float64)
    n = np.asarray(normals, dtype=f32).reshape(-1, 3).astype(np.float64)
    idx = np.asarray(knn_index)
    N, k = idx.shape
    A, b, m = np.zeros((N, 3, 3)), np.zeros((N, 3)), np.zeros(N, dtype=np.int64)
    with np.errstate(all="ignore"):
        for c in range(k):
            j = idx[:, c]
            ok = (j >= 0) & (j < N)
            jj = np.where(ok, j, 0)
            e = p[jj] - p
            en = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
            u = e - en[:, None] * n
            dI = I[jj] - I
            for a in range(3):
                for bb in range(a, 3):
                    A[:, a, bb] = np.where(ok, A[:, a, bb] + u[:, a] * u[:, bb], A[:, a, bb])
                b[:, a] = np.where(ok, b[:, a] + u[:, a] * dI, b[:, a])
            m += ok
        mm = (m * m).astype(np.float64)
        for a in range(3):
            for bb in range(a, 3):
                A[:, a, bb] = A[:, a, bb] + mm * (n[:, a] * n[:, bb])
                A[:, bb, a] = A[:, a, bb]
    return A, b, m


def color_gradient_f64(points, normals, colors, knn_index, intensities=None):
    """(N,3) float64: the kernel's gradient before its one rounding to fp32.  intensities (N,) float64: used in place of the uint8
    colours' (a field that is exempt from the quantisation, for the comparison with the truth)"""
    pts = np.asarray(points, dtype=f32).reshape(-1, 3)
    nrm = np.asarray(normals, dtype=f32).reshape(-1, 3)
    I = intensity(colors) if intensities is None else np.asarray(intensities, dtype=np.float64)
    A, b, m = gradient_system(pts, nrm, knn_index, I)
    out = np.full((len(pts), 3), np.nan)
    good = np.isfinite(pts).all(1) & np.isfinite(nrm).all(1) & (m >= 3)
    with np.errstate(all="ignore"):
        for i in np.flatnonzero(good):
            g = IO.cholesky_solve(A[i], b[i])         # (the update's factorisation, pivot rule and solves, on three unknowns)
            if g is not None:
                out[i] = g
    return out


def color_gradient(points, normals, colors, knn_index, intensities=None):
    """(N,3) fp32: sgam_points_color_gradient_f32"""
    with np.errstate(all="ignore"):
        return color_gradient_f64(points, normals, colors, knn_index, intensities).astype(f32)


# ---------------------------------------------------------------- the coloured accumulation
def rows(p, q, n, d, I_s, I_t, lam):
    """the two rows of correspondences, vectorised over them, float64 in the kernel's expressions:
    -> (J_G (M,6), r_G (M,), J_I (M,6), r_I (M,))"""
    sg, sp = np.sqrt(np.float64(lam)), np.sqrt(np.float64(1.0) - np.float64(lam))
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    ex, ey, ez = px - q[:, 0], py - q[:, 1], pz - q[:, 2]
    en = (ex * nx + ey * ny) + ez * nz
    JG = np.stack([sg * (py * nz - pz * ny), sg * (pz * nx - px * nz), sg * (px * ny - py * nx), sg * nx, sg * ny, sg * nz], 1)
    rG = sg * en
    wx, wy, wz = ex - en * nx, ey - en * ny, ez - en * nz
    Iproj = ((dx * wx + dy * wy) + dz * wz) + I_t
    dn = (dx * nx + dy * ny) + dz * nz
    mx, my, mz = -dx + dn * nx, -dy + dn * ny, -dz + dn * nz
    JI = np.stack([sp * (py * mz - pz * my), sp * (pz * mx - px * mz), sp * (px * my - py * mx), sp * mx, sp * my, sp * mz], 1)
    rI = sp * (I_s - Iproj)
    return JG, rG, JI, rI


def summands(moved, source_colors, target, normals, target_colors, gradient, index, d2, lam):
    """(2 N, 32) float64: rows 2 i and 2 i + 1 are what entry i adds to every slot FIRST (its geometric row's products; d2, the
    counts) and SECOND (its photometric row's products); zero rows for what is no correspondence (slot 30 apart)"""
    p32 = np.asarray(moved, dtype=f32).reshape(-1, 3)
    target = np.asarray(target, dtype=f32).reshape(-1, 3)
    index = np.asarray(index)
    ok = (index >= 0) & (index < len(target))
    j = np.where(ok, index, 0)
    n32, g32 = np.asarray(normals, dtype=f32).reshape(-1, 3)[j], np.asarray(gradient, dtype=f32).reshape(-1, 3)[j]
    ok &= np.isfinite(n32).all(1) & np.isfinite(g32).all(1)
    N = len(p32)
    S = np.zeros((N, 2, IO.SLOTS))
    with np.errstate(all="ignore"):
        JG, rG, JI, rI = rows(p32.astype(np.float64), target[j].astype(np.float64), n32.astype(np.float64), g32.astype(np.float64),
                              intensity(source_colors), intensity(target_colors)[j], lam)
        for half, (J, r) in enumerate(((JG, rG), (JI, rI))):
            for a in range(6):
                for b in range(a, 6):
                    S[:, half, IO.tri(a, b)] = J[:, a] * J[:, b]
                S[:, half, 21 + a] = J[:, a] * r
            S[:, half, 27] = r * r
        S[:, 0, 28] = np.asarray(d2, dtype=f32).astype(np.float64)
    S[:, 0, 29] = 1.0
    S[~ok] = 0.0
    S[:, 0, 30] = np.isfinite(p32).all(1)
    return S.reshape(2 * N, IO.SLOTS)


def accumulate(moved, source_colors, target, normals, target_colors, gradient, index, d2, lam):
    """-> (partials (blocks, 32), magnitude (blocks, 32): the sum of |summand| per slot and chunk), a chunk's slot the plain sum of
    its summands in index order, an entry's geometric summand before its photometric one"""
    S = summands(moved, source_colors, target, normals, target_colors, gradient, index, d2, lam)
    blocks = (len(S) // 2 + IO.CHUNK - 1) // IO.CHUNK
    part, mag = np.zeros((blocks, IO.SLOTS)), np.zeros((blocks, IO.SLOTS))
    for b in range(blocks):
        part[b] = np.cumsum(S[2 * b * IO.CHUNK:2 * (b + 1) * IO.CHUNK], axis=0)[-1]
        mag[b] = np.cumsum(np.abs(S[2 * b * IO.CHUNK:2 * (b + 1) * IO.CHUNK]), axis=0)[-1]
    return part, mag


def residuals(xi, p, q, n, d, I_s, I_t, lam):
    """(r_G, r_I) of ONE correspondence with the point p moved by the pose increment xi = (omega, v): exp([omega]x) p + v.  The
    function whose derivative at xi = 0 the two rows are."""
    xi = np.asarray(xi, dtype=np.float64)
    pm = IO.rodrigues(xi[:3]) @ np.asarray(p, dtype=np.float64) + xi[3:]
    e = pm - q
    en = e @ n
    w = e - en * n
    return np.sqrt(lam) * en, np.sqrt(1.0 - lam) * (I_s - (d @ w + I_t))


# ---------------------------------------------------------------- the loop
def register_icp(source, source_colors, target, target_colors, normals, gradient, max_distance, lam=LAMBDA, init=None, max_iterations=30,
                 relative_fitness=1e-6, relative_rmse=1e-6):
    """the loop of geometry.register_icp(estimation="colored"): icp_oracle's with the coloured sums"""
    state, hist = IO.new_state(init), []
    for it in range(max_iterations):
        moved = IO.transform(source, state[:16])
        d2, index = IO.search(moved, target, max_distance)
        part = accumulate(moved, source_colors, target, normals, target_colors, gradient, index, d2, lam)[0]
        state, row = IO.update(part, it, relative_fitness, relative_rmse, state)
        hist.append(row)
        if state[18] != 0.0:
            break
    T = state[:16].reshape(4, 4).copy()
    out = IO.evaluate(source, target, max_distance, T)
    out.update(transformation=T, iterations=int(state[19]), status=int(state[18]), converged=int(state[18]) == 1, history=np.array(hist))
    return out


# ---------------------------------------------------------------- the textured test surfaces
def texture_field(x, y):
    """three smooth channels in [0.1, 0.9] over the plane: (N,3) float64.  Wavelengths of 3 to 7 units, in different directions per
    channel, so that the intensity varies along both axes everywhere but on curves"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    r = 0.5 + 0.4 * np.sin(1.1 * x + 0.3) * np.cos(0.9 * y - 0.2)
    g = 0.5 + 0.4 * np.sin(0.8 * x - 1.3 * y + 1.0)
    b = 0.5 + 0.4 * np.cos(1.7 * y + 0.5 * x)
    return np.stack([r, g, b], axis=-1)


def texture(x, y):
    """the field as uint8 colours: round(255 * value)"""
    return np.rint(255.0 * texture_field(x, y)).astype(np.uint8)


def textured_plane(n, seed, lo=0.0, hi=4.0):
    """(points (n,3) fp32 on z = 0, normals (0, 0, 1), colours (n,3) uint8 of the texture at the fp32 coordinates)"""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(lo, hi, n), rng.uniform(lo, hi, n), np.zeros(n)], axis=1).astype(f32)
    return p, np.tile(np.array([0, 0, 1], dtype=f32), (n, 1)), texture(p[:, 0], p[:, 1])


def textured_surface(n, seed, lo=0.0, hi=4.0):
    """icp_oracle.surface with the texture at (x, y): (points, normals, colours)"""
    p, nrm = IO.surface(n, seed, lo, hi)
    return p, nrm, texture(p[:, 0], p[:, 1])


def plane_motion(angle_deg=1.0, translation=(0.03, -0.02, 0.0)):
    """the motion of the plane tests: about the plane's normal through the centre of the square, then in the plane"""
    C = np.eye(4)
    C[:3, 3] = [2.0, 2.0, 0.0]
    return C @ IO.rigid(angle_deg, [0.0, 0.0, 1.0], translation) @ np.linalg.inv(C)


def moved_target(points, normals, colors, T):
    """a cloud moved by T as a registration target: (points fp32, normals fp32, the colours as they are)"""
    return IO.transform(points, T), (np.asarray(normals, dtype=np.float64) @ T[:3, :3].T).astype(f32), colors


def plane_exact_copy(n, seed=5):
    """-> (source, source colours, target, target colours, target normals, the motion): the target is the moved source"""
    p, nrm, col = textured_plane(n, seed)
    T = plane_motion()
    tgt, tn, tc = moved_target(p, nrm, col, T)
    return p, col, tgt, tc, tn, T


def plane_resampled(n, m, seed=5):
    """the source: n samples 0.3 inside the square; the target: m OTHER samples of the same textured plane, moved"""
    p, _, col = textured_plane(n, seed, 0.3, 3.7)
    o, nrm, ocol = textured_plane(m, seed + 1)
    T = plane_motion()
    tgt, tn, tc = moved_target(o, nrm, ocol, T)
    return p, col, tgt, tc, tn, T


def surface_exact_copy(n, seed=5):
    """the curved surface of icp_oracle with the texture, moved by icp_oracle's 5 degree / 0.11 perturbation"""
    p, nrm, col = textured_surface(n, seed)
    T = IO.perturbation()
    tgt, tn, tc = moved_target(p, nrm, col, T)
    return p, col, tgt, tc, tn, T
