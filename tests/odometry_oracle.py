"""The numpy twin of csrc/rgbd_odometry.hip (the rule: include/sgam_hip.h): the pyramid and the geometry of a pixel
in float32, one numpy operation per operator in the written order (bit-equal to the kernels); the rows of the normal equations in
float64 with the kernel's expressions (and the sum of their magnitudes, the yardstick of the GPU comparison); the update through
icp_oracle's, with the pyramid's one addition; the loops of geometry.rgbd_odometry and geometry.multiway_rgbd.  Written from the
rule, on the CPU, with nothing of the package in it.  Also the analytic scenes of tests/test_odometry_cpu.py and
tests/test_gpu_odometry.py: frames rendered by ray-surface intersection, so that the true motion between two of them is known."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import icp_oracle as IO  # noqa: E402
import posegraph_oracle as PO  # noqa: E402

f32 = np.float32
F32_MAX = f32(3.4028234663852886e38)
CHUNK, SLOTS = 1024, 32
MAX_LEVELS = 4
LAMBDA_GEOMETRIC = 0.968


# ---------------------------------------------------------------- pyramid
def level_sizes(H, W, levels):
    sizes = [(H, W)]
    for _ in range(1, levels):
        H, W = (H + 1) // 2, (W + 1) // 2
        sizes.append((H, W))
    return sizes


def level_K(K, level):
    """diag(2^-l, 2^-l, 1) K: every entry of the first two rows halved per level (exact)"""
    K = np.array(K, dtype=np.float64)
    K[:2] *= 0.5 ** level
    return K


def intensity0(rgb):
    """(H,W,3) uint8 -> (H,W) fp32: (float)(r + g + b) / 765.0f"""
    c = np.asarray(rgb, np.uint8).astype(np.int32)
    return ((c[..., 0] + c[..., 1] + c[..., 2]).astype(f32) / f32(765.0)).astype(f32)


def down(I, D):
    """one level down: the 3 x 3 binomial filter at (2i, 2j) with clamped borders for I, plain subsampling for D"""
    I, D = np.asarray(I, f32), np.asarray(D, f32)
    H, W = I.shape[-2:]
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    r = [np.clip(2 * np.arange(Ho) + k - 1, 0, H - 1) for k in range(3)]
    c = [np.clip(2 * np.arange(Wo) + k - 1, 0, W - 1) for k in range(3)]
    two = f32(2.0)
    with np.errstate(all="ignore"):
        h = [(I[..., r[a], :][..., c[0]] + two * I[..., r[a], :][..., c[1]]) + I[..., r[a], :][..., c[2]] for a in range(3)]
        out = ((h[0] + two * h[1]) + h[2]) * f32(0.0625)
    assert out.dtype == f32
    return out, np.ascontiguousarray(D[..., ::2, ::2])


def pyramid(depths, rgbs, levels):
    """-> [(I (F,H_l,W_l) fp32, D (F,H_l,W_l) fp32) per level], level 0 first"""
    I = np.stack([intensity0(c) for c in rgbs])
    D = np.stack([np.asarray(d, f32) for d in depths])
    out = [(I, D)]
    for _ in range(1, levels):
        if min(out[-1][0].shape[-2:]) < 3:                   # (the next level would be smaller than 2 x 2)
            raise ValueError("a level smaller than 2 x 2")
        out.append(down(*out[-1]))
    return out


# ---------------------------------------------------------------- one pair on one level
def _valid(x, zn, zf):
    return (np.abs(x) <= F32_MAX) & (zn <= x) & (x <= zf)


def geometry(Ds, Dt, K, T, z_near, z_far, tau):
    """view_consistency's expressions for every source pixel, in fp32 -> dict of flat arrays: valid (class != 0), cov (class 6),
    X, Y, Z, wx, wy (fp32), x0, y0 (int, 0 where not in view)"""
    H, W = Ds.shape
    K = np.asarray(K, np.float64)
    kinv = np.linalg.inv(K).astype(f32).reshape(9)
    fx, fy, cx, cy = f32(K[0, 0]), f32(K[1, 1]), f32(K[0, 2]), f32(K[1, 2])
    zn, zf, tau = f32(z_near), f32(z_far), f32(tau)
    T = np.asarray(T, np.float64).reshape(-1)[:12].astype(f32)
    d = np.ascontiguousarray(Ds, f32)
    Dt = np.ascontiguousarray(Dt, f32)
    fi, fj = np.meshgrid(np.arange(H).astype(f32), np.arange(W).astype(f32), indexing="ij")
    with np.errstate(all="ignore"):
        a = (kinv[0] * fj + kinv[1] * fi) + kinv[2]
        b = (kinv[3] * fj + kinv[4] * fi) + kinv[5]
        c = (kinv[6] * fj + kinv[7] * fi) + kinv[8]
        x, y, z = a * d, b * d, c * d
        X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3]
        Y = ((T[4] * x + T[5] * y) + T[6] * z) + T[7]
        Z = ((T[8] * x + T[9] * y) + T[10] * z) + T[11]
        u = (fx * X) / Z + cx
        v = (fy * Y) / Z + cy
        x0f, y0f = np.floor(u), np.floor(v)
        valid_d = _valid(d, zn, zf)
        in_view = valid_d & (zn <= Z) & (Z <= zf) & (f32(0) <= x0f) & (x0f <= f32(W - 2)) & (f32(0) <= y0f) & (y0f <= f32(H - 2))
        wx, wy = u - x0f, v - y0f
        x0 = np.where(in_view, x0f, f32(0)).astype(np.int64)
        y0 = np.where(in_view, y0f, f32(0)).astype(np.int64)
        D = [Dt[y0, x0], Dt[y0, x0 + 1], Dt[y0 + 1, x0], Dt[y0 + 1, x0 + 1]]
        right, down_ = wx >= f32(0.5), wy >= f32(0.5)
        Dn = np.where(down_, np.where(right, D[3], D[2]), np.where(right, D[1], D[0]))
        e = Z - Dn
        all_ok = np.ones((H, W), bool)
        for Dk in D:
            all_ok &= _valid(Dk, zn, zf) & (np.abs(Z - Dk) <= tau)
        cov = in_view & _valid(Dn, zn, zf) & ~(e > tau) & ~(-e > tau) & all_ok
    for t in (X, Y, Z, wx, wy):
        assert t.dtype == f32
    flat = lambda t: t.reshape(-1)  # noqa: E731
    return {"valid": flat(valid_d), "cov": flat(cov), "X": flat(X), "Y": flat(Y), "Z": flat(Z), "wx": flat(wx), "wy": flat(wy),
            "x0": flat(x0), "y0": flat(y0), "fx": float(fx), "fy": float(fy)}


def _corners(plane, g):
    p = np.ascontiguousarray(plane, f32).astype(np.float64)
    y0, x0 = g["y0"], g["x0"]
    return p[y0, x0], p[y0, x0 + 1], p[y0 + 1, x0], p[y0 + 1, x0 + 1]


def _lerp3(c, wx, wy):
    """(L, L_u, L_v) of the four corners, fp64, the rule's order"""
    c00, c01, c10, c11 = c
    top = c00 + wx * (c01 - c00)
    bot = c10 + wx * (c11 - c10)
    return top + wy * (bot - top), (c01 - c00) + wy * ((c11 - c10) - (c01 - c00)), bot - top


def _row(w, X, Y, Z, gx, gy, gz):
    return [w * (Y * gz - Z * gy), w * (Z * gx - X * gz), w * (X * gy - Y * gx), w * gx, w * gy, w * gz]


def rows(Is, Ds, It, Dt, K, T, z_near, z_far, tau, lam=LAMBDA_GEOMETRIC):
    """-> (g, J_I (6 x (HW,)), r_I, J_Z, r_Z, ez): the two rows of every pixel, fp64 (garbage where g["cov"] is False)"""
    g = geometry(Ds, Dt, K, T, z_near, z_far, tau)
    sg, sp = np.sqrt(np.float64(lam)), np.sqrt(1.0 - np.float64(lam))
    with np.errstate(all="ignore"):
        wx, wy = g["wx"].astype(np.float64), g["wy"].astype(np.float64)
        X, Y, Z = g["X"].astype(np.float64), g["Y"].astype(np.float64), g["Z"].astype(np.float64)
        iz = 1.0 / Z
        ux = g["fx"] * iz
        uz = -((ux * X) * iz)
        vy = g["fy"] * iz
        vz = -((vy * Y) * iz)
        L, Lu, Lv = _lerp3(_corners(It, g), wx, wy)
        JI = _row(sp, X, Y, Z, -(Lu * ux), -(Lv * vy), -(Lu * uz + Lv * vz))
        rI = sp * (np.ascontiguousarray(Is, f32).reshape(-1).astype(np.float64) - L)
        L, Lu, Lv = _lerp3(_corners(Dt, g), wx, wy)
        ez = Z - L
        JZ = _row(sg, X, Y, Z, -(Lu * ux), -(Lv * vy), 1.0 - (Lu * uz + Lv * vz))
        rZ = sg * ez
    return g, JI, rI, JZ, rZ, ez


def summands(Is, Ds, It, Dt, K, T, z_near, z_far, tau, lam=LAMBDA_GEOMETRIC, information=False, frame=None):
    """-> (S (HW,32): every pixel's summand of every slot, M (HW,32): its magnitude)"""
    n = Ds.size
    S = np.zeros((n, SLOTS))
    with np.errstate(all="ignore"):
        if information:
            g = geometry(Ds, Dt, K, T, z_near, z_far, tau)
            q = np.stack([g["X"], g["Y"], g["Z"]], axis=1)
            if frame is not None:
                Fr = np.asarray(frame, f32).reshape(12)
                x, y, z = q[:, 0], q[:, 1], q[:, 2]
                q = np.stack([((Fr[0] * x + Fr[1] * y) + Fr[2] * z) + Fr[3], ((Fr[4] * x + Fr[5] * y) + Fr[6] * z) + Fr[7],
                              ((Fr[8] * x + Fr[9] * y) + Fr[10] * z) + Fr[11]], axis=1)
                assert q.dtype == f32
            px, py, pz = (q[:, k].astype(np.float64) for k in range(3))
            one = np.ones(n)
            S[:, 0], S[:, 1], S[:, 2] = py * py + pz * pz, -(px * py), -(px * pz)
            S[:, 4], S[:, 5] = -pz, py
            S[:, 6], S[:, 7] = px * px + pz * pz, -(py * pz)
            S[:, 8], S[:, 10] = pz, -px
            S[:, 11] = px * px + py * py
            S[:, 12], S[:, 13] = -py, px
            S[:, 15], S[:, 18], S[:, 20] = one, one, one
        else:
            g, JI, rI, JZ, rZ, ez = rows(Is, Ds, It, Dt, K, T, z_near, z_far, tau, lam)
            for a in range(6):
                for b in range(a, 6):
                    S[:, IO.tri(a, b)] = JI[a] * JI[b] + JZ[a] * JZ[b]
                S[:, 21 + a] = JI[a] * rI + JZ[a] * rZ
            S[:, 27] = rI * rI + rZ * rZ
            S[:, 28] = ez * ez
    S[:, 29] = 1.0
    S[~g["cov"]] = 0.0
    S[:, 30] = g["valid"]
    return S, np.abs(S)


def accumulate(Is, Ds, It, Dt, K, T, z_near, z_far, tau, lam=LAMBDA_GEOMETRIC, information=False, frame=None):
    """-> (partials (chunks, 32), magnitude (chunks, 32)): a chunk's slot is the plain sum of its summands in pixel order (the kernel
    adds the same numbers in another fixed order)"""
    S, M = summands(Is, Ds, It, Dt, K, T, z_near, z_far, tau, lam, information, frame)
    blocks = (len(S) + CHUNK - 1) // CHUNK
    part, mag = np.zeros((blocks, SLOTS)), np.zeros((blocks, SLOTS))
    for b in range(blocks):
        part[b] = np.cumsum(S[b * CHUNK:(b + 1) * CHUNK], axis=0)[-1]
        mag[b] = np.cumsum(M[b * CHUNK:(b + 1) * CHUNK], axis=0)[-1]
    return part, mag


def fold(partials):
    total = np.zeros(SLOTS)
    for row in np.asarray(partials, np.float64).reshape(-1, SLOTS):
        total = total + row
    return total


def update(partials, level_first, relative_fitness, relative_rmse, state):
    """rules 1-6 of the ICP update (icp_oracle.update) with the pyramid's addition: on the first iteration of a level a status 1
    returns to 0 first and the stop test is skipped -> (state, history row)"""
    s = np.array(state, dtype=np.float64)
    if level_first and s[18] == 1.0:
        s[18] = 0.0
    return IO.update(partials, 0 if level_first else 1, relative_fitness, relative_rmse, s)


def information_matrix(total):
    A = np.zeros((6, 6))
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = total[IO.tri(a, b)]
    return A


def odometry(depths, rgbs, K, pairs, z_near, z_far, tau, init=None, iterations=(20, 10, 5), lam=LAMBDA_GEOMETRIC, relative_fitness=1e-6,
             relative_rmse=1e-6, information=True, information_frames=None, pyr=None):
    """the loop of geometry.rgbd_odometry -> dict of transformation (P,4,4), status, fitness, rmse, iterations (P,), history
    (P,rows,8), information (P,6,6)"""
    levels = len(iterations)
    pyr = pyramid(depths, rgbs, levels) if pyr is None else pyr
    F, P, nrows = len(depths), len(pairs), int(sum(iterations))
    states = np.stack([IO.new_state(None if init is None else init[p]) for p in range(P)])
    history = np.zeros((P, nrows, 8))
    info = np.zeros((P, 6, 6))
    empty = np.zeros((1, SLOTS))
    for p, (s, t) in enumerate(pairs):
        ok = 0 <= s < F and 0 <= t < F
        row = 0
        for level in range(levels - 1, -1, -1):
            I, D = pyr[level]
            Kl = level_K(K, level)
            for it in range(iterations[levels - 1 - level]):
                first = it == 0
                frozen = states[p][18] == 2.0 or (states[p][18] == 1.0 and not first)
                part = empty if (frozen or not ok) else accumulate(I[s], D[s], I[t], D[t], Kl, states[p][:16], z_near, z_far, tau, lam)[0]
                states[p], history[p, row] = update(part, first, relative_fitness, relative_rmse, states[p])
                row += 1
        if information and ok:
            fr = None if information_frames is None else np.asarray(information_frames[p], np.float64)[:3].reshape(12).astype(f32)
            I, D = pyr[0]
            info[p] = information_matrix(fold(accumulate(I[s], D[s], I[t], D[t], K, states[p][:16], z_near, z_far, tau, lam, True, fr)[0]))
    return {"transformation": states[:, :16].reshape(P, 4, 4).copy(), "status": states[:, 18].copy(), "fitness": states[:, 16].copy(),
            "rmse": states[:, 17].copy(), "iterations": states[:, 19].copy(), "history": history, "information": info, "state": states}


def candidate_pairs(n, covisibility, min_covisibility=0.3, stride=1):
    """[(i, j, uncertain)]: consecutive pairs always, the others where (j - i) % stride == 0 and covisibility(i, j) >= the minimum"""
    out = [(i, i + 1, False) for i in range(n - 1)]
    for i in range(n):
        for j in range(i + 2, n):
            if (j - i) % stride == 0 and covisibility(i, j) >= min_covisibility:
                out.append((i, j, True))
    return out


def covisibility(depths, rgbs, K, Ts, z_near, z_far, tau, i, j):
    """sums[6] / (H W - sums[0]) of view_consistency at the nominal poses, through this twin's geometry"""
    g = geometry(depths[i], depths[j], K, np.asarray(Ts[j], np.float64) @ np.linalg.inv(np.asarray(Ts[i], np.float64)), z_near, z_far, tau)
    n = int(g["valid"].sum())
    return g["cov"].sum() / n if n else float("nan")


def multiway(depths, rgbs, K, Ts, z_near, z_far, tau, min_covisibility=0.3, stride=1, extra_edges=(), iterations=(20, 10, 5), **pg):
    """geometry.multiway_rgbd on the twins: candidates, one odometry over all of them from T_j T_i^-1, edges T_j^-1 M_ij T_i with the
    information taken in frame T_j^-1, then posegraph_oracle.optimize.  extra_edges [(i, j, 4x4 world-frame edge)]: fabricated
    uncertain edges (the tests' wrong loop closure), with the information of the genuine odometry of that pair."""
    Ts = np.asarray(Ts, np.float64)
    n = len(depths)
    cand = candidate_pairs(n, lambda i, j: covisibility(depths, rgbs, K, Ts, z_near, z_far, tau, i, j), min_covisibility, stride)
    cand += [(i, j, True) for i, j, _ in extra_edges]
    pairs = [(i, j) for i, j, _ in cand]
    inv = [np.linalg.inv(T) for T in Ts]
    init = [Ts[j] @ inv[i] for i, j in pairs]
    res = odometry(depths, rgbs, K, pairs, z_near, z_far, tau, init=init, iterations=iterations, information_frames=[inv[j] for _, j in pairs])
    src, dst, T, Lam, unc, missing = [], [], [], [], [], []
    n_real = len(cand) - len(extra_edges)
    for k, (i, j, uncertain) in enumerate(cand):
        if res["status"][k] == 2.0:
            if not uncertain:
                missing.append((i, j))
            continue
        edge = inv[j] @ res["transformation"][k] @ Ts[i] if k < n_real else np.asarray(extra_edges[k - n_real][2], np.float64)
        src.append(i), dst.append(j), T.append(edge), Lam.append(res["information"][k]), unc.append(uncertain)
    mu = pg.pop("line_process_weight", None)
    if mu is None:
        mu = PO.default_mu(Lam, unc, tau)
    out = PO.optimize(n, src, dst, T, Lam, unc, mu, **pg)
    out.update(edges=list(zip(src, dst, unc)), missing_odometry=missing, odometry=res)
    return out


# ---------------------------------------------------------------- analytic scenes
TRUE_XI = np.array([0.02, -0.03, 0.04, 0.15, -0.1, 0.05])


def se3_exp(xi):
    """exp of (omega, v) as a 4x4: [exp([omega]x) | V v] with V = I + b [w]x + c [w]x^2"""
    xi = np.asarray(xi, np.float64)
    w, v = xi[:3], xi[3:]
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    T = np.eye(4)
    T[:3, :3] = IO.rodrigues(w)
    if th < 1e-8:
        V = np.eye(3) + 0.5 * Kx
    else:
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * Kx + (th - np.sin(th)) / th ** 3 * (Kx @ Kx)
    T[:3, 3] = V @ v
    return T


def texture(x, y):
    """a sum of sinusoids over the surface coordinates, in [0, 1]: no direction of the image is without gradient"""
    t = 0.5 + 0.16 * np.sin(2.1 * x + 0.4) + 0.14 * np.sin(2.7 * y - 0.3) + 0.1 * np.sin(1.3 * x + 1.9 * y) + 0.08 * np.cos(3.4 * x - 2.2 * y)
    return np.clip(t, 0.0, 1.0)


def _hit_plane(o, d):
    """the tilted plane z = 2 + 0.2 x - 0.15 y"""
    n, c = np.array([-0.2, 0.15, 1.0]), 2.0
    return (c - o @ n) / (d @ n)


def _hit_paraboloid(o, d):
    """z = 2 + 0.15 (x^2 + y^2) - 0.1 x y: the smaller positive root of the quadratic in the ray parameter"""
    q = lambda a, b: 0.15 * (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) - 0.05 * (a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0])  # noqa: E731
    A, B, C = q(d, d), 2.0 * q(o, d) - d[..., 2], q(o, o) + 2.0 - o[..., 2]
    disc = np.sqrt(np.maximum(B * B - 4.0 * A * C, 0.0))
    lin = -C / np.where(B == 0, 1.0, B)
    A_ = np.where(np.abs(A) < 1e-14, 1.0, A)
    r1, r2 = (-B - disc) / (2 * A_), (-B + disc) / (2 * A_)
    t = np.where(r1 > 0, r1, r2)
    t = np.where((r1 > 0) & (r2 > 0), np.minimum(r1, r2), t)
    return np.where(np.abs(A) < 1e-14, lin, t)


SURFACES = {"plane": _hit_plane, "paraboloid": _hit_paraboloid}


def render(surface, T_w2c, K, H, W):
    """(depth (H,W) fp32, rgb (H,W,3) uint8) of the surface seen by the camera T_w2c: ray-surface intersection per pixel centre,
    the texture (three shifted copies) rounded to uint8"""
    K = np.asarray(K, np.float64)
    c2w = np.linalg.inv(np.asarray(T_w2c, np.float64))
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays = np.stack([jj, ii, np.ones_like(jj)], axis=-1) @ np.linalg.inv(K).T            # camera frame, z = 1
    d = rays @ c2w[:3, :3].T
    o = np.broadcast_to(c2w[:3, 3], d.shape)
    t = SURFACES[surface](o, d)
    pt = o + t[..., None] * d
    depth = t.astype(f32)                                                               # rays have z = 1: t is the camera depth
    x, y = pt[..., 0], pt[..., 1]
    rgb = np.stack([texture(x, y), texture(x + 0.7, y - 0.4), texture(x - 0.5, y + 0.9)], axis=-1)
    return depth, np.round(rgb * 255.0).astype(np.uint8)


def camera(H, W, f=None):
    """K with focal length f (default max(H, W)) and the principal point at the image centre"""
    f = float(max(H, W) if f is None else f)
    return np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]])


def scene_pair(surface, H, W, xi=TRUE_XI, f=None):
    """two frames of `surface`: frame 0 from the identity, frame 1 from T = exp(xi); the true odometry of pair (0, 1) is T"""
    K = camera(H, W, f)
    T = se3_exp(xi)
    d0, c0 = render(surface, np.eye(4), K, H, W)
    d1, c1 = render(surface, T, K, H, W)
    return [d0, d1], [c0, c1], K, T


def hand_case():
    """the issue's exact case: K = [[16,0,8],[0,16,4],[0,0,1]], 8 x 16, depth 2, grey = 4 * column"""
    K = np.array([[16.0, 0, 8], [0, 16, 4], [0, 0, 1]])
    depth = np.full((8, 16), 2.0, f32)
    grey = np.broadcast_to((4 * np.arange(16)).astype(np.uint8)[None, :, None], (8, 16, 3)).copy()
    return depth, grey, K


def pose_error(T, T_true):
    """(angle in degrees, translation distance)"""
    e = IO.pose_error(T, T_true)
    return e[2], e[1]
