"""numpy restatement of the registration kernels (csrc/point_icp.hip) for tests: the fp32 transform in its spelled order, the
search through geometry_oracle, the sums of one Gauss-Newton step with the kernel's summand expressions in float64 (and the sum of
their magnitudes, the yardstick of the GPU comparison), the update with its own Cholesky solve and np.sin / np.cos, and the
register_icp loop.  Also the test surface of tests/test_icp_cpu.py and tests/test_gpu_icp.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import geometry_oracle as GO  # noqa: E402

f32 = np.float32
CHUNK, SLOTS = 4096, 32
PIVOT_REL = 1e-12                 # csrc/point_icp.hip: ICP_PIVOT_REL
SMALL_THETA2 = 1e-16


def tri(a, b):
    """slot of entry (a, b), a <= b, of the row-major upper triangle of a 6 x 6 matrix"""
    return a * 6 - a * (a - 1) // 2 + (b - a)


def transform(points, T):
    """points (N,3) fp32 moved by the 4x4 float64 T: T[0..11] rounded to fp32 once, X = ((T0 x + T1 y) + T2 z) + T3 in fp32"""
    p = np.asarray(points, dtype=f32).reshape(-1, 3)
    t = np.asarray(T, dtype=np.float64).reshape(16)[:12].astype(f32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        out = np.stack([((t[0] * x + t[1] * y) + t[2] * z) + t[3], ((t[4] * x + t[5] * y) + t[6] * z) + t[7],
                        ((t[8] * x + t[9] * y) + t[10] * z) + t[11]], axis=1)
    assert out.dtype == f32
    out[~np.isfinite(p).all(1)] = np.nan
    return out


def search(moved, target, max_distance):
    """(d2 fp32, index int32) of the moved source against the target: geometry_oracle's exact nearest neighbour"""
    return GO.nn_brute(moved, target, GO.max_d2_of(max_distance))


def summands(moved, target, normals, index, d2):
    """(N, 32) float64: every entry's summand of every slot, zero rows for the entries that are no correspondence (slot 30: 1 for
    every source point that is a point), in the kernel's expressions"""
    p32 = np.asarray(moved, dtype=f32).reshape(-1, 3)
    index = np.asarray(index)
    target = np.asarray(target, dtype=f32).reshape(-1, 3)
    ok = (index >= 0) & (index < len(target))
    j = np.where(ok, index, 0)
    n = None
    if normals is not None:
        n32 = np.asarray(normals, dtype=f32).reshape(-1, 3)[j]
        ok &= np.isfinite(n32).all(1)
        n = n32.astype(np.float64)
    p = p32.astype(np.float64)
    q = target[j].astype(np.float64)
    S = np.zeros((len(p), SLOTS))
    with np.errstate(all="ignore"):
        px, py, pz = p[:, 0], p[:, 1], p[:, 2]
        ex, ey, ez = px - q[:, 0], py - q[:, 1], pz - q[:, 2]
        if n is not None:
            nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
            J = [py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz]
            r = (ex * nx + ey * ny) + ez * nz
            for a in range(6):
                for b in range(a, 6):
                    S[:, tri(a, b)] = J[a] * J[b]
                S[:, 21 + a] = J[a] * r
            S[:, 27] = r * r
        else:
            one = np.ones(len(p))
            S[:, 0], S[:, 1], S[:, 2] = py * py + pz * pz, -(px * py), -(px * pz)
            S[:, 4], S[:, 5] = -pz, py
            S[:, 6], S[:, 7] = px * px + pz * pz, -(py * pz)
            S[:, 8], S[:, 10] = pz, -px
            S[:, 11] = px * px + py * py
            S[:, 12], S[:, 13] = -py, px
            S[:, 15], S[:, 18], S[:, 20] = one, one, one
            S[:, 21], S[:, 22], S[:, 23] = py * ez - pz * ey, pz * ex - px * ez, px * ey - py * ex
            S[:, 24], S[:, 25], S[:, 26] = ex, ey, ez
            S[:, 27] = (ex * ex + ey * ey) + ez * ez
        S[:, 28] = np.asarray(d2, dtype=f32).astype(np.float64)
    S[:, 29] = 1.0
    S[~ok] = 0.0
    S[:, 30] = np.isfinite(p32).all(1)
    return S


def accumulate(moved, target, normals, index, d2):
    """-> (partials (blocks, 32) float64, magnitude (blocks, 32): the sum of |summand| per slot and chunk).  A chunk's slot is the
    plain sum of its summands in index order: the kernel adds the same numbers in another fixed order."""
    S = summands(moved, target, normals, index, d2)
    blocks = (len(S) + CHUNK - 1) // CHUNK
    part, mag = np.zeros((blocks, SLOTS)), np.zeros((blocks, SLOTS))
    for b in range(blocks):                                             # (cumsum: one addition after the other, in index order)
        part[b] = np.cumsum(S[b * CHUNK:(b + 1) * CHUNK], axis=0)[-1]
        mag[b] = np.cumsum(np.abs(S[b * CHUNK:(b + 1) * CHUNK]), axis=0)[-1]
    return part, mag


def cholesky_solve(A, b):
    """x with A x = b by A = L L^T, column by column, and the two triangular solves; None where a pivot A_jj - sum L_jk^2 is not
    finite or <= PIVOT_REL * A_jj"""
    A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = len(b)
    L = np.zeros((n, n))
    for j in range(n):
        piv = A[j, j]
        for k in range(j):
            piv -= L[j, k] * L[j, k]
        if not np.isfinite(piv) or piv <= PIVOT_REL * A[j, j]:
            return None
        L[j, j] = np.sqrt(piv)
        for i in range(j + 1, n):
            t = A[i, j]
            for k in range(j):
                t -= L[i, k] * L[j, k]
            L[i, j] = t / L[j, j]
    x = np.zeros(n)
    for i in range(n):
        t = b[i]
        for k in range(i):
            t -= L[i, k] * x[k]
        x[i] = t / L[i, i]
    for i in range(n - 1, -1, -1):
        t = x[i]
        for k in range(i + 1, n):
            t -= L[k, i] * x[k]
        x[i] = t / L[i, i]
    return x


def rodrigues(w):
    """the rotation matrix exp([w]x): I + a [w]x + b (w w^T - theta^2 I), a = sin(theta) / theta, b = (1 - cos(theta)) / theta^2"""
    w = np.asarray(w, dtype=np.float64)
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    a, b = 1.0, 0.5
    if not th2 < SMALL_THETA2:
        th = np.sqrt(th2)
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + a * K + b * (np.outer(w, w) - th2 * np.eye(3))


def matrices(total):
    """(A 6x6 symmetric, J^T r) of 32 folded sums"""
    A = np.zeros((6, 6))
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = total[tri(a, b)]
    return A, np.array(total[21:27])


def new_state(T=None):
    s = np.zeros(24)
    s[:16] = np.eye(4).reshape(16) if T is None else np.asarray(T, dtype=np.float64).reshape(16)
    return s


def update(partials, iteration, relative_fitness, relative_rmse, state):
    """-> (state after the call, the history row): the kernel's rule on a copy of the 24-double state"""
    s = np.array(state, dtype=np.float64)
    if s[18] != 0.0:
        return s, np.array([s[16], s[17], s[20], s[21], 0.0, 0.0, s[18], 0.0])
    total = np.zeros(SLOTS)
    for row in np.asarray(partials, dtype=np.float64).reshape(-1, SLOTS):
        total = total + row
    with np.errstate(all="ignore"):
        count = total[29]
        fitness, rmse = count / total[30], np.sqrt(total[28] / count)
    status, wn, vn = 0.0, 0.0, 0.0
    if count < 6:
        status = 2.0
    elif iteration > 0 and abs(fitness - s[16]) < relative_fitness and abs(rmse - s[17]) < relative_rmse:
        status = 1.0
    else:
        A, g = matrices(total)
        x = cholesky_solve(A, g)
        if x is None:
            status = 2.0
        else:
            xi = -x
            w, v = xi[:3], xi[3:]
            dT = np.eye(4)
            dT[:3, :3], dT[:3, 3] = rodrigues(w), v
            T = dT @ s[:16].reshape(4, 4)
            T[3] = s[12:16]
            s[:16] = T.reshape(16)
            s[19] += 1.0
            wn, vn = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]), np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    s[16], s[17], s[18], s[20], s[21] = fitness, rmse, status, count, total[27]
    return s, np.array([fitness, rmse, count, total[27], wn, vn, status, 0.0])


def evaluate(source, target, max_distance, T=None):
    moved = transform(source, np.eye(4) if T is None else T)
    d2, index = search(moved, target, max_distance)
    total = accumulate(moved, target, None, index, d2)[0].sum(0)
    count, points = int(total[29]), int(total[30])
    return {"fitness": count / points if points else float("nan"), "inlier_rmse": np.sqrt(total[28] / count) if count else float("nan"),
            "correspondences": count}


def register_icp(source, target, max_distance, init=None, normals=None, max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """the loop of geometry.register_icp: normals given = point-to-plane.  -> dict(transformation, iterations, status, converged,
    history (rows, 8), fitness, inlier_rmse)"""
    state, rows = new_state(init), []
    for it in range(max_iterations):
        moved = transform(source, state[:16])
        d2, index = search(moved, target, max_distance)
        state, row = update(accumulate(moved, target, normals, index, d2)[0], it, relative_fitness, relative_rmse, state)
        rows.append(row)
        if state[18] != 0.0:
            break
    T = state[:16].reshape(4, 4).copy()
    out = evaluate(source, target, max_distance, T)
    out.update(transformation=T, iterations=int(state[19]), status=int(state[18]), converged=int(state[18]) == 1, history=np.array(rows))
    return out


# ---------------------------------------------------------------- the test surface
def surface(n, seed, lo=0.0, hi=4.0):
    """(points (n,3) fp32, unit normals (n,3) fp32) of z = 0.3 sin 1.7x + 0.2 cos 2.3y + 0.1xy sampled over [lo, hi]^2: the
    surface constrains all six degrees of freedom of a rigid motion"""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    z = 0.3 * np.sin(1.7 * x) + 0.2 * np.cos(2.3 * y) + 0.1 * x * y
    zx, zy = 0.3 * 1.7 * np.cos(1.7 * x) + 0.1 * y, -0.2 * 2.3 * np.sin(2.3 * y) + 0.1 * x
    nrm = np.stack([-zx, -zy, np.ones(n)], axis=1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.stack([x, y, z], axis=1).astype(f32), nrm.astype(f32)


def rigid(angle_deg, axis, translation):
    """4x4 float64: the rotation by angle_deg about `axis` through the origin, then the translation"""
    axis = np.asarray(axis, dtype=np.float64)
    T = np.eye(4)
    T[:3, :3] = rodrigues(np.radians(angle_deg) * axis / np.linalg.norm(axis))
    T[:3, 3] = translation
    return T


def perturbation():
    """the 5 degree / 0.11 motion of the loop tests, about the centre of the surface's square"""
    C = np.eye(4)
    C[:3, 3] = [2.0, 2.0, 0.5]
    return C @ rigid(5.0, [1.0, -2.0, 1.5], [0.06, -0.07, 0.06]) @ np.linalg.inv(C)


def pose_error(T, T_true):
    """(Frobenius norm of R - R_true, norm of t - t_true, angle of R R_true^T in degrees)"""
    T, T_true = np.asarray(T, dtype=np.float64), np.asarray(T_true, dtype=np.float64)
    dR = T[:3, :3] @ T_true[:3, :3].T
    cos = min(1.0, max(-1.0, (np.trace(dR) - 1.0) / 2.0))
    # (the angle from the skew part: arccos loses half the digits near 0)
    skew = np.linalg.norm([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2.0
    return (float(np.linalg.norm(T[:3, :3] - T_true[:3, :3])), float(np.linalg.norm(T[:3, 3] - T_true[:3, 3])),
            float(np.degrees(np.arctan2(skew, cos))))
