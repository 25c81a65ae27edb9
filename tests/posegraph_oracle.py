"""numpy restatement of the pose-graph kernels (csrc/pose_graph.hip; rules in include/sgam_hip.h) for tests: the per-edge
linearisation and the assembly in the kernels' operation order (every operator one IEEE operation: the GPU results are compared
bit for bit), the fixed-order folds, and the Levenberg-Marquardt loop with numpy.linalg.cholesky for the solve and np.sin / np.cos
in the retraction.  Also the ring scenarios of tests/test_posegraph_cpu.py and tests/test_gpu_posegraph.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import icp_oracle as IO  # noqa: E402

MAX_NODES, MAX_EDGES = 1024, 65536
TAU, PIVOT_REL = 1e-5, 1e-12
STATE, ROW = 16, 8
S_LAMBDA, S_NU, S_COST, S_STATUS, S_ITER, S_ATTEMPTS, S_LIVE, S_ACCEPTED, S_TRIAL_COST, S_DENOM, S_GMAX, S_MU = range(12)


# ---------------------------------------------------------------- rigid arithmetic, vectorised over a leading axis
def inv_rigid(P):
    """P (..., 16) -> the 12 entries of rows 0..2 of the inverse [R^T | -(R^T t)]"""
    P = np.asarray(P, dtype=np.float64)
    A = [None] * 12
    A[0], A[1], A[2] = P[..., 0], P[..., 4], P[..., 8]
    A[4], A[5], A[6] = P[..., 1], P[..., 5], P[..., 9]
    A[8], A[9], A[10] = P[..., 2], P[..., 6], P[..., 10]
    A[3] = -((P[..., 0] * P[..., 3] + P[..., 4] * P[..., 7]) + P[..., 8] * P[..., 11])
    A[7] = -((P[..., 1] * P[..., 3] + P[..., 5] * P[..., 7]) + P[..., 9] * P[..., 11])
    A[11] = -((P[..., 2] * P[..., 3] + P[..., 6] * P[..., 7]) + P[..., 10] * P[..., 11])
    return A


def mul_rigid(x, y):
    Z = [None] * 12
    for r in range(3):
        for c in range(4):
            t = (x[r * 4] * y[c] + x[r * 4 + 1] * y[4 + c]) + x[r * 4 + 2] * y[8 + c]
            if c == 3:
                t = t + x[r * 4 + 3]
            Z[r * 4 + c] = t
    return Z


def dot6(m, v):
    """sum_b m(b) * v(b) in ascending b, the first product the start of the sum"""
    t = m(0) * v(0)
    for b in range(1, 6):
        t = t + m(b) * v(b)
    return t


def linearize(poses, src, dst, transforms, information, uncertain, mu):
    """-> dict of r (E,6), J (E,6,6), q, l, cost (E,), K (E,6,6), g (E,6): the kernel's expressions, one edge per row"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 16)
    src, dst = np.asarray(src), np.asarray(dst)
    T = np.asarray(transforms, dtype=np.float64).reshape(-1, 16)
    Lam = np.asarray(information, dtype=np.float64).reshape(-1, 6, 6)
    unc = np.asarray(uncertain).astype(bool)
    E = len(src)
    with np.errstate(all="ignore"):
        Ps = [poses[src, i] for i in range(16)]
        A = inv_rigid(poses[dst])
        Ti = inv_rigid(T)
        B = mul_rigid(Ps, Ti)
        M = mul_rigid(A, B)
        r = [(M[9] - M[6]) * 0.5, (M[2] - M[8]) * 0.5, (M[4] - M[1]) * 0.5, M[3], M[7], M[11]]
        zero = np.zeros(E)
        J = [[None] * 6 for _ in range(6)]
        for k in range(3):
            k1, k2 = (k + 1) % 3, (k + 2) % 3
            Q = [A[(i // 4) * 4 + k2] * B[k1 * 4 + i % 4] - A[(i // 4) * 4 + k1] * B[k2 * 4 + i % 4] for i in range(12)]
            J[0][k], J[1][k], J[2][k] = (Q[9] - Q[6]) * 0.5, (Q[2] - Q[8]) * 0.5, (Q[4] - Q[1]) * 0.5
            J[3][k], J[4][k], J[5][k] = Q[3], Q[7], Q[11]
            J[0][3 + k], J[1][3 + k], J[2][3 + k] = zero, zero, zero
            J[3][3 + k], J[4][3 + k], J[5][3 + k] = A[k], A[4 + k], A[8 + k]
        L = [[Lam[:, a, b] for b in range(6)] for a in range(6)]
        y = [dot6(lambda b: L[a][b], lambda b: r[b]) for a in range(6)]
        q = dot6(lambda b: r[b], lambda b: y[b])
        t = mu / (mu + q)
        l = np.where(unc, t * t, 1.0)
        d = np.sqrt(l) - 1.0
        cost = l * q
        cost = np.where(unc, cost + mu * (d * d), cost)
        W = [[l * L[a][b] for b in range(6)] for a in range(6)]
        wr = [dot6(lambda b: W[a][b], lambda b: r[b]) for a in range(6)]
        K = np.zeros((E, 6, 6))
        for k in range(6):
            wj = [dot6(lambda b: W[a][b], lambda b: J[b][k]) for a in range(6)]
            for j in range(6):
                K[:, j, k] = dot6(lambda b: J[b][j], lambda b: wj[b])
        g = np.stack([dot6(lambda b: J[b][j], lambda b: wr[b]) for j in range(6)], axis=1)
    return {"r": np.stack(r, axis=1), "J": np.stack([np.stack(row, axis=1) for row in J], axis=1), "q": q, "l": l, "cost": cost,
            "K": K, "g": g}


def assemble(K, g, src, dst, n_nodes, fixed):
    """-> (H (6N,6N), b (6N,)): every block summed over its edges in ascending edge index, starting from 0.0; H_ss += K, H_tt += K,
    H_st -= K, H_ts -= K^T, b_s -= g, b_t += g; the fixed node's rows and columns the identity, its b 0"""
    n = 6 * n_nodes
    H, b = np.zeros((n, n)), np.zeros(n)
    for e in range(len(src)):
        s, t = int(src[e]), int(dst[e])
        S, T = slice(6 * s, 6 * s + 6), slice(6 * t, 6 * t + 6)
        H[S, S] = H[S, S] + K[e]
        H[T, T] = H[T, T] + K[e]
        # the block (lo, hi) is summed and mirrored into (hi, lo): H_st -= K for s < t, H_ts -= K^T read as block (t, s) for t < s
        if s < t:
            H[S, T] = H[S, T] - K[e]
            H[T, S] = H[S, T].T
        else:
            H[T, S] = H[T, S] - K[e].T
            H[S, T] = H[T, S].T
        b[S] = b[S] - g[e]
        b[T] = b[T] + g[e]
    F = slice(6 * fixed, 6 * fixed + 6)
    H[F, :], H[:, F], b[F] = 0.0, 0.0, 0.0
    H[F, F] = np.eye(6)
    return H, b


def fold(values):
    """the workgroup fold: lane t of 256 takes the items t, t + 256, ... in ascending order, then s[t] = s[t] + s[t + h] for
    h = 128, 64, ..., 1"""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    lanes = np.zeros(256)
    for c in range(0, len(v), 256):
        chunk = v[c:c + 256]
        lanes[:len(chunk)] = lanes[:len(chunk)] + chunk
    h = 128
    while h > 0:
        lanes[:h] = lanes[:h] + lanes[h:2 * h]
        h //= 2
    return float(lanes[0])


def retract(poses, delta):
    """P'_i = [dR(omega_i) | v_i] P_i with rule 6 of the ICP update"""
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    out = P.copy()
    for i, x in enumerate(np.asarray(delta).reshape(-1, 6)):
        dT = np.eye(4)
        dT[:3, :3], dT[:3, 3] = IO.rodrigues(x[:3]), x[3:]
        out[i, :3] = (dT @ P[i])[:3]
    return out


def default_mu(information, uncertain, max_correspondence_distance, preference_loop_closure=2.0):
    Lam = np.asarray(information, dtype=np.float64).reshape(-1, 6, 6)
    unc = np.asarray(uncertain).astype(bool)
    if not unc.any():
        return 1.0
    return float(preference_loop_closure * max_correspondence_distance ** 2 * Lam[unc, 5, 5].mean())


def run(poses, src, dst, transforms, information, uncertain, mu, fixed=0, max_iterations=100, gradient_tolerance=1e-6,
        relative_cost=1e-12, solve=None):
    """one Levenberg-Marquardt run -> dict(poses (N,4,4), l, state (16,), history (max_iterations, 8), H, b: the last assembled)"""
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4).copy()
    N, E = len(P), len(src)
    n = 6 * N
    state, history = np.zeros(STATE), np.zeros((max_iterations, ROW))
    state[S_MU] = mu
    lin = linearize(P, src, dst, transforms, information, uncertain, mu)
    H, b = assemble(lin["K"], lin["g"], src, dst, N, fixed)
    l = lin["l"].copy()
    state[S_COST] = fold(lin["cost"])
    free = np.arange(n) // 6 != fixed
    state[S_LAMBDA] = TAU * max(0.0, float(np.diag(H)[free].max())) if free.any() else 0.0
    state[S_NU] = 2.0
    for k in range(max_iterations):
        F, lam, nu = state[S_COST], state[S_LAMBDA], state[S_NU]
        if state[S_STATUS] != 0.0:
            history[k] = [F, lam, 0, 0, 0, 0, state[S_STATUS], nu]
            continue
        gmax = float(np.abs(b).max())
        state[S_GMAX] = gmax
        if gmax < gradient_tolerance:
            state[S_STATUS] = 1.0
            history[k] = [F, lam, 0, gmax, 0, 0, 1.0, nu]
            continue
        state[S_ATTEMPTS] += 1.0
        delta = (solve or cholesky_solve)(H, lam, b)
        if delta is None:
            state[S_STATUS] = 2.0
            history[k] = [F, lam, 0, gmax, 0, 0, 2.0, nu]
            continue
        Pt = retract(P, delta)
        lt = linearize(Pt, src, dst, transforms, information, uncertain, mu)
        Ft = fold(lt["cost"])
        den = fold(delta * (lam * delta + b))
        rho, status, accept = 0.0, 0.0, False
        if np.isfinite(den) and den > 0.0:
            rho = (F - Ft) / den
            accept = bool(rho > 0.0)
        if accept:
            s = 2.0 * rho - 1.0
            lam_n, nu_n = lam * max(1.0 / 3.0, 1.0 - (s * s) * s), 2.0
            state[S_ITER] += 1.0
            if F - Ft <= relative_cost * F:
                status = 1.0
            P, l, Fn = Pt, lt["l"].copy(), Ft
            H, b = assemble(lt["K"], lt["g"], src, dst, N, fixed)
        elif abs(F - Ft) <= relative_cost * F:
            lam_n, nu_n, Fn, status = lam, nu, F, 1.0
        else:
            lam_n, nu_n, Fn = lam * nu, 2.0 * nu, F
            if not np.isfinite(lam_n):
                status = 2.0
        state[S_COST], state[S_LAMBDA], state[S_NU], state[S_STATUS] = Fn, lam_n, nu_n, status
        history[k] = [Fn, lam_n, rho, gmax, float(accept), Ft, status, nu_n]
    return {"poses": P, "l": l, "state": state, "history": history, "H": H, "b": b}


def cholesky_solve(H, lam, b):
    """(H + lam I) x = b from the lower triangle by numpy.linalg.cholesky; None where a pivot fails the kernel's rule (judged on
    the finished factor: L_jj^2 against the damped diagonal entry) or numpy refuses the matrix"""
    A = np.tril(H) + np.tril(H, -1).T + lam * np.eye(len(b))
    if not np.isfinite(A).all():
        return None
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    if (np.diag(L) ** 2 <= PIVOT_REL * np.diag(A)).any():
        return None
    y = np.linalg.solve(L, b)
    return np.linalg.solve(L.T, y)


def optimize(n_nodes, src, dst, transforms, information, uncertain, mu, fixed=0, max_iterations=100, edge_prune_threshold=0.25,
             reoptimize=True, poses=None, gradient_tolerance=1e-6, relative_cost=1e-12):
    """geometry.optimize_pose_graph: the run, the pruning, the second run on the kept edges from the first run's poses"""
    src, dst, unc = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64), np.asarray(uncertain).astype(bool)
    T, Lam = np.asarray(transforms, dtype=np.float64).reshape(-1, 4, 4), np.asarray(information, dtype=np.float64).reshape(-1, 6, 6)
    P0 = np.tile(np.eye(4), (n_nodes, 1, 1)) if poses is None else np.asarray(poses, dtype=np.float64).reshape(n_nodes, 4, 4)
    if len(src) == 0:
        return {"poses": P0, "line_weights": np.zeros(0), "kept": np.zeros(0, bool), "history": np.zeros((0, ROW)), "history_second": None,
                "status": 1, "iterations": 0, "cost": 0.0, "converged": True}
    first = run(P0, src, dst, T, Lam, unc, mu, fixed, max_iterations, gradient_tolerance, relative_cost)
    kept = ~(unc & (first["l"] < edge_prune_threshold))
    out, second = first, None
    if reoptimize and kept.any() and not kept.all():
        second = run(first["poses"], src[kept], dst[kept], T[kept], Lam[kept], unc[kept], mu, fixed, max_iterations, gradient_tolerance,
                     relative_cost)
        out = second
    st = out["state"]
    return {"poses": out["poses"], "line_weights": first["l"], "kept": kept, "history": first["history"],
            "history_second": None if second is None else second["history"], "status": int(st[S_STATUS]),
            "iterations": int(first["state"][S_ITER]) + (0 if second is None else int(second["state"][S_ITER])),
            "cost": float(st[S_COST]), "converged": int(st[S_STATUS]) == 1}


# ---------------------------------------------------------------- the test scenarios
def random_pose(rng, angle, shift):
    """a rigid 4x4 with rotation angle `angle` (radians) about a random axis and a translation of length `shift`"""
    a, t = rng.normal(size=3), rng.normal(size=3)
    T = np.eye(4)
    T[:3, :3] = IO.rodrigues(angle * a / np.linalg.norm(a))
    T[:3, 3] = shift * t / np.linalg.norm(t)
    return T


INFORMATION = 10.0 * np.diag([50.0, 60.0, 70.0, 100.0, 100.0, 100.0])


def ring(n_nodes, seed, stride=3, noise=0.0, certain_closures=False):
    """true poses P_i (node 0 the identity) on a loop, the odometry edges (i, i+1) and the loop closures (i, i + stride) with the
    measurements T_st = P_t^-1 P_s (the model's zero-residual registration), optionally perturbed on the left by `noise`
    (radians / length units, normal).  -> (truth (N,4,4), src, dst, T (E,4,4), information (E,6,6), uncertain (E,))"""
    rng = np.random.default_rng(seed)
    truth = [np.eye(4)]
    for i in range(1, n_nodes):
        truth.append(random_pose(rng, rng.uniform(0.05, 0.4), rng.uniform(0.1, 0.5)) @ truth[-1])
    truth = np.array(truth)
    pairs = [(i, i + 1, False) for i in range(n_nodes - 1)]
    if n_nodes > 2:
        pairs.append((n_nodes - 1, 0, not certain_closures))
    if stride > 1:
        pairs += [(i, i + stride, not certain_closures) for i in range(0, n_nodes - stride, 2)]
    src, dst, unc = (np.array([p[k] for p in pairs]) for k in range(3))
    T = np.array([np.linalg.inv(truth[t]) @ truth[s] for s, t in zip(src, dst)])
    if noise:
        for e in range(len(T)):
            x = rng.normal(size=6) * noise
            dT = np.eye(4)
            dT[:3, :3], dT[:3, 3] = IO.rodrigues(x[:3]), x[3:]
            T[e] = dT @ T[e]
    info = np.tile(INFORMATION, (len(src), 1, 1))
    return truth, src.astype(np.int64), dst.astype(np.int64), T, info, unc.astype(bool)


def perturbed(truth, seed, angle=0.15, shift=0.3, fixed=0):
    """the initial guess of the convergence scenarios: every pose but the fixed one moved by `angle` rad / `shift`"""
    rng = np.random.default_rng(seed)
    out = truth.copy()
    for i in range(len(out)):
        if i != fixed:
            out[i] = random_pose(rng, angle, shift) @ truth[i]
    return out


def residual_numeric(poses, s, t, T):
    """vee(P_t^-1 P_s T^-1) with numpy's own inverses: the model, not the kernel's expressions"""
    M = np.linalg.inv(poses[t]) @ poses[s] @ np.linalg.inv(T)
    return np.array([(M[2, 1] - M[1, 2]) / 2, (M[0, 2] - M[2, 0]) / 2, (M[1, 0] - M[0, 1]) / 2, M[0, 3], M[1, 3], M[2, 3]])


def se3_exp(x):
    """exp of a twist (omega, v) as a 4x4: scipy-free series-exact closed form"""
    w, v = np.asarray(x[:3], dtype=np.float64), np.asarray(x[3:], dtype=np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    T = np.eye(4)
    if th < 1e-12:
        T[:3, :3], T[:3, 3] = np.eye(3) + K, v
        return T
    T[:3, :3] = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K
    T[:3, 3] = V @ v
    return T


# ---------------------------------------------------------------- the multiway registration scenario
WINDOW_STRIPS, STRIP_WIDTH, STRIP_GAP = 4, 0.2375, 0.3


def windows(n_windows=5, samples=17000, seed=21):
    """Overlapping windows of the ICP tests' surface, each moved by a known motion.  The square [0, 4]^2 is cut into strips in x
    (0.2375 wide, 0.3 apart) over 1 <= y <= 3; window i is the strips i .. i + 3, about 2000 points, so windows i and j share
    4 - |i - j| strips: the SAME samples, exact copies of each other, while the strips they do not share lie a gap away from
    every point of the other window (beyond the correspondence distance, whatever the motions below do to them).  Window i > 0 is
    moved by D_i, 1 to 2 degrees about its centre and 0.02 along a random direction.
    -> (clouds [(n_i,3) fp32], normals [(n_i,3) fp32], motions (n_windows,4,4))"""
    pts, nrm = IO.surface(samples, seed)
    rng = np.random.default_rng(seed)
    pitch = STRIP_WIDTH + STRIP_GAP
    strip = np.floor(pts[:, 0].astype(np.float64) / pitch).astype(int)
    inside = (pts[:, 0] - strip * pitch < STRIP_WIDTH) & (pts[:, 1] >= 1.0) & (pts[:, 1] <= 3.0)
    clouds, normals, motions = [], [], []
    for i in range(n_windows):
        m = inside & (strip >= i) & (strip < i + WINDOW_STRIPS)
        D = np.eye(4)
        if i:
            C = np.eye(4)
            C[:3, 3] = pts[m].astype(np.float64).mean(0)
            t = rng.normal(size=3)
            D = C @ IO.rigid(rng.uniform(1.0, 2.0), rng.normal(size=3), 0.02 * t / np.linalg.norm(t)) @ np.linalg.inv(C)
        clouds.append(IO.transform(pts[m], D))
        normals.append((nrm[m].astype(np.float64) @ D[:3, :3].T).astype(IO.f32))
        motions.append(D)
    return clouds, normals, np.array(motions)


def information(source, target, max_distance, T):
    """geometry.registration_information in numpy: slots 0..20 of the point-to-point sums at T, mirrored"""
    moved = IO.transform(source, T)
    d2, index = IO.search(moved, target, max_distance)
    total = np.zeros(IO.SLOTS)
    for row in IO.accumulate(moved, target, None, index, d2)[0]:
        total = total + row
    return IO.matrices(total)[0]
