"""The numpy twin of csrc/view_consistency.hip (the rule: include/sgam_hip.h): every fp32 step is one numpy float32
operation in the written order (numpy rounds each elementwise float32 operation once, like the kernel's __f*_rn), the sums are
float64.  Written from the rule, on the CPU, with nothing of the package in it; tests/test_consistency_cpu.py checks it against
cases derived by hand, tests/test_gpu_consistency.py compares the kernel with it bit for bit."""
import math

import numpy as np

F32_MAX = np.float32(3.4028234663852886e38)
INVALID, OUT_OF_VIEW, TARGET_HOLE, OCCLUDED, VIOLATION, EDGE, COVISIBLE = range(7)
CLASSES = ("invalid", "out_of_view", "target_hole", "occluded", "violation", "edge", "covisible")
f32 = np.float32


def relative_pose(T_s, T_t):
    """(12,) fp32: the top 3 x 4 of T_t T_s^-1, float64, rounded once"""
    return (np.asarray(T_t, np.float64) @ np.linalg.inv(np.asarray(T_s, np.float64)))[:3].reshape(12).astype(f32)


def _valid(x, zn, zf):
    return (np.abs(x) <= F32_MAX) & (zn <= x) & (x <= zf)


def _lerp(p00, p01, p10, p11, wx, wy):
    top = p00 + wx * (p01 - p00)
    bot = p10 + wx * (p11 - p10)
    return top + wy * (bot - top)


def pair(depth_s, rgb_s, depth_t, rgb_t, K, T, z_near, z_far, tau):
    """one pair: (class_map (H,W) uint8, color_error (H,W) fp32, depth_error (H,W) fp32, sums (12,) float64)"""
    H, W = depth_s.shape
    K = np.asarray(K, np.float64)
    kinv = np.linalg.inv(K).astype(f32).reshape(9)
    fx, fy, cx, cy = f32(K[0, 0]), f32(K[1, 1]), f32(K[0, 2]), f32(K[1, 2])
    zn, zf, tau = f32(z_near), f32(z_far), f32(tau)
    T = np.asarray(T, f32).reshape(12)
    d = np.ascontiguousarray(depth_s, f32)
    Dt = np.ascontiguousarray(depth_t, f32)
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
        D00, D01, D10, D11 = Dt[y0, x0], Dt[y0, x0 + 1], Dt[y0 + 1, x0], Dt[y0 + 1, x0 + 1]
        right, down = wx >= f32(0.5), wy >= f32(0.5)
        Dn = np.where(down, np.where(right, D11, D10), np.where(right, D01, D00))
        e = Z - Dn
        all_ok = np.ones((H, W), bool)
        for Dk in (D00, D01, D10, D11):
            all_ok &= _valid(Dk, zn, zf) & (np.abs(Z - Dk) <= tau)
        cls = np.where(~_valid(Dn, zn, zf), TARGET_HOLE,
                       np.where(e > tau, OCCLUDED, np.where(-e > tau, VIOLATION, np.where(~all_ok, EDGE, COVISIBLE))))
        cls = np.where(in_view, cls, np.where(valid_d, OUT_OF_VIEW, INVALID)).astype(np.uint8)
        cov = cls == COVISIBLE
        ez = np.where(cov, Z - _lerp(D00, D01, D10, D11, wx, wy), f32(0)).astype(f32)
        ct = np.ascontiguousarray(rgb_t, np.uint8).astype(f32)
        ech = []
        for ch in range(3):
            got = _lerp(ct[y0, x0, ch], ct[y0, x0 + 1, ch], ct[y0 + 1, x0, ch], ct[y0 + 1, x0 + 1, ch], wx, wy)
            ech.append(np.where(cov, np.asarray(rgb_s, np.uint8)[..., ch].astype(f32) - got, f32(0)).astype(f32))
        ce = ((np.abs(ech[0]) + np.abs(ech[1])) + np.abs(ech[2])).astype(f32)
        rel = np.where(cov, np.abs(ez) / Z, f32(0)).astype(f32)
    sums = np.zeros(12, np.float64)
    for k in range(7):
        sums[k] = float((cls == k).sum())
    e64 = [ch.astype(np.float64) for ch in ech]
    sums[7] = ce.astype(np.float64).sum()
    sums[8] = ((e64[0] * e64[0] + e64[1] * e64[1]) + e64[2] * e64[2]).sum()
    sums[9] = np.abs(ez).astype(np.float64).sum()
    sums[10] = (ez.astype(np.float64) ** 2).sum()
    sums[11] = rel.astype(np.float64).sum()
    return cls, ce, ez, sums


def view_consistency(depths, rgbs, K, Ts_w2c, z_near, z_far, tau, pairs=None):
    """every pair (None: every ordered pair with s != t) -> {"pairs", "class_map" (P,H,W) uint8, "color_error", "depth_error"
    (P,H,W) fp32, "sums" (P,12) float64}; a pair that occurs twice is computed once"""
    F = len(depths)
    if pairs is None:
        pairs = [(s, t) for s in range(F) for t in range(F) if s != t]
    done = {}
    for s, t in pairs:
        if (s, t) not in done:
            done[(s, t)] = pair(depths[s], rgbs[s], depths[t], rgbs[t], K, relative_pose(Ts_w2c[s], Ts_w2c[t]), z_near, z_far, tau)
    return {"pairs": list(pairs), "class_map": np.stack([done[p][0] for p in pairs]), "color_error": np.stack([done[p][1] for p in pairs]),
            "depth_error": np.stack([done[p][2] for p in pairs]), "sums": np.stack([done[p][3] for p in pairs])}


def summary(rows):
    """the summary arithmetic of geometry.consistency_summary, restated: plain floats, NaN where a denominator is 0"""
    rows = np.asarray(rows, np.float64)
    r = [float(v) for v in (rows.sum(axis=0) if rows.ndim == 2 else rows)]
    div = lambda a, b: a / b if b > 0 else math.nan  # noqa: E731
    n_cov = r[6]
    out = {name: int(r[k]) for k, name in enumerate(CLASSES)}
    out["n_valid"] = int(r[1] + r[2] + r[3] + r[4] + r[5] + r[6])
    out["covisibility"] = div(n_cov, r[1] + r[2] + r[3] + r[4] + r[5] + r[6])
    out["violation_rate"] = div(r[4], r[3] + r[4] + r[5] + r[6])
    out["color_mae"] = div(r[7], 3.0 * n_cov)
    out["psnr"] = math.nan if not n_cov > 0 else (math.inf if r[8] == 0 else 10.0 * math.log10(255.0 ** 2 * 3.0 * n_cov / r[8]))
    out["depth_mae"] = div(r[9], n_cov)
    out["depth_rmse"] = math.sqrt(r[10] / n_cov) if n_cov > 0 else math.nan
    out["depth_rel"] = div(r[11], n_cov)
    return out
