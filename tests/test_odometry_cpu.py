"""CPU: the numpy twin of direct RGB-D odometry (tests/odometry_oracle.py; the rule: include/sgam_hip.h) against
cases derived by hand, its Jacobian against central differences of a float64 restatement of the residuals, its convergence to a
known motion on analytically rendered frames (whose final errors, measured here, are the constants the GPU tests hold the kernels
to), the pyramid, the level transition, the information matrix, multiway registration on the twins, and every refusal of the C
entries and of the Python fronts that needs no GPU."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import _lib, geometry
from sgam_neurips22_amd.ops import SgamHipError

sys.path.insert(0, os.path.dirname(__file__))
import icp_oracle as IO  # noqa: E402
import odometry_oracle as OO  # noqa: E402

f32 = np.float32
Z_RANGE, TAU = (0.05, 4.8), 0.1
HAND_Z, HAND_TAU = (1.0, 4.0), 0.05

# The final errors (degrees, distance) of the TWIN on the analytic scenes from the identity to exp(OO.TRUE_XI) — a start 3.09 degrees
# and 0.187 away — measured by test_convergence_to_the_truth below and written down.  What is left is the model error of uint8
# colours and of the bilinear interpolant of a curved image, not rounding: it does not shrink with precision, and it is not the same
# number on another libm.  FACTOR = 2 on top of the measured value is the room given to that, here and for the kernels
# (tests/test_gpu_odometry.py: these constants * FACTOR + 1e-9).
FACTOR = 2.0
CASES = {("plane", 64, 64): (20, 10, 5), ("paraboloid", 64, 64): (20, 10, 5), ("plane", 33, 64): (20, 10, 5),
         ("paraboloid", 33, 64): (20, 10, 5), ("plane", 17, 19): (20, 10), ("paraboloid", 17, 19): (20, 10)}
MEASURED = {("plane", 64, 64): (0.00897, 7.64e-5), ("paraboloid", 64, 64): (0.01571, 1.283e-3), ("plane", 33, 64): (0.00408, 3.49e-4),
            ("paraboloid", 33, 64): (0.02271, 1.040e-3), ("plane", 17, 19): (0.00670, 2.873e-3), ("paraboloid", 17, 19): (0.10063, 3.637e-3)}


@functools.lru_cache(maxsize=None)
def analytic(surface, H, W):
    return OO.scene_pair(surface, H, W)


@functools.lru_cache(maxsize=None)
def twin_result(surface, H, W):
    d, c, K, T = analytic(surface, H, W)
    return OO.odometry(d, c, K, [(0, 1)], *Z_RANGE, TAU, iterations=CASES[(surface, H, W)])


# ---------------------------------------------------------------- the hand case
def test_hand_case_is_exact_and_degenerate():
    depth, grey, K = OO.hand_case()
    I = OO.intensity0(grey)
    assert np.array_equal(I, np.broadcast_to((12 * np.arange(16)).astype(f32) / f32(765), (8, 16)))
    part, _ = OO.accumulate(I, depth, I, depth, K, np.eye(4), *HAND_Z, HAND_TAU)
    total = OO.fold(part)
    assert part.shape == (1, 32)
    assert total[29] == 7 * 15 == 105 and total[30] == 128 and total[31] == 0
    assert not total[21:29].any()                                  # J^T r, sum r^2 and the depth error: exactly 0
    A = OO.information_matrix(total)
    assert A[4, 4] == 0.0                                          # a ramp along x on a fronto-parallel plane leaves v_y free
    assert A[3, 3] > 0 and A[5, 5] > 0
    state, row = OO.update(part, True, 1e-6, 1e-6, IO.new_state())
    assert state[18] == 2.0 and np.array_equal(state[:16], np.eye(4).reshape(16)) and state[19] == 0
    assert row[0] == 105 / 128 and row[1] == 0.0 and row[2] == 105 and row[6] == 2.0


# ---------------------------------------------------------------- the Jacobian
def _residuals64(xi, T, K, i, j, d, Is, It, Dt, x0, y0, lam):
    """(r_I, r_Z) of one source pixel under exp(xi) T, all in float64: the function the rule differentiates, the cell (x0, y0) held"""
    p = d * (np.linalg.inv(K) @ np.array([j, i, 1.0]))
    q = (OO.se3_exp(xi) @ T @ np.r_[p, 1.0])[:3]
    u, v = K[0, 0] * q[0] / q[2] + K[0, 2], K[1, 1] * q[1] / q[2] + K[1, 2]
    wx, wy = u - x0, v - y0

    def lerp(c):
        top = c[y0, x0] + wx * (c[y0, x0 + 1] - c[y0, x0])
        bot = c[y0 + 1, x0] + wx * (c[y0 + 1, x0 + 1] - c[y0 + 1, x0])
        return top + wy * (bot - top)
    return np.sqrt(1 - lam) * (Is[i, j] - lerp(It)), np.sqrt(lam) * (q[2] - lerp(Dt))


def test_jacobian_rows_against_central_differences():
    H, W, lam = 33, 64, 0.7
    d, c, K, T_true = analytic("paraboloid", H, W)
    T = OO.se3_exp(0.6 * OO.TRUE_XI)                                  # (not at the solution: the residuals are not small)
    Is, It = (OO.intensity0(x) for x in c)
    g, JI, rI, JZ, rZ, _ = OO.rows(Is, d[0], It, d[1], K, T, *Z_RANGE, TAU, lam)
    inner = g["cov"] & (g["wx"] > 0.15) & (g["wx"] < 0.85) & (g["wy"] > 0.15) & (g["wy"] < 0.85)
    picks = np.flatnonzero(inner)[::37]
    assert len(picks) >= 20
    I64, D64, Is64 = It.astype(np.float64), d[1].astype(np.float64), Is.astype(np.float64)
    h, worst = 2e-4, 0.0
    for q in picks:
        i, j = divmod(int(q), W)
        args = (T, K, i, j, float(d[0][i, j]), Is64, I64, D64, int(g["x0"][q]), int(g["y0"][q]), lam)
        r0 = _residuals64(np.zeros(6), *args)
        # the twin's residuals are those of fp32 geometry: u, v carry a few 2^-24 of |u| <= 64, times the gradient
        assert abs(r0[0] - rI[q]) <= 1e-4 and abs(r0[1] - rZ[q]) <= 1e-5
        for a in range(6):
            e = np.zeros(6)
            e[a] = 1.0
            full = [(np.array(_residuals64(s * e, *args)) - np.array(_residuals64(-s * e, *args))) / (2 * s) for s in (h, h / 2)]
            for k, J in enumerate((JI, JZ)):
                # A central difference with step s is off by s^2 f''' / 6: the two steps differ by three quarters of the coarser one's
                # error, so the finer one is within a third of their difference; its rounding is 2^-52 |r| / s.  The twin's J is
                # formed from fp32 X, Y, Z, wx, wy: 2^-23 relative of the row's own scale (its largest entry), with the weights wx,
                # wy carrying the absolute rounding of u, v (2^-24 * 64) against cell differences.
                scale = max(abs(J[b][q]) for b in range(6))
                tol = abs(full[0][k] - full[1][k]) + 2.0 ** -52 * 4 * (abs(r0[k]) + 1) / (h / 2) + 64 * 2.0 ** -23 * (scale + 1)
                err = abs(J[a][q] - full[1][k])
                worst = max(worst, err / tol)
                assert err <= tol, (q, a, k, J[a][q], full[1][k], tol)
    print(f"Jacobian against central differences: {len(picks)} pixels, largest error / tolerance {worst:.3g}")


# ---------------------------------------------------------------- convergence
@pytest.mark.parametrize("case", sorted(CASES))
def test_convergence_to_the_truth(case):
    surface, H, W = case
    T = analytic(surface, H, W)[3]
    res = twin_result(surface, H, W)
    start, end = OO.pose_error(np.eye(4), T), OO.pose_error(res["transformation"][0], T)
    print(f"{surface} {H}x{W}: from {start[0]:.4g} deg / {start[1]:.4g} to {end[0]:.6g} deg / {end[1]:.6g}; status {res['status'][0]}, "
          f"{int(res['iterations'][0])} steps, fitness {res['fitness'][0]:.4f}, depth rmse {res['rmse'][0]:.3g}")
    assert res["status"][0] != 2.0 and not (res["history"][0][:, 6] == 2.0).any()
    assert end[0] <= FACTOR * MEASURED[case][0] and end[1] <= FACTOR * MEASURED[case][1]
    assert end[0] < start[0] / 25 and end[1] < start[1] / 25
    # the measured constants are the twin's own: not stale by more than their last digit
    assert end[0] >= MEASURED[case][0] / FACTOR and end[1] >= MEASURED[case][1] / FACTOR


def test_convergence_from_three_times_the_motion():
    for surface in ("plane", "paraboloid"):
        d, c, K, T = OO.scene_pair(surface, 64, 64, xi=3 * OO.TRUE_XI)
        res = OO.odometry(d, c, K, [(0, 1)], *Z_RANGE, TAU, iterations=(20, 10, 5))
        start, end = OO.pose_error(np.eye(4), T), OO.pose_error(res["transformation"][0], T)
        print(f"{surface} 64x64, three times the motion: from {start[0]:.4g} deg / {start[1]:.4g} to {end[0]:.6g} deg / {end[1]:.6g}")
        assert res["status"][0] != 2.0 and end[0] < start[0] / 25 and end[1] < start[1] / 25


# ---------------------------------------------------------------- pyramid
def test_pyramid():
    rs = np.random.RandomState(3)
    # a constant image stays constant (the weights sum to 16, every partial sum of a dyadic constant is exact)
    const = np.full((9, 13, 3), 85, np.uint8)                          # I = 255 / 765 = 1/3 rounded: h = 4 I, sum = 16 I, exact
    depth = rs.uniform(1, 3, (9, 13)).astype(f32)
    depth[2, 4], depth[4, 8], depth[0, 0], depth[8, 12] = np.nan, np.inf, -np.inf, 0.0
    pyr = OO.pyramid([depth], [const], 3)
    assert [p[0].shape for p in pyr] == [(1, 9, 13), (1, 5, 7), (1, 3, 4)] == [(1, h, w) for h, w in OO.level_sizes(9, 13, 3)]
    for I, _ in pyr:
        assert (I == pyr[0][0][0, 0, 0]).all()
    # depth is pure subsampling, NaN and inf included
    assert pyr[1][1].tobytes() == depth[::2, ::2].tobytes() and pyr[2][1].tobytes() == depth[::4, ::4].tobytes()
    assert np.isnan(pyr[1][1][0, 1, 2]) and np.isinf(pyr[2][1][0, 1, 2]) and pyr[2][1][0, 2, 3] == 0.0
    # a dyadic ramp stays the ramp of the coarser grid away from the clamped border: I(i, j) = (3 j + 6 i) / 1024
    ii, jj = np.meshgrid(np.arange(12), np.arange(16), indexing="ij")
    ramp = ((3 * jj + 6 * ii) / 1024.0).astype(f32)
    down, _ = OO.down(ramp, ramp)
    want = ((3 * 2 * jj[:6, :8] + 6 * 2 * ii[:6, :8]) / 1024.0).astype(f32)
    assert np.array_equal(down[1:, 1:], want[1:, 1:]) and down.shape == (6, 8)
    assert down[0, 0] != want[0, 0]                                    # (the clamped corner is not the ramp)
    # level intrinsics halve exactly
    K = OO.camera(33, 64)
    assert np.array_equal(OO.level_K(K, 2)[:2], K[:2] / 4) and np.array_equal(OO.level_K(K, 2)[2], K[2])
    assert np.array_equal(geometry.level_intrinsics(K, 2), OO.level_K(K, 2))
    with pytest.raises(ValueError):
        OO.pyramid([depth[:3, :3]], [const[:3, :3]], 3)                # 3x3 -> 2x2 -> 1x1


# ---------------------------------------------------------------- update across levels
def test_level_transition_clears_converged_but_not_degenerate():
    d, c, K, T = analytic("plane", 17, 19)
    pyr = OO.pyramid(d, c, 2)
    part = OO.accumulate(pyr[1][0][0], pyr[1][1][0], pyr[1][0][1], pyr[1][1][1], OO.level_K(K, 1), np.eye(4), *Z_RANGE, TAU)[0]
    s0, _ = OO.update(part, True, 1e-6, 1e-6, IO.new_state())
    assert s0[18] == 0.0 and s0[19] == 1.0
    # the same sums again with criteria nothing can miss: converged, frozen for the rest of the level
    s1, row = OO.update(part, False, 1e9, 1e9, s0)
    assert s1[18] == 1.0 and s1[19] == 1.0 and row[6] == 1.0
    s2, row = OO.update(part, False, 1e9, 1e9, s1)
    assert np.array_equal(s2, s1) and row[6] == 1.0 and row[4] == row[5] == 0.0
    # the next level's first iteration clears it, skips the stop test (the criteria would stop it) and steps
    s3, row = OO.update(part, True, 1e9, 1e9, s1)
    assert s3[18] == 0.0 and s3[19] == 2.0 and row[6] == 0.0 and not np.array_equal(s3[:16], s1[:16])
    # status 2 is final
    dead = s1.copy()
    dead[18] = 2.0
    s4, row = OO.update(part, True, 1e9, 1e9, dead)
    assert np.array_equal(s4, dead) and row[6] == 2.0
    # in the loop: a pair that converges on the coarse level still moves on the fine one
    res = OO.odometry(d, c, K, [(0, 1)], *Z_RANGE, TAU, iterations=(20, 10), relative_fitness=1e-2, relative_rmse=1e-2)
    h = res["history"][0]
    assert (h[:20, 6] == 1.0).any() and h[20, 6] == 0.0 and h[20, 4] > 0.0


# ---------------------------------------------------------------- information
def test_information_is_the_point_to_point_sum():
    depth, grey, K = OO.hand_case()
    I = OO.intensity0(grey)
    part, _ = OO.accumulate(I, depth, I, depth, K, np.eye(4), *HAND_Z, HAND_TAU, information=True)
    total = OO.fold(part)
    # the direct sum: the covisible pixels are rows 0..6, columns 0..14; p = 2 * ((j - 8) / 16, (i - 4) / 16, 1), exact in fp32
    want = np.zeros((6, 6))
    for i in range(7):
        for j in range(15):
            p = np.array([(j - 8) / 8.0, (i - 4) / 8.0, 2.0])
            G = np.hstack([-np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]]), np.eye(3)])
            want += G.T @ G
    A = OO.information_matrix(total)
    assert np.array_equal(A, want) and A[5, 5] == total[29] == 105 and not total[21:29].any() and total[30] == 128
    # a frame moves q: a translation by (1, 0, 0) changes the rotational block and leaves the count
    Fr = np.eye(4)
    Fr[0, 3] = 1.0
    moved = OO.information_matrix(OO.fold(OO.accumulate(I, depth, I, depth, K, np.eye(4), *HAND_Z, HAND_TAU, information=True,
                                                        frame=Fr[:3].reshape(12))[0]))
    assert moved[5, 5] == 105 and moved[1, 5] == A[1, 5] - 105 and not np.array_equal(moved, A)
    # the twin's loop returns it per pair
    res = OO.odometry([depth, depth], [grey, grey], K, [(0, 1)], *HAND_Z, HAND_TAU, iterations=(1,))
    assert res["status"][0] == 2.0 and np.array_equal(res["information"][0], A)


# ---------------------------------------------------------------- multiway registration on the twins
@functools.lru_cache(maxsize=None)
def five_frames():
    """five frames of the paraboloid along a small motion; the nominal pose of frame 2 is wrong by a known motion"""
    H, W = 33, 64
    K = OO.camera(H, W)
    true = [OO.se3_exp(0.35 * k * OO.TRUE_XI) for k in range(5)]
    frames = [OO.render("paraboloid", T, K, H, W) for T in true]
    wrong = OO.se3_exp(0.4 * OO.TRUE_XI[[1, 2, 0, 4, 5, 3]])
    nominal = [T.copy() for T in true]
    nominal[2] = wrong @ true[2]
    return [f[0] for f in frames], [f[1] for f in frames], K, np.stack(true), np.stack(nominal)


def test_multiway_rgbd_on_the_twin_recovers_a_wrong_pose_and_prunes_a_wrong_closure():
    depths, rgbs, K, true, nominal = five_frames()
    bad = np.linalg.inv(nominal[4]) @ OO.se3_exp([0.2, 0.1, -0.15, 0.4, -0.3, 0.35]) @ nominal[0]
    out = OO.multiway(depths, rgbs, K, nominal, *Z_RANGE, TAU, stride=3, extra_edges=[(0, 4, bad)])
    edges = out["edges"]
    assert [e[:2] for e in edges] == [(0, 1), (1, 2), (2, 3), (3, 4), (0, 3), (1, 4), (0, 4)] and out["missing_odometry"] == []
    assert [e[2] for e in edges] == [False] * 4 + [True] * 3
    assert out["kept"].tolist() == [True] * 6 + [False], out["line_weights"]
    # corrected pose T'_i P_i^-1 against the truth; P_i = true_i^-1 nominal_i up to what the odometry leaves, summed along the chain
    rot, trans = MEASURED[("paraboloid", 33, 64)]
    chain = 4
    for i in range(5):
        err = OO.pose_error(nominal[i] @ np.linalg.inv(out["poses"][i]), true[i])
        before = OO.pose_error(nominal[i], true[i])
        print(f"frame {i}: pose off by {before[0]:.4g} deg / {before[1]:.4g} before, {err[0]:.4g} deg / {err[1]:.4g} after")
        assert err[0] <= FACTOR * rot * chain and err[1] <= FACTOR * trans * chain
    assert OO.pose_error(nominal[2], true[2])[1] > 5 * FACTOR * trans * chain          # (the wrong pose was far outside that bound)


# ---------------------------------------------------------------- refusals without a GPU
def test_c_entries_refuse_without_launching():
    lib = _lib.load()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    kinv = (ctypes.c_float * 9)()
    EINVAL = -1
    assert lib.sgam_rgbd_odometry_workspace_bytes(16, 16, 3) == 3 * 1 * 32 * 8
    assert lib.sgam_rgbd_odometry_workspace_bytes(33, 64, 2) == 2 * 3 * 32 * 8
    for H, W, P in ((1, 16, 1), (16, 1, 1), (16, 16, 0), (16, 16, 65536)):
        assert lib.sgam_rgbd_odometry_workspace_bytes(H, W, P) == EINVAL
    pyr = lambda *a: lib.sgam_rgbd_pyramid_f32(*a, None)  # noqa: E731
    assert pyr(None, p, 1, 8, 8, 1, p, p) == pyr(p, None, 1, 8, 8, 1, p, p) == pyr(p, p, 1, 8, 8, 1, None, p) == pyr(p, p, 1, 8, 8, 1, p, None) == EINVAL
    assert pyr(p, p, 0, 8, 8, 1, p, p) == pyr(p, p, 1, 1, 8, 1, p, p) == pyr(p, p, 1, 8, 1, 1, p, p) == EINVAL
    assert pyr(p, p, 1, 8, 8, 0, p, p) == pyr(p, p, 1, 8, 8, 5, p, p) == EINVAL
    assert pyr(p, p, 1, 5, 8, 4, p, p) == EINVAL                     # 5 -> 3 -> 2 -> 1: a level smaller than 2 x 2
    good = dict(depth=p, inten=p, F=2, H=8, W=8, kinv=ctypes.cast(kinv, ctypes.c_void_p), zn=0.5, zf=4.0, tau=0.1, lam=0.968, pairs=p,
                state=p, P=1, first=1, info=0, frames=None, ws=p, bytes=4096 * 8)

    def acc(**kw):
        a = dict(good, **kw)
        return lib.sgam_rgbd_odometry_accumulate_f32(a["depth"], a["inten"], a["F"], a["H"], a["W"], a["kinv"], 8.0, 8.0, 4.0, 4.0, a["zn"], a["zf"],
                                                     a["tau"], a["lam"], a["pairs"], a["state"], a["P"], a["first"], a["info"], a["frames"],
                                                     a["ws"], a["bytes"], None)
    nan = float("nan")
    for bad in (dict(depth=None), dict(inten=None), dict(kinv=None), dict(pairs=None), dict(state=None), dict(ws=None), dict(F=0), dict(H=1),
                dict(W=1), dict(P=0), dict(P=65536), dict(tau=-0.1), dict(tau=nan), dict(lam=-0.1), dict(lam=1.5), dict(lam=nan),
                dict(zn=5.0), dict(zn=nan), dict(zf=nan), dict(bytes=255), dict(ws=ctypes.c_void_p(p.value + 8)), dict(frames=p)):
        assert acc(**bad) == EINVAL, bad

    def upd(ws=p, nbytes=4096 * 8, H=8, W=8, P=1, row=0, rows=4, rf=1e-6, rr=1e-6, state=p, history=p, sums=None):
        return lib.sgam_rgbd_odometry_update(ws, nbytes, H, W, P, row, rows, 1, rf, rr, state, history, sums, None)
    for bad in (dict(ws=None), dict(nbytes=255), dict(H=1), dict(W=1), dict(P=0), dict(P=65536), dict(row=4), dict(row=-2), dict(rf=-1.0),
                dict(rf=nan), dict(rr=-1.0), dict(rr=nan), dict(state=None), dict(history=None), dict(row=-1, sums=None)):
        assert upd(**bad) == EINVAL, bad


def test_python_fronts_refuse_without_a_gpu():
    d = [torch.zeros((8, 8)), torch.zeros((8, 8))]
    c = [torch.zeros((8, 8, 3), dtype=torch.uint8)] * 2
    K = OO.camera(8, 8)
    ok = dict(pairs=[(0, 1)], z_near=0.5, z_far=4.0, max_depth_diff=0.1)
    odo = lambda **kw: geometry.rgbd_odometry(d, c, kw.pop("K", K), **dict(ok, **kw))  # noqa: E731
    for kw, match in ((dict(max_depth_diff=-1.0), "max_depth_diff"), (dict(max_depth_diff=float("nan")), "max_depth_diff"),
                      (dict(z_near=5.0), "z_near"), (dict(K=np.eye(4)), "3x3"), (dict(iterations=()), "iterations"),
                      (dict(iterations=(1, 1, 1, 1, 1)), "iterations"), (dict(iterations=5), "iterations"), (dict(iterations=(3, 0)), "iterations"),
                      (dict(iterations=(3, 2.5)), "iterations"), (dict(lambda_geometric=1.5), "lambda_geometric"),
                      (dict(lambda_geometric=-0.1), "lambda_geometric"), (dict(relative_fitness=-1.0), "relative"),
                      (dict(pairs=[]), "no pairs"), (dict(pairs=[(0, 2)]), "target"), (dict(pairs=[(-1, 0)]), "source"), (dict(pairs=[(0, 1, 2)]), "pairs"),
                      (dict(init=np.eye(4)), "init"), (dict(init=np.full((1, 4, 4), np.nan)), "init"),
                      (dict(information_frames=np.eye(4)[None], information=False), "information_frames"),
                      (dict(information_frames=np.zeros((2, 4, 4))), "information_frames"), (dict(_max_pairs=0), "_max_pairs")):
        with pytest.raises(ValueError, match=match):
            odo(**kw)
    with pytest.raises(SgamHipError):                                  # everything else is in order: the frames are not on the device
        odo()
    for levels in (0, 5, 2.0):
        with pytest.raises(ValueError, match="levels"):
            geometry.rgbd_pyramid(d, c, K, levels)
    with pytest.raises(ValueError, match="2 x 2"):
        geometry.rgbd_pyramid(d, c, K, 4)                              # 8 -> 4 -> 2 -> 1
    with pytest.raises(ValueError, match="3x3"):
        geometry.rgbd_pyramid(d, c, np.eye(2), 1)
    with pytest.raises(SgamHipError):
        geometry.rgbd_pyramid(d, c, K, 2)
    Ts = np.stack([np.eye(4)] * 2)
    mw = lambda **kw: geometry.multiway_rgbd(d, c, K, kw.pop("Ts", Ts), 0.5, 4.0, kw.pop("tau", 0.1), **kw)  # noqa: E731
    for kw, match in ((dict(tau=0.0), "max_depth_diff"), (dict(min_covisibility=1.5), "min_covisibility"), (dict(loop_closure_stride=0), "stride"),
                      (dict(Ts=np.eye(4)), "Ts_w2c"), (dict(iterations=()), "iterations"), (dict(lambda_geometric=2.0), "lambda_geometric")):
        with pytest.raises(ValueError, match=match):
            mw(**kw)
    with pytest.raises(SgamHipError):
        mw()
    assert geometry.rgbd_odometry.__defaults__[3:5] == geometry.register_icp.__defaults__[4:6] == (1e-6, 1e-6)
    assert geometry.LAMBDA_GEOMETRIC == OO.LAMBDA_GEOMETRIC == 0.968
