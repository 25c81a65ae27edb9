"""CPU: the coloured-ICP twin (tests/colored_icp_oracle.py) against the TRUTH — its gradient against the field's, its two rows
against a central finite difference of the residuals, its loop against a known motion of a textured PLANE, the input point-to-plane
ICP refuses (status 2) — plus the argument checks of the two new sgam_points_* entry points through ctypes and the new ValueErrors
of geometry.py and inference_pipeline.py.  The bounds the GPU tests (tests/test_gpu_colored_icp.py) then ask of the kernels are set
here.

Measured with the twin on the CPU (plane z = 0 over [0,4]^2, the texture of colored_icp_oracle.texture, k = 16, lambda = 0.968,
correspondence distance 0.3, a motion of 1 degree about the normal and (0.03, -0.02, 0) in the plane; seed 5, the one the tests use):
    exact copy,  n = 257:   3 iterations,  |R - R_true|_F 1.3e-8,  |t - t_true| 5.0e-8
    exact copy,  n = 4000:  3 iterations,  |R - R_true|_F 1.3e-8,  |t - t_true| 3.5e-8      (bounds: test_icp_cpu's EXACT_R, EXACT_T)
    resampled,   257 / 514:    4 iterations,  angle 0.03396 degrees,  |t - t_true| 1.369e-3  -> bounds 0.068 degrees, 2.74e-3
    resampled,   2000 / 4000:  3 iterations,  angle 9.15e-4 degrees,  |t - t_true| 5.98e-5   -> bounds 1.84e-3 degrees, 1.2e-4
The resampled error is a property of the sampling and of the uint8 texture, not of rounding: the bound is twice the measured value.
Other seeds, for the record (not asserted): 257 / 514 gave 0.026 degrees / 1.19e-3 (seed 11) and 0.0065 degrees / 4.2e-3 (seed 23: its
translation is outside twice seed 5's); 2000 / 4000 gave 2.0e-3 degrees / 5.7e-5 (seed 11) and 4.3e-4 degrees / 1.5e-4 (seed 23).
cond(J^T J) of the coloured system on the textured plane: 2.6e4 (n = 500), 2.5e4 (n = 4000)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import _lib, geometry

sys.path.insert(0, os.path.dirname(__file__))
import colored_icp_oracle as CIO  # noqa: E402
import icp_oracle as IO  # noqa: E402
from test_icp_cpu import EXACT_R, EXACT_T  # noqa: E402

f32 = np.float32
PLANE_DISTANCE = 0.3
GRADIENT_K = 16
# twice the twin's measured error (the header): {(source points, target points): (degrees, translation)}
RESAMPLED_BOUNDS = {(257, 514): (0.068, 2.74e-3), (2000, 4000): (1.84e-3, 1.2e-4)}
# the largest second derivative of the texture's intensity in any direction: a channel 0.4 sin(a x + ..) cos(b y + ..) has a
# Hessian of norm <= 0.4 (a^2 + b^2), 0.4 sin / cos of (a x + b y) likewise: 0.81, 0.93 and 1.26 for the three, their mean 1.0
TEXTURE_HESSIAN = 1.0


def plane_gradients(tgt, tn, tc):
    return CIO.color_gradient(tgt, tn, tc, CIO.knn_rows(tgt, GRADIENT_K))


def twin_on_plane(case):
    p, col, tgt, tc, tn, T = case
    out = CIO.register_icp(p, col, tgt, tc, tn, plane_gradients(tgt, tn, tc), PLANE_DISTANCE)
    return out, IO.pose_error(out["transformation"], T)


# ---------------------------------------------------------------- the gradient
def test_gradient_of_a_linear_field_is_the_fields_tangential_gradient():
    p, nrm, _ = CIO.textured_plane(600, 3)
    a, b = 0.11, -0.07
    I = 0.3 + a * p[:, 0].astype(np.float64) + b * p[:, 1].astype(np.float64)          # (float64: exempt from the uint8 rounding)
    g = CIO.color_gradient_f64(p, nrm, None, CIO.knn_rows(p, GRADIENT_K), intensities=I)
    err = np.abs(g - np.array([a, b, 0.0])).max() / np.hypot(a, b)
    print("linear field: largest relative error of the gradient", err)
    assert np.isfinite(g).all() and err <= 1e-12
    # and on a tilted plane with a field that also varies along the normal: only the tangential part comes back.  The points are
    # fp32, so they lie off the plane by a rounding: the field is taken linear in the TANGENT coordinates of the rounded points,
    # which is what the kernel fits.  The fp32 normal is off unit length by up to 2^-24 per component, so u = e - (e . n) n keeps
    # a normal part of that relative size and the fit is consistent only to it: 2^-22 (measured: 5.1e-9)
    rs = np.random.RandomState(4)
    n = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    t1 = np.cross(n, [1.0, 0.0, 0.0])
    t1 /= np.linalg.norm(t1)
    t2 = np.cross(n, t1)
    q = (rs.uniform(0, 4, (600, 1)) * t1 + rs.uniform(0, 4, (600, 1)) * t2 + 1.0).astype(f32)
    n32 = n.astype(f32)
    n64 = n32.astype(np.float64)
    grad = np.array([0.2, 0.1, -0.15])
    tangential = grad - (grad @ n64) * n64
    q64 = q.astype(np.float64)
    I = (q64 - (q64 @ n64)[:, None] * n64) @ grad
    g = CIO.color_gradient_f64(q, np.tile(n32, (600, 1)), None, CIO.knn_rows(q, GRADIENT_K), intensities=I)
    err = np.abs(g - tangential).max() / np.linalg.norm(tangential)
    print("tilted plane: largest relative error", err)
    assert err <= 2.0 ** -22


def test_gradient_of_the_uint8_texture_within_the_quantisation_bound():
    """With uint8 colours the intensity of a point is off by at most 3 * 0.5 / 765 = 1 / 510, a difference of two by 1 / 255.  The
    fit's answer in the tangent plane is A_t^-1 sum_j u_j dI_j with A_t = sum_j u_j u_j^T, so an error delta_j of dI_j moves it by
    at most sum_j |u_j| |delta_j| / lambda_min(A_t); and a smooth field is off its linear part by at most H |u_j|^2 / 2, H the
    largest second derivative (TEXTURE_HESSIAN).  Per point:
        |g - g_true| <= sum_j |u_j| (1 / 255 + H |u_j|^2 / 2) / lambda_min(A_t),
    1 / 255 over the neighbourhood radius in order of magnitude.  Measured on this input (n = 2000, k = 16): the largest error is
    0.101 (a point at the border of the square, its neighbours on one side), the bound there 1.47 and 0.20 to 1.47 over the cloud;
    the largest error / bound 0.24."""
    p, nrm, col = CIO.textured_plane(2000, 5)
    rows = CIO.knn_rows(p, GRADIENT_K)
    g = CIO.color_gradient(p, nrm, col, rows).astype(np.float64)
    x, y = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64)
    h = 1e-6
    field = lambda x, y: CIO.texture_field(x, y).sum(-1) / 3.0                                  # noqa: E731
    truth = np.stack([(field(x + h, y) - field(x - h, y)) / (2 * h), (field(x, y + h) - field(x, y - h)) / (2 * h), np.zeros(len(p))], 1)
    u = p.astype(np.float64)[rows] - p.astype(np.float64)[:, None, :]                           # (the plane z = 0: e is tangential)
    un = np.linalg.norm(u, axis=2)
    lam_min = np.linalg.eigvalsh(np.einsum("nka,nkb->nab", u[:, :, :2], u[:, :, :2]))[:, 0]
    bound = (un * (1.0 / 255.0 + TEXTURE_HESSIAN * un * un / 2.0)).sum(1) / lam_min
    err = np.linalg.norm(g - truth, axis=1)
    print("uint8 texture: largest gradient error", err.max(), "its bound", bound[err.argmax()], "bounds", bound.min(), bound.max(),
          "largest error / bound", (err / bound).max())
    assert np.isfinite(g).all() and (rows >= 0).all() and (err <= bound).all()
    assert np.abs(g[:, 2]).max() <= 1e-7                                                        # in the tangent plane


# ---------------------------------------------------------------- the rows
def test_rows_equal_a_central_finite_difference_of_the_residuals():
    """Three random correspondences: J_G, J_I against (r(+h) - r(-h)) / 2h in the six pose parameters.  h = 1e-5: the truncation
    is h^2 / 6 times a third derivative (the rotation of a point of norm <= 7 against unit vectors and a gradient of norm <= 2:
    below 1e-9), the rounding 2^-53 |r| / h (1e-11): 1e-8 covers both with room."""
    rs = np.random.RandomState(7)
    lam, h = CIO.LAMBDA, 1e-5
    for _ in range(3):
        p, q = rs.uniform(0, 4, 3), rs.uniform(0, 4, 3)
        n = rs.normal(size=3)
        n /= np.linalg.norm(n)
        d = rs.normal(size=3)
        I_s, I_t = rs.uniform(size=2)
        JG, rG, JI, rI = (v[0] for v in CIO.rows(p[None], q[None], n[None], d[None], np.array([I_s]), np.array([I_t]), lam))
        r0 = CIO.residuals(np.zeros(6), p, q, n, d, I_s, I_t, lam)
        assert abs(r0[0] - rG) <= 1e-14 and abs(r0[1] - rI) <= 1e-14
        for a in range(6):
            xi = np.zeros(6)
            xi[a] = h
            plus, minus = CIO.residuals(xi, p, q, n, d, I_s, I_t, lam), CIO.residuals(-xi, p, q, n, d, I_s, I_t, lam)
            assert abs((plus[0] - minus[0]) / (2 * h) - JG[a]) <= 1e-8, ("geometric", a)
            assert abs((plus[1] - minus[1]) / (2 * h) - JI[a]) <= 1e-8, ("photometric", a)


def _plane_sums(n):
    p, col, tgt, tc, tn, _ = CIO.plane_exact_copy(n)
    d2, idx = IO.search(p, tgt, PLANE_DISTANCE)
    grad = plane_gradients(tgt, tn, tc)
    colored = CIO.accumulate(p, col, tgt, tn, tc, grad, idx, d2, CIO.LAMBDA)[0]
    return colored, IO.accumulate(p, tgt, tn, idx, d2)[0], (p, col, tgt, tc, tn, grad, idx, d2)


@pytest.mark.parametrize("n", [500, 4000])
def test_a_textured_plane_constrains_all_six_parameters(n):
    """cond(J^T J) of the coloured system is finite and far inside what the update's pivot rule accepts (1 / ICP_PIVOT_REL = 1e12);
    the same correspondences through the point-to-plane sums are refused.

    The texture, not a linear field: a plane whose intensity is LINEAR has one constant gradient d, every photometric row is
    [p x (-d), -d], and the translation along the lines of equal intensity appears in no row — the coloured system of such a
    plane is singular however many points it has (asserted below with the exact gradient).  What constrains all six is an
    intensity whose gradient turns over the plane."""
    colored, plane, (p, col, tgt, tc, tn, grad, idx, d2) = _plane_sums(n)
    A, _ = IO.matrices(colored.sum(0))
    cond = np.linalg.cond(A)
    print("textured plane n", n, "cond(J^T J) coloured", cond)
    assert np.isfinite(cond) and cond < 1e-3 / IO.PIVOT_REL and IO.cholesky_solve(A, np.ones(6)) is not None
    state, row = IO.update(colored, 0, 1e-6, 1e-6, IO.new_state())
    assert state[18] == 0 and state[19] == 1
    state, row = IO.update(plane, 0, 1e-6, 1e-6, IO.new_state())
    assert state[18] == 2 and state[19] == 0 and row[2] == n
    # lambda = 1 is point-to-plane: the same sums bit for bit, and refused alike
    same = CIO.accumulate(p, col, tgt, tn, tc, grad, idx, d2, 1.0)[0]
    assert np.array_equal(same, plane)
    # a linear field: the slide along its lines of equal intensity is free
    P = p.astype(np.float64)
    d = np.tile(np.array([0.11, -0.07, 0.0]), (n, 1))
    JG, _, JI, _ = CIO.rows(P, P, np.tile(np.array([0.0, 0.0, 1.0]), (n, 1)), d, np.zeros(n), np.zeros(n), CIO.LAMBDA)
    eig = np.linalg.eigvalsh(JG.T @ JG + JI.T @ JI)
    slide = np.array([0, 0, 0, 0.07, 0.11, 0.0])
    assert eig[0] <= 1e-12 * eig[-1] and np.abs(JG @ slide).max() == 0 and np.abs(JI @ slide).max() <= 1e-17


# ---------------------------------------------------------------- the twin meets the truth
@pytest.mark.parametrize("n", [257, 4000])
def test_twin_recovers_an_exact_copy_of_the_textured_plane(n):
    case = CIO.plane_exact_copy(n)
    out, (eR, et, deg) = twin_on_plane(case)
    print("plane exact copy n", n, "iterations", out["iterations"], "R error", eR, "t error", et)
    assert out["converged"] and out["status"] == 1 and out["iterations"] <= 30 and len(out["history"]) == out["iterations"] + 1
    assert out["fitness"] == 1.0 and eR <= EXACT_R and et <= EXACT_T
    p, col, tgt, tc, tn, T = case
    assert IO.register_icp(p, tgt, PLANE_DISTANCE, normals=tn)["status"] == 2


@pytest.mark.parametrize("n,m", sorted(RESAMPLED_BOUNDS))
def test_twin_recovers_a_resampled_textured_plane(n, m):
    case = CIO.plane_resampled(n, m)
    out, (eR, et, deg) = twin_on_plane(case)
    print("plane resampled", n, m, "iterations", out["iterations"], "angle", deg, "t error", et, "bounds", RESAMPLED_BOUNDS[n, m])
    assert out["converged"] and out["iterations"] <= 30
    assert deg <= RESAMPLED_BOUNDS[n, m][0] and et <= RESAMPLED_BOUNDS[n, m][1]
    p, col, tgt, tc, tn, T = case
    refused = IO.register_icp(p, tgt, PLANE_DISTANCE, normals=tn)
    assert refused["status"] == 2 and refused["iterations"] == 0


# ---------------------------------------------------------------- the C entry points and the Python checks
def test_colored_argument_validation_without_gpu():
    lib = _lib.load()
    assert lib.sgam_abi_version() == 10                                 # additive: the ABI version stays
    for name in ("sgam_points_color_gradient_f32", "sgam_points_icp_accumulate_colored"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    p = ctypes.c_void_p(256)                                            # never dereferenced: every check comes before a launch

    def gradient(points=p, normals=p, colors=p, N=10, knn=p, k=16, out=p):
        return lib.sgam_points_color_gradient_f32(points, normals, colors, N, knn, k, out, None)

    for kw in (dict(points=None), dict(normals=None), dict(colors=None), dict(knn=None), dict(out=None), dict(N=0), dict(N=-4), dict(k=0),
               dict(k=33), dict(k=-1)):
        assert gradient(**kw) == -1, kw

    def accumulate(moved=p, sc=p, target=p, normals=p, tc=p, grad=p, index=p, d2=p, N=10, Nr=10, lam=0.968, partials=p):
        return lib.sgam_points_icp_accumulate_colored(moved, sc, target, normals, tc, grad, index, d2, N, Nr, lam, partials, None)

    for kw in (dict(moved=None), dict(sc=None), dict(target=None), dict(normals=None), dict(tc=None), dict(grad=None), dict(index=None),
               dict(d2=None), dict(partials=None), dict(N=0), dict(Nr=0), dict(N=-1), dict(lam=-1e-9), dict(lam=1.0 + 1e-9),
               dict(lam=float("nan")), dict(lam=float("inf"))):
        assert accumulate(**kw) == -1, kw


def test_python_argument_checks_of_the_colored_estimation():
    src, nrm = torch.zeros((10, 3)), torch.zeros((10, 3))
    col = torch.zeros((10, 3), dtype=torch.uint8)
    assert "colored" in geometry.ICP_ESTIMATIONS and geometry.LAMBDA_GEOMETRIC == 0.968
    kw = dict(estimation="colored", target_normals=nrm, source_colors=col, target_colors=col)

    def refused(match, **change):
        with pytest.raises(ValueError, match=match):
            geometry.register_icp(src, src, 0.5, **dict(kw, **change))

    refused("needs target_normals", target_normals=None)
    refused("needs source_colors", source_colors=None)
    refused("needs target_colors", target_colors=None)
    refused("source_colors are", source_colors=torch.zeros((10, 3)))                    # dtype
    refused("target_colors are", target_colors=col[:9])                                 # length
    refused("source_colors are", source_colors=torch.zeros((10, 4), dtype=torch.uint8))
    refused("target_gradients are", target_gradients=torch.zeros((9, 3)))
    refused("target_gradients are", target_gradients=torch.zeros((10, 3), dtype=torch.float64))
    for lam in (-0.1, 1.5, float("nan")):
        refused("lambda_geometric", lambda_geometric=lam)
    refused("k is an integer", gradient_k=40)
    for estimation in ("point_to_plane", "point_to_point"):
        with pytest.raises(ValueError, match="belong to estimation='colored'"):
            geometry.register_icp(src, src, 0.5, estimation=estimation, target_normals=nrm if estimation == "point_to_plane" else None,
                                  source_colors=col)
    with pytest.raises(ValueError, match="normals are"):
        geometry.color_gradients(src, nrm[:5], col)
    with pytest.raises(ValueError, match="needs colors"):
        geometry.color_gradients(src, nrm, None)
    with pytest.raises(ValueError, match="colors are"):
        geometry.color_gradients(src, nrm, col.to(torch.int32))
    with pytest.raises(ValueError, match="k is an integer"):
        geometry.color_gradients(src, nrm, col, k=0)
    idx, d2 = torch.zeros((10,), dtype=torch.int32), torch.zeros((10,))
    with pytest.raises(ValueError, match="lambda_geometric"):
        geometry.icp_accumulate_colored(src, col, src, nrm, col, nrm, idx, d2, 2.0)
    with pytest.raises(ValueError, match="target_gradients"):
        geometry.icp_accumulate_colored(src, col, src, nrm, col, None, idx, d2, 0.5)
    with pytest.raises(ValueError, match="partials"):
        geometry.icp_accumulate_colored(src, col, src, nrm, col, nrm, idx, d2, 0.5, partials=torch.zeros((2, 32), dtype=torch.float64))
    # the multi-scale loop
    with pytest.raises(ValueError, match="same levels"):
        geometry.register_icp_multiscale(src, src, [0.1, 0.05], [0.3], 30, estimation="point_to_point")
    with pytest.raises(ValueError, match="same levels"):
        geometry.register_icp_multiscale(src, src, [], [], 30, estimation="point_to_point")
    with pytest.raises(ValueError, match="needs source_colors"):
        geometry.register_icp_multiscale(src, src, [0.1], [0.3], 30, estimation="colored", target_colors=col)
    with pytest.raises(ValueError, match="belong to estimation='colored'"):
        geometry.register_icp_multiscale(src, src, [0.1], [0.3], 30, source_colors=col)
    with pytest.raises(ValueError, match="estimation"):
        geometry.register_icp_multiscale(src, src, [0.1], [0.3], 30, estimation="coloured")


def test_scene_level_checks_of_the_colored_estimation():
    """"colored" needs colours on both sides: source="mesh" and a reference without colours are refused before anything runs"""
    from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, _register_clouds
    scene = object.__new__(InfiniteSceneGeneration)                     # (the checks come before the scene is looked at)
    align = dict(max_correspondence_distance=0.1, estimation="colored")
    with pytest.raises(ValueError, match="needs source='frames'"):
        scene.geometry_metrics(torch.zeros((4, 3)), 0.01, align=align, source="mesh")
    with pytest.raises(ValueError, match="needs source='frames'"):
        scene.geometry_metrics(scene, 0.01, align=align, source="mesh", surface_samples=100)
    with pytest.raises(ValueError, match="a reference with colours"):
        scene.geometry_metrics(torch.zeros((4, 3)), 0.01, align=align)
    with pytest.raises(ValueError, match="a reference with colours"):
        scene.geometry_metrics({"depths": [], "Ts_w2c": np.zeros((0, 4, 4)), "K": np.eye(3)}, 0.01, align=align)
    with pytest.raises(ValueError, match="belong to estimation 'colored'"):
        scene.geometry_metrics(torch.zeros((4, 3)), 0.01, align=dict(max_correspondence_distance=0.1, lambda_geometric=0.5))
    with pytest.raises(ValueError, match="estimation"):
        scene.frame_drift(0.1, estimation="coloured")
    opts = InfiniteSceneGeneration._align_options(align)
    assert opts["lambda_geometric"] == 0.968 and opts["gradient_k"] == 16
    assert InfiniteSceneGeneration._align_options(dict(max_correspondence_distance=0.1))["estimation"] == "point_to_plane"
    with pytest.raises(ValueError, match="colours go with estimation 'colored'"):
        _register_clouds(torch.zeros((4, 3)), torch.zeros((4, 3)), None, 0.1, "colored", 30, 16, None, "test")
