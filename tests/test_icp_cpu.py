"""CPU: the registration kernels' numpy twin (tests/icp_oracle.py) against outside references — numpy.linalg.solve for its Cholesky
solve, scipy's Rotation for its Rodrigues formula — and against the TRUTH on the test surface: the twin's register_icp loop recovers
a known rigid motion within the bounds the GPU tests (tests/test_gpu_icp.py) then ask of the kernels.  Also the degenerate and short
inputs, the argument checks of the new sgam_points_* entry points through ctypes and the ValueErrors of geometry.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import _lib, geometry

sys.path.insert(0, os.path.dirname(__file__))
import icp_oracle as IO  # noqa: E402

f32 = np.float32
MAX_DISTANCE = 0.5
# the truth bounds of the loop tests, here for the twin and in tests/test_gpu_icp.py for the kernels.  Exact copy: the target is the
# fp32-rounded moved source, so the truth itself is known to a rounding of coordinates of size 6 (6 * 2^-24 = 3.6e-7); 2e-5 / 1e-5
# are above 20 times that and four orders below the 5 degree / 0.11 perturbation.  Resampled: other samples of the same surface.
EXACT_R, EXACT_T = 2e-5, 1e-5
RESAMPLED_DEG, RESAMPLED_T = 0.01, 5e-4


def exact_copy(n, seed=5):
    """(source, target = the source moved by the perturbation (fp32), the target's normals, the motion)"""
    src, nrm = IO.surface(n, seed)
    T = IO.perturbation()
    return src, IO.transform(src, T), (nrm.astype(np.float64) @ T[:3, :3].T).astype(f32), T


def resampled(n=4000, m=12000):
    src, _ = IO.surface(n, 5)
    other, nrm = IO.surface(m, 6, -0.3, 4.3)          # (a margin: every moved source point has the surface under it)
    T = IO.perturbation()
    return src, IO.transform(other, T), (nrm.astype(np.float64) @ T[:3, :3].T).astype(f32), T


def gating_case(n=1000):
    """the exact-copy source plus 30 % points 5 to 10 away from everything: they must find no correspondence"""
    src, tgt, nrm, T = exact_copy(n)
    rs = np.random.RandomState(3)
    far = np.stack([rs.uniform(0, 4, 3 * n // 10), rs.uniform(0, 4, 3 * n // 10), rs.uniform(5, 10, 3 * n // 10) * rs.choice([-1, 1], 3 * n // 10)], 1)
    return np.concatenate([src, far.astype(f32)]), tgt, nrm, T


def plane_case(n=500):
    """an exact plane z = 0 with normals (0, 0, 1): three directions of the pose are free"""
    rs = np.random.RandomState(9)
    p = np.stack([rs.uniform(0, 4, n), rs.uniform(0, 4, n), np.zeros(n)], 1).astype(f32)
    return p, p.copy(), np.tile(np.array([0, 0, 1], dtype=f32), (n, 1))


# ---------------------------------------------------------------- the twin's pieces
def test_cholesky_solve_equals_numpy():
    rs = np.random.RandomState(0)
    for _ in range(20):
        M = rs.normal(size=(40, 6))
        A, b = M.T @ M, rs.normal(size=6)
        x = IO.cholesky_solve(A, b)
        assert np.abs(x - np.linalg.solve(A, b)).max() <= 1e-12 * np.linalg.cond(A) * np.abs(x).max()
    singular = np.diag([1.0, 1.0, 0.0, 1.0, 1.0, 1.0])
    assert IO.cholesky_solve(singular, np.ones(6)) is None
    assert IO.cholesky_solve(np.diag([1.0, 1.0, 1e-13, 1.0, 1.0, 1.0]), np.ones(6)) is not None          # relative to A_jj itself
    nearly = np.eye(6)
    nearly[0, 1] = nearly[1, 0] = 1.0 - 1e-14
    assert IO.cholesky_solve(nearly, np.ones(6)) is None
    assert IO.cholesky_solve(np.full((6, 6), np.nan), np.ones(6)) is None


def test_rodrigues_equals_scipy():
    from scipy.spatial.transform import Rotation
    rs = np.random.RandomState(1)
    for scale in (1e-12, 1e-9, 1e-7, 1e-3, 0.1, 1.0, 3.0):
        for _ in range(5):
            w = rs.normal(size=3) * scale
            # an entry is three terms of size <= 2 (b w_i w_j at |w| = 3 ...), some eight roundings of 2^-53 relative each in the
            # twin and as many in scipy's quaternion route: 16 * 2 * 2^-53 = 3.6e-15
            assert np.abs(IO.rodrigues(w) - Rotation.from_rotvec(w).as_matrix()).max() <= 4e-15
    assert np.array_equal(IO.rodrigues(np.zeros(3)), np.eye(3))


def test_slot_layout():
    assert [IO.tri(a, b) for a in range(6) for b in range(a, 6)] == list(range(21))
    # the point-to-point summands are the rows J = [-[p]x | I] with residuals e
    src, tgt, _, _ = exact_copy(50)
    d2, idx = IO.search(src, tgt, None)
    S = IO.summands(src, tgt, None, idx, d2)
    p, q = src.astype(np.float64), tgt[idx].astype(np.float64)
    for i in (0, 7, 49):
        px, py, pz = p[i]
        J = np.array([[0, pz, -py, 1, 0, 0], [-pz, 0, px, 0, 1, 0], [py, -px, 0, 0, 0, 1]])
        A, g = IO.matrices(S[i])
        assert np.allclose(A, J.T @ J, rtol=1e-15, atol=0) and np.allclose(g, J.T @ (p[i] - q[i]), rtol=1e-13, atol=1e-18)
        assert np.isclose(S[i, 27], ((p[i] - q[i]) ** 2).sum(), rtol=1e-15)


def test_surface_constrains_all_six_degrees_of_freedom():
    src, tgt, nrm, T = exact_copy(4000)
    moved = IO.transform(src, np.eye(4))
    d2, idx = IO.search(moved, tgt, MAX_DISTANCE)
    for normals in (nrm, None):
        A, _ = IO.matrices(IO.accumulate(moved, tgt, normals, idx, d2)[0].sum(0))
        cond = np.linalg.cond(A)
        print("cond(J^T J)", "point_to_plane" if normals is not None else "point_to_point", cond)
        assert cond < 1e4


# ---------------------------------------------------------------- the twin meets the truth bounds
@pytest.mark.parametrize("plane", [True, False], ids=["point_to_plane", "point_to_point"])
@pytest.mark.parametrize("n", [257, 4000])
def test_twin_recovers_an_exact_copy(n, plane):
    src, tgt, nrm, T = exact_copy(n)
    out = IO.register_icp(src, tgt, MAX_DISTANCE, normals=nrm if plane else None)
    eR, et, deg = IO.pose_error(out["transformation"], T)
    print(n, plane, "iterations", out["iterations"], "R error", eR, "t error", et, "fitness", out["history"][:, 0])
    assert out["converged"] and out["status"] == 1 and out["iterations"] <= 30 and len(out["history"]) == out["iterations"] + 1
    assert (out["history"][:, 0] == 1.0).all() and out["fitness"] == 1.0
    assert eR <= EXACT_R and et <= EXACT_T


def test_twin_recovers_a_resampled_surface():
    src, tgt, nrm, T = resampled()
    out = IO.register_icp(src, tgt, MAX_DISTANCE, normals=nrm)
    _, et, deg = IO.pose_error(out["transformation"], T)
    print("resampled: iterations", out["iterations"], "angle", deg, "t error", et)
    assert out["converged"] and out["iterations"] <= 30 and deg <= RESAMPLED_DEG and et <= RESAMPLED_T


def test_twin_gates_far_points():
    src, tgt, nrm, T = gating_case()
    out = IO.register_icp(src, tgt, MAX_DISTANCE, normals=nrm)
    eR, et, _ = IO.pose_error(out["transformation"], T)
    assert out["history"][0, 2] == 1000 and out["fitness"] == 1000 / 1300 and out["converged"] and eR <= EXACT_R and et <= EXACT_T


# ---------------------------------------------------------------- degenerate and short inputs
def test_degenerate_and_short_inputs_leave_the_pose_alone():
    p, q, nrm = plane_case()
    init = IO.rigid(1.0, [0, 0, 1], [0.01, 0.0, 0.0])
    out = IO.register_icp(p, q, MAX_DISTANCE, init=init, normals=nrm)
    assert out["status"] == 2 and not out["converged"] and out["iterations"] == 0 and len(out["history"]) == 1
    assert np.array_equal(out["transformation"], init) and out["history"][0, 2] == 500
    few = IO.register_icp(p[:5], q[:5], MAX_DISTANCE, normals=None)
    assert few["status"] == 2 and few["iterations"] == 0 and np.array_equal(few["transformation"], np.eye(4)) and few["history"][0, 2] == 5
    none = IO.register_icp(p + f32(50.0), q, MAX_DISTANCE, normals=nrm)
    assert none["status"] == 2 and none["fitness"] == 0.0 and np.isnan(none["inlier_rmse"])
    # the frozen state: another call changes nothing
    s = IO.new_state()
    s[16:22] = [0.5, 0.25, 2.0, 3.0, 40.0, 7.0]
    s2, row = IO.update(np.zeros((1, 32)), 4, 1e-6, 1e-6, s)
    assert np.array_equal(s2, s) and list(row) == [0.5, 0.25, 40.0, 7.0, 0.0, 0.0, 2.0, 0.0]


# ---------------------------------------------------------------- the C entry points and the Python checks
def test_icp_argument_validation_without_gpu():
    lib = _lib.load()
    assert lib.sgam_abi_version() == 10                                 # additive: the ABI version stays
    for name in ("sgam_points_transform_f32", "sgam_points_icp_partials", "sgam_points_icp_accumulate", "sgam_points_icp_update"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    p = ctypes.c_void_p(256)                                            # never dereferenced: every check comes before a launch
    for args in ((None, 10, p, p), (p, 10, None, p), (p, 10, p, None), (p, 0, p, p), (p, -3, p, p)):
        assert lib.sgam_points_transform_f32(*args, None) == -1, args
    parts = lib.sgam_points_icp_partials
    assert [parts(n) for n in (1, 4096, 4097, 65536)] == [32, 32, 64, 512] and parts(0) == parts(-1) == -1

    def accumulate(moved=p, target=p, normals=None, index=p, d2=p, N=10, Nr=10, partials=p):
        return lib.sgam_points_icp_accumulate(moved, target, normals, index, d2, N, Nr, partials, None)

    for kw in (dict(moved=None), dict(target=None), dict(index=None), dict(d2=None), dict(partials=None), dict(N=0), dict(Nr=0), dict(N=-1),
               dict(normals=p, Nr=0)):
        assert accumulate(**kw) == -1, kw

    def update(partials=p, blocks=1, iteration=0, rf=1e-6, rr=1e-6, state=p, history=p):
        return lib.sgam_points_icp_update(partials, blocks, iteration, rf, rr, state, history, None)

    for kw in (dict(partials=None), dict(state=None), dict(history=None), dict(blocks=0), dict(blocks=-2), dict(blocks=1 << 40),
               dict(iteration=-1), dict(rf=-1.0), dict(rr=float("nan"))):
        assert update(**kw) == -1, kw


def test_python_argument_checks():
    src = torch.zeros((10, 3))
    with pytest.raises(ValueError, match="needs target_normals"):
        geometry.register_icp(src, src, 0.5)
    with pytest.raises(ValueError, match="takes no target_normals"):
        geometry.register_icp(src, src, 0.5, estimation="point_to_point", target_normals=src)
    with pytest.raises(ValueError, match="estimation"):
        geometry.register_icp(src, src, 0.5, estimation="plane")
    with pytest.raises(ValueError, match="max_iterations"):
        geometry.register_icp(src, src, 0.5, estimation="point_to_point", max_iterations=0)
    with pytest.raises(ValueError, match="check_every"):
        geometry.register_icp(src, src, 0.5, estimation="point_to_point", check_every=0)
    with pytest.raises(ValueError, match="relative_fitness"):
        geometry.register_icp(src, src, 0.5, estimation="point_to_point", relative_rmse=-1.0)
    with pytest.raises(ValueError, match="method"):
        geometry.register_icp(src, src, 0.5, estimation="point_to_point", method="tree")
    with pytest.raises(ValueError, match="max_correspondence_distance"):
        geometry.evaluate_registration(src, src, 0.0)
    with pytest.raises(ValueError, match="cloud"):
        geometry.evaluate_registration(torch.zeros((10, 2)), src, 0.5)
    with pytest.raises(ValueError, match="4x4"):
        geometry._pose(np.eye(3), "cpu", "test")
    with pytest.raises(ValueError, match="fp64"):
        geometry._pose(torch.eye(4), "cpu", "test")
    # a partials buffer that does not match the chunk count of the points, and a history without the row
    idx, d2 = torch.zeros((10,), dtype=torch.int32), torch.zeros((10,))
    with pytest.raises(ValueError, match="partials"):
        geometry.icp_accumulate(src, src, None, idx, d2, partials=torch.zeros((2, 32), dtype=torch.float64))
    with pytest.raises(ValueError, match="partials"):
        geometry.icp_update(torch.zeros((1, 31), dtype=torch.float64), 0, 1e-6, 1e-6, torch.zeros(24, dtype=torch.float64),
                            torch.zeros((4, 8), dtype=torch.float64))
    with pytest.raises(ValueError, match="history"):
        geometry.icp_update(torch.zeros((1, 32), dtype=torch.float64), 4, 1e-6, 1e-6, torch.zeros(24, dtype=torch.float64),
                            torch.zeros((4, 8), dtype=torch.float64))
    with pytest.raises(ValueError, match="state"):
        geometry.icp_update(torch.zeros((1, 32), dtype=torch.float64), 0, 1e-6, 1e-6, torch.zeros(20, dtype=torch.float64),
                            torch.zeros((4, 8), dtype=torch.float64))
