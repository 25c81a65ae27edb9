"""CPU: the cloud clean-up kernels' numpy twin (tests/cloud_oracle.py) against outside references — scipy's k-d tree on float64
copies for the k-NN, a hand example for the voxel sampling — the argument checks of geometry.knn / voxel_grid_for and of the new
sgam_points_* entry points through ctypes, and the conditions the GPU tests (tests/test_gpu_cloud.py) put on their inputs, which
are built here: the twin alone keeps the guards of the outlier and normal comparisons within their caps."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import _lib, geometry

sys.path.insert(0, os.path.dirname(__file__))
import cloud_oracle as CO  # noqa: E402
import geometry_oracle as GO  # noqa: E402
from test_geometry_cpu import cloud  # noqa: E402

f32 = np.float32
JACOBI_SWEEPS = 6                 # csrc/point_cloud.hip


# ---------------------------------------------------------------- the inputs of the GPU tests
def outlier_case():
    """a 2000-point noisy plane (a 4 x 4 patch, noise 0.01) and 20 points 5 to 10 away from it"""
    rs = np.random.RandomState(41)
    plane = np.stack([rs.uniform(0, 4, 2000), rs.uniform(0, 4, 2000), rs.normal(0, 0.01, 2000)], 1)
    far = np.stack([rs.uniform(0, 4, 20), rs.uniform(0, 4, 20), rs.uniform(5, 10, 20) * rs.choice([-1, 1], 20)], 1)
    return np.concatenate([plane, far]).astype(f32)


def normal_cases():
    """{"plane", "sphere", "cylinder"}: 2000 points each with a little noise, of size 1 - 4"""
    rs = np.random.RandomState(42)
    plane = np.stack([rs.uniform(0, 4, 2000), rs.uniform(0, 4, 2000), rs.normal(0, 0.005, 2000)], 1)
    d = rs.normal(0, 1, (2000, 3))
    sphere = d / np.linalg.norm(d, axis=1, keepdims=True) * (2.0 + rs.normal(0, 0.002, (2000, 1))) + np.array([1.0, -2.0, 3.0])
    a, z = rs.uniform(0, 2 * np.pi, 2000), rs.uniform(0, 3, 2000)
    r = 1.5 + rs.normal(0, 0.002, 2000)
    cylinder = np.stack([r * np.cos(a), r * np.sin(a), z], 1)
    return {"plane": plane.astype(f32), "sphere": sphere.astype(f32), "cylinder": cylinder.astype(f32)}


SPHERE_CENTRE = np.array([1.0, -2.0, 3.0])


def normal_guard(w):
    """the points whose normal is well defined: lambda1 - lambda0 >= 1e-3 lambda2"""
    with np.errstate(invalid="ignore"):
        return (w[:, 1] - w[:, 0]) >= 1e-3 * w[:, 2]


# ---------------------------------------------------------------- k-NN
@pytest.mark.parametrize("nq,nr,k", [(300, 2000, 8), (257, 65, 32), (64, 40, 9), (100, 500, 1)])
def test_twin_knn_against_a_kd_tree(nq, nr, k):
    from scipy.spatial import cKDTree
    q, r = cloud(nq, 1), cloud(nr, 2)
    d2, idx = CO.knn_brute(q, r, k)
    assert d2.shape == idx.shape == (nq, k) and d2.dtype == f32 and idx.dtype == np.int32
    assert (idx >= 0).all() and (np.diff(d2.astype(np.float64), axis=1) >= 0).all()
    dist, want_idx = cKDTree(r.astype(np.float64)).query(q.astype(np.float64), k=k + 1)
    dist, want_idx = dist.reshape(nq, -1), want_idx.reshape(nq, -1)
    want = dist[:, :k] ** 2
    tol = 2.0 ** -20                                                     # test_geometry_cpu's bound on an fp32 d2
    assert (np.abs(d2.astype(np.float64) - want) <= tol * want).all()
    # the index is the tree's wherever the neighbours on either side of a rank are farther apart than that
    w = dist ** 2
    lo = np.concatenate([np.full((nq, 1), -np.inf), w[:, :k - 1]], 1) if k > 1 else np.full((nq, 1), -np.inf)
    clear = (w[:, 1:k + 1] - w[:, :k] > 2 * tol * w[:, 1:k + 1]) & (w[:, :k] - lo > 2 * tol * w[:, :k])
    assert clear.mean() > 0.99 and np.array_equal(idx[clear], want_idx[:, :k][clear])
    if k == 1:
        a = GO.nn_brute(q, r)
        assert np.array_equal(a[0].view(np.uint32), d2[:, 0].view(np.uint32)) and np.array_equal(a[1], idx[:, 0])


def test_twin_knn_rules():
    r = np.array([[1, 1, 1], [np.nan, 0, 0], [1, 1, 1], [5, 5, 5], [0, np.inf, 0], [1, 1, 3]], dtype=f32)
    q = np.array([[1, 1, 2], [np.nan, 1, 1], [5, 5, 4]], dtype=f32)
    d2, idx = CO.knn_brute(q, r, 3)
    assert idx.tolist() == [[0, 2, 5], [-1, -1, -1], [3, 5, 0]] and d2[0].tolist() == [1, 1, 1] and np.isinf(d2[1]).all()
    d2, idx = CO.knn_brute(q, r, 6)                                      # four valid reference points: a tail of -1 / +inf
    assert idx[0].tolist() == [0, 2, 5, 3, -1, -1] and np.isinf(d2[0, 4:]).all()
    d2, idx = CO.knn_brute(q, r, 3, CO.max_d2_of(1.0))                   # on the limit is inside
    assert idx.tolist() == [[0, 2, 5], [-1, -1, -1], [3, -1, -1]]
    d2, idx = CO.knn_brute(r, r, 2, exclude_self=True)                   # the duplicate of point 0 is point 2, not itself
    assert idx[0].tolist() == [2, 5] and idx[2].tolist() == [0, 5] and idx[1].tolist() == [-1, -1] and d2[0, 0] == 0
    with pytest.raises(ValueError):
        CO.knn_brute(q, r, 0)
    with pytest.raises(ValueError):
        CO.knn_brute(q, r, 33)
    with pytest.raises(ValueError):
        CO.knn_brute(q, r, 2, exclude_self=True)


def test_knn_argument_checks_without_gpu():
    q, r = torch.zeros((5, 3)), torch.zeros((7, 3))
    assert geometry.KNN_MAX_K == 32
    for k in (0, -1, 33, 2.0, None, True):
        with pytest.raises(ValueError, match="1..32"):
            geometry.knn(q, r, k)
    with pytest.raises(ValueError, match="exclude_self"):
        geometry.knn(q, r, 2, exclude_self=True)
    with pytest.raises(ValueError, match="method"):
        geometry.knn(q, r, 2, method="tree")
    with pytest.raises(ValueError, match="cell_size"):
        geometry.knn(q, r, 2, method="brute", cell_size=1.0)
    with pytest.raises(ValueError, match="max_distance"):
        geometry.knn(q, r, 2, max_distance=-1.0)
    with pytest.raises(ValueError):
        geometry.knn(torch.zeros((5, 2)), r, 2)
    with pytest.raises(ValueError):
        geometry.knn(q.double(), r, 2)
    for fn in (geometry.statistical_outliers, geometry.estimate_normals):
        with pytest.raises(ValueError, match="1..32"):
            fn(q, 40)
    with pytest.raises(ValueError, match="together"):
        geometry.estimate_normals(q, 4, viewpoints=torch.zeros((1, 3)))


# ---------------------------------------------------------------- voxel sampling
def test_voxel_sampling_on_a_hand_example():
    # voxels of edge 1 from the origin (0, 0, 0); centres at .5
    p = np.array([[0.1, 0.1, 0.1],        # voxel (0,0,0), d2 to the centre 0.48
                  [0.5, 0.5, 0.25],       # voxel (0,0,0), d2 0.0625: kept
                  [np.nan, 0, 0],
                  [1.0, 0.0, 0.0],        # on the face: voxel (1,0,0), d2 0.75
                  [1.5, 0.5, 0.75],       # voxel (1,0,0), d2 0.0625
                  [1.5, 0.5, 0.25],       # voxel (1,0,0), d2 0.0625: an exact tie, the lower index (4) is kept
                  [0.0, 0.0, 2.0],        # voxel (0,0,2) alone
                  [0.5, 0.25, 0.5]],      # voxel (0,0,0), d2 0.0625: ties with 1, which stays
                 dtype=f32)
    index, count = CO.voxel_sample(p, 1.0)
    assert index.tolist() == [1, 4, 6] and count.tolist() == [3, 3, 1] and index.dtype == count.dtype == np.int32
    index, count = CO.voxel_sample(p, 4.0)                               # one voxel, centre (2,2,2): (1.5, .5, .75) is nearest
    assert index.tolist() == [4] and count.tolist() == [7]
    index, count = CO.voxel_sample(p, 1.0, origin=(0.5, 0.5, 0.5))       # an origin inside the box: negative voxel numbers
    assert count.sum() == 7 and set(index.tolist()) >= {6}
    assert CO.voxel_sample(np.full((3, 3), np.nan, f32), 1.0)[0].size == 0
    same = np.repeat(cloud(1, 3), 512, axis=0)
    index, count = CO.voxel_sample(same, 0.01)
    assert index.tolist() == [0] and count.tolist() == [512]


def test_voxel_extent_refusal():
    lo, hi = np.array([0.0, 0.0, 0.0]), np.array([1.0, 2.0, 4.0])
    o, h = geometry.voxel_grid_for(lo, hi, 0.5)
    assert o.dtype == f32 and o.tolist() == [0, 0, 0] and h == 0.5
    assert geometry.voxel_grid_for(lo, hi, 0.1)[1] == float(f32(0.1))
    assert geometry.voxel_grid_for(lo, hi, 0.5, origin=(0.5, 1.0, 2.0))[0].tolist() == [0.5, 1.0, 2.0]
    geometry.voxel_grid_for(lo, hi, 4.0 / 2 ** 20 * 1.001)               # just under 2^20 voxels along z
    with pytest.raises(ValueError, match="2\\^20"):
        geometry.voxel_grid_for(lo, hi, 4.0 / 2 ** 20)
    with pytest.raises(ValueError, match="2\\^20"):
        geometry.voxel_grid_for(lo, hi, 1e-7)
    with pytest.raises(ValueError, match="2\\^20"):                      # a far origin counts like an extent
        geometry.voxel_grid_for(lo, hi, 1e-3, origin=(0.0, 0.0, -2000.0))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            geometry.voxel_grid_for(lo, hi, bad)
    with pytest.raises(ValueError, match="origin"):
        geometry.voxel_grid_for(lo, hi, 0.5, origin=(0.0, float("nan"), 0.0))


# ---------------------------------------------------------------- the conditions on the GPU tests' inputs
def test_outlier_case_leaves_nothing_out_and_drops_the_far_points():
    p = outlier_case()
    so = CO.statistical_outliers(p, 20, 2.0)
    md = so["mean_distance"]
    assert np.isfinite(md).all() and so["std"] > 0
    assert (np.abs(md - so["threshold"]) > 1e-9 * so["threshold"]).all()      # no point within the comparison's guard
    assert not so["keep"][2000:].any() and so["keep"][:2000].mean() > 0.9
    assert so["threshold"] == so["mean"] + 2.0 * so["std"]
    # the rule by hand on one point
    d2, idx = CO.knn_brute(p, p, 20)
    assert idx[7, 0] == 7 and md[7] == pytest.approx(np.sqrt(d2[7].astype(np.float64)).mean(), rel=1e-15)
    q = p.copy()
    q[::50] = np.nan
    so = CO.statistical_outliers(q, 20, 2.0)
    assert np.isnan(so["mean_distance"][::50]).all() and not so["keep"][::50].any() and np.isfinite(so["mean"])


@pytest.mark.parametrize("name", ["plane", "sphere", "cylinder"])
def test_normal_cases_stay_within_the_guard_and_the_sweep_count_holds(name):
    p = normal_cases()[name]
    idx = CO.knn_brute(p, p, 16)[1]
    n, w = CO.normals(p, knn_index=idx)
    guard = normal_guard(w)
    assert guard.mean() >= 0.9                                           # the GPU comparison may leave out at most 10 %
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-12)
    # the shapes' own normals, roughly (noise and curvature tilt them)
    if name == "plane":
        assert (np.abs(n[:, 2]) > 0.95).mean() > 0.95 and (n[guard][:, 2] > 0).mean() > 0.95      # largest component made positive
    if name == "sphere":
        radial = (p.astype(np.float64) - SPHERE_CENTRE) / 2.0
        assert (np.abs((n * radial).sum(1)) > 0.95).mean() > 0.95
        out = CO.normals(p, knn_index=idx, viewpoints=(SPHERE_CENTRE + 10 * radial).astype(f32), view_of=np.arange(2000))[0]
        assert ((out * radial).sum(1) > 0).all()
    # the kernel's eigen-solver restated: the fixed sweep count reaches the eigh normal far inside the GPU test's bound
    C, m = CO.covariances(p, idx)
    diag, V, off = CO.jacobi_eigh(C, JACOBI_SWEEPS)
    assert off.max() < 1e-60
    for sweeps in (JACOBI_SWEEPS - 2, JACOBI_SWEEPS):                    # two sweeps of margin: four already reach the rounding floor
        diag, V, off = CO.jacobi_eigh(C, sweeps)
        nj = V[np.arange(len(V)), :, np.argmin(diag, axis=1)]
        assert off.max() < 1e-20 and (1 - np.abs((nj * n).sum(1)))[guard].max() <= 1e-14
    assert np.allclose(np.sort(diag, axis=1), w, rtol=1e-9, atol=1e-15 * w.max())


def test_fewer_than_three_neighbours_give_nan():
    p = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 1, 0.5]], dtype=f32)
    n, w = CO.normals(p, 2)
    assert np.isnan(n).all()
    n, w = CO.normals(p, 3)
    assert np.isfinite(n[[0, 1, 3]]).all() and np.isnan(n[2]).all()


# ---------------------------------------------------------------- the C entry points
def test_cloud_argument_validation_without_gpu():
    lib = _lib.load()
    assert lib.sgam_abi_version() == 10                                 # additive: the ABI version stays
    for name in ("sgam_points_knn_brute_f32", "sgam_points_knn_grid_f32", "sgam_points_voxel_workspace_bytes",
                 "sgam_points_voxel_sample_f32", "sgam_points_knn_mean_distance", "sgam_points_md_reduce_partials",
                 "sgam_points_md_reduce", "sgam_points_normals_f32"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    p = ctypes.c_void_p(256)                                            # never dereferenced: every check comes before a launch

    def brute(q=p, r=p, Nq=10, Nr=10, k=4, m=np.inf, ex=0, d2=p, idx=p):
        return lib.sgam_points_knn_brute_f32(q, r, Nq, Nr, k, m, ex, d2, idx, None)

    for kw in (dict(q=None), dict(r=None), dict(d2=None), dict(idx=None), dict(Nq=0), dict(Nr=0), dict(k=0), dict(k=33), dict(k=-1),
               dict(m=-1.0), dict(m=float("nan")), dict(ex=2), dict(ex=1, Nq=9)):
        assert brute(**kw) == -1, kw
    ws = lib.sgam_points_grid_workspace_bytes(100, 4, 3, 2)

    def grid(q=p, Nq=100, Nr=100, h=0.5, g=(4, 3, 2), w=p, wb=ws, k=4, m=np.inf, ex=0, d2=p, idx=p):
        return lib.sgam_points_knn_grid_f32(q, Nq, Nr, 0.0, 0.0, 0.0, h, *g, w, wb, k, m, ex, d2, idx, None)

    for kw in (dict(q=None), dict(d2=None), dict(idx=None), dict(Nq=0), dict(k=0), dict(k=33), dict(m=-0.5), dict(ex=1, Nq=7), dict(ex=-1),
               dict(h=0.0), dict(g=(0, 3, 2)), dict(w=None), dict(wb=ws - 1), dict(w=ctypes.c_void_p(264)), dict(Nr=101)):
        assert grid(**kw) == -1, kw

    size = lib.sgam_points_voxel_workspace_bytes
    assert size(1) == 20 * 256 + 16 and size(128) == 20 * 256 + 512 and size(129) == 20 * 512 + 528 and size(5000) == 20 * 16384 + 20000
    assert size(0) == size(-1) == size((1 << 29) + 1) == -1

    def voxel(pts=p, N=100, o=(0.0, 0.0, 0.0), h=0.5, w=p, wb=size(100), keep=p, count=p, flag=p):
        return lib.sgam_points_voxel_sample_f32(pts, N, *o, h, w, wb, keep, count, flag, None)

    for kw in (dict(pts=None), dict(keep=None), dict(count=None), dict(flag=None), dict(N=0), dict(h=0.0), dict(h=-1.0), dict(h=float("nan")),
               dict(h=float("inf")), dict(o=(0.0, float("nan"), 0.0)), dict(w=None), dict(wb=size(100) - 1), dict(w=ctypes.c_void_p(264)),
               dict(N=200)):
        assert voxel(**kw) == -1, kw

    for args in ((None, p, 10, 4, p), (p, None, 10, 4, p), (p, p, 10, 4, None), (p, p, 0, 4, p), (p, p, 10, 0, p), (p, p, 10, 33, p)):
        assert lib.sgam_points_knn_mean_distance(*args, None) == -1, args
    parts = lib.sgam_points_md_reduce_partials
    assert [parts(n) for n in (1, 4096, 4097)] == [2, 2, 4] and parts(0) == -1
    for args in ((None, 10, 0.0, 0, p), (p, 10, 0.0, 0, None), (p, 0, 0.0, 0, p), (p, 10, float("nan"), 1, p), (p, 10, 0.0, 2, p)):
        assert lib.sgam_points_md_reduce(*args, None) == -1, args

    def normals(pts=p, N=10, idx=p, k=4, vp=None, V=0, vo=None, out=p):
        return lib.sgam_points_normals_f32(pts, N, idx, k, vp, V, vo, out, None)

    for kw in (dict(pts=None), dict(idx=None), dict(out=None), dict(N=0), dict(k=0), dict(k=33), dict(vp=p, V=2), dict(vo=p),
               dict(vp=p, vo=p, V=0), dict(V=3)):
        assert normals(**kw) == -1, kw
