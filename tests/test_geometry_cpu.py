"""CPU: the geometry kernels' numpy twin (tests/geometry_oracle.py) against outside references — scipy's k-d tree on float64
copies, pointcloud.unproject_frame in float64, the written chamfer formula on a hand example — the host side of the grid
(geometry.grid_for) and the argument checks of the new sgam_points_* entry points through ctypes, without a GPU.  The cases
built here are the ones tests/test_gpu_geometry.py runs on the device."""
import ctypes
import os
import sys

import numpy as np
import pytest

from sgam_neurips22_amd import _lib, geometry, pointcloud
from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, intrinsics

sys.path.insert(0, os.path.dirname(__file__))
import geometry_oracle as GO  # noqa: E402
from test_pointview_cpu import small_pose  # noqa: E402

f32 = np.float32
EPS = 2.0 ** -24


def cloud(n, seed, lo=1.0, hi=10.0):
    """n points with coordinates of order 1 - 10"""
    return np.random.RandomState(seed).uniform(lo, hi, (n, 3)).astype(f32)


def frames_case(data, Hs, Ws, F=3, seed=0):
    """F frames of a dataset: depths inside its z range seeded with values that must become NaN points, colours, poses"""
    rs = np.random.RandomState(seed)
    z0, z1 = InfiniteSceneGeneration._Z_RANGE[data]
    depths, rgbs, Ts = [], [], []
    for _ in range(F):
        d = rs.uniform(z0 * 1.05, z1 * 0.95, (Hs, Ws)).astype(f32)
        flat = d.reshape(-1)
        bad = rs.choice(flat.size, 10, replace=False)
        flat[bad] = np.array([0, -1.5, np.nan, np.inf, -np.inf, z0 * 0.5, z1 * 1.5, np.nextafter(f32(z0), f32(0)),
                              np.nextafter(f32(z1), f32(np.inf)), -0.0], dtype=f32)
        flat[rs.choice(np.setdiff1d(np.arange(flat.size), bad), 2, replace=False)] = [f32(z0), f32(z1)]       # the ends are inside
        depths.append(d)
        rgbs.append(rs.randint(0, 256, (Hs, Ws, 3)).astype(np.uint8))
        Ts.append(small_pose(rs, 0.5, 3.0))
    return dict(depths=depths, rgbs=rgbs, K=intrinsics(data, (Hs, Ws)), Ts=Ts, z_near=z0, z_far=z1)


def twin_unproject(case):
    return GO.unproject(case["depths"], geometry.inverse_intrinsics(case["K"]), geometry.camera_to_world(case["Ts"]), case["z_near"],
                        case["z_far"])


@pytest.mark.parametrize("nq,nr", [(500, 2000), (257, 65), (64, 1)])
def test_twin_distances_against_a_kd_tree(nq, nr):
    from scipy.spatial import cKDTree
    q, r = cloud(nq, 1), cloud(nr, 2)
    d2, idx = GO.nn_brute(q, r)
    assert d2.dtype == f32 and idx.dtype == np.int32 and (idx >= 0).all() and (idx < nr).all()
    dist, _ = cKDTree(r.astype(np.float64)).query(q.astype(np.float64), k=1)
    want = dist * dist
    # three rounded differences, three products and two sums: at most 8 roundings of 2^-24, doubled through the square -> below
    # 2^-20 of the float64 minimum (the fp32 winner may be another point at a near tie: d2 is compared, not the index)
    assert (np.abs(d2.astype(np.float64) - want) <= 2.0 ** -20 * want).all()
    # the index is the lowest one that reaches the fp32 minimum
    for k in range(0, nq, 37):
        d = r - q[k]
        row = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert idx[k] == int(np.flatnonzero(row == row.min())[0]) and d2[k] == row.min()


def test_twin_rules_ties_nan_and_max_distance():
    r = np.array([[1, 1, 1], [np.nan, 0, 0], [1, 1, 1], [5, 5, 5], [0, np.inf, 0]], dtype=f32)
    q = np.array([[1, 1, 2], [np.nan, 1, 1], [5, 5, 4], [1, 1, 1], [0, np.inf, 0]], dtype=f32)
    d2, idx = GO.nn_brute(q, r)
    assert idx.tolist() == [0, -1, 3, 0, -1] and d2.tolist() == [1.0, np.inf, 1.0, 0.0, np.inf]
    d2, idx = GO.nn_brute(q, r, GO.max_d2_of(0.5))
    assert idx.tolist() == [-1, -1, -1, 0, -1] and d2[3] == 0 and np.isinf(d2[[0, 1, 2, 4]]).all()
    d2, idx = GO.nn_brute(q, r, GO.max_d2_of(1.0))                     # on the limit is inside
    assert idx.tolist() == [0, -1, 3, 0, -1]
    d2, idx = GO.nn_brute(q, np.full((4, 3), np.nan, dtype=f32))
    assert (idx == -1).all() and np.isinf(d2).all()
    assert GO.reduce(np.array([4.0, np.inf, 0.25, 1.0], dtype=f32), 1.0) == (5.25, 3.5, 3, 2)


@pytest.mark.parametrize("data", ["google_earth", "clevr-infinite"])
def test_twin_unprojection_against_float64(data):
    case = frames_case(data, 48, 40)
    got = twin_unproject(case).reshape(3, 48 * 40, 3)
    Kinv = np.abs(np.linalg.inv(case["K"]))
    i, j = np.meshgrid(np.arange(48.0), np.arange(40.0), indexing="ij")
    ray = np.stack([Kinv[r, 0] * j.ravel() + Kinv[r, 1] * i.ravel() + Kinv[r, 2] for r in range(3)])      # |a|, |b|, |c| bounds
    for f, (d, c, T) in enumerate(zip(case["depths"], case["rgbs"], case["Ts"])):
        with np.errstate(invalid="ignore"):
            ok = (np.isfinite(d) & (d >= f32(case["z_near"])) & (d <= f32(case["z_far"]))).ravel()
        assert ok.sum() == d.size - 10 and np.isnan(got[f][~ok]).all() and np.isfinite(got[f][ok]).all()
        want, _ = pointcloud.unproject_frame(np.where(ok.reshape(d.shape), d, 1).astype(np.float64), c, case["K"], T)
        # fp32 rounding of the stated expression: per term of X the rounding of Kinv, two products and two sums of the ray, the
        # product with d, the rounding of T, the product with T and the three sums: 10 roundings, bounded by 16 * 2^-24 times the
        # sum of the term magnitudes |T0| |x| + |T1| |y| + |T2| |z| + |T3|
        Tinv = np.abs(np.linalg.inv(T)[:3])
        mag = (Tinv[:, :3] @ (ray * np.abs(np.where(ok, d.ravel(), 1)).astype(np.float64))).T + Tinv[:, 3]
        err = np.abs(got[f].astype(np.float64) - want)
        assert (err[ok] <= 16 * EPS * mag[ok]).all(), float((err[ok] / mag[ok]).max() / EPS)
        assert err[ok].max() > 0                                         # (fp32 it is)


def test_chamfer_on_a_hand_example():
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], dtype=f32)
    y = np.array([[0, 0, 1], [1, 0, 0], [3, 0, 0]], dtype=f32)
    # x -> y: 1, 0, 5 (mean 2); y -> x: 1, 0, 4 (mean 5/3); summed
    assert GO.nn_brute(x, y)[0].tolist() == [1.0, 0.0, 5.0] and GO.nn_brute(y, x)[0].tolist() == [1.0, 0.0, 4.0]
    assert GO.nn_brute(x, y)[1].tolist() == [0, 1, 0]                   # (0,2,0) is 5 away from both y0 and y1: the lower index
    assert GO.chamfer(x, y) == pytest.approx(2.0 + 5.0 / 3.0, rel=1e-15)
    m = GO.cloud_metrics(x, y, 1.0)
    assert m["chamfer"] == pytest.approx(11.0 / 3.0, rel=1e-15)
    assert m["accuracy"] == pytest.approx((1 + 0 + 5 ** 0.5) / 3) and m["completeness"] == pytest.approx((1 + 0 + 2) / 3)
    assert m["precision"] == pytest.approx(2 / 3) and m["recall"] == pytest.approx(2 / 3) and m["fscore"] == pytest.approx(2 / 3)
    assert (m["n_pred"], m["n_ref"]) == (3, 3)


def test_default_grid_rule():
    lo, hi = np.array([1.0, 2.0, 3.0]), np.array([9.0, 6.0, 5.0])
    origin, h, g = geometry.grid_for(lo, hi, 64000)
    assert origin.dtype == f32 and origin.tolist() == [1.0, 2.0, 3.0]
    assert h == pytest.approx((8 * 4 * 2 * geometry.GRID_OCCUPANCY / 64000) ** (1 / 3), rel=1e-6)
    assert g == tuple(int(np.floor(e / h)) + 1 for e in (8, 4, 2)) and np.prod(g) <= 1.3 * 64000 / geometry.GRID_OCCUPANCY
    # degenerate boxes: a plane, a line, a point
    assert geometry.grid_for(lo, np.array([9.0, 6.0, 3.0]), 1000)[2][2] == 1
    o, h1, g1 = geometry.grid_for(lo, np.array([9.0, 2.0, 3.0]), 1000)
    assert g1[1:] == (1, 1) and 1 < g1[0] <= 8 * 1024 + 1
    assert geometry.grid_for(lo, lo, 5)[1:] == (1.0, (1, 1, 1))
    # a requested size is kept when the grid fits the cap, grown when it does not
    assert geometry.grid_for(lo, hi, 10, cell_size=0.5)[1:] == (0.5, (17, 9, 5))
    o, h2, g2 = geometry.grid_for(lo, hi, 10, cell_size=1e-4)
    assert h2 > 1e-4 and np.prod(g2) <= geometry.GRID_MAX_CELLS < np.prod(g2) * 1.25 ** 3 * 1.1
    with pytest.raises(ValueError):
        geometry.grid_for(lo, hi, 10, cell_size=0.0)
    assert geometry.max_d2_of(None) == np.inf and geometry.max_d2_of(0.1) == float(f32(0.1) * f32(0.1)) == float(GO.max_d2_of(0.1))


def test_geometry_argument_validation_without_gpu():
    lib = _lib.load()
    assert lib.sgam_abi_version() == 10                                 # additive: the ABI version stays
    names = ("sgam_points_unproject_f32", "sgam_points_nn_brute_f32", "sgam_points_grid_workspace_bytes", "sgam_points_grid_build",
             "sgam_points_nn_grid_f32", "sgam_points_nn_reduce_partials", "sgam_points_nn_reduce")
    for name in names:
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    # fake non-null pointers are never dereferenced: every check comes before the first device call
    p = ctypes.c_void_p(256)
    kinv = (ctypes.c_float * 9)(*([1.0] * 9))
    kp = ctypes.cast(kinv, ctypes.c_void_p)

    def unproject(depth_ptrs=p, rgb_ptrs=p, F=3, Hs=6, Ws=5, Kinv=kp, T=p, zn=0.1, zf=4.0, pts=p, cols=p):
        return lib.sgam_points_unproject_f32(depth_ptrs, rgb_ptrs, F, Hs, Ws, Kinv, T, zn, zf, pts, cols, None)

    for kw in (dict(depth_ptrs=None), dict(Kinv=None), dict(T=None), dict(pts=None), dict(F=0), dict(F=-1), dict(Hs=0), dict(Ws=-2),
               dict(rgb_ptrs=None), dict(cols=None),                    # colours in and out go together
               dict(F=1 << 15, Hs=1 << 8, Ws=1 << 8),                   # F * Hs * Ws = 2^31: the point index would not fit
               dict(zn=4.0, zf=0.1), dict(zn=float("nan")), dict(zf=float("nan"))):
        assert unproject(**kw) == -1, kw

    def brute(q=p, r=p, B=2, Nq=10, Nr=10, m=np.inf, d2=p, idx=p):
        return lib.sgam_points_nn_brute_f32(q, r, B, Nq, Nr, m, d2, idx, None)

    for kw in (dict(q=None), dict(r=None), dict(d2=None), dict(idx=None), dict(B=0), dict(B=65536), dict(Nq=0), dict(Nr=0), dict(Nq=-5),
               dict(m=-1.0), dict(m=float("nan"))):
        assert brute(**kw) == -1, kw

    size = lib.sgam_points_grid_workspace_bytes

    def r16(n):
        return (n + 15) // 16 * 16

    for nr, g in ((1, (1, 1, 1)), (1000, (7, 5, 3)), (6553600, (256, 256, 256)), (12345, (1 << 24, 1, 1)), (3, (1025, 1, 1))):
        c = g[0] * g[1] * g[2]
        assert size(nr, *g) == 16 * nr + r16(4 * (c + 1)) + r16(4 * c) + r16(4 * ((c + 1023) // 1024)), (nr, g)
    for bad in ((0, 1, 1, 1), (-1, 1, 1, 1), (10, 0, 1, 1), (10, 1, -1, 1), (10, 1, 1, 0), (10, (1 << 24) + 1, 1, 1), (10, 4096, 4096, 2),
                (10, 1 << 16, 1 << 16, 1 << 16)):
        assert size(*bad) == -1, bad
    ws = size(100, 4, 3, 2)

    def build(ref=p, Nr=100, o=(0.0, 0.0, 0.0), h=0.5, g=(4, 3, 2), w=p, wb=ws):
        return lib.sgam_points_grid_build(ref, Nr, *o, h, *g, w, wb, None)

    def query(q=p, Nq=7, Nr=100, o=(0.0, 0.0, 0.0), h=0.5, g=(4, 3, 2), w=p, wb=ws, m=np.inf, d2=p, idx=p):
        return lib.sgam_points_nn_grid_f32(q, Nq, Nr, *o, h, *g, w, wb, m, d2, idx, None)

    shared = (dict(Nr=0), dict(h=0.0), dict(h=-1.0), dict(h=float("nan")), dict(h=float("inf")), dict(o=(float("nan"), 0.0, 0.0)),
              dict(o=(0.0, float("inf"), 0.0)), dict(g=(0, 3, 2)), dict(g=(4, 3, -2)), dict(g=((1 << 24) + 1, 1, 1), wb=1 << 40),
              dict(g=(4096, 4096, 2), wb=1 << 40), dict(w=None), dict(wb=ws - 1), dict(wb=0), dict(w=ctypes.c_void_p(264)),
              dict(Nr=101))                                             # more points than the workspace was sized for
    for kw in shared + (dict(ref=None),):
        assert build(**kw) == -1, kw
    for kw in shared + (dict(q=None), dict(d2=None), dict(idx=None), dict(Nq=0), dict(m=-0.5), dict(m=float("nan"))):
        assert query(**kw) == -1, kw

    parts = lib.sgam_points_nn_reduce_partials
    assert [parts(n) for n in (1, 4096, 4097, 6553600)] == [4, 4, 8, 4 * 1600] and parts(0) == parts(-3) == -1
    for args in ((None, 10, 0.1, p), (p, 10, 0.1, None), (p, 0, 0.1, p), (p, -1, 0.1, p), (p, 10, -0.1, p), (p, 10, float("nan"), p)):
        assert lib.sgam_points_nn_reduce(*args, None) == -1, args
