"""GPU: the cloud clean-up kernels (csrc/point_nn.hip's k-NN kernels and csrc/point_cloud.hip through sgam_neurips22_amd/geometry.py)
against the numpy twin (tests/cloud_oracle.py): brute-force and grid k nearest neighbours bit for bit (d2 as uint32, index exactly)
at edge sizes, every k bucket, short rows, ties, exclude_self, NaN points, a distance limit and varied cell sizes; uniform voxel
sampling (index and count exactly); the statistical outlier rule and the normals within the stated fp64 bounds; and the scene-level
callers merged_point_cloud / export_point_clouds / geometry_metrics with their new arguments on both warp branches."""
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import geometry, pointcloud, testing

sys.path.insert(0, os.path.dirname(__file__))
import cloud_oracle as CO  # noqa: E402
import geometry_oracle as GO  # noqa: E402
from test_cloud_cpu import SPHERE_CENTRE, normal_cases, normal_guard, outlier_case  # noqa: E402
from test_geometry_cpu import cloud  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _knn(q, r, k, method, **kw):
    out = geometry.knn(_t(q), _t(r), k, method=method, **kw)
    assert out["d2"].is_cuda and out["d2"].dtype == torch.float32 and out["index"].dtype == torch.int32
    assert out["d2"].shape == out["index"].shape == (len(q), k)
    return out["d2"].cpu().numpy(), out["index"].cpu().numpy()


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(_bits(got[0]), _bits(want[0])), what


def _check(q, r, k, max_distance=None, exclude_self=False, cell_sizes=(None,), what=""):
    """brute and grid (at every cell size) against the twin; returns the twin's (d2, index)"""
    want = CO.knn_brute(q, r, k, CO.max_d2_of(max_distance), exclude_self)
    _same(_knn(q, r, k, "brute", max_distance=max_distance, exclude_self=exclude_self), want, ("brute", k, what))
    for cs in cell_sizes:
        _same(_knn(q, r, k, "grid", max_distance=max_distance, exclude_self=exclude_self, cell_size=cs), want, ("grid", k, cs, what))
    return want


SIZES = (1, 63, 64, 65, 257)
KS = (1, 2, 8, 9, 32)


# ---------------------------------------------------------------- k-NN
@pytest.mark.parametrize("nq", SIZES)
def test_knn_edge_sizes_equal_the_twin(nq):
    for nr in SIZES:
        q, r = cloud(nq, 10 + nq), cloud(nr, 20 + nr)
        for k in KS:
            d2, idx = _check(q, r, k, what=(nq, nr))
            held = min(k, nr)                                           # fewer reference points than k: a tail of -1 / +inf
            assert (idx[:, :held] >= 0).all() and (idx[:, held:] == -1).all() and np.isinf(d2[:, held:]).all()


@pytest.mark.parametrize("k", [8, 32])
def test_knn_more_than_one_tile_and_workgroup(k):
    _check(cloud(2500, 1), cloud(3001, 2), k, what="2500 x 3001")


def test_knn_of_one_is_nearest_neighbors():
    q, r = cloud(900, 3, 0.0, 11.0), cloud(3000, 4)
    r[::7] = np.nan
    for method in ("brute", "grid"):
        for md in (None, 0.4):
            nn = geometry.nearest_neighbors(_t(q), _t(r), method=method, max_distance=md)
            d2, idx = _knn(q, r, 1, method, max_distance=md)
            assert np.array_equal(_bits(nn["d2"].cpu().numpy()), _bits(d2[:, 0])) and np.array_equal(nn["index"].cpu().numpy(), idx[:, 0])
    want = GO.nn_brute(q, r)
    _same((d2[:, 0], idx[:, 0]), GO.nn_brute(q, r, GO.max_d2_of(0.4)), "the twin of the nearest neighbour")
    assert (want[1] >= 0).all()


def test_knn_duplicates_ties_and_exclude_self():
    r = cloud(600, 11)
    r2 = np.concatenate([r, r])                                          # every point twice: ties go by index
    q = np.concatenate([cloud(100, 12), r[::5]])
    for k in (2, 9):
        d2, idx = _check(q, r2, k, what="duplicated")
        assert (d2[100:, :2] == 0).all() and (idx[100:, 0] < 600).all() and (idx[100:, 1] == idx[100:, 0] + 600).all()
    for k in (1, 8, 32):
        d2, idx = _check(r2, r2, k, exclude_self=True, what="exclude_self")
        assert (idx != np.arange(1200)[:, None]).all() and (d2[:, 0] == 0).all()      # the copy, not the point itself
        assert (idx[:600, 0] == np.arange(600, 1200)).all() and (idx[600:, 0] == np.arange(600)).all()
    lattice = np.stack(np.meshgrid(*[np.arange(5.0)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    d2, idx = _check(lattice + f32(0.5), lattice, 8, cell_sizes=(None, 1.0, 0.37), what="cell centres: eight equal neighbours")
    inner = (lattice < 4).all(1)
    assert (d2[inner] == 0.75).all() and (np.diff(idx[inner], axis=1) > 0).all()
    with pytest.raises(ValueError, match="exclude_self"):
        geometry.knn(_t(q), _t(r2), 2, exclude_self=True)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="1..32"):
            geometry.knn(_t(q), _t(r2), bad)


def test_knn_nan_points_are_not_points():
    rs = np.random.RandomState(18)
    r, q = cloud(2000, 19), cloud(700, 20)
    r[rs.choice(2000, 600, replace=False), rs.randint(0, 3, 600)] = np.nan          # 30 %
    r[rs.choice(2000, 20, replace=False), 1] = np.inf
    q[rs.choice(700, 200, replace=False), rs.randint(0, 3, 200)] = np.nan
    q[5, 2] = -np.inf
    for k in (2, 16):
        d2, idx = _check(q, r, k, cell_sizes=(None, 0.4), what="NaN share")
        bad_q = ~np.isfinite(q).all(1)
        assert (idx[bad_q] == -1).all() and np.isinf(d2[bad_q]).all() and (idx[~bad_q] >= 0).all()
        assert np.isfinite(r[idx[~bad_q]]).all()
    d2, idx = _check(q, np.full((300, 3), np.nan, dtype=f32), 4, what="all-NaN reference")
    assert (idx == -1).all() and (d2 == np.inf).all()
    d2, idx = _check(r, r, 8, exclude_self=True, cell_sizes=(None, 0.4), what="NaN share on itself")
    assert (idx[~np.isfinite(r).all(1)] == -1).all()


def test_knn_max_distance_just_inside_and_just_outside():
    q, r = cloud(300, 23), cloud(2000, 24)
    k = 9
    d2, idx = CO.knn_brute(q, r, k + 1)
    row = 17
    inside = np.sqrt(np.float64(d2[row, k - 1]))                         # the k-th neighbour of query 17 ...
    for md in (float(np.nextafter(f32(inside), f32(np.inf))), float(np.nextafter(f32(inside), f32(0)))):
        got_d2, got_idx = _check(q, r, k, max_distance=md, cell_sizes=(None, 0.2, 3.0), what=("limit", md))
        lim = CO.max_d2_of(md)
        assert (got_idx[row, k - 1] >= 0) == bool(d2[row, k - 1] <= lim)
        assert (got_d2[got_idx >= 0] <= lim).all()
    assert CO.knn_brute(q, r, k, CO.max_d2_of(float(np.nextafter(f32(inside), f32(0)))))[1][row, k - 1] == -1     # ... just outside
    assert CO.knn_brute(q, r, k, CO.max_d2_of(float(np.nextafter(f32(inside), f32(np.inf)))))[1][row, k - 1] == idx[row, k - 1]
    d2, idx = _check(q, r, 4, max_distance=0.0, what="limit 0")
    assert (idx == -1).all()


def test_knn_queries_outside_the_box_and_degenerate_clouds():
    r = cloud(3000, 13)
    lo, hi = r.min(0), r.max(0)
    rs = np.random.RandomState(14)
    q = [cloud(50, 15)]
    for axes in ((0,), (1,), (2,), (0, 1), (0, 1, 2)):
        for sign, far in ((1, 3.0), (-1, 3.0), (1, 5e3), (-1, 1e6)):
            p = rs.uniform(lo, hi, (6, 3)).astype(f32)
            for a in axes:
                p[:, a] = (hi[a] if sign > 0 else lo[a]) + sign * f32(far)
            q.append(p)
    q.append(np.stack([lo, hi, f32(0.5) * (lo + hi)]))
    q = np.concatenate(q)
    for k in (2, 16):
        d2, idx = _check(q, r, k, cell_sizes=(None, 0.3, 2.5), what="outside")
        assert (idx >= 0).all()
    plane = cloud(700, 5)
    plane[:, 1] = 3.25
    _check(q, plane, 8, what="coplanar")
    _check(plane, plane, 9, exclude_self=True, what="coplanar on itself")
    line = cloud(400, 6)
    line[:, 0], line[:, 2] = 2.5, -1.0
    _check(q, line, 8, what="collinear")
    _check(line, line, 32, what="collinear on itself")
    _check(q, np.repeat(cloud(1, 8), 5, axis=0), 8, what="one point five times")


def test_knn_results_do_not_depend_on_the_cell_size():
    r, q = cloud(5000, 16), cloud(1000, 17, 0.0, 11.0)
    grid = geometry.PointGrid(_t(r))
    h = grid.cell_size
    for k in (8, 32):
        d2, idx = _check(q, r, k, cell_sizes=(0.25 * h, h, 4 * h), what="cell sizes")
        md = float(np.sqrt(np.median(d2[:, k // 2])))
        d2m, idxm = _check(q, r, k, max_distance=md, cell_sizes=(0.25 * h, h, 4 * h), what="cell sizes with a limit")
        assert 0.1 < (idxm >= 0).mean() < 0.9
    out = grid.query_knn(_t(q), 8)                                       # one grid, queried again
    _same((out["d2"].cpu().numpy(), out["index"].cpu().numpy()), CO.knn_brute(q, r, 8), "PointGrid.query_knn")


# ---------------------------------------------------------------- voxel sampling
def _voxel(p, voxel, origin=None):
    out = geometry.voxel_sample(_t(p), voxel, origin)
    assert out["index"].dtype == out["count"].dtype == torch.int32 and out["index"].is_cuda and out["index"].shape == out["count"].shape
    got = out["index"].cpu().numpy(), out["count"].cpu().numpy()
    want = CO.voxel_sample(p, voxel, origin)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (len(p), voxel, origin)
    assert (np.diff(got[0]) > 0).all() and got[1].sum() == np.isfinite(p).all(1).sum()
    return got


@pytest.mark.parametrize("n", [1, 64, 257, 5000])
def test_voxel_sample_equals_the_twin(n):
    p = cloud(n, 30 + n)                                                 # a 9 x 9 x 9 box
    index, count = _voxel(p, 100.0)
    assert len(index) == 1 and count[0] == n
    quarter = 9.0 / max(1.0, (n / 4.0) ** (1 / 3))                       # about n / 4 occupied voxels
    index, count = _voxel(p, quarter)
    assert n == 1 or len(index) < n
    index, count = _voxel(p, 9.0 / (8 * n ** (1 / 3)))                   # about one point per occupied voxel
    assert len(index) > 0.9 * n
    _voxel(p, quarter, origin=(5.0, 5.5, 6.0))                           # an origin inside the box
    rs = np.random.RandomState(n)
    q = p.copy()
    q[rs.rand(n) < 0.3] = np.nan
    _voxel(q, quarter)
    if n >= 64:
        assert np.isfinite(q[_voxel(q, quarter, origin=(5.0, 5.5, 6.0))[0]]).all()


def test_voxel_sample_copies_faces_and_shuffles():
    same = np.repeat(cloud(1, 3), 512, axis=0)
    index, count = _voxel(same, 0.01)
    assert index.tolist() == [0] and count.tolist() == [512]
    # exactly on voxel faces: o + j * voxel with o and voxel powers of two (every operation of the rule is exact)
    j = np.stack(np.meshgrid(*[np.arange(6.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    faces = (4.0 + j * 0.25).astype(f32)
    index, count = _voxel(np.concatenate([faces, faces + f32(0.0625)]), 0.25, origin=(4.0, 4.0, 4.0))
    assert len(index) == 216 and (count == 2).all() and (index >= 216).all()       # the copy nearer the centre
    index, count = _voxel(faces, 0.5, origin=(4.0, 4.0, 4.0))
    assert len(index) == 27 and (count == 8).all()
    # a shuffled cloud keeps the same coordinates (random points: no two members of a voxel tie exactly)
    p = cloud(5000, 77)
    perm = np.random.RandomState(78).permutation(5000)
    a, b = _voxel(p, 0.9), _voxel(p[perm], 0.9, origin=p.min(0))
    ka, kb = p[a[0]], p[perm][b[0]]
    order_a, order_b = np.lexsort(ka.T), np.lexsort(kb.T)
    assert np.array_equal(ka[order_a], kb[order_b]) and np.array_equal(a[1][order_a], b[1][order_b])
    empty = geometry.voxel_sample(_t(np.full((5, 3), np.nan, f32)), 1.0)
    assert empty["index"].numel() == 0 and empty["count"].numel() == 0


def test_voxel_sample_refuses_a_box_of_too_many_voxels():
    p = _t(cloud(100, 5))
    with pytest.raises(ValueError, match="2\\^20"):
        geometry.voxel_sample(p, 1e-6)
    with pytest.raises(ValueError, match="2\\^20"):
        geometry.voxel_sample(p, 0.01, origin=(0.0, 0.0, -20000.0))
    with pytest.raises(ValueError, match="voxel_size"):
        geometry.voxel_sample(p, 0.0)


# ---------------------------------------------------------------- statistical outliers
def test_statistical_outliers_equal_the_twin():
    p = outlier_case()
    want = CO.statistical_outliers(p, 20, 2.0)
    got = geometry.statistical_outliers(_t(p), 20, 2.0)
    assert got["keep"].dtype == torch.bool and got["mean_distance"].dtype == torch.float64 and got["keep"].is_cuda
    md, keep = got["mean_distance"].cpu().numpy(), got["keep"].cpu().numpy()
    rel = np.abs(md - want["mean_distance"]) / want["mean_distance"]
    print("mean_distance rel", rel.max(), *[(k, got[k], want[k]) for k in ("mean", "std", "threshold")])
    assert rel.max() <= 1e-12                                            # the tolerance of test_gpu_geometry's fp64 sums
    for k in ("mean", "std", "threshold"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), k
    compared = np.abs(want["mean_distance"] - want["threshold"]) > 1e-9 * want["threshold"]
    assert compared.mean() >= 0.99 and np.array_equal(keep[compared], want["keep"][compared])
    assert not keep[2000:].any()                                         # all 20 far points are removed
    q = p.copy()
    q[::50] = np.nan
    got, want = geometry.statistical_outliers(_t(q), 20, 2.0), CO.statistical_outliers(q, 20, 2.0)
    assert np.isnan(got["mean_distance"].cpu().numpy()[::50]).all() and not got["keep"].cpu().numpy()[::50].any()
    assert abs(got["threshold"] - want["threshold"]) <= 1e-12 * want["threshold"]
    for method in ("brute", "grid"):
        again = geometry.statistical_outliers(_t(p), 20, 2.0, method=method)
        assert torch.equal(again["keep"], geometry.statistical_outliers(_t(p), 20, 2.0)["keep"])


@pytest.mark.parametrize("n", [1, 255, 4095, 4096, 4097])
def test_md_reduce_at_the_edges_of_its_chunk(n):
    """sgam_points_md_reduce (one workgroup per 4096 values) in the library's two uses — the sum of md, then of (md - mean)^2 — on
    positive values of which about one in seven is NaN: the counts exactly, the sums within 1e-12 of numpy's float64 sum (the fold
    orders differ; every summand is non-negative, so either order stays within n * 2^-53 <= 5e-13 of the true sum)."""
    rs = np.random.RandomState(n)
    md = rs.uniform(0.5, 2.0, n)
    md[rs.rand(n) < 1.0 / 7.0] = np.nan
    finite = md[np.isfinite(md)]
    mean = float(finite.mean()) if len(finite) else 0.0
    for shift, squared, want in ((0.0, 0, finite.sum()), (mean, 1, ((finite - mean) ** 2).sum())):
        total, count = geometry._md_sum(_t(md), shift, squared)
        print("md_reduce", n, squared, total, float(want), count, len(finite))
        assert count == len(finite)
        assert abs(total - want) <= 1e-12 * want


# ---------------------------------------------------------------- normals
@pytest.mark.parametrize("name", ["plane", "sphere", "cylinder"])
def test_normals_equal_the_twin(name):
    p = normal_cases()[name]
    want, w = CO.normals(p, 16)
    got = geometry.estimate_normals(_t(p), 16)
    assert got.dtype == torch.float32 and got.shape == (2000, 3) and got.is_cuda
    n = got.cpu().numpy().astype(np.float64)
    guard = normal_guard(w)
    assert guard.mean() >= 0.9
    # fp32 rounding of a unit vector moves it by at most 2^-24 per component: 1 - |n . n_twin| grows by about 1e-14, no more
    dot = (n * want).sum(1) / np.linalg.norm(n, axis=1)
    print(name, "1 - |n . n_twin| max", (1 - np.abs(dot[guard])).max(), "guarded", guard.mean())
    assert (1 - np.abs(dot[guard]) <= 1e-9).all() and (dot[guard] > 0).all()
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6


def test_normals_orientation_and_short_neighbourhoods():
    p = normal_cases()["sphere"]
    radial = (p.astype(np.float64) - SPHERE_CENTRE) / 2.0
    # four viewpoints far outside, each point looked at from the one on its side
    views = (SPHERE_CENTRE + 50.0 * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]])).astype(f32)
    view_of = np.argmax(radial @ np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]]).T, axis=1).astype(np.int32)
    n = geometry.estimate_normals(_t(p), 16, _t(views), _t(view_of)).cpu().numpy().astype(np.float64)
    # where the viewpoint (50 away) stands well on the outside of the point — more than 25 along the radius, which a normal within
    # 0.44 of the radial direction (|n . radial| > 0.9) cannot outweigh — the normal points outwards
    facing = ((views[view_of].astype(np.float64) - p) * radial).sum(1) > 25.0
    assert facing.mean() > 0.5 and (np.abs((n * radial).sum(1)) > 0.9).all() and ((n * radial).sum(1)[facing] > 0.9).all()
    assert ((n * (views[view_of] - p)).sum(1) >= 0).all()
    want, w = CO.normals(p, 16, views, view_of)
    assert ((n * want).sum(1)[normal_guard(w)] > 0).all()
    # two valid neighbours: NaN
    few = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 1, 0.5]], dtype=f32)
    assert torch.isnan(geometry.estimate_normals(_t(few), 2)).all()
    n3 = geometry.estimate_normals(_t(few), 3).cpu().numpy()
    assert np.isfinite(n3[[0, 1, 3]]).all() and np.isnan(n3[2]).all()
    want3 = CO.normals(few, 3)[0]
    assert np.abs(np.abs((n3[[0, 1, 3]] * want3[[0, 1, 3]]).sum(1)) - 1).max() < 1e-6


# ---------------------------------------------------------------- scenes
@pytest.fixture(scope="module")
def model(golden):
    """the synthetic-weights model of test_gpu_geometry"""
    from sgam_neurips22_amd.config import default_params
    from sgam_neurips22_amd.generative_sensing_module.model import VQModel
    g = golden("vqgan_full_ge256.npz")
    m = VQModel(**default_params("google_earth"))
    sd = testing.synthetic_state_dict(m.state_dict(), seed=0)
    sd["quantize.embedding.weight"] = testing.codebook_from_stats(float(g["zmean"]), float(g["zstd"]), 4096, 256, int(g["cb_seed"]))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@pytest.mark.parametrize("branch", ["splat", "rgbd"])
def test_scene_clean_cloud_and_export(model, branch, tmp_path):
    from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
    kw = dict(use_rgbd_integration=True, tsdf_memory_budget_bytes=1 << 30) if branch == "rgbd" else {}
    scene = InfiniteSceneGeneration(model, "google_earth", output_dim=(3, 1), seed_frame=synthetic_seed_frame("google_earth", 0), **kw)
    scene.scene_expansion()
    assert len(scene.frames) == 3
    coords = [c for c, _ in sorted(scene.frames.items(), key=lambda kv: (kv[1]["index"], kv[0]))]
    z0, z1 = scene._Z_RANGE[scene.data]
    Ts = [scene.transform_grid[c[0]][c[1]]["T"] for c in coords]
    raw = geometry.unproject_frames([scene.frames[c]["depth"] for c in coords], [scene.frames[c]["rgb_u8"] for c in coords], scene.K, Ts, z0, z1)
    # the defaults: today's keys and bits
    for plain in (scene.merged_point_cloud(), scene.merged_point_cloud(voxel_size=None, nb_neighbors=None, normals=False)):
        assert set(plain) == {"points", "colors"} and torch.equal(plain["colors"], raw["colors"])
        assert torch.equal(plain["points"].view(torch.int32), raw["points"].view(torch.int32))
    pts, cols = raw["points"].cpu().numpy(), raw["colors"].cpu().numpy()
    valid = np.isfinite(pts).all(1)
    extent = pts[valid].max(0) - pts[valid].min(0)
    voxel = float(f32(extent.max() / 24))
    centres = geometry.camera_to_world(Ts)[:, :, 3]
    # the whole clean-up against the twin pipeline on the uncompacted cloud
    clean = scene.merged_point_cloud(voxel_size=voxel, nb_neighbors=20, std_ratio=2.0, normals=True, normal_k=16)
    assert set(clean) == {"points", "colors", "index", "normals"} and clean["index"].dtype == torch.int32
    want = CO.clean_pipeline(pts, 256 * 256, centres, voxel, 20, 2.0, True, 16)
    index = clean["index"].cpu().numpy()
    assert 100 < len(want["index"]) < 20000 and np.array_equal(index, want["index"])
    assert np.array_equal(_bits(clean["points"].cpu().numpy()), _bits(pts[index])) and np.array_equal(clean["colors"].cpu().numpy(), cols[index])
    n = clean["normals"].cpu().numpy().astype(np.float64)
    guard = normal_guard(want["eigenvalues"])
    dot = ((n * want["normals"]).sum(1) / np.linalg.norm(n, axis=1))[guard]           # (the fp32 rounding moves the length, first order)
    assert guard.mean() > 0.5 and (1 - np.abs(dot) <= 1e-9).all()
    to_view = centres[index // (256 * 256)].astype(np.float64) - pts[index]
    assert ((n * to_view).sum(1)[np.isfinite(n).all(1)] >= 0).all()                   # towards the frame's own camera
    # a sign can differ from the twin's only where the view direction is in the tangent plane within the normals' tolerance
    decided = np.abs((want["normals"] * to_view).sum(1)[guard]) > 1e-4 * np.linalg.norm(to_view, axis=1)[guard]
    assert (dot[decided] > 0).all()
    # the steps one at a time
    only_voxel = scene.merged_point_cloud(voxel_size=voxel)
    assert set(only_voxel) == {"points", "colors", "index"}
    assert np.array_equal(only_voxel["index"].cpu().numpy(), CO.clean_pipeline(pts, 256 * 256, centres, voxel)["index"])
    # the export: merged_pcds.ply untouched, merged_pcds_clean.ply read back
    a, b = tmp_path / "plain", tmp_path / "clean"
    counts_a = scene.export_point_clouds(str(a))
    counts_b = scene.export_point_clouds(str(b), clean=dict(voxel_size=voxel, nb_neighbors=20, normals=True))
    assert "merged_pcds_clean.ply" not in counts_a and not (a / "merged_pcds_clean.ply").exists()
    assert (a / "merged_pcds.ply").read_bytes() == (b / "merged_pcds.ply").read_bytes()
    assert counts_b["merged_pcds_clean.ply"] == len(index) and {k: v for k, v in counts_b.items() if k != "merged_pcds_clean.ply"} == counts_a
    ply = pointcloud.read_ply(str(b / "merged_pcds_clean.ply"))
    assert ply["points"].shape == (len(index), 3) and np.array_equal(ply["points"], pts[index].astype(np.float64))
    assert np.array_equal(ply["normals"], clean["normals"].cpu().numpy().astype(np.float64)) and np.array_equal(ply["colors_u8"], cols[index])
    with pytest.raises(ValueError, match="does not take"):
        scene.export_point_clouds(str(b), clean=dict(voxel=1.0))
    # metrics on one shared voxel grid: the cloud against itself, and against a copy with one frame repeated
    m = scene.geometry_metrics(raw["points"], 0.01, voxel_size=voxel)
    n_vox = len(CO.voxel_sample(pts, voxel)[0])
    assert m["fscore"] == 1.0 and m["chamfer"] == 0.0 and m["n_pred"] == m["n_ref"] == n_vox
    doubled = torch.cat([raw["points"], raw["points"][:256 * 256]])
    m2 = scene.geometry_metrics(doubled, 0.01, voxel_size=voxel)
    assert m2 == m                                                       # overlap does not change the resampled scores
    assert scene.geometry_metrics(doubled, 0.01)["n_ref"] > m["n_ref"]
