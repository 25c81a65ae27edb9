"""GPU: csrc/point_segment.hip against its numpy twin (tests/segmentation_oracle.py) — fixed-radius counts and DBSCAN bit for bit
at the workgroup and tile edges, brute force against the grid at every cell size, the plane RANSAC's hypotheses, labels and counts
bit for bit and its refit to one fp32 ulp, the cluster boxes exactly, run-to-run determinism, and scene.segment / the segmented
export on both warp branches."""
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import geometry, testing

sys.path.insert(0, os.path.dirname(__file__))
import segmentation_oracle as S  # noqa: E402
from test_segmentation_cpu import sklearn_cloud  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
NAN = np.nan
EPS, MINP = 0.12, 6


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def random_cloud(n, seed):
    """n points at 350 per unit volume (three neighbours within 0.12 on average: many clusters, borders and noise), a NaN point
    among them from 8 on"""
    rs = np.random.RandomState(seed)
    side = (n / 350.0) ** (1.0 / 3.0)
    p = (rs.rand(n, 3) * side).astype(f32)
    if n >= 8:
        p[n // 2] = NAN
    return p


def check_dbscan(points, eps, min_points, twin=None, **kw):
    twin = S.dbscan(points, eps, min_points) if twin is None else twin
    got = _host(geometry.cluster_dbscan(_t(points), eps, min_points, **kw))
    assert got["flag"].tolist() == [0]
    assert np.array_equal(got["count"], twin["count"])
    assert np.array_equal(got["core"], twin["core"])
    assert int(got["n_clusters"]) == int(twin["n_clusters"])
    assert np.array_equal(got["labels"], twin["labels"])
    assert np.array_equal(got["sizes"], twin["sizes"])
    rc = geometry.radius_count(_t(points), eps, **{k: v for k, v in kw.items() if k != "mask"}).cpu().numpy()
    if "mask" not in kw:
        assert np.array_equal(rc, twin["count"])
    return got


# ---------------------------------------------------------------- fixed radius and DBSCAN
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1024, 1025])
def test_dbscan_edge_sizes_equal_the_twin(n):
    p = random_cloud(n, n)
    twin = S.dbscan(p, EPS, 4)
    if n >= 255:
        assert int(twin["n_clusters"]) >= 2 and (twin["labels"] == -1).any() and (~twin["core"] & (twin["labels"] >= 0)).any()
    check_dbscan(p, EPS, 4, twin, method="brute")
    check_dbscan(p, EPS, 4, twin, method="grid")


@pytest.fixture(scope="module")
def cloud0():
    p = sklearn_cloud(0)
    return p, S.dbscan(p, EPS, MINP)


def test_dbscan_on_the_sklearn_cloud(cloud0):
    p, twin = cloud0
    assert 8 <= int(twin["n_clusters"]) <= 14
    check_dbscan(p, EPS, MINP, twin, method="brute")
    check_dbscan(p, EPS, MINP, twin, method="auto")


def test_dbscan_with_duplicated_points():
    rs = np.random.RandomState(7)
    base = (rs.rand(150, 3) * [0.6, 0.6, 0.2]).astype(f32)
    p = np.concatenate([base, base[:90], base[:40], base[10:20]])[rs.permutation(290)]
    for eps, mp in ((0.0, 2), (0.0, 3), (0.08, 5)):
        twin = S.dbscan(p, eps, mp)
        assert int(twin["n_clusters"]) >= 1
        check_dbscan(p, eps, mp, twin, method="brute")
        check_dbscan(p, eps, mp, twin, method="grid", cell_size=0.05)


def test_a_long_chain_is_one_cluster():
    # 3000 collinear points spaced 0.9 eps, indices shuffled: the union-find's trees span workgroups
    n = 3000
    x = (np.arange(n) * (0.9 * EPS)).astype(f32)
    p = np.stack([x, np.zeros(n, dtype=f32), np.zeros(n, dtype=f32)], axis=1)[np.random.RandomState(3).permutation(n)]
    for method in ("brute", "grid"):
        got = _host(geometry.cluster_dbscan(_t(p), EPS, 2, method=method))
        assert got["flag"].tolist() == [0] and int(got["n_clusters"]) == 1
        assert (got["labels"] == 0).all() and got["core"].all() and got["sizes"][0] == n and not got["sizes"][1:].any()
        assert np.array_equal(got["count"], S.radius_count(p, EPS))


def test_brute_force_equals_the_grid_at_every_cell_size(cloud0):
    p, twin = cloud0
    for cell in (EPS / 3, EPS, 4 * EPS, 100.0):                               # (100: one cell covers everything)
        check_dbscan(p, EPS, MINP, twin, method="grid", cell_size=cell)


def test_mask_equals_nan_by_hand(cloud0):
    p, _ = cloud0
    mask = np.random.RandomState(5).rand(len(p)) < 0.7
    q = p.copy()
    q[~mask] = NAN
    twin = S.dbscan(q, EPS, MINP)
    for method in ("brute", "grid"):
        got = check_dbscan(p, EPS, MINP, twin, method=method, mask=_t(mask))
        by_hand = _host(geometry.cluster_dbscan(_t(q), EPS, MINP, method=method))
        assert all(np.array_equal(got[k], by_hand[k]) for k in got)


def test_dbscan_boundary_cases_on_the_device():
    p = random_cloud(20, 0)
    got = _host(geometry.cluster_dbscan(_t(p), 10.0, 21, method="brute"))
    assert (got["labels"] == -1).all() and int(got["n_clusters"]) == 0 and not got["core"].any() and not got["sizes"].any()
    for method in ("brute", "grid"):
        got = _host(geometry.cluster_dbscan(_t(np.full((7, 3), NAN, dtype=f32)), 1.0, 1, method=method))
        assert (got["labels"] == -1).all() and int(got["n_clusters"]) == 0 and not got["count"].any()
    # the border point at equal d2 from two clusters (test_segmentation_cpu): the lower core index
    tie = np.array([[1.0, 0, 0], [0.75, 0, 0], [1.25, 0, 0], [-1.0, 0, 0], [-0.75, 0, 0], [-1.25, 0, 0], [0, 0, 0]], dtype=f32)
    for cloud in (tie, tie * f32(-1)):
        for method in ("brute", "grid"):
            assert geometry.cluster_dbscan(_t(cloud), 0.75, 4, method=method)["labels"].cpu().tolist() == [0, 0, 0, 1, 1, 1, 0]


# ---------------------------------------------------------------- planes
def plane_cloud(n, seed, noise=0.002):
    """a tilted plane (unit normal, |d| < 2) with z noise under a slab of clutter"""
    rs = np.random.RandomState(seed)
    m = (2 * n) // 3
    xy = rs.rand(m, 2) * 2 - 1
    z = 0.3 * xy[:, 0] - 0.2 * xy[:, 1] + 0.5 + rs.randn(m) * noise
    p = np.concatenate([np.c_[xy, z], rs.rand(n - m, 3) * [2, 2, 1.5] - [1, 1, 0.2]]).astype(f32)[rs.permutation(n)]
    p[5] = NAN
    return p


def check_planes(p, thr, max_planes, min_inliers, H, seed, **kw):
    twin = S.segment_planes(p, thr, max_planes, min_inliers, H, seed)
    got = _host(geometry.segment_planes(_t(p), thr, max_planes, min_inliers, H, seed, **kw))
    assert np.array_equal(_bits(got["ransac_planes"]), _bits(twin["ransac_planes"]))
    assert np.array_equal(got["counts"], twin["counts"])
    assert np.array_equal(got["labels"], twin["labels"])
    # the refit against the twin's float64 value rounded to fp32, within 2^-22: a unit normal and |d| < 2 make one fp32 ulp at most
    # 2^-23; the fp64 work differs by about 1e-13, which can move the rounding by one ulp; the bound is that, doubled
    want = twin["planes64"].astype(f32)
    assert np.array_equal(np.isnan(got["planes"]), np.isnan(want))
    found = ~np.isnan(want).any(axis=1)
    if found.any():
        assert np.abs(want[found, 3]).max() < 2
        assert np.abs(got["planes"][found].astype(np.float64) - want[found].astype(np.float64)).max() <= 2.0 ** -22
    return got, twin


@pytest.mark.parametrize("H", [1, 257, 1000])
def test_planes_equal_the_twin(H):
    p = plane_cloud(1500, H)                                                  # (1500: not a multiple of the 1024-point tile)
    got, twin = check_planes(p, 0.01, 1, 3, H, 11)
    if H >= 257:
        assert twin["counts"][0] >= 900
        assert abs(float(np.dot(twin["planes64"][0, :3], np.array([-0.3, 0.2, 1.0]) / np.sqrt(1.13)))) > 0.9999


def test_every_hypothesis_scores_n_on_a_flat_cloud():
    rs = np.random.RandomState(2)
    p = np.c_[rs.rand(700, 2), np.full(700, 0.5)].astype(f32)
    got, twin = check_planes(p, 0.01, 1, 3, 100, 4)
    hyp = S.hypotheses(p, np.arange(700), 100, 0, 4)
    first = int(np.flatnonzero(np.isfinite(hyp).all(axis=1))[0])
    assert got["counts"].tolist() == [700] and np.array_equal(_bits(got["ransac_planes"][0]), _bits(hyp[first]))
    assert (S.score(p, np.ones(700, dtype=bool), hyp, 0.01)[np.isfinite(hyp).all(axis=1)] == 700).all()


def floor_and_blobs(seed=0):
    rs = np.random.RandomState(50 + seed)
    g = np.stack(np.meshgrid(np.arange(24), np.arange(24), indexing="ij"), -1).reshape(-1, 2) / 12.0
    floor = np.c_[g, rs.randn(576) * 0.002]
    blobs = [rs.randn(60, 3) * 0.05 + c for c in ([0.4, 0.4, 0.35], [1.5, 0.5, 0.3], [1.0, 1.5, 0.4])]
    return np.concatenate([floor] + blobs).astype(f32)


@pytest.mark.parametrize("seed", range(8))
def test_floor_under_three_blobs(seed):
    p = floor_and_blobs()
    got, twin = check_planes(p, 0.01, 1, 3, 64, seed)
    assert got["counts"][0] == twin["counts"][0] > 288                        # the floor is found: more than half of its 576 points
    assert abs(got["planes"][0, 2]) > 0.999 and (got["labels"][576:] == -1).all()


def test_two_planes_and_an_empty_third_slot():
    rs = np.random.RandomState(9)
    a = np.c_[rs.rand(900, 2) * 2, rs.randn(900) * 0.001]                     # z = 0, 900 points
    b = np.c_[rs.randn(400) * 0.001 - 1.0, rs.rand(400, 2) * 2]               # x = -1, 400 points
    c = rs.rand(60, 3) * [1, 1, 1] + [0.5, 0.5, 1.0]                          # clutter: no plane holds 100 of these
    p = np.concatenate([a, b, c]).astype(f32)[rs.permutation(1360)]
    got, twin = check_planes(p, 0.01, 3, 100, 200, 1)
    assert got["counts"][0] > got["counts"][1] >= 300 and got["counts"][2] == 0 and np.isnan(got["planes"][2]).all()
    assert np.isnan(got["ransac_planes"][2]).all() and not np.isnan(got["planes"][:2]).any()
    assert [(got["labels"] == r).sum() for r in range(3)] == got["counts"].tolist()      # disjoint: one label per point
    assert abs(got["planes"][0, 2]) > 0.999 and abs(got["planes"][1, 0]) > 0.999


def test_plane_boundary_cases_on_the_device():
    thr = f32(0.01)
    beyond = np.nextafter(thr, f32(np.inf))
    z = np.array([0, thr, -thr, beyond, -beyond, NAN], dtype=f32)
    p = np.stack([np.arange(6, dtype=f32), np.zeros(6, dtype=f32), z], axis=1)
    planes = np.array([[0, 0, 1, 0], [NAN, NAN, NAN, NAN], [0, 0, 1, 0]], dtype=f32)
    labels = np.array([-1, -1, 0, -1, -1, -1], dtype=np.int32)
    for R in (0, 1, 2, 4):
        assert geometry.plane_score(_t(p), _t(planes), 0.01, hypotheses_per_lane=R).cpu().tolist() == [3, 0, 3]
        assert geometry.plane_score(_t(p), _t(planes), float(beyond), hypotheses_per_lane=R).cpu().tolist() == [5, 0, 5]
        assert geometry.plane_score(_t(p), _t(planes), 0.01, labels=_t(labels), hypotheses_per_lane=R).cpu().tolist() == [2, 0, 2]
    line = np.stack([np.arange(40, dtype=f32), 2 * np.arange(40, dtype=f32), np.zeros(40, dtype=f32)], axis=1)
    few = np.array([[0, 0, 0], [NAN, 0, 0], [1, 0, 0], [NAN, NAN, NAN]], dtype=f32)
    for cloud in (line, few):
        got = _host(geometry.segment_planes(_t(cloud), 0.01, 2, 3, 50, 1))
        assert np.isnan(got["planes"]).all() and np.isnan(got["ransac_planes"]).all()
        assert got["counts"].tolist() == [0, 0] and (got["labels"] == -1).all()
    one = geometry.segment_plane(_t(line), 0.01, 50, 1)
    assert set(one) == {"plane", "ransac_plane", "inliers", "count"} and not bool(one["inliers"].any()) and int(one["count"]) == 0


@pytest.mark.parametrize("R", [1, 2, 4])
def test_plane_score_layouts_equal_the_twin(R):
    p = plane_cloud(2500, 21)                                                 # more than two tiles, a ragged last one
    active = np.random.RandomState(1).rand(2500) < 0.8
    labels = np.where(active, -1, 0).astype(np.int32)
    hyp = S.hypotheses(p, np.flatnonzero(active & S.finite3(p)), 1100, 0, 5)  # 1100: a ragged last hypothesis tile for every R
    want = S.score(p, active & S.finite3(p), hyp, 0.02)
    assert want.max() > 1000
    assert np.array_equal(geometry.plane_score(_t(p), _t(hyp), 0.02, labels=_t(labels), hypotheses_per_lane=R).cpu().numpy(), want)


def test_segment_plane_is_the_one_plane_case():
    p = plane_cloud(1500, 3)
    mask = np.random.RandomState(2).rand(1500) < 0.9
    one = _host(geometry.segment_plane(_t(p), 0.01, 100, 2, mask=_t(mask)))
    q = p.copy()
    q[~mask] = NAN
    twin = S.segment_planes(q, 0.01, 1, 3, 100, 2)
    assert np.array_equal(_bits(one["ransac_plane"]), _bits(twin["ransac_planes"][0])) and int(one["count"]) == twin["counts"][0]
    assert np.array_equal(one["inliers"], twin["labels"] == 0)


# ---------------------------------------------------------------- determinism, boxes
def test_two_runs_give_the_same_bits(cloud0):
    p, _ = cloud0
    for fn in (lambda: geometry.cluster_dbscan(_t(p), EPS, MINP, method="grid"), lambda: geometry.cluster_dbscan(_t(p), EPS, MINP, method="brute"),
               lambda: geometry.segment_planes(_t(floor_and_blobs()), 0.01, 2, 20, 300, 3),
               lambda: geometry.segment_cloud(_t(floor_and_blobs()), 0.01, 0.12, 5, num_iterations=100)):
        a, b = _host(fn()), _host(fn())
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_cluster_boxes_equal_numpy(cloud0):
    p, twin = cloud0
    n = int(twin["n_clusters"])
    labels = twin["labels"].copy()
    labels[10] = n + 5                                                        # a label outside the range is ignored
    got = _host(geometry.cluster_boxes(_t(p), _t(labels), n + 1))             # (one label more than there are clusters: it stays empty)
    want = S.cluster_boxes(p, labels, n + 1)
    assert np.array_equal(got["count"], want["count"]) and got["count"][n] == 0
    assert np.array_equal(_bits(got["lo"]), _bits(want["lo"])) and np.array_equal(_bits(got["hi"]), _bits(want["hi"]))
    assert np.array_equal(got["count"][:n], np.bincount(labels[(labels >= 0) & (labels < n)], minlength=n))
    signs = np.array([[-1.5, 0.0, 2.0], [-0.25, -0.0, 1.0], [-3.0, 1e-30, -1e-30]], dtype=f32)           # negative and tiny keys
    got = _host(geometry.cluster_boxes(_t(signs), _t(np.zeros(3, dtype=np.int32)), 1))
    assert np.array_equal(got["lo"][0], signs.min(axis=0)) and np.array_equal(got["hi"][0], signs.max(axis=0))
    assert geometry.cluster_boxes(_t(signs), _t(np.zeros(3, dtype=np.int32)), 0)["count"].shape == (0,)


def test_segment_cloud_separates_floor_and_blobs():
    p = floor_and_blobs()
    out = _host(geometry.segment_cloud(_t(p), 0.01, 0.12, 5, num_iterations=100))
    assert int(out["n_clusters"]) == 3 and out["flag"].tolist() == [0]
    assert (out["cluster_labels"][out["plane_labels"] >= 0] == -1).all()       # a point on a plane is in no cluster
    assert [len(set(out["cluster_labels"][576 + 60 * b:636 + 60 * b].tolist()) - {-1}) for b in range(3)] == [1, 1, 1]


# ---------------------------------------------------------------- scenes
@pytest.fixture(scope="module")
def model(golden):
    """the synthetic-weights model of test_gpu_pointview"""
    from sgam_neurips22_amd.config import default_params
    from sgam_neurips22_amd.generative_sensing_module.model import VQModel
    g = golden("vqgan_full_ge256.npz")
    m = VQModel(**default_params("google_earth"))
    sd = testing.synthetic_state_dict(m.state_dict(), seed=0)
    sd["quantize.embedding.weight"] = testing.codebook_from_stats(float(g["zmean"]), float(g["zstd"]), 4096, 256, int(g["cb_seed"]))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@pytest.mark.parametrize("branch", ["splat", "rgbd"])
def test_scene_segment_and_export(model, branch, tmp_path):
    from sgam_neurips22_amd import pointcloud
    from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
    scene = InfiniteSceneGeneration(model, "google_earth", output_dim=(4, 1), seed_frame=synthetic_seed_frame("google_earth", 0),
                                    **(dict(use_rgbd_integration=True, tsdf_memory_budget_bytes=1 << 30) if branch == "rgbd" else {}))
    scene.scene_expansion()
    coords = [c for c, _ in sorted(scene.frames.items(), key=lambda kv: (kv[1]["index"], kv[0]))]
    # the first frame's depth: a floor at depth 3 and the tops of two separated boxes at depth 2.6
    depth = np.full((256, 256), 3.0, dtype=f32)
    depth[40:100, 40:100] = 2.6
    depth[150:220, 140:210] = 2.6
    scene.frames[coords[0]]["depth"] = _t(depth)
    args = dict(plane_threshold=0.02, eps=0.12, min_points=5, voxel_size=0.05, frames=[coords[0]], num_iterations=64)
    seg = scene.segment(**args)
    n = seg["points"].shape[0]
    assert 1000 < n < 65536 and seg["colors"].shape == (n, 3) and seg["plane_labels"].shape == (n,) and seg["cluster_labels"].shape == (n,)
    assert seg["planes"].shape == (1, 4) and int(seg["plane_counts"][0]) > n // 2 and seg["plane_ratio"] > 0.5
    assert seg["plane_ratio"] == int(seg["plane_counts"][0]) / n
    assert seg["n_clusters"] == 2 and seg["cluster_sizes"].shape == (2,) and seg["cluster_boxes"]["lo"].shape == (2, 3)
    assert int(seg["cluster_sizes"].sum()) + int(seg["plane_counts"][0]) == n           # nothing is noise here
    assert np.array_equal(seg["cluster_boxes"]["count"].cpu().numpy(), seg["cluster_sizes"].cpu().numpy())
    # the export: the palette's colours, and without `segment` the files of today
    plain = scene.export_point_clouds(str(tmp_path / "plain"))
    full = scene.export_point_clouds(str(tmp_path / "full"), segment=args)
    assert "merged_pcds_segmented.ply" not in plain and sorted(os.listdir(tmp_path / "plain")) == sorted(plain)
    assert sorted(os.listdir(tmp_path / "full")) == sorted(list(plain) + ["merged_pcds_segmented.ply"])
    assert full["merged_pcds_segmented.ply"] == n
    ply = pointcloud.read_ply(str(tmp_path / "full" / "merged_pcds_segmented.ply"))
    assert np.array_equal(ply["points"].astype(f32), seg["points"].cpu().numpy())
    grey = geometry.SEGMENT_PLANE_GREYS[0]
    want = {(grey, grey, grey), geometry.SEGMENT_PALETTE[0], geometry.SEGMENT_PALETTE[1]}
    assert {tuple(int(v) for v in c) for c in np.unique(ply["colors_u8"], axis=0)} == want
    on_plane = seg["plane_labels"].cpu().numpy() == 0
    assert (ply["colors_u8"][on_plane] == grey).all()
