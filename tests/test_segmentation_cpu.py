"""CPU: the numpy twin of the segmentation kernels (tests/segmentation_oracle.py) against hand-derived cases and against
sklearn's DBSCAN, and the argument validation of the new entry points (no launch, no GPU)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import segmentation_oracle as S  # noqa: E402

from sgam_neurips22_amd import _lib  # noqa: E402

f32 = np.float32
NAN = np.nan


def sklearn_cloud(s):
    rs = np.random.RandomState(100 + s)
    cloud = np.concatenate([rs.rand(500, 3) * [2, 1, .3], rs.rand(300, 3) * .5 + [3, 0, 0]]).astype(f32)
    cloud[3] = NAN
    return cloud


# ---------------------------------------------------------------- DBSCAN: hand-derived cases
def test_eps_zero_only_exact_duplicates_are_neighbours():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [1, 0, 0], [1, 0, 0], [2, 2, 2], [NAN, 0, 0]], dtype=f32)
    assert S.radius_count(p, 0.0).tolist() == [2, 3, 2, 3, 3, 1, 0]
    r = S.dbscan(p, 0.0, 2)
    assert r["labels"].tolist() == [0, 1, 0, 1, 1, -1, -1]
    assert int(r["n_clusters"]) == 2 and r["sizes"][:2].tolist() == [2, 3] and not r["sizes"][2:].any()
    assert r["core"].tolist() == [True] * 5 + [False, False]


def test_min_points_one_gives_the_components_of_the_eps_graph():
    # a chain 0 - 1 - 2 at spacing 1, a pair 3 - 4, a single 5; eps 1: every point is core
    p = np.array([[5, 0, 0], [6, 0, 0], [7, 0, 0], [0, 0, 0], [0, 1, 0], [20, 0, 0]], dtype=f32)[[3, 0, 5, 1, 4, 2]]
    #   index:    0: (0,0,0)  1: (5,0,0)  2: (20,0,0)  3: (6,0,0)  4: (0,1,0)  5: (7,0,0)
    r = S.dbscan(p, 1.0, 1)
    assert r["core"].all()
    assert r["labels"].tolist() == [0, 1, 2, 1, 0, 1]                        # numbered by the least index of each component
    assert int(r["n_clusters"]) == 3 and r["sizes"][:3].tolist() == [2, 3, 1]


def test_min_points_above_n_is_all_noise_and_an_all_nan_cloud_too():
    p = np.random.RandomState(0).rand(20, 3).astype(f32)
    r = S.dbscan(p, 10.0, 21)
    assert (r["count"] == 20).all() and not r["core"].any() and (r["labels"] == -1).all() and int(r["n_clusters"]) == 0
    r = S.dbscan(np.full((7, 3), NAN, dtype=f32), 1.0, 1)
    assert not r["count"].any() and not r["core"].any() and (r["labels"] == -1).all() and int(r["n_clusters"]) == 0


def test_border_point_at_equal_d2_goes_to_the_lower_core_index():
    # two clusters of three cores each around x = -1 and x = +1 (exact binary coordinates), a border point at the origin at the
    # same fp32 d2 = 0.5625 from core 4 (x = +0.75) and core 1 (x = -0.75); listed so that the higher cluster holds the lower index
    p = np.array([[1.0, 0, 0],        # 0  cluster A
                  [0.75, 0, 0],       # 1  cluster A, in reach of the border point
                  [1.25, 0, 0],       # 2  cluster A
                  [-1.0, 0, 0],       # 3  cluster B
                  [-0.75, 0, 0],      # 4  cluster B, in reach at the same d2
                  [-1.25, 0, 0],      # 5  cluster B
                  [0.0, 0, 0]],       # 6  the border point: 3 neighbours (itself, 1, 4) < min_points
                 dtype=f32)
    r = S.dbscan(p, 0.75, 4)
    assert r["count"].tolist() == [3, 4, 3, 3, 4, 3, 3]
    # cores: 1 and 4 only (count 4); each is its own cluster; 0 and 2 are borders of 1; 3 and 5 of 4; 6 ties -> core 1
    assert r["core"].tolist() == [False, True, False, False, True, False, False]
    assert r["labels"].tolist() == [0, 0, 0, 1, 1, 1, 0]
    # the same cloud with the two sides swapped: the tie still goes to the lower core index, now on the other side
    q = p * f32(-1)
    assert S.dbscan(q, 0.75, 4)["labels"].tolist() == [0, 0, 0, 1, 1, 1, 0]
    # and moving core 4 closer by one ulp takes the border point away from the lower index
    p2 = p.copy()
    p2[4, 0] = np.nextafter(f32(-0.75), f32(0))
    assert S.dbscan(p2, 0.75, 4)["labels"][6] == 1


# ---------------------------------------------------------------- planes: hand-derived cases
def test_points_at_exactly_the_threshold_are_inliers_and_one_ulp_beyond_are_not():
    thr = f32(0.01)                                                           # (not a dyadic number: fp32(0.01) is what is compared)
    beyond = np.nextafter(thr, f32(np.inf))
    plane = np.array([[0, 0, 1, 0]], dtype=f32)                               # the distance of (x, y, z) is |z|, exactly
    z = np.array([0, thr, -thr, beyond, -beyond, NAN], dtype=f32)
    p = np.stack([np.arange(6, dtype=f32), np.zeros(6, dtype=f32), z], axis=1)
    assert S.inlier(plane, p, 0.01)[0].tolist() == [True, True, True, False, False, False]
    assert S.inlier(plane, p, beyond)[0].tolist() == [True, True, True, True, True, False]
    assert S.score(p, np.array([1, 1, 0, 1, 1, 1], dtype=bool), plane, thr).tolist() == [2]
    # with an offset: ((0 * x + 0 * y) + 1 * z) + -0.5 at z = 0.625 is 0.125 exactly; one ulp of z more is beyond it
    plane = np.array([[0, 0, 1, -0.5]], dtype=f32)
    p[:, 2] = [0.5, 0.625, 0.375, np.nextafter(f32(0.625), f32(np.inf)), np.nextafter(f32(0.375), f32(-np.inf)), NAN]
    assert S.inlier(plane, p, 0.125)[0].tolist() == [True, True, True, False, False, False]


def test_collinear_cloud_and_fewer_than_three_points_give_nan_and_zero():
    line = np.stack([np.arange(40, dtype=f32), 2 * np.arange(40, dtype=f32), np.zeros(40, dtype=f32)], axis=1)
    few = np.array([[0, 0, 0], [NAN, 0, 0], [1, 0, 0], [NAN, NAN, NAN]], dtype=f32)
    for cloud in (line, few):
        r = S.segment_planes(cloud, 0.01, 2, 3, 50, 1)
        assert np.isnan(r["planes"]).all() and np.isnan(r["ransac_planes"]).all()
        assert r["counts"].tolist() == [0, 0] and (r["labels"] == -1).all()


def test_draws_are_distinct_in_range_and_differ_by_round():
    a, b = S.draw(500, 7, 0, 3), S.draw(500, 7, 1, 3)
    ok = (a >= 0).all(axis=1)
    assert ok.sum() > 450 and (a[ok] < 7).all()
    assert all(len(set(row)) == 3 for row in a[ok].tolist())
    assert (a != b).any()
    assert (S.draw(10, 2, 0, 0) == -1).all()                                  # fewer than three active points


def test_plane_on_a_grid_cloud_is_found_and_refitted():
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 2).astype(f32) * f32(0.25)
    p = np.concatenate([np.c_[g, np.full(64, 0.5, dtype=f32)], np.random.RandomState(1).rand(20, 3).astype(f32) + [0, 0, 2]]).astype(f32)
    r = S.segment_planes(p, 0.01, 1, 3, 32, 0)
    assert r["counts"].tolist() == [64] and (r["labels"][:64] == 0).all() and (r["labels"][64:] == -1).all()
    n = r["planes"][0]
    assert abs(abs(n[2]) - 1) < 1e-6 and abs(n[0]) < 1e-6 and abs(n[1]) < 1e-6 and abs(abs(n[3]) - 0.5) < 1e-6
    assert float(np.dot(r["planes"][0, :3], r["ransac_planes"][0, :3])) > 0


# ---------------------------------------------------------------- against sklearn
@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_twin_matches_sklearn_dbscan(s):
    cluster = pytest.importorskip("sklearn.cluster")
    cloud, eps, min_points = sklearn_cloud(s), 0.12, 6
    ok = S.finite3(cloud)
    # the condition first: no pairwise distance within a relative 1e-6 of eps, so fp32 and float64 cannot disagree
    v = cloud[ok].astype(np.float64)
    d = np.sqrt(((v[:, None, :] - v[None, :, :]) ** 2).sum(-1))
    assert np.abs(d - eps).min() > 1e-6 * eps
    ref = cluster.DBSCAN(eps=eps, min_samples=min_points).fit(v)
    ref_labels = np.full(len(cloud), -1)
    ref_labels[ok] = ref.labels_
    ref_core = np.zeros(len(cloud), dtype=bool)
    ref_core[np.flatnonzero(ok)[ref.core_sample_indices_]] = True
    r = S.dbscan(cloud, eps, min_points)
    assert (r["core"] == ref_core).all()                                     # core set
    assert (r["labels"][ref_core] == ref_labels[ref_core]).all()             # core partition and numbering
    assert ((r["labels"] == -1) == (ref_labels == -1)).all()                 # noise set
    assert int(r["n_clusters"]) == ref_labels.max() + 1 and 8 <= int(r["n_clusters"]) <= 14
    assert r["labels"][3] == -1 and r["count"][3] == 0                       # the NaN point
    # (border labels are not compared: the least (d2, index) rule is the stated difference from first come, first served)


# ---------------------------------------------------------------- the ABI without a GPU
def test_new_entry_points_validate_before_any_launch():
    lib = _lib.load()
    E, W = -1, -3
    one = ctypes.c_void_p(16)                 # a non-NULL, 16-byte aligned address that is never dereferenced: every call is refused
    grid = (0.0, 0.0, 0.0, 1.0, 1, 1, 1)
    assert lib.sgam_points_radius_count_brute_f32(None, 4, 1.0, one, None) == E
    assert lib.sgam_points_radius_count_brute_f32(one, 4, 1.0, None, None) == E
    assert lib.sgam_points_radius_count_brute_f32(one, 0, 1.0, one, None) == E
    assert lib.sgam_points_radius_count_brute_f32(one, 4, -1.0, one, None) == E
    assert lib.sgam_points_radius_count_brute_f32(one, 4, float("nan"), one, None) == E
    gbytes = lib.sgam_points_grid_workspace_bytes(4, 1, 1, 1)
    assert lib.sgam_points_radius_count_grid_f32(None, 4, *grid, one, gbytes, 1.0, one, None) == E
    assert lib.sgam_points_radius_count_grid_f32(one, 0, *grid, one, gbytes, 1.0, one, None) == E
    assert lib.sgam_points_radius_count_grid_f32(one, 4, *grid, one, gbytes - 1, 1.0, one, None) == E      # short grid tables
    assert lib.sgam_points_radius_count_grid_f32(one, 4, 0.0, 0.0, 0.0, 0.0, 1, 1, 1, one, gbytes, 1.0, one, None) == E

    assert lib.sgam_points_dbscan_workspace_bytes(0) == E
    need = lib.sgam_points_dbscan_workspace_bytes(1000)
    assert need == 2 * 4000 + (4000 + 4016 + 16)
    outs = (one,) * 6
    assert lib.sgam_points_dbscan_brute_f32(None, 1000, 1.0, 4, one, need, *outs, None) == E
    assert lib.sgam_points_dbscan_brute_f32(one, 0, 1.0, 4, one, need, *outs, None) == E
    assert lib.sgam_points_dbscan_brute_f32(one, 1000, 1.0, 0, one, need, *outs, None) == E
    assert lib.sgam_points_dbscan_brute_f32(one, 1000, 1.0, 4, one, need, one, one, one, one, one, None, None) == E
    assert lib.sgam_points_dbscan_brute_f32(one, 1000, 1.0, 4, one, need - 1, *outs, None) == W
    assert lib.sgam_points_dbscan_brute_f32(one, 1000, 1.0, 4, None, need, *outs, None) == W
    assert lib.sgam_points_dbscan_brute_f32(one, 1000, 1.0, 4, ctypes.c_void_p(20), need, *outs, None) == W
    g1000 = lib.sgam_points_grid_workspace_bytes(1000, 1, 1, 1)
    assert lib.sgam_points_dbscan_grid_f32(None, 1000, *grid, one, g1000, 1.0, 4, one, need, *outs, None) == E
    assert lib.sgam_points_dbscan_grid_f32(one, 0, *grid, one, g1000, 1.0, 4, one, need, *outs, None) == E
    assert lib.sgam_points_dbscan_grid_f32(one, 1000, *grid, one, g1000 - 1, 1.0, 4, one, need, *outs, None) == E
    assert lib.sgam_points_dbscan_grid_f32(one, 1000, *grid, one, g1000, 1.0, 4, one, need - 1, *outs, None) == W

    assert lib.sgam_points_planes_workspace_bytes(0, 10) == E and lib.sgam_points_planes_workspace_bytes(10, 0) == E
    assert lib.sgam_points_planes_workspace_bytes(10, (1 << 24) + 1) == E
    pneed = lib.sgam_points_planes_workspace_bytes(1000, 64)
    assert pneed > 0 and pneed % 16 == 0
    pouts = (one,) * 4
    assert lib.sgam_points_segment_planes_f32(None, 1000, 64, 1, 0.01, 3, 0, one, pneed, *pouts, None) == E
    assert lib.sgam_points_segment_planes_f32(one, 0, 64, 1, 0.01, 3, 0, one, pneed, *pouts, None) == E
    assert lib.sgam_points_segment_planes_f32(one, 1000, 0, 1, 0.01, 3, 0, one, pneed, *pouts, None) == E
    assert lib.sgam_points_segment_planes_f32(one, 1000, 64, 0, 0.01, 3, 0, one, pneed, *pouts, None) == E
    assert lib.sgam_points_segment_planes_f32(one, 1000, 64, 1, -0.01, 3, 0, one, pneed, *pouts, None) == E
    assert lib.sgam_points_segment_planes_f32(one, 1000, 64, 1, 0.01, -1, 0, one, pneed, *pouts, None) == E
    assert lib.sgam_points_segment_planes_f32(one, 1000, 64, 1, 0.01, 3, 0, one, pneed, one, one, one, None, None) == E
    assert lib.sgam_points_segment_planes_f32(one, 1000, 64, 1, 0.01, 3, 0, one, pneed - 1, *pouts, None) == W
    assert lib.sgam_points_segment_planes_f32(one, 1000, 64, 1, 0.01, 3, 0, None, pneed, *pouts, None) == W

    assert lib.sgam_points_plane_score_f32(None, None, 1000, one, 64, 0.01, 0, one, None) == E
    assert lib.sgam_points_plane_score_f32(one, None, 1000, None, 64, 0.01, 0, one, None) == E
    assert lib.sgam_points_plane_score_f32(one, None, 0, one, 64, 0.01, 0, one, None) == E
    assert lib.sgam_points_plane_score_f32(one, None, 1000, one, 0, 0.01, 0, one, None) == E
    assert lib.sgam_points_plane_score_f32(one, None, 1000, one, 64, 0.01, 3, one, None) == E
    assert lib.sgam_points_plane_score_f32(one, None, 1000, one, 64, float("nan"), 0, one, None) == E

    assert lib.sgam_points_cluster_boxes_f32(None, one, 10, 2, one, one, one, None) == E
    assert lib.sgam_points_cluster_boxes_f32(one, None, 10, 2, one, one, one, None) == E
    assert lib.sgam_points_cluster_boxes_f32(one, one, 0, 2, one, one, one, None) == E
    assert lib.sgam_points_cluster_boxes_f32(one, one, 10, 0, one, one, one, None) == E
    assert lib.sgam_points_cluster_boxes_f32(one, one, 10, 2, one, one, None, None) == E
