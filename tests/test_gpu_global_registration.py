"""GPU: the global registration kernels (csrc/point_global.hip) against their numpy twin (tests/global_registration_oracle.py) —
FPFH counts and features, the nearest feature, the RANSAC samples and validity bit for bit (the fp64 poses within 1e-9), the scores
on the device's own poses — and against the truth: register_global from a 140 degree motion on the test surface within the bounds
tests/test_global_registration_cpu.py asserts of the twin, and geometry_metrics(align={"init": "global", ...}) on both warp
branches."""
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import geometry, testing

sys.path.insert(0, os.path.dirname(__file__))
import cloud_oracle as CO  # noqa: E402
import global_registration_oracle as GR  # noqa: E402
import icp_oracle as IO  # noqa: E402
from test_global_registration_cpu import (FEATURE_K, FEATURE_RADIUS, RANSAC_DISTANCE, SAME_END_R, SAME_END_T, SEEDS,  # noqa: E402
                                          recovery_case)
from test_icp_cpu import EXACT_R, EXACT_T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_f32(got, want):
    got, want = np.ascontiguousarray(got, dtype=f32), np.ascontiguousarray(want, dtype=f32)
    return got.shape == want.shape and bool(((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all())


# ---------------------------------------------------------------- FPFH
def _fpfh_case(n, dirty):
    pts, nrm = IO.surface(n, 40 + n)
    if dirty:
        rows = np.arange(n)
        pts[rows % 13 == 6] = pts[np.maximum(rows[rows % 13 == 6] - 1, 0)]          # duplicated points: d = 0 pairs
        pts[rows % 7 == 3] = np.nan                                                 # one NaN point in seven
        nrm[rows % 11 == 5] = np.nan
    return pts, nrm


@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "nan_and_duplicates"])
@pytest.mark.parametrize("radius", [None, 0.6])
@pytest.mark.parametrize("k", [2, 16, 32])
@pytest.mark.parametrize("n", [1, 2, 255, 257])
def test_fpfh_equals_the_twin(n, k, radius, dirty):
    pts, nrm = _fpfh_case(n, dirty)
    want, want_counts = GR.fpfh(pts, nrm, k, radius)
    p, q = _t(pts), _t(nrm)
    feats = {m: geometry.fpfh(p, q, k, radius, method=m).cpu().numpy() for m in ("brute", "grid")}
    nn = geometry.knn(p, p, k, max_distance=radius)
    counts = geometry.fpfh_counts(p, q, nn["index"]).cpu().numpy()
    assert counts.shape == (n, 34) and np.array_equal(counts, want_counts)
    assert _same_f32(feats["brute"], want) and _same_f32(feats["grid"], feats["brute"])
    regular = np.isfinite(want).all(1)
    assert (np.isnan(want) | np.isfinite(want)).all() and np.array_equal(regular, np.isfinite(pts).all(1) & np.isfinite(nrm).all(1))
    if n >= 255:
        assert counts[:, 33].max() > 0 and (dirty or regular.all())


# ---------------------------------------------------------------- the nearest feature
def _features(n, seed):
    return np.random.RandomState(seed).uniform(0, 100, (n, 33)).astype(f32)


@pytest.mark.parametrize("nt", [1, 255, 256, 257])
@pytest.mark.parametrize("ns", [1, 63, 65, 257])
def test_matching_equals_the_twin(ns, nt):
    a, b = _features(ns, ns), _features(nt, 1000 + nt)
    if nt > 1:
        b[nt - 1] = b[0]                                                   # exact ties: the lower index
        b[nt // 2] = np.nan
        a[0] = b[0]
    if ns > 1:
        a[ns // 2] = np.nan
        a[ns - 1] = b[nt // 3]
    want_d2, want_idx = GR.match(a, b)
    got = geometry.match_features(_t(a), _t(b))
    assert got["index"].dtype == torch.int32 and np.array_equal(got["index"].cpu().numpy(), want_idx)
    assert _same_f32(got["d2"].cpu().numpy(), want_d2)
    if nt > 1:
        assert want_idx[0] == 0 and want_d2[0] == 0 and (want_idx != nt // 2).all() and (want_idx != nt - 1).all()
    if ns > 1:
        assert want_idx[ns // 2] == -1 and want_d2[ns // 2] == np.inf
    mutual = geometry.match_features(_t(a), _t(b), mutual=True)
    idx = mutual["index"].cpu().numpy()
    assert {(i, int(j)) for i, j in enumerate(idx) if j >= 0} == GR.match_mutual(a, b)
    assert (mutual["d2"].cpu().numpy()[idx < 0] == np.inf).all() and _same_f32(mutual["d2"].cpu().numpy()[idx >= 0], want_d2[idx >= 0])


# ---------------------------------------------------------------- RANSAC
def _ransac_case(C, seed=0):
    """C correspondences between a cloud and its moved copy, three in ten of them wrong; a NaN point and a row out of range"""
    n = max(C, 8)
    src, _ = IO.surface(n, 60 + seed)
    T = GR.far_motion()
    tgt = IO.transform(src, T)
    rs = np.random.RandomState(seed)
    corr = np.stack([np.arange(C), np.arange(C)], axis=1).astype(np.int32)
    wrong = rs.uniform(size=C) < 0.3
    corr[wrong, 1] = rs.randint(0, n, wrong.sum())
    if C > 100:
        src[7] = np.nan
        corr[11] = (n + 5, 2)
        corr[12] = (3, -1)
    return src, tgt, corr, T


@pytest.mark.parametrize("ransac_n", [3, 4])
@pytest.mark.parametrize("H,C", [(1, 3), (63, 255), (64, 257), (65, 4097), (4097, 255), (4097, 4097)])
def test_hypotheses_equal_the_twin(H, C, ransac_n):
    src, tgt, corr, T = _ransac_case(C)
    seed = (5 << 32) | (H + C)
    picks, valid, poses = GR.hypotheses(src, tgt, corr, H, ransac_n, 0.9, 0.05, seed)
    got = geometry.ransac_hypotheses(_t(src), _t(tgt), _t(corr), 0.05, H, ransac_n, 0.9, seed)
    assert np.array_equal(got["samples"].cpu().numpy(), picks) and np.array_equal(got["valid"].cpu().numpy(), valid)
    err = np.abs(got["poses"].cpu().numpy() - poses).max()
    print("hypotheses H", H, "C", C, "n", ransac_n, "valid", int(valid.sum()), "largest pose difference", err)
    assert err <= 1e-9                                                    # DESIGN §4.4.5's bound for fp64 results
    if C < ransac_n:
        assert not valid.any()
    if H >= 4097:
        assert 0 < valid.sum() < H


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("H,C", [(1, 3), (65, 257), (4097, 255), (300, 4097)])
def test_scores_equal_the_twin_on_the_device_poses(H, C, compact):
    src, tgt, corr, T = _ransac_case(C)
    s, t, c = _t(src), _t(tgt), _t(corr)
    hyp = geometry.ransac_hypotheses(s, t, c, 0.05, H, 3, 0.9, 17)
    poses, valid = hyp["poses"].cpu().numpy(), hyp["valid"].cpu().numpy()
    counts, best = GR.score(src, tgt, corr, poses, valid, 0.05)
    got = geometry.ransac_score(s, t, c, hyp["poses"], hyp["valid"], 0.05, compact=compact)
    assert np.array_equal(got["counts"].cpu().numpy(), counts) and int(got["best"].item()) == best
    mask, index, Tb, info = GR.inliers(src, tgt, corr, poses, best, 0.05)
    win = geometry.ransac_inliers(s, t, c, hyp["poses"], got["best"], 0.05)
    assert np.array_equal(win["mask"].cpu().numpy(), mask) and np.array_equal(win["index"].cpu().numpy(), index)
    assert tuple(win["info"].cpu().numpy()) == info
    state = win["state"].cpu().numpy()
    assert np.array_equal(state[:16].reshape(4, 4), np.eye(4) if Tb is None else Tb) and (state[16:] == 0).all()
    if H >= 300:
        assert info[0] >= 0 and info[1] > 0.5 * C and mask.sum() == info[1]
    # no hypothesis valid: every count -1, best 0, the state untouched
    none = geometry.ransac_score(s, t, c, hyp["poses"], torch.zeros_like(hyp["valid"]), 0.05, compact=compact)
    assert (none["counts"].cpu().numpy() == -1).all() and int(none["best"].item()) == 0
    before = torch.arange(24, dtype=torch.float64, device=DEV)
    win = geometry.ransac_inliers(s, t, c, hyp["poses"], none["best"], 0.05, state=before.clone())
    assert torch.equal(win["state"], before) and tuple(win["info"].cpu().numpy()) == (-1, 0)
    assert not win["mask"].any() and (win["index"] == -1).all()


def test_register_ransac_is_reproducible_equals_the_twin_and_reports_degenerate():
    src, tgt, corr, T = _ransac_case(4097, seed=2)
    s, t, c = _t(src), _t(tgt), _t(corr)
    a = geometry.register_ransac(s, t, c, 0.05, max_iterations=5000, seed=9)
    b = geometry.register_ransac(s, t, c, 0.05, max_iterations=5000, seed=9)
    assert torch.equal(a["transformation"].view(torch.int64), b["transformation"].view(torch.int64))
    assert torch.equal(a["inliers"]["mask"], b["inliers"]["mask"])
    assert {k: a[k] for k in ("fitness", "inlier_rmse", "hypothesis", "valid_hypotheses", "status")} == \
           {k: b[k] for k in ("fitness", "inlier_rmse", "hypothesis", "valid_hypotheses", "status")}
    assert set(a) == {"transformation", "fitness", "inlier_rmse", "hypothesis", "inliers", "valid_hypotheses", "status"}
    twin = GR.register_ransac(src, tgt, corr, 0.05, max_iterations=5000, seed=9)
    eR, et, _ = IO.pose_error(a["transformation"].cpu().numpy(), T)
    dR, dt, _ = IO.pose_error(a["transformation"].cpu().numpy(), twin["transformation"])
    print("register_ransac: hypothesis", a["hypothesis"], "inliers", a["inliers"]["count"], "valid", a["valid_hypotheses"], "off the truth by", eR, et,
          "off the twin by", dR, dt)
    assert (a["hypothesis"], a["inliers"]["count"], a["valid_hypotheses"], a["status"]) == \
           (twin["hypothesis"], twin["inliers"]["count"], twin["valid_hypotheses"], 0)
    assert np.array_equal(a["inliers"]["mask"].cpu().numpy(), twin["inliers"]["mask"])
    # the refit ends within fp64 rounding of the twin's.  Against the truth: a least-squares fit over some 2850 inliers, each
    # within 0.05; a scrambled row passes as an inlier when it lands within 0.05 of the right point (pi 0.05^2 / 16 = 5e-4 of the
    # surface's square: 0.6 expected among the 1229 scrambled rows) and then moves the fit by up to 0.05 / 2850 = 1.8e-5: five
    # such rows stay below 1e-4
    assert dR <= 1e-9 and dt <= 1e-9 and eR <= 1e-4 and et <= 1e-4
    none = geometry.register_ransac(s, t, c[:40].contiguous(), 1e-9, max_iterations=200)
    assert none["status"] == 2 and none["hypothesis"] == -1 and none["valid_hypotheses"] == 0 and none["inliers"]["count"] == 0
    assert np.array_equal(none["transformation"].cpu().numpy(), np.eye(4)) and not none["inliers"]["mask"].any()


# ---------------------------------------------------------------- end to end on the test surface
VIEWPOINT = np.array([2.0, 2.0, 50.0])       # far above the surface z = f(x, y): every normal turned towards it points up
TINY_VOXEL = 1e-4                             # keeps every point of the test clouds (asserted): the sampled clouds are the clouds


def _global(src, tgt, T, seed):
    moved_view = (T[:3, :3] @ VIEWPOINT + T[:3, 3]).astype(f32)
    return geometry.register_global(_t(src), _t(tgt), TINY_VOXEL, source_viewpoints=_t(VIEWPOINT.astype(f32)), target_viewpoints=_t(moved_view),
                                    feature_k=FEATURE_K, feature_radius=FEATURE_RADIUS, max_correspondence_distance=RANSAC_DISTANCE, seed=seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_register_global_recovers_an_exact_copy(seed):
    src, _, tgt, _, T = recovery_case(seed, True)
    alone = geometry.register_icp(_t(src), _t(tgt), 0.5, target_normals=geometry.estimate_normals(_t(tgt), 16))
    assert IO.pose_error(alone["transformation"].cpu().numpy(), T)[2] > 90.0
    out = _global(src, tgt, T, seed)
    eR, et, _ = IO.pose_error(out["transformation"].cpu().numpy(), T)
    r = out["ransac"]
    print("exact copy, seed", seed, "correspondences", out["correspondences"], "valid hypotheses", r["valid_hypotheses"], "inliers",
          r["inliers"]["count"], "RANSAC off by (degrees)", IO.pose_error(r["transformation"].cpu().numpy(), T)[2], "after ICP: R", eR, "t", et)
    assert (out["n_source"], out["n_target"]) == (1500, 2000) and out["icp"]["converged"] and r["status"] == 0
    assert eR <= EXACT_R and et <= EXACT_T


@pytest.mark.parametrize("seed", SEEDS)
def test_register_global_ends_where_icp_from_the_truth_ends(seed):
    src, _, tgt, _, T = recovery_case(seed, False)
    out = _global(src, tgt, T, seed)
    moved_view = (T[:3, :3] @ VIEWPOINT + T[:3, 3]).astype(f32)
    normals = geometry.estimate_normals(_t(tgt), 16, _t(moved_view)[None], torch.zeros((2000,), dtype=torch.int32, device=DEV))
    ref = geometry.register_icp(_t(src), _t(tgt), RANSAC_DISTANCE, init=T, target_normals=normals)
    dR, dt, _ = IO.pose_error(out["transformation"].cpu().numpy(), ref["transformation"].cpu().numpy())
    print("resampled, seed", seed, "correspondences", out["correspondences"], "valid hypotheses", out["ransac"]["valid_hypotheses"],
          "RANSAC off by (degrees)", IO.pose_error(out["ransac"]["transformation"].cpu().numpy(), T)[2], "against ICP from the truth: R", dR, "t", dt)
    assert (out["n_source"], out["n_target"]) == (1500, 2000) and out["icp"]["converged"] and ref["converged"]
    assert dR <= SAME_END_R and dt <= SAME_END_T
    # refine=None stops after RANSAC
    coarse = geometry.register_global(_t(src), _t(tgt), TINY_VOXEL, source_viewpoints=_t(VIEWPOINT.astype(f32)), target_viewpoints=_t(moved_view),
                                      feature_k=FEATURE_K, feature_radius=FEATURE_RADIUS, max_correspondence_distance=RANSAC_DISTANCE, seed=seed,
                                      refine=None)
    assert coarse["icp"] is None and torch.equal(coarse["transformation"], out["ransac"]["transformation"])


# ---------------------------------------------------------------- scenes
@pytest.fixture(scope="module")
def model(golden):
    """the synthetic-weights model of test_gpu_cloud"""
    from sgam_neurips22_amd.config import default_params
    from sgam_neurips22_amd.generative_sensing_module.model import VQModel
    g = golden("vqgan_full_ge256.npz")
    m = VQModel(**default_params("google_earth"))
    sd = testing.synthetic_state_dict(m.state_dict(), seed=0)
    sd["quantize.embedding.weight"] = testing.codebook_from_stats(float(g["zmean"]), float(g["zstd"]), 4096, 256, int(g["cb_seed"]))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


SCENE_DISTANCE = 0.1                          # tests/test_gpu_icp.py's correspondence distance on this scene
SCENE_VOXEL = 0.05                            # half of it: RANSAC's distance 1.5 voxels = 0.075, the feature radius 0.25


@pytest.mark.parametrize("branch", ["splat", "rgbd"])
def test_scene_alignment_from_another_frame_of_reference(model, branch):
    from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
    kw = dict(use_rgbd_integration=True, tsdf_memory_budget_bytes=1 << 30) if branch == "rgbd" else {}
    scene = InfiniteSceneGeneration(model, "google_earth", output_dim=(3, 1), seed_frame=synthetic_seed_frame("google_earth", 0), **kw)
    scene.scene_expansion()
    assert len(scene.frames) == 3
    cloud = scene.merged_point_cloud()["points"]
    pts = cloud.cpu().numpy()
    centre = pts[np.isfinite(pts).all(1)].astype(np.float64).mean(0)
    C = np.eye(4)
    C[:3, 3] = centre
    align = dict(max_correspondence_distance=SCENE_DISTANCE, max_iterations=60)
    # align without "init": today's keys and values, on test_gpu_icp's 2 degree motion
    near = C @ IO.rigid(2.0, [0.2, 1.0, -0.4], [0.012, -0.01, 0.012]) @ np.linalg.inv(C)
    ref = geometry.transform_points(cloud, near)
    got = scene.geometry_metrics(ref, 0.01, align=align)
    keep = torch.isfinite(cloud).all(dim=1)
    tgt = ref[keep].contiguous()
    reg = geometry.register_icp(cloud[keep].contiguous(), tgt, SCENE_DISTANCE, target_normals=geometry.estimate_normals(tgt, 16), max_iterations=60)
    want = geometry.cloud_metrics(geometry.transform_points(cloud, reg["transformation"]), ref, 0.01)
    assert set(got) == set(want) | {"transformation", "alignment"} and set(got["alignment"]) == {"fitness", "inlier_rmse", "iterations", "converged"}
    assert {k: got[k] for k in want} == want and torch.equal(got["transformation"], reg["transformation"])
    assert got["alignment"] == {k: reg[k] for k in ("fitness", "inlier_rmse", "iterations", "converged")}
    near_chamfer = got["chamfer"]
    # the reference in another frame of reference: the 140 degree motion about the scene's centre
    far = C @ GR.far_motion() @ np.linalg.inv(C)
    ref = geometry.transform_points(cloud, far)
    centres, view_of = scene._frame_viewpoints(None)
    moved_centres = geometry.transform_points(centres, far)
    plain = scene.geometry_metrics(ref, 0.01)
    local = scene.geometry_metrics(ref, 0.01, align=align)
    got = scene.geometry_metrics(ref, 0.01, align=dict(align, init="global", **{"global": dict(voxel_size=SCENE_VOXEL,
                                                                                              target_viewpoints=(moved_centres, view_of))}))
    eR, et, deg = IO.pose_error(got["transformation"].cpu().numpy(), far)
    print(branch, "chamfer unaligned", plain["chamfer"], "ICP alone", local["chamfer"], "global + ICP", got["chamfer"], "(2 degree case:", near_chamfer,
          ") R error", eR, "t error", et, "alignment", {k: v for k, v in got["alignment"].items() if k != "global"},
          "global", {k: v for k, v in got["alignment"]["global"].items() if k != "transformation"})
    assert set(got["alignment"]) == {"fitness", "inlier_rmse", "iterations", "converged", "global"}
    assert set(got["alignment"]["global"]) == {"fitness", "inlier_rmse", "correspondences", "transformation", "hypothesis", "inliers",
                                               "valid_hypotheses"}
    assert local["chamfer"] > 0.5 * plain["chamfer"]
    assert got["chamfer"] < 1e-8 and got["alignment"]["converged"] and eR <= EXACT_R and et <= EXACT_T
    with pytest.raises(ValueError, match="voxel_size"):
        scene.geometry_metrics(ref, 0.01, align=dict(align, init="global"))
    with pytest.raises(ValueError, match="init"):
        scene.geometry_metrics(ref, 0.01, align=dict(align, init="icp"))
    with pytest.raises(ValueError, match="belongs to"):
        scene.geometry_metrics(ref, 0.01, align=dict(align, **{"global": dict(voxel_size=SCENE_VOXEL)}))
