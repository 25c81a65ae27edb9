"""CPU: the global registration kernels' numpy twin (tests/global_registration_oracle.py) against outside references — numpy's
arctan2 for the transcendental-free bin rule of theta, numpy.linalg.svd (Kabsch) for Horn's closed form on the kernel's Jacobi
loop, sampler_oracle's integer Philox for the draw rule — and against the TRUTH on the test surface: from a 140 degree motion, where
ICP alone fails, features + RANSAC + ICP end where the GPU tests (tests/test_gpu_global_registration.py) then ask the kernels to
end.  Also the argument checks of the new C entry points through ctypes and the ValueErrors of geometry.py."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import _lib, geometry

sys.path.insert(0, os.path.dirname(__file__))
import global_registration_oracle as GR  # noqa: E402
import icp_oracle as IO  # noqa: E402
import sampler_oracle as SO  # noqa: E402
from test_icp_cpu import EXACT_R, EXACT_T, MAX_DISTANCE  # noqa: E402

f32 = np.float32
SEEDS = (0, 1, 2)
# the recovery case: 1500 source points against a 2000-point target moved by GR.far_motion()
RANSAC_DISTANCE, FEATURE_K, FEATURE_RADIUS, HYPOTHESES = 0.15, 24, 0.5, 3000
# resampled pair: global + ICP against register_icp(init = the truth) on the same clouds.  Both are fixed points of the same
# iteration reached from different starts; what separates them is ICP's stop rule (fitness and RMSE moving less than 1e-6), not
# rounding.  Measured on the twin over the seeds 0..2 (printed below): at most 9.5e-6 in R (Frobenius) and 1.4e-5 in t; the bounds
# are 10 times that.
SAME_END_R, SAME_END_T = 9.5e-5, 1.4e-4


def recovery_case(seed, exact):
    """(source, its normals, target, its normals, the motion): the target is a 2000-point sample of the surface moved by the 140
    degree motion; the source is 1500 of its points before the motion, permuted (exact), or 1500 other points of the surface"""
    T = GR.far_motion()
    tgt0, nrm0 = IO.surface(2000, 10 + seed)
    if exact:
        pick = np.random.RandomState(seed).permutation(2000)[:1500]
        src, src_n = tgt0[pick], nrm0[pick]
    else:
        src, src_n = IO.surface(1500, 20 + seed)
    return src, src_n, IO.transform(tgt0, T), GR.moved_normals(nrm0, T), T


@functools.lru_cache(maxsize=None)
def twin_recovery(seed, exact):
    src, src_n, tgt, tgt_n, T = recovery_case(seed, exact)
    return GR.register_global(src, src_n, tgt, tgt_n, RANSAC_DISTANCE, feature_k=FEATURE_K, feature_radius=FEATURE_RADIUS,
                              max_iterations=HYPOTHESES, seed=seed)


# ---------------------------------------------------------------- the twin's pieces
def test_theta_bins_without_the_arctangent():
    rs = np.random.RandomState(0)
    theta = rs.uniform(-np.pi, np.pi, 2_000_000)
    edges = -np.pi + 2.0 * np.pi * np.arange(12) / 11.0
    theta = theta[np.abs(theta[:, None] - edges[None, :]).min(axis=1) > 1e-9]     # (away from the edges: there arctan2's last bit decides)
    r = rs.uniform(0.01, 2.0, len(theta))
    x, y = r * np.cos(theta), r * np.sin(theta)
    assert len(theta) > 1_900_000 and np.array_equal(GR.theta_bin(x, y), GR.theta_bin_arctan(x, y))
    # the literals are the edge directions
    for b, (c, s) in enumerate(GR.EDGES, start=1):
        assert abs(c - np.cos(edges[b])) <= 2.0 ** -52 and abs(s - np.sin(edges[b])) <= 2.0 ** -52
    # the axes (no edge lies on one but theta = pi, the last bin) and the origin
    assert list(GR.theta_bin(np.array([1.0, 0.0, -1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0, -1.0, 0.0]))) == [5, 8, 10, 2, 5]
    assert list(GR.theta_bin_arctan(np.array([1.0, 0.0, -1.0, 0.0]), np.array([0.0, 1.0, 0.0, -1.0]))) == [5, 8, 10, 2]
    assert list(GR.unit_bin(np.array([-1.0, -0.9999, 0.0, 0.9999, 1.0, 1.0 + 1e-12, -1.0 - 1e-12]))) == [0, 0, 5, 10, 10, 10, 0]


def test_horn_on_the_jacobi_loop_equals_kabsch():
    rs = np.random.RandomState(1)
    worst = 0.0
    for n in (3, 4):
        p = rs.uniform(-1, 1, (2000, n, 3))
        R = np.stack([IO.rodrigues(w) for w in rs.normal(size=(2000, 3)) * 1.5])
        q = np.einsum("hab,hnb->hna", R, p) + rs.uniform(-2, 2, (2000, 1, 3)) + rs.normal(size=(2000, n, 3)) * 0.01
        T = GR.horn(p, q)
        for h in range(2000):
            c = p[h] - p[h].mean(0)
            sv = np.linalg.svd(c.T @ (q[h] - q[h].mean(0)), compute_uv=False)
            if sv[1] < 0.05 * sv[0]:
                continue                                                   # (a needle of a triangle: the pose about its axis is soft)
            # the quaternion is an eigenvector of a matrix of norm ~ sv[0] whose gap to the next eigenvalue is >= 2 sv[1]: rounding
            # of 2^-53 in the matrix moves it by about 2^-53 sv[0] / sv[1] <= 20 * 2^-53; 64 such roundings in both routes, and the
            # translation multiplies the rotation's error by the centroids' size (<= 3.5)
            err = np.abs(T[h] - GR.kabsch(p[h], q[h])).max()
            worst = max(worst, err)
            assert err <= 64 * 20 * 2.0 ** -53 * 3.5, (n, h, err)
        RtR = np.einsum("hab,hac->hbc", T[:, :, :3], T[:, :, :3])
        assert np.abs(RtR - np.eye(3)).max() <= 1e-14 and np.allclose(np.linalg.det(T[:, :, :3]), 1.0, atol=1e-14)
    print("Horn against Kabsch: largest difference of an entry", worst)


def test_degenerate_samples_are_void_or_finite():
    """collinear and coincident triples: a pose that scores is never NaN"""
    line = np.array([[0, 0, 0], [1, 2, 3], [2, 4, 6], [-1, -2, -3]], dtype=f32)
    same = np.tile(np.array([[0.5, -1.0, 2.0]], dtype=f32), (4, 1))
    M = IO.rigid(70.0, [0.3, 1.0, 0.2], [0.5, 0.1, -0.4])
    for src, n in ((line, 3), (line, 4), (same, 3), (same, 4)):
        tgt = IO.transform(src, M)
        corr = np.stack([np.arange(4), np.arange(4)], 1).astype(np.int32)
        picks, valid, poses = GR.hypotheses(src, tgt, corr, 64, n, 0.9, 0.05, 3)
        assert np.isfinite(poses).all() and set(valid) <= {0, 1} and valid.sum() > 0          # (the samples do land: exact copies)
        counts, best = GR.score(src, tgt, corr, poses, valid, 0.05)
        assert (counts[valid != 0] == 4).all() and (counts[valid == 0] == -1).all() and GR.unpack(best)[1] == 4
    # NaN points and rows out of range void their hypotheses instead of scoring
    src = np.concatenate([line, [[np.nan, 0, 0]]]).astype(f32)
    corr = np.array([[0, 0], [1, 1], [2, 2], [4, 3], [9, 0], [0, -1]], dtype=np.int32)
    picks, valid, poses = GR.hypotheses(src, IO.transform(line, M), corr, 256, 3, 0.9, 0.05, 0)
    bad = (picks[:, :3] >= 3).any(axis=1)
    assert bad.any() and (valid[bad] == 0).all() and (poses[bad] == 0).all() and np.isfinite(poses).all()
    counts, best = GR.score(src, IO.transform(line, M), corr, poses, np.zeros_like(valid), 0.05)
    assert (counts == -1).all() and best == 0 and GR.unpack(best) == (-1, 0)


def _draw_scalar(h, C, n, seed):
    """the draw rule in Python integers on sampler_oracle's Philox"""
    picks, q = [], 0
    for _ in range(n):
        got = -1
        while q < GR.MAX_DRAWS:
            w = int(SO.philox4x32_10((h, q, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))[0])
            q += 1
            if (w * C) >> 32 not in picks:
                got = (w * C) >> 32
                break
        picks.append(got)
    return picks + [-1] * (4 - n)


def test_draw_rule_on_the_integer_philox():
    for C, n, seed in ((1500, 3, 0), (1500, 4, 1), (5, 4, (7 << 32) | 9), (3, 3, 2), (2, 3, 0), (4, 4, 5)):
        got = GR.draw(300, C, n, seed)
        assert got.shape == (300, 4) and got.dtype == np.int32
        for h in list(range(40)) + [299]:
            assert list(got[h]) == _draw_scalar(h, C, n, seed), (C, n, seed, h)
        ok = (got[:, :n] >= 0).all(axis=1)
        assert (got[:, n:] == -1).all() and got.max() < C
        assert all(len(set(row[:n])) == n for row in got[ok])
        if C < n:
            assert not ok.any()                                            # never n distinct picks: every hypothesis is void
        if C >= 1000:
            assert ok.all()
    assert not np.array_equal(GR.draw(50, 1500, 3, 0), GR.draw(50, 1500, 3, 1))


def test_fpfh_blocks_sum_to_200():
    src, nrm = IO.surface(600, 4)
    feats, counts = GR.fpfh(src, nrm, 16, 0.6)
    m = counts[:, 33]
    assert feats.shape == (600, 33) and feats.dtype == f32 and (m > 0).all() and (counts[:, :33].reshape(600, 3, 11).sum(2) == m[:, None]).all()
    sums = feats.astype(np.float64).reshape(600, 3, 11).sum(axis=2)
    # 11 values that sum to 200, each rounded to fp32 once: half an ulp of each, 200 * 2^-24 in all (the fp64 error is 1e-13)
    print("FPFH block sums: largest distance from 200", np.abs(sums - 200.0).max())
    assert np.abs(sums - 200.0).max() <= 200.0 * 2.0 ** -24 + 1e-10
    # a NaN point and a NaN normal: NaN rows, counted by no neighbour; a duplicated point: the d = 0 pair is skipped
    pts, nn = src.copy(), nrm.copy()
    pts[5], nn[9], pts[21] = np.nan, np.nan, pts[20]
    feats, counts = GR.fpfh(pts, nn, 16, 0.6)
    assert np.isnan(feats[[5, 9]]).all() and np.isfinite(np.delete(feats, [5, 9], axis=0)).all() and (counts[[5, 9]] == 0).all()
    assert counts[20, 33] <= 14 and counts[21, 33] <= 14                      # 16 columns less the point itself and its twin


def test_matching_ties_and_nan_rows():
    rs = np.random.RandomState(3)
    a, b = rs.uniform(0, 100, (40, 33)).astype(f32), rs.uniform(0, 100, (30, 33)).astype(f32)
    b[17] = b[4]                                                           # an exact tie: the lower index
    a[0] = b[4]
    a[3], b[8] = np.nan, np.nan
    d2, idx = GR.match(a, b)
    want = ((a[:, None, :].astype(np.float64) - b[None].astype(np.float64)) ** 2).sum(2)
    want[:, 8] = np.inf
    assert idx[0] == 4 and d2[0] == 0 and idx[3] == -1 and d2[3] == np.inf and (idx != 8).all()
    keep = np.arange(40) != 3
    assert np.array_equal(idx[keep], want[keep].argmin(1)) and np.allclose(d2[keep], want[keep].min(1), rtol=1e-5)
    assert GR.match_mutual(a, b) <= {(i, int(j)) for i, j in enumerate(idx) if j >= 0}


# ---------------------------------------------------------------- the twin meets the truth
@pytest.mark.parametrize("seed", SEEDS)
def test_icp_alone_fails_from_the_far_motion(seed):
    src, src_n, tgt, tgt_n, T = recovery_case(seed, True)
    out = IO.register_icp(src, tgt, MAX_DISTANCE, normals=tgt_n)
    deg = IO.pose_error(out["transformation"], T)[2]
    print("ICP alone, seed", seed, "ends", deg, "degrees from the truth at fitness", out["fitness"])
    assert deg > 90.0


@pytest.mark.parametrize("seed", SEEDS)
def test_twin_recovers_an_exact_copy_from_the_far_motion(seed):
    src, src_n, tgt, tgt_n, T = recovery_case(seed, True)
    out = twin_recovery(seed, True)
    r = out["ransac"]
    eR, et, _ = IO.pose_error(out["transformation"], T)
    print("exact copy, seed", seed, "valid hypotheses", r["valid_hypotheses"], "best", r["hypothesis"], "inliers", r["inliers"]["count"], "of",
          len(out["correspondences"]), "RANSAC off by (degrees)", IO.pose_error(r["transformation"], T)[2], "after ICP: R", eR, "t", et,
          "iterations", out["icp"]["iterations"])
    assert r["status"] == 0 and r["valid_hypotheses"] > 0 and out["icp"]["converged"]
    assert eR <= EXACT_R and et <= EXACT_T


@pytest.mark.parametrize("seed", SEEDS)
def test_twin_ends_where_icp_from_the_truth_ends(seed):
    src, src_n, tgt, tgt_n, T = recovery_case(seed, False)
    out = twin_recovery(seed, False)
    ref = IO.register_icp(src, tgt, RANSAC_DISTANCE, init=T, normals=tgt_n)
    dR, dt, _ = IO.pose_error(out["transformation"], ref["transformation"])
    print("resampled, seed", seed, "valid hypotheses", out["ransac"]["valid_hypotheses"], "RANSAC off by (degrees)",
          IO.pose_error(out["ransac"]["transformation"], T)[2], "after ICP off the truth by", IO.pose_error(out["transformation"], T)[2],
          "against ICP from the truth: R", dR, "t", dt)
    assert out["icp"]["converged"] and ref["converged"]
    assert dR <= SAME_END_R and dt <= SAME_END_T


def test_twin_is_a_function_of_the_seed_and_all_void_is_degenerate():
    src, src_n, tgt, tgt_n, T = recovery_case(0, True)
    corr = twin_recovery(0, True)["correspondences"]
    a = GR.register_ransac(src, tgt, corr, RANSAC_DISTANCE, max_iterations=500, seed=4)
    b = GR.register_ransac(src, tgt, corr, RANSAC_DISTANCE, max_iterations=500, seed=4)
    assert np.array_equal(a["transformation"], b["transformation"]) and a["best"] == b["best"]
    # nothing can be valid at a distance no sample lands within: status degenerate, the identity
    none = GR.register_ransac(src, tgt, corr[:40], 1e-9, max_iterations=200, seed=0)
    assert none["status"] == 2 and none["hypothesis"] == -1 and none["valid_hypotheses"] == 0 and none["best"] == 0
    assert np.array_equal(none["transformation"], np.eye(4)) and (none["counts"] == -1).all() and not none["inliers"]["mask"].any()


# ---------------------------------------------------------------- the C entry points and the Python checks
def test_global_registration_argument_validation_without_gpu():
    lib = _lib.load()
    assert lib.sgam_abi_version() == 10                                 # additive: the ABI version stays
    p = ctypes.c_void_p(256)                                            # never dereferenced: every check comes before a launch

    def counts(points=p, normals=p, N=10, index=p, k=8, out=p):
        return lib.sgam_points_fpfh_counts(points, normals, N, index, k, out, None)

    for kw in (dict(points=None), dict(normals=None), dict(index=None), dict(out=None), dict(N=0), dict(k=0), dict(k=33)):
        assert counts(**kw) == -1, kw

    def combine(counts=p, points=p, normals=p, N=10, index=p, d2=p, k=8, out=p):
        return lib.sgam_points_fpfh_combine_f32(counts, points, normals, N, index, d2, k, out, None)

    for kw in (dict(counts=None), dict(points=None), dict(normals=None), dict(index=None), dict(d2=None), dict(out=None), dict(N=-1),
               dict(k=0), dict(k=33)):
        assert combine(**kw) == -1, kw

    def match(source=p, Ns=10, target=p, Nt=10, dim=33, d2=p, index=p):
        return lib.sgam_features_match_f32(source, Ns, target, Nt, dim, d2, index, None)

    for kw in (dict(source=None), dict(target=None), dict(d2=None), dict(index=None), dict(Ns=0), dict(Nt=0), dict(dim=32), dict(dim=34)):
        assert match(**kw) == -1, kw

    def hyp(source=p, Ns=10, target=p, Nt=10, corr=p, C=10, H=100, n=3, sim=0.9, dist=0.1, seed=0, samples=p, valid=p, poses=p):
        return lib.sgam_points_ransac_hypotheses(source, Ns, target, Nt, corr, C, H, n, sim, dist, seed, samples, valid, poses, None)

    for kw in (dict(source=None), dict(target=None), dict(corr=None), dict(samples=None), dict(valid=None), dict(poses=None), dict(Ns=0),
               dict(Nt=0), dict(C=0), dict(H=0), dict(n=2), dict(n=5), dict(sim=-0.1), dict(sim=1.5), dict(sim=float("nan")), dict(dist=0.0),
               dict(dist=float("inf")), dict(dist=float("nan"))):
        assert hyp(**kw) == -1, kw

    ws = lib.sgam_points_ransac_score_workspace_bytes
    assert [ws(h) for h in (1, 4, 5, 100000)] == [32, 32, 48, 16 + 400000] and ws(0) == ws(-1) == -1

    def score(source=p, Ns=10, target=p, Nt=10, corr=p, C=10, poses=p, valid=p, H=100, max_d2=0.01, compact=1, work=p, nbytes=1 << 20,
              counts=p, best=p):
        return lib.sgam_points_ransac_score(source, Ns, target, Nt, corr, C, poses, valid, H, max_d2, compact, work, nbytes, counts, best, None)

    for kw in (dict(source=None), dict(target=None), dict(corr=None), dict(poses=None), dict(valid=None), dict(counts=None), dict(best=None),
               dict(Ns=0), dict(Nt=0), dict(C=0), dict(H=0), dict(max_d2=-1.0), dict(max_d2=float("nan"))):
        assert score(**kw) == -1, kw
    for kw in (dict(work=None), dict(nbytes=16 + 400 - 1), dict(work=ctypes.c_void_p(264))):
        assert score(**kw) == -3, kw                                       # SGAM_EWORKSPACE: missing, too small, not 16-byte aligned

    def inliers(source=p, Ns=10, target=p, Nt=10, corr=p, C=10, poses=p, H=100, best=p, max_d2=0.01, mask=p, index=p, state=p, info=p):
        return lib.sgam_points_ransac_inliers(source, Ns, target, Nt, corr, C, poses, H, best, max_d2, mask, index, state, info, None)

    for kw in (dict(source=None), dict(target=None), dict(corr=None), dict(poses=None), dict(best=None), dict(mask=None), dict(index=None),
               dict(state=None), dict(info=None), dict(Ns=0), dict(Nt=0), dict(C=0), dict(H=0), dict(max_d2=float("nan"))):
        assert inliers(**kw) == -1, kw


def test_python_argument_checks():
    pts, feats = torch.zeros((10, 3)), torch.zeros((10, 33))
    corr = torch.zeros((5, 2), dtype=torch.int32)
    with pytest.raises(ValueError, match="normals"):
        geometry.fpfh(pts, torch.zeros((9, 3)))
    with pytest.raises(ValueError, match="k is an integer"):
        geometry.fpfh(pts, pts, k=33)
    with pytest.raises(ValueError, match="radius"):
        geometry.fpfh(pts, pts, radius=0.0)
    with pytest.raises(ValueError, match="method"):
        geometry.fpfh(pts, pts, method="tree")
    with pytest.raises(ValueError, match="knn_index"):
        geometry.fpfh_counts(pts, pts, torch.zeros((10, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match="source_features"):
        geometry.match_features(torch.zeros((10, 32)), feats)
    with pytest.raises(ValueError, match="target_features"):
        geometry.match_features(feats, feats.double())
    with pytest.raises(ValueError, match="correspondences"):
        geometry.register_ransac(pts, pts, corr.long(), 0.1)
    with pytest.raises(ValueError, match="correspondences"):
        geometry.register_ransac(pts, pts, torch.zeros((0, 2), dtype=torch.int32), 0.1)
    with pytest.raises(ValueError, match="ransac_n"):
        geometry.register_ransac(pts, pts, corr, 0.1, ransac_n=5)
    with pytest.raises(ValueError, match="max_iterations"):
        geometry.register_ransac(pts, pts, corr, 0.1, max_iterations=0)
    with pytest.raises(ValueError, match="edge_length_similarity"):
        geometry.register_ransac(pts, pts, corr, 0.1, edge_length_similarity=1.1)
    with pytest.raises(ValueError, match="max_correspondence_distance"):
        geometry.register_ransac(pts, pts, corr, 0.0)
    with pytest.raises(ValueError, match="seed"):
        geometry.register_ransac(pts, pts, corr, 0.1, seed=-1)
    with pytest.raises(ValueError, match="refit_iterations"):
        geometry.register_ransac(pts, pts, corr, 0.1, refit_iterations=-1)
    with pytest.raises(ValueError, match="refine"):
        geometry.register_global(pts, pts, 0.1, refine="colored")
    with pytest.raises(ValueError, match="voxel_size"):
        geometry.register_global(pts, pts, 0.0)
    with pytest.raises(ValueError, match="feature_radius"):
        geometry.register_global(pts, pts, 0.1, feature_radius=-1.0)
    with pytest.raises(ValueError, match="k is an integer"):
        geometry.register_global(pts, pts, 0.1, feature_k=40)
