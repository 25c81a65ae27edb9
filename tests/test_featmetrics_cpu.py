"""CPU: the feature-set metrics (sgam_neurips22_amd/feature_metrics.py, csrc/feature_metrics.hip) without a GPU — the numpy twin
(tests/featmetrics_oracle.py) on hand-worked examples, the host-side argument rules, and the refusals of the C entry points."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import _lib
from sgam_neurips22_amd import feature_metrics as FM

sys.path.insert(0, os.path.dirname(__file__))
import featmetrics_oracle as FO  # noqa: E402


# ---- subset rule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2,m,S", [(29, 29, 29, 1), (67, 50, 50, 7), (130, 67, 2, 3), (5, 9, 3, 4)])
def test_subsets_are_sorted_distinct_and_in_range(n1, n2, m, S):
    idx = FO.kid_subsets(n1, n2, m, S, seed=11)
    assert idx.shape == (S, 2, m) and idx.dtype == np.int32
    for s in range(S):
        for side, n in enumerate((n1, n2)):
            row = idx[s, side]
            assert np.all(np.diff(row) > 0) and row[0] >= 0 and row[-1] < n          # ascending => distinct
            if m == n:
                assert np.array_equal(row, np.arange(n))                               # the identity, whatever the seed


def test_subsets_depend_on_seed_subset_and_side_only():
    a = FO.kid_subsets(67, 67, 20, 5, seed=0)
    b = FO.kid_subsets(67, 67, 20, 5, seed=1)
    assert not np.array_equal(a, b)
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[0, 0], a[0, 1])
    assert np.array_equal(a, FO.kid_subsets(67, 67, 20, 5, seed=0))
    assert np.array_equal(a[:3], FO.kid_subsets(67, 67, 20, 3, seed=0))                # subset s does not depend on how many are drawn
    # the 64-bit seed is the Philox key (low word, high word)
    assert not np.array_equal(FO.kid_subsets(67, 67, 20, 2, seed=1 << 32), FO.kid_subsets(67, 67, 20, 2, seed=0))


def test_subset_rule_is_the_m_smallest_key_index_pairs():
    n, m, s, side, seed = 40, 7, 2, 1, 5
    keys = [int(FO.philox4x32_10((i, s, side, 0), (seed, 0))[0]) for i in range(n)]
    want = sorted(sorted(range(n), key=lambda i: (keys[i], i))[:m])
    assert FO.kid_subsets(3 * n, n, m, s + 1, seed)[s, side].tolist() == want


# ---- MMD^2 ---------------------------------------------------------------------------------------------------------------------
def test_mmd2_of_two_plus_two_points_by_hand():
    """a = {e0, e1}, b = {e0 + e1, 2 e2} in d = 4, gamma = 1/4, coef0 = 1.  a.a' = 0 and b.b' = 0: K = 1, so both within-set terms
    are 2 * 1 / (2 * 1) = 1.  a.b: (e0, e0 + e1) = (e1, e0 + e1) = 1 -> K = 1.25^3 = 1.953125; (., 2 e2) = 0 -> K = 1; the cross
    sum is 2 * 1.953125 + 2 = 5.90625, its term 2 * 5.90625 / 4 = 2.953125.  mmd^2 = 1 + 1 - 2.953125 = -0.953125."""
    a = np.array([[1, 0, 0, 0], [0, 1, 0, 0]], np.float64)
    b = np.array([[1, 1, 0, 0], [0, 0, 2, 0]], np.float64)
    got = FO.kid(a, b)
    assert got["subsets"] == 1 and got["subset_size"] == 2 and got["kid_std"] == 0.0
    assert got["kid"] == -0.953125 and got["values"].tolist() == [-0.953125]
    # the majorant estimator on the same points adds the three terms
    idx = FO.kid_subsets(2, 2, 2, 1, 0)
    assert FO.kid_values(FO.gram_majorant(np.concatenate([a, b])), 2, idx, 0.25, 1.0, majorant=True)[0] == 1 + 1 + 2.953125


def test_twin_kid_equals_the_estimator_written_on_the_features():
    rng = np.random.default_rng(3)
    f1, f2 = np.abs(rng.standard_normal((23, 8))), np.abs(rng.standard_normal((17, 8))) * 1.1 + 0.05
    got = FO.kid(f1, f2, subsets=4, subset_size=9, seed=2)
    k = lambda x, y: (x @ y.T / 8 + 1.0) ** 3            # noqa: E731
    for s in range(4):
        a, b = f1[got["idx"][s, 0]], f2[got["idx"][s, 1]]
        kaa, kbb, kab = k(a, a), k(b, b), k(a, b)
        want = (kaa.sum() - np.trace(kaa)) / 72 + (kbb.sum() - np.trace(kbb)) / 72 - 2 * kab.mean()
        assert abs(got["values"][s] - want) <= 1e-12 * abs(want)
    assert got["kid"] == got["values"].mean() and got["kid_std"] == got["values"].std()


# ---- precision / recall / density / coverage ----------------------------------------------------------------------------------
def test_prdc_of_a_hand_placed_configuration():
    """On a line in d = 4, k = 1.  Reference x = 0, 1, 10, 12, 100: squared radii 1, 1, 4, 4, 7744.  Generated x = 0.5, 11, 5, 5.5:
    squared radii 20.25, 30.25, 0.25, 0.25.
    precision: 0.5 is inside the balls of 0 and 1 (0.25 <= 1), 11 inside those of 10 and 12 (1 <= 4), 5 and 5.5 inside none
      (nearest reference 10: 25 and 20.25 > 4; 100: 9025, 8930.25 > 7744) -> 2 / 4; those four memberships -> density 4 / (1 * 4).
    recall: 0 and 1 are within 0.25 <= 20.25 of 0.5, 10 and 12 within 1 <= 30.25 of 11; 100 is 7921 from 11 -> 4 / 5.
    coverage: nearest generated point at 0.25, 0.25, 1, 1 (inside the own ball), 100: 7921 > 7744 -> 4 / 5."""
    ref = np.zeros((5, 4))
    ref[:, 0] = [0, 1, 10, 12, 100]
    gen = np.zeros((4, 4))
    gen[:, 0] = [0.5, 11, 5, 5.5]
    out = FO.prdc(FO.gram(np.concatenate([ref, gen])), 5, 4, 1)
    assert out["radius2"].tolist() == [1, 1, 4, 4, 7744, 20.25, 30.25, 0.25, 0.25]
    assert out["counts"].tolist() == [2, 4, 4, 4]
    assert FO.prdc_values(out["counts"], 5, 4, 1) == {"precision": 0.5, "recall": 0.8, "density": 1.0, "coverage": 0.8}
    assert out["margin"] == 0.75                          # 0.25 against the radius 1
    # k = 2 on the reference side: second neighbours; a duplicate row is a neighbour at distance 0 (exclusion is by index)
    dup = np.concatenate([ref, ref[:1], gen])
    r2 = FO.prdc(FO.gram(dup), 6, 4, 2)["radius2"]
    assert r2[0] == 1.0 and r2[5] == 1.0 and r2[1] == 1.0


# ---- host-side argument rules (before anything touches the device) --------------------------------------------------------------
def test_subset_size_and_k_are_validated():
    f1, f2 = torch.zeros((10, 8)), torch.zeros((6, 8))
    with pytest.raises(ValueError, match="exceeds the smaller set"):
        FM.kid_from_features(f1, f2, subset_size=7)
    with pytest.raises(ValueError, match="at least 2"):
        FM.kid_from_features(f1, f2, subset_size=1)
    with pytest.raises(ValueError, match="subsets"):
        FM.kid_from_features(f1, f2, subsets=0)
    with pytest.raises(ValueError, match="multiple of 4"):
        FM.kid_from_features(torch.zeros((10, 6)), torch.zeros((6, 6)))
    with pytest.raises(ValueError, match="feature dimensions"):
        FM.kid_from_features(f1, torch.zeros((6, 4)))
    for k in (0, 33):
        with pytest.raises(ValueError, match="between 1 and 32"):
            FM.prdc_from_features(f1, f2, k=k)
    with pytest.raises(ValueError, match="at least 7 rows"):
        FM.prdc_from_features(f1, f2, k=6)
    big = torch.zeros((1, 4)).expand(16380, 4)
    with pytest.raises(ValueError, match="16384"):
        FM.kid_from_features(big, torch.zeros((5, 4)))
    with pytest.raises(ValueError, match="16384"):
        FM.prdc_from_features(big, torch.zeros((5, 4)))
    # valid arguments on CPU tensors: an error, never a CPU substitute
    with pytest.raises(_lib.SgamHipError, match="no CPU fallback"):
        FM.kid_from_features(f1, f2)
    with pytest.raises(_lib.SgamHipError, match="no CPU fallback"):
        FM.prdc_from_features(f1, f2, k=3)
    with pytest.raises(_lib.SgamHipError, match="no CPU fallback"):
        FM.feature_gram(f1)


def test_statistics_only_side_is_refused(tmp_path):
    np.savez(tmp_path / "stats.npz", mu=np.zeros(4), sigma=np.eye(4))
    frames = torch.zeros((4, 8, 8, 3), dtype=torch.uint8)
    for fn in (FM.kid_between, FM.prdc_between):
        with pytest.raises(ValueError, match="needs the features themselves"):
            fn(str(tmp_path / "stats.npz"), frames, model=None, dims=64)


# ---- the C entry points refuse before any launch ---------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_gpu():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)               # a non-NULL pointer that is never dereferenced: every call returns first
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.sgam_feature_gram_f64(None, 4, 4, 4, p, None) == -1
    assert lib.sgam_feature_gram_f64(p, 4, 4, 4, None, None) == -1
    assert lib.sgam_feature_gram_f64(p, 4, 6, 6, p, None) == -1                 # d % 4 != 0
    assert lib.sgam_feature_gram_f64(p, 4, 8, 4, p, None) == -1                 # pitch below d
    assert lib.sgam_feature_gram_f64(p, 16385, 4, 4, p, None) == -1             # beyond the 16384-row cap
    assert lib.sgam_feature_gram_f64(p, 0, 4, 4, p, None) == -1
    assert lib.sgam_kid_subsets_u32(8, 8, 4, 2, 0, p, 64, None, None) == -1
    assert lib.sgam_kid_subsets_u32(8, 8, 9, 2, 0, p, 64, p, None) == -1        # m above the smaller set
    assert lib.sgam_kid_subsets_u32(16385, 8, 4, 2, 0, p, 1 << 20, p, None) == -1
    assert lib.sgam_kid_subsets_u32(8, 8, 4, 0, 0, p, 64, p, None) == -1
    assert lib.sgam_kid_subsets_u32(8, 8, 4, 2, 0, None, 0, p, None) == -3      # SGAM_EWORKSPACE
    assert lib.sgam_kid_subsets_u32(8, 8, 4, 2, 0, p, 31, p, None) == -3        # 2 * 2 * 8 bytes needed
    assert lib.sgam_kid_mmd_f64(None, 8, 8, p, 4, 2, 0.25, 1.0, p, 1 << 10, p, None) == -1
    assert lib.sgam_kid_mmd_f64(p, 8, 8, None, 4, 2, 0.25, 1.0, p, 1 << 10, p, None) == -1
    assert lib.sgam_kid_mmd_f64(p, 8, 8, p, 4, 2, 0.25, 1.0, p, 1 << 10, None, None) == -1
    assert lib.sgam_kid_mmd_f64(p, 8, 8, p, 1, 2, 0.25, 1.0, p, 1 << 10, p, None) == -1         # m < 2
    assert lib.sgam_kid_mmd_f64(p, 16000, 385, p, 4, 2, 0.25, 1.0, p, 1 << 10, p, None) == -1   # n1 + n2 > 16384
    assert lib.sgam_kid_mmd_f64(p, 8, 8, p, 4, 2, 0.25, 1.0, None, 0, p, None) == -3
    assert lib.sgam_feature_prdc_f64(None, 8, 8, 3, p, p, None) == -1
    assert lib.sgam_feature_prdc_f64(p, 8, 8, 3, None, p, None) == -1
    assert lib.sgam_feature_prdc_f64(p, 8, 8, 3, p, None, None) == -1
    assert lib.sgam_feature_prdc_f64(p, 40, 40, 33, p, p, None) == -1           # k > 32
    assert lib.sgam_feature_prdc_f64(p, 8, 8, 0, p, p, None) == -1
    assert lib.sgam_feature_prdc_f64(p, 8, 3, 3, p, p, None) == -1              # k + 1 > the smaller set
    assert lib.sgam_feature_prdc_f64(p, 16000, 385, 3, p, p, None) == -1        # beyond the cap
