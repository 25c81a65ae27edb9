"""GPU: KID and precision / recall / density / coverage on the device fp64 Gram (sgam_neurips22_amd/feature_metrics.py,
csrc/feature_metrics.hip) against the numpy twin (tests/featmetrics_oracle.py).

Tolerances.  Gram: products of fp32 values are exact in fp64, so device and twin are each a sum of d exact terms, each within
d 2^-53 (|Z| |Z|^T) / 2 of the exact value: |G - G_twin| <= d 2^-53 (|Z| |Z|^T) entrywise.  KID, per subset:
(3 d + 2 m + 16) 2^-53 S, S = the same estimator with every kernel value replaced by its majorant (gamma (|Z| |Z|^T)_ij + coef0)^3
and the three terms added (the Gram bound, times 3 through the cube, plus row sums of m terms and their join).  The four PRDC
counts are integers and must equal the twin's; that is demanded only after the twin has shown that no comparison sits within
1e-9 max G_ii of its radius (the Gram error is 1e6 times smaller).  Every figure is printed before it is asserted.

Measured on one MI355X: Gram max|G - G_twin| / bound 0 (d = 4), 0.048 (17 x 64), 0.042 (70 x 192), 0.023 (130 x 2048); KID
max|diff| / tol 0.0054, 0.0032, 0.0005 for the three cases in order; PRDC margins 1.3e-3 to 5.1e-2 against floors of 1e-7 to 3e-6."""
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import feature_metrics as FM
from sgam_neurips22_amd import fid

sys.path.insert(0, os.path.dirname(__file__))
import featmetrics_oracle as FO  # noqa: E402
import inception_oracle as IO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -53


def features(n, d, seed):
    """|N(0, 1)| rows in fp32"""
    return np.abs(np.random.default_rng(seed).standard_normal((n, d))).astype(np.float32)


def two_sets(n1, n2, d, seed):
    """the second set scaled by 1.1 plus 0.05: KID of 0.2 - 0.3"""
    return features(n1, d, seed), (features(n2, d, seed + 1000) * np.float32(1.1) + np.float32(0.05)).astype(np.float32)


def pitched(z, pad=8):
    """the rows on the device with a pitch of d + pad floats; the padding holds NaN, so a read past d shows in the result"""
    buf = torch.full((z.shape[0], z.shape[1] + pad), float("nan"), device=DEV)
    buf[:, :z.shape[1]] = torch.from_numpy(z).to(DEV)
    return buf[:, :z.shape[1]]


# ---- Gram ---------------------------------------------------------------------------------------------------------------------
GRAM_SHAPES = [(1, 4), (5, 4), (17, 64), (70, 192), (130, 2048)]


@pytest.mark.parametrize("n,d", GRAM_SHAPES)
def test_gram_against_the_twin(n, d):
    z = features(n, d, 100 + n)
    if (n, d) == (70, 192):
        z[40] = z[3]
    zd = pitched(z)
    assert zd.stride(0) == d + 8
    G = FM.feature_gram(zd)
    assert G.shape == (n, n) and G.dtype == torch.float64 and G.is_cuda
    g = G.cpu().numpy()
    bound = d * EPS * FO.gram_majorant(z)
    err = np.abs(g - FO.gram(z))
    print(f"gram ({n}, {d}): max|G - twin| / bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all())
    assert np.array_equal(g, g.T)                                              # symmetric bit for bit
    assert torch.equal(FM.feature_gram(zd), G)                                 # run to run: the same bits
    assert torch.equal(FM.feature_gram(torch.from_numpy(z).to(DEV)), G)        # the pitch changes nothing
    if (n, d) == (70, 192):
        assert np.array_equal(g[3], g[40]) and np.array_equal(g[:, 3], g[:, 40])
        assert (g[3, 3] + g[40, 40]) - 2.0 * g[3, 40] == 0.0


def test_gram_refuses_what_it_cannot_take():
    with pytest.raises(ValueError, match="multiple of 4"):
        FM.feature_gram(torch.zeros((3, 6), device=DEV))
    with pytest.raises(ValueError, match="16384"):
        FM.feature_gram(torch.zeros((1, 4), device=DEV).expand(16385, 4))


# ---- KID ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2,m,S", [(29, 29, 29, 1), (67, 67, 50, 7), (130, 67, 2, 3)])
def test_kid_subsets_equal_the_twin(n1, n2, m, S):
    for seed in (0, (7 << 32) + 5):
        got = FM.kid_subsets(n1, n2, m, S, seed, DEV).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, FO.kid_subsets(n1, n2, m, S, seed))


KID_CASES = [(37, 29, 64, None, 5), (130, 67, 192, 50, 7), (64, 64, 2048, None, 100)]


@pytest.mark.parametrize("n1,n2,d,m,S", KID_CASES)
def test_kid_values_against_the_twin(n1, n2, d, m, S):
    f1, f2 = two_sets(n1, n2, d, 7 * d)
    got = FM.kid_from_features(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), subsets=S, subset_size=m, seed=3)
    want = FO.kid(f1, f2, subsets=S, subset_size=m, seed=3)
    m_eff = min(n1, n2) if m is None else m
    s_eff = 1 if m_eff == n1 == n2 else S
    assert got["subset_size"] == want["subset_size"] == m_eff and got["subsets"] == want["subsets"] == s_eff
    values = got["values"].cpu().numpy()
    assert values.shape == (s_eff,) and got["values"].is_cuda
    scale = FO.kid_values(FO.gram_majorant(np.concatenate([f1, f2])), n1, want["idx"], 1.0 / d, 1.0, majorant=True)
    tol = (3 * d + 2 * m_eff + 16) * EPS * scale
    diff = np.abs(values - want["values"])
    print(f"kid ({n1} vs {n2}, d {d}, m {m_eff}, S {s_eff}): kid {got['kid']:.6f} twin {want['kid']:.6f}  max|diff| / tol "
          f"{float((diff / tol).max()):.4f}")
    assert bool((diff <= tol).all())
    assert 0.1 < got["kid"] < 0.5
    assert got["kid"] == float(values.mean()) and got["kid_std"] == (float(values.std()) if s_eff > 1 else 0.0)
    again = FM.kid_from_features(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), subsets=S, subset_size=m, seed=3)
    assert torch.equal(again["values"], got["values"])                         # run to run: the same bits
    if s_eff > 1:
        other = FM.kid_from_features(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), subsets=S, subset_size=m, seed=4)
        assert not torch.equal(other["values"], got["values"])


# ---- precision / recall / density / coverage ----------------------------------------------------------------------------------
def prdc_sets(case):
    nr, nf, d, k = case
    ref, gen = two_sets(nr, nf, d, 11 * d + nr)
    if d == 2048:               # half of the generated rows next to reference rows: precision is not trivially 0
        rng = np.random.default_rng(5)
        h = nf // 2
        gen[:h] = ref[:h] + np.float32(1e-2) * rng.standard_normal((h, d)).astype(np.float32)
    return ref, gen


PRDC_CASES = [(37, 29, 64, 3), (5, 4, 64, 3), (64, 64, 192, 1), (130, 67, 2048, 3)]


@pytest.mark.parametrize("case", PRDC_CASES, ids=lambda c: "-".join(map(str, c)))
def test_prdc_counts_equal_the_twin(case):
    nr, nf, d, k = case
    ref, gen = prdc_sets(case)
    z = np.concatenate([ref, gen])
    twin = FO.prdc(FO.gram(z), nr, nf, k)
    floor = 1e-9 * float(np.diag(FO.gram(z)).max())
    print(f"prdc {case}: twin counts {twin['counts'].tolist()}  margin {twin['margin']:.3e}  neighbour gap {twin['gap']:.3e}  "
          f"(floor {floor:.3e}, largest radius2 {float(twin['radius2'].max()):.3e})")
    assert twin["margin"] > floor and twin["gap"] > floor       # no comparison on the boundary: equality of counts is a fair demand
    G = FM.feature_gram(torch.from_numpy(z).to(DEV))
    counts, radius2 = FM.prdc_counts(G, nr, nf, k)
    assert counts.dtype == torch.int64 and counts.cpu().tolist() == twin["counts"].tolist()
    # a squared distance carries the Gram bound of G_ii, G_jj and twice that of G_ij (4 d 2^-53 max(|Z| |Z|^T)); the three
    # roundings of its own arithmetic are below 1 / d of that
    r2 = radius2.cpu().numpy()
    assert bool((np.abs(r2 - twin["radius2"]) <= 4 * d * EPS * float(FO.gram_majorant(z).max())).all())
    got = FM.prdc_from_features(torch.from_numpy(ref).to(DEV), torch.from_numpy(gen).to(DEV), k=k)
    want = FO.prdc_values(twin["counts"], nr, nf, k)
    assert got == {**{key: float(v) for key, v in want.items()}, "k": k}
    if d == 2048:
        assert got["precision"] >= (nf // 2) / nf                  # the rows placed next to reference rows are inside their balls
    counts2, _ = FM.prdc_counts(G, nr, nf, k)
    assert torch.equal(counts2, counts)


@pytest.mark.parametrize("n,d,k", [(29, 64, 3), (4, 64, 3), (130, 192, 1)])
def test_a_set_against_itself(n, d, k):
    f = torch.from_numpy(features(n, d, 77)).to(DEV)
    got = FM.prdc_from_features(f, f.clone(), k=k)
    assert got["precision"] == 1.0 and got["recall"] == 1.0 and got["coverage"] == 1.0 and got["density"] >= 1.0 / k


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd():
    return IO.synthetic_state_dict(0)


@pytest.fixture(scope="module")
def inception(sd):
    return fid.InceptionV3([fid.InceptionV3.BLOCK_INDEX_BY_DIM[64]], weights=sd).to(DEV)


def frame_sets(n=12):
    g = torch.Generator().manual_seed(41)
    a = torch.randint(0, 256, (n, 24, 32, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (n, 24, 32, 3), generator=g, dtype=torch.uint8)
    b[..., 1] //= 2                                   # the two sets differ in their colour statistics
    return a, b


def test_between_equals_from_features_bit_for_bit(inception):
    a, b = (s.to(DEV) for s in frame_sets())
    fa, fb = inception.features(a, 64), inception.features(b, 64)
    kid = FM.kid_between(a, b, inception, dims=64, subsets=6, subset_size=8, seed=9)
    want = FM.kid_from_features(fa, fb, subsets=6, subset_size=8, seed=9)
    assert torch.equal(kid["values"], want["values"]) and kid["kid"] == want["kid"] and kid["kid_std"] == want["kid_std"]
    assert (kid["subsets"], kid["subset_size"]) == (6, 8) and kid["kid_std"] > 0.0
    assert FM.prdc_between(a, b, inception, dims=64, k=3) == FM.prdc_from_features(fa, fb, k=3)
    whole = FM.kid_between(a, b, inception, dims=64)
    assert (whole["subsets"], whole["subset_size"], whole["kid_std"]) == (1, 12, 0.0)


def test_get_kid_score_on_two_directories(inception, tmp_path):
    from PIL import Image
    sets = frame_sets()
    for name, imgs in zip(("generated", "gt"), sets):
        os.makedirs(tmp_path / name)
        for i in range(imgs.shape[0]):
            Image.fromarray(imgs[i].numpy()).save(tmp_path / name / f"im_{i:03d}.png")
    # both routes run the twelve images as one batch (batch sizes 64 and 50 are cut to the data size), so the convolutions see the
    # same shapes and the features the same roundings: what remains is inside the KID tolerance
    got = FM.get_kid_score(str(tmp_path / "generated"), str(tmp_path / "gt"), dims=64, model=inception, subsets=4, subset_size=9, seed=1)
    frames = FM.kid_between(sets[0].to(DEV), sets[1].to(DEV), inception, dims=64, subsets=4, subset_size=9, seed=1)
    f = [inception.features(s.to(DEV), 64).cpu().numpy() for s in sets]
    idx = FO.kid_subsets(12, 12, 9, 4, 1)
    tol = (3 * 64 + 2 * 9 + 16) * EPS * FO.kid_values(FO.gram_majorant(np.concatenate(f)), 12, idx, 1.0 / 64, 1.0, majorant=True)
    diff = np.abs(got["values"].cpu().numpy() - frames["values"].cpu().numpy())
    print(f"get_kid_score {got['kid']:.9g}  frames {frames['kid']:.9g}  max|diff| / tol {float((diff / tol).max()):.4f}")
    assert bool((diff <= tol).all()) and got["subsets"] == 4 and got["subset_size"] == 9
    with pytest.raises(RuntimeError, match="Invalid path"):
        FM.get_kid_score(str(tmp_path / "nowhere"), str(tmp_path / "gt"), model=inception, dims=64)


def test_statistics_only_side_raises(inception, tmp_path):
    a, _ = frame_sets()
    mu, sigma = fid.calculate_activation_statistics(a, inception, 50, 64, DEV)
    np.savez(tmp_path / "a.npz", mu=mu, sigma=sigma)
    for fn in (FM.kid_between, FM.prdc_between):
        with pytest.raises(ValueError, match="needs the features themselves"):
            fn(a.to(DEV), str(tmp_path / "a.npz"), inception, dims=64)


@pytest.mark.parametrize("branch", ["splat", "rgbd"])
def test_scene_kid_and_sample_quality(inception, golden, branch):
    from sgam_neurips22_amd import testing
    from sgam_neurips22_amd.config import default_params
    from sgam_neurips22_amd.generative_sensing_module.model import VQModel
    from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
    g = golden("vqgan_full_ge256.npz")
    vq = VQModel(**default_params("google_earth"))
    vsd = testing.synthetic_state_dict(vq.state_dict(), seed=0)
    vsd["quantize.embedding.weight"] = testing.codebook_from_stats(float(g["zmean"]), float(g["zstd"]), 4096, 256, int(g["cb_seed"]))
    vq.load_state_dict(vsd)
    kw = dict(use_rgbd_integration=True, tsdf_memory_budget_bytes=1 << 30) if branch == "rgbd" else {}
    scene = InfiniteSceneGeneration(vq.to(DEV).eval(), "google_earth", output_dim=(4, 1), seed_frame=synthetic_seed_frame("google_earth", 0),
                                    **kw)
    scene.scene_expansion()
    assert len(scene.frames) == 4
    kid = scene.kid(scene, dims=64, inception=inception)
    assert (kid["subsets"], kid["subset_size"], kid["kid_std"]) == (1, 4, 0.0) and np.isfinite(kid["kid"])
    q = scene.sample_quality(scene, dims=64, inception=inception)
    assert q["precision"] == 1.0 and q["recall"] == 1.0 and q["coverage"] == 1.0 and q["k"] == 3
    # against other frames, through the same entry points as kid_between / prdc_between
    frames = torch.stack([scene.frames[c]["rgb_u8"] for c in scene._stored_coords(None, "test")])
    shifted = torch.cat([(frames.roll(40, dims=2) // 2), frames.flip(1)]).contiguous()
    assert scene.kid(shifted, dims=64, inception=inception, subsets=3, subset_size=3, seed=2)["values"].shape == (3,)
    assert scene.sample_quality(shifted, dims=64, inception=inception, k=2) == FM.prdc_between(shifted, frames, inception, dims=64, k=2)
    with pytest.raises(ValueError, match="k = 3 needs at least 4 rows"):
        scene.sample_quality(shifted, frames=list(scene.frames)[:3], dims=64, inception=inception)
