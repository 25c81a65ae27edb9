"""CPU: the FID evaluation's host side (sgam_neurips22_amd/fid.py) and its test twin (tests/inception_oracle.py) — the twin's
pieces against torch.nn.functional, its layer table, the synthetic weights' activation range, both Fréchet-distance routes, the
reference's import paths and the argument validation of the new C entry points (no launch)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sgam_neurips22_amd import _lib, fid

sys.path.insert(0, os.path.dirname(__file__))
import inception_oracle as IO  # noqa: E402


# ---- the twin's pieces --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 4, 3, 3), (2, 5, 5, 7), (1, 3, 1, 2)])
def test_twin_pools_match_torch(shape):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    assert torch.allclose(IO.avgpool_nopad(x), F.avg_pool2d(x, 3, 1, 1, count_include_pad=False), rtol=0, atol=1e-14)
    assert torch.equal(IO.maxpool_s1p1(x), F.max_pool2d(x, 3, 1, 1))
    if shape[2] >= 3 and shape[3] >= 3:
        assert torch.equal(IO.maxpool_s2(x), F.max_pool2d(x, 3, 2))


@pytest.mark.parametrize("hw", [(37, 53), (512, 384), (299, 299)])
def test_twin_bilinear_matches_interpolate(hw):
    x = torch.rand((1, 3) + hw, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    want = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    # the twin forms the source coordinate in fp32 (the kernel's and fp32 PyTorch's arithmetic), F.interpolate on fp64 input in
    # fp64: the weights differ by ulps of a coordinate below 512, 512 * 2^-24 = 3e-5
    assert float((IO.bilinear(x, 299, 299) - want).abs().max()) <= 2 * 512 * 2.0 ** -24
    want32 = F.interpolate(x.float(), size=(299, 299), mode="bilinear", align_corners=False)
    # fp32 against fp32: both sides round the source coordinate (< max(hw)) in fp32, possibly in a different order of
    # operations: a few ulps of the coordinate on each axis, times a pixel difference <= 1, plus the blend's own few ulps of 1
    assert float((IO.bilinear(x.float(), 299, 299) - want32).abs().max()) <= (8 * max(hw) + 8) * 2.0 ** -24
    if hw == (299, 299):
        assert torch.equal(IO.bilinear(x, 299, 299), x)


def test_twin_layer_table():
    table = IO.conv_table()
    assert len(table) == 94
    by_name = {r[0]: r for r in table}
    assert by_name["Conv2d_1a_3x3"][1:] == (3, 32, (3, 3), 2, (0, 0))
    assert by_name["Mixed_5b.branch5x5_2"][1:] == (48, 64, (5, 5), 1, (2, 2))
    assert by_name["Mixed_6c.branch7x7dbl_4"][1:] == (160, 160, (7, 1), 1, (3, 0))
    assert by_name["Mixed_7a.branch7x7x3_4"][1:] == (192, 192, (3, 3), 2, (0, 0))
    assert by_name["Mixed_7c.branch3x3dbl_2"][1:] == (448, 384, (3, 3), 1, (1, 1))
    # channels of the concatenated outputs
    out = lambda name, keys: sum(by_name[f"{name}.{k}"][2] for k in keys)       # noqa: E731
    assert out("Mixed_5b", ["branch1x1", "branch5x5_2", "branch3x3dbl_3", "branch_pool"]) == 256
    assert out("Mixed_5d", ["branch1x1", "branch5x5_2", "branch3x3dbl_3", "branch_pool"]) == 288
    assert out("Mixed_6a", ["branch3x3", "branch3x3dbl_3"]) + 288 == 768
    assert out("Mixed_6e", ["branch1x1", "branch7x7_3", "branch7x7dbl_5", "branch_pool"]) == 768
    assert out("Mixed_7a", ["branch3x3_2", "branch7x7x3_4"]) + 768 == 1280
    e = [out("Mixed_7c", ["branch1x1"]), out("Mixed_7c", ["branch3x3_2a", "branch3x3_2b"]),
         out("Mixed_7c", ["branch3x3dbl_3a", "branch3x3dbl_3b"]), out("Mixed_7c", ["branch_pool"])]
    assert e == [320, 768, 768, 192] and sum(e) == 2048
    # every distinct conv geometry the GPU test covers
    assert {(r[3], r[4], r[5]) for r in table} == {
        ((1, 1), 1, (0, 0)), ((3, 3), 1, (0, 0)), ((3, 3), 1, (1, 1)), ((3, 3), 2, (0, 0)), ((5, 5), 1, (2, 2)),
        ((1, 7), 1, (0, 3)), ((7, 1), 1, (3, 0)), ((1, 3), 1, (0, 1)), ((3, 1), 1, (1, 0))}


def test_module_state_dict_is_the_twins_key_list():
    sd = IO.synthetic_state_dict(0)
    m = fid.InceptionV3(weights=sd)
    got = m.state_dict()
    assert list(got.keys()) == list(IO.state_dict_shapes().keys())
    assert all(tuple(got[k].shape) == s for k, s in IO.state_dict_shapes().items())
    assert "Mixed_6c.branch7x7dbl_4.conv.weight" in got and "Conv2d_1a_3x3.bn.num_batches_tracked" in got and "fc.bias" in got
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    assert not any(p.requires_grad for p in m.parameters())


def test_synthetic_weights_keep_activations_of_order_one():
    sd = IO.synthetic_state_dict(0)
    x = torch.rand((2, 3, 75, 91), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        outs = IO.forward(sd, x, (0, 1, 2, 3), resize_input=False)
    assert [tuple(o.shape[1:]) for o in outs] == [(64, 17, 21), (192, 7, 9), (768, 3, 4), (2048, 1, 1)]
    for o in outs:
        assert 0.5 < float(o.abs().max()) < 50.0
        assert 0.25 < float((o > 0).float().mean()) <= 1.0


def test_constructor_contract(tmp_path, monkeypatch):
    assert fid.InceptionV3.BLOCK_INDEX_BY_DIM == {64: 0, 192: 1, 768: 2, 2048: 3} and fid.InceptionV3.DEFAULT_BLOCK_INDEX == 3
    with pytest.raises(NotImplementedError):
        fid.InceptionV3(use_fid_inception=False, weights={})
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path))
    with pytest.raises(FileNotFoundError, match="pt_inception-2015-12-05-6726825d.pth"):
        fid.InceptionV3()
    os.makedirs(tmp_path / "checkpoints")
    torch.save(IO.synthetic_state_dict(1), tmp_path / "checkpoints" / fid.FID_WEIGHTS_FILE)
    m = fid.InceptionV3(output_blocks=(2, 0))
    assert m.output_blocks == [0, 2] and m.last_needed_block == 2
    with pytest.raises(_lib.SgamHipError, match="GPU"):
        m(torch.zeros(1, 3, 80, 80))                 # no CPU fallback


def test_no_url_in_the_module():
    text = open(fid.__file__).read()
    assert "http://" not in text and "https://" not in text and "load_url" not in text and "urlopen" not in text


# ---- distances ----------------------------------------------------------------------------------------------------------------
def test_frechet_distance_matches_recorded_reference(golden):
    g = golden("frechet_small.npz")
    assert list(g["cases"]) == ["d8_n200", "d8_n40", "d64_n200", "d64_n40"]
    for c in g["cases"]:
        got = fid.calculate_frechet_distance(g[f"{c}_mu1"], g[f"{c}_sigma1"], g[f"{c}_mu2"], g[f"{c}_sigma2"])
        want = float(g[f"{c}_fid"])
        print(c, got, want)
        assert abs(got - want) <= 1e-9 * abs(want)
        twin = IO.frechet_sqrtm(g[f"{c}_mu1"], g[f"{c}_sigma1"], g[f"{c}_mu2"], g[f"{c}_sigma2"])
        assert abs(twin - want) <= 1e-9 * abs(want)


def _features(seed, n, d, shift):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)) @ (rng.standard_normal((d, d)) / np.sqrt(d) + np.eye(d)) + shift


def test_lowrank_route_matches_eigh_on_full_rank():
    f1, f2 = _features(10, 40, 8, 0.3), _features(11, 50, 8, -0.2)
    want = IO.frechet_eigh(*IO.statistics(f1), *IO.statistics(f2))
    got = fid.frechet_distance_from_features(f1, f2)
    print(got, want)
    assert abs(got - want) <= 1e-10 * abs(want)
    assert abs(IO.frechet_lowrank(f1, f2) - want) <= 1e-10 * abs(want)
    assert abs(fid.frechet_distance_from_features(torch.from_numpy(f1), torch.from_numpy(f2)) - got) == 0.0


def test_lowrank_route_on_fewer_samples_than_dims(capsys):
    f1, f2 = _features(20, 12, 64, 0.3), _features(21, 9, 64, -0.2)
    got = fid.frechet_distance_from_features(f1, f2)
    assert np.isfinite(got) and got > 0.0
    assert "singular" not in capsys.readouterr().out          # no eps retry on this route
    # the same features against themselves: zero up to round-off of the traces
    scale = 2.0 * np.trace(np.cov(f1, rowvar=False))
    assert abs(fid.frechet_distance_from_features(f1, f1)) <= 1e-12 * scale
    # and the value is the eigh evaluation's (exact for any rank: symmetric factorizations only)
    want = IO.frechet_eigh(*IO.statistics(f1), *IO.statistics(f2))
    assert abs(got - want) <= 1e-7 * abs(want)      # sqrt of eigenvalues that are zero up to 1e-16 tr: error sqrt(1e-16) per null direction
    with pytest.raises(ValueError):
        fid.frechet_distance_from_features(f1, f2[:, :32])


def test_sqrtm_route_announces_its_retry(capsys, monkeypatch):
    """the singular branch of calculate_frechet_distance: a root that is not finite is retried with eps on the diagonals"""
    from scipy import linalg
    real, calls = linalg.sqrtm, []

    def sqrtm(a, disp=True):
        calls.append(a)
        if len(calls) == 1:
            return np.full_like(a, np.nan), np.inf
        return real(a)
    monkeypatch.setattr(linalg, "sqrtm", sqrtm)
    mu, s = IO.statistics(_features(30, 20, 4, 0.0))
    v = fid.calculate_frechet_distance(mu, s, mu + 1.0, s, eps=1e-6)
    assert "singular product" in capsys.readouterr().out and len(calls) == 2
    assert np.allclose(calls[1], (s + 1e-6 * np.eye(4)) @ (s + 1e-6 * np.eye(4)))
    assert abs(v - 4.0) <= 1e-4             # |diff|^2 = 4, tr(2 s - 2 sqrt((s + eps)^2)) = -2 * 4 * eps


def test_compute_statistics_of_path_npz_branch(tmp_path):
    mu, s = np.arange(4.0), np.eye(4)
    np.savez(tmp_path / "stats.npz", mu=mu, sigma=s)
    m, sg = fid.compute_statistics_of_path(str(tmp_path / "stats.npz"), None, 50, 4, "cuda")
    assert np.array_equal(m, mu) and np.array_equal(sg, s)
    with pytest.raises(RuntimeError, match="Invalid path"):
        fid.get_fid_score(str(tmp_path / "nope"), str(tmp_path / "stats.npz"), model=object())


# ---- import paths -------------------------------------------------------------------------------------------------------------
def test_reference_import_paths_resolve_to_this_backend():
    from sgam.generative_sensing_module.modules.misc.pytorch_fid import fid_score, inception
    from sgam.generative_sensing_module.modules.misc.pytorch_fid.fid_score import get_fid_score
    from sgam.generative_sensing_module.modules.misc.pytorch_fid.inception import InceptionV3
    assert get_fid_score is fid.get_fid_score and InceptionV3 is fid.InceptionV3
    for name in ("get_activations", "calculate_activation_statistics", "compute_statistics_of_path", "calculate_frechet_distance",
                 "calculate_fid_given_paths", "InceptionV3"):
        assert getattr(fid_score, name) is getattr(fid, name)
    assert inception.InceptionV3 is fid.InceptionV3
    import inspect
    sig = inspect.signature(get_fid_score)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[:6]] == [
        ("generated_path", inspect.Parameter.empty), ("gt_path", inspect.Parameter.empty), ("batch_size", 64), ("num_workers", 0),
        ("device", "cuda:0"), ("dims", 2048)]
    sig = inspect.signature(fid.get_activations)
    assert [(p.name, p.default) for p in sig.parameters.values()][2:4] == [("batch_size", 50), ("dims", 2048)]


# ---- argument validation of the new entry points, without a GPU ---------------------------------------------------------------
def test_argument_validation_without_gpu():
    lib = _lib.load()
    ref = ctypes.byref
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    d = _lib.ConvDesc(B=1, Hi=8, Wi=8, Cin=48, Ho=8, Wo=8, N=64, KH=5, KW=5, stride=1, pad_t=2, pad_l=2, upsample2x=0,
                      lda=48, ldb=25 * 48, ldc=256, ldr=0, n_valid=64, bias_per_row=0)
    assert lib.sgam_conv2d_workspace_bytes(ref(d)) >= 0                  # Cin = 48: a descriptor the fp32-in MFMA conv takes
    assert lib.sgam_conv2d_relu_nhwc_f32(ref(d), None, None, None, None, None, 0, None) == -1
    d.Cin = 3
    assert lib.sgam_conv2d_relu_nhwc_f32(ref(d), p, p, p, p, None, 0, None) == -1      # Cin % 4 != 0
    assert lib.sgam_inception_preprocess_f32(None, 1, 1, 8, 8, None, 299, 299, 1, None) == -1
    assert lib.sgam_inception_preprocess_f32(p, 1, 1, 0, 8, p, 299, 299, 1, None) == -1
    assert lib.sgam_inception_preprocess_f32(p, 1, 1, 8, 8, p, 0, 299, 1, None) == -1
    ho, wo = ctypes.c_int32(), ctypes.c_int32()
    assert lib.sgam_pool3x3_out_size(7, 9, 0, ref(ho), ref(wo)) == 0 and (ho.value, wo.value) == (3, 4)
    assert lib.sgam_pool3x3_out_size(1, 2, 1, ref(ho), ref(wo)) == 0 and (ho.value, wo.value) == (1, 2)
    assert lib.sgam_pool3x3_out_size(2, 9, 0, ref(ho), ref(wo)) == -1    # stride-2 pool without padding needs 3 rows
    assert lib.sgam_pool3x3_out_size(7, 9, 3, ref(ho), ref(wo)) == -1
    assert lib.sgam_pool3x3_nhwc_f32(None, 1, 5, 5, 4, 4, None, 4, 0, None) == -1
    assert lib.sgam_pool3x3_nhwc_f32(p, 1, 5, 5, 4, 3, p, 4, 0, None) == -1             # ldx < C
    assert lib.sgam_pool3x3_nhwc_f32(p, 1, 5, 5, 4, 4, p, 2, 0, None) == -1             # ldo < C
    assert lib.sgam_pool3x3_nhwc_f32(p, 1, 2, 2, 4, 4, p, 4, 0, None) == -1
    assert lib.sgam_pool3x3_nhwc_f32(p, 1, 5, 5, 4, 4, p, 4, 7, None) == -1
    assert lib.sgam_global_avgpool_nhwc_f32(None, 1, 4, 4, 4, None, None) == -1
    assert lib.sgam_global_avgpool_nhwc_f32(p, 1, 4, 8, 4, p, None) == -1               # ldx < C
    assert lib.sgam_global_avgpool_nhwc_f32(p, 0, 4, 4, 4, p, None) == -1
    assert lib.sgam_activation_stats_state_doubles(2048) == 1 + 2 * 2048 + 2048 * 2048
    assert lib.sgam_activation_stats_state_doubles(0) == -1
    assert lib.sgam_activation_stats_update_f64(None, 4, 8, 8, None, 1, None) == -1
    assert lib.sgam_activation_stats_update_f64(p, 0, 8, 8, p, 1, None) == -1
    assert lib.sgam_activation_stats_update_f64(p, 4, 8, 4, p, 1, None) == -1           # ldx < d
    assert lib.sgam_activation_stats_finalize_f64(p, 8, None, p, None) == -1
    assert lib.sgam_activation_stats_finalize_f64(p, 0, p, p, None) == -1
