"""CPU: the validation-step / image-metric additions (csrc/eval.hip, training.validation_step, sgam_neurips22_amd/metrics.py) as far
as they can be checked without a GPU: symbols and argument validation, the epoch arithmetic, the internal consistency of
tests/golden/eval_step_small.npz (generated from the reference by tests/golden/gen_golden_eval.py), and the test-side fp64
restatement of PSNR / SSIM (`psnr_ref`, `ssim_ref` below, also used by tests/test_gpu_eval.py) against that fixture."""
import ctypes

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import _lib, testing, training
from sgam_neurips22_amd.config import default_params

NEW = ("sgam_recon_stats_f32", "sgam_ssim_f32", "sgam_index_histogram_i32", "sgam_recon_stats_partials", "sgam_ssim_partials")


# ---- fp64 restatement of the reference's metrics (modules/misc/metrics.py), images (H,W,C) on the 0..255 scale
def to255(a):
    """clip((v + 1) * 127.5, 0, 255) in fp32, no uint8 truncation"""
    return np.clip((np.asarray(a, np.float32) + np.float32(1.0)) * np.float32(127.5), np.float32(0), np.float32(255)).astype(np.float32)


def psnr_ref(img1, img2, mask=None):
    """mask (H,W): visible mse = sum_c sum_p d^2 m / (C sum_p m) — the reference's formula with its channel-repeated mask"""
    a, b = np.asarray(img1, np.float64), np.asarray(img2, np.float64)
    a, b = (a[..., None], b[..., None]) if a.ndim == 2 else (a, b)
    d2 = (a - b) ** 2
    out = 20 * np.log10(255.0 / np.sqrt(d2.mean()))
    if mask is None:
        return out
    m = np.asarray(mask, np.float64)[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return out, 20 * np.log10(255.0 / np.sqrt((d2 * m).sum() / (m.sum() * a.shape[-1])))


def gauss11():
    i = np.arange(11, dtype=np.float64) - 5.0
    k = np.exp(-(i * i) / (2 * 1.5 ** 2))
    return k / k.sum()


def _valid_filter(a):
    """11 x 11 Gaussian (outer product of gauss11) over the valid region: (H,W) -> (H-10, W-10), fp64"""
    k = gauss11()
    H, W = a.shape
    rows = sum(k[j] * a[:, j:j + W - 10] for j in range(11))
    return sum(k[i] * rows[i:i + H - 10] for i in range(11))


def ssim_ref(img1, img2, mask=None):
    """mean over the channels of SSIM._ssim; mask (H,W)"""
    a, b = np.asarray(img1, np.float64), np.asarray(img2, np.float64)
    a, b = (a[..., None], b[..., None]) if a.ndim == 2 else (a, b)
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    alls, vis = [], []
    for c in range(a.shape[-1]):
        x, y = a[..., c], b[..., c]
        mu1, mu2 = _valid_filter(x), _valid_filter(y)
        s1, s2, s12 = _valid_filter(x * x) - mu1 ** 2, _valid_filter(y * y) - mu2 ** 2, _valid_filter(x * y) - mu1 * mu2
        smap = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))
        alls.append(smap.mean())
        if mask is not None:
            m = np.asarray(mask, np.float64)[5:-5, 5:-5]
            with np.errstate(invalid="ignore", divide="ignore"):
                vis.append((smap * m).sum() / m.sum())
    return float(np.mean(alls)) if mask is None else (float(np.mean(alls)), float(np.mean(vis)))


def fixture_images(g):
    """per image: (xrec RGB, x_dst RGB) as (H,W,3) fp32 on the 0..255 scale, visibility (H,W) fp32"""
    _, mask, x_dst = testing.train_batch()
    out = []
    for b in range(x_dst.shape[0]):
        vis = (~mask[b].bool()).reshape(x_dst.shape[2], x_dst.shape[3]).numpy().astype(np.float32)
        out.append((to255(g["xrec_rgb"][b].transpose(1, 2, 0)), to255(x_dst[b, :3].permute(1, 2, 0).numpy()), vis))
    return out


# ---- tests
def test_new_symbols_are_exported_and_bound():
    lib = _lib.load()
    assert lib.sgam_abi_version() == 10                 # additive change
    for name in NEW:
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)           # host memory: a launch would fault, a validation failure must come first
    EINVAL = -1
    # recon stats
    assert lib.sgam_recon_stats_f32(None, p, None, p, 1, 64, 4, 4, 0, 0, None) == EINVAL
    assert lib.sgam_recon_stats_f32(p, None, None, p, 1, 64, 4, 4, 0, 0, None) == EINVAL
    assert lib.sgam_recon_stats_f32(p, p, None, None, 1, 64, 4, 4, 0, 0, None) == EINVAL
    assert lib.sgam_recon_stats_f32(p, p, None, p, 0, 64, 4, 4, 0, 0, None) == EINVAL
    assert lib.sgam_recon_stats_f32(p, p, None, p, 1, 0, 4, 4, 0, 0, None) == EINVAL
    assert lib.sgam_recon_stats_f32(p, p, None, p, 1, 64, 0, 4, 0, 0, None) == EINVAL
    assert lib.sgam_recon_stats_f32(p, p, None, p, 1, 64, 4, 3, 0, 0, None) == EINVAL          # ld_rec < C
    assert lib.sgam_recon_stats_f32(p, p, p, p, 1, 64, 4, 4, 0, 0, None) == EINVAL             # a mask needs with_sq
    assert lib.sgam_recon_stats_partials(2, 64 * 64) == 2 * 4 * 6 and lib.sgam_recon_stats_partials(1, 1025) == 12
    assert lib.sgam_recon_stats_partials(0, 64) == EINVAL
    # SSIM
    assert lib.sgam_ssim_f32(None, p, None, p, 1, 16, 16, 3, 3, 3, 0, None) == EINVAL
    assert lib.sgam_ssim_f32(p, None, None, p, 1, 16, 16, 3, 3, 3, 0, None) == EINVAL
    assert lib.sgam_ssim_f32(p, p, None, None, 1, 16, 16, 3, 3, 3, 0, None) == EINVAL
    assert lib.sgam_ssim_f32(p, p, None, p, 1, 10, 16, 3, 3, 3, 0, None) == EINVAL             # H < 11
    assert lib.sgam_ssim_f32(p, p, None, p, 1, 16, 10, 3, 3, 3, 0, None) == EINVAL             # W < 11
    assert lib.sgam_ssim_f32(p, p, None, p, 0, 16, 16, 3, 3, 3, 0, None) == EINVAL
    assert lib.sgam_ssim_f32(p, p, None, p, 1, 16, 16, 0, 3, 3, 0, None) == EINVAL
    assert lib.sgam_ssim_f32(p, p, None, p, 1, 16, 16, 3, 2, 3, 0, None) == EINVAL             # ld < C
    assert lib.sgam_ssim_partials(1, 10, 64, 3) == EINVAL and lib.sgam_ssim_partials(1, 11, 11, 1) == 3
    assert lib.sgam_ssim_partials(3, 37, 53, 3) == 3 * 3 * (2 * 3) * 3 and lib.sgam_ssim_partials(1, 256, 256, 3) == 3 * 16 * 16 * 3
    # histogram
    assert lib.sgam_index_histogram_i32(None, 4, p, 8, None) == EINVAL
    assert lib.sgam_index_histogram_i32(p, 4, None, 8, None) == EINVAL
    assert lib.sgam_index_histogram_i32(p, 0, p, 8, None) == EINVAL
    assert lib.sgam_index_histogram_i32(p, 4, p, 0, None) == EINVAL


def _small_trainer(phase):
    from sgam_neurips22_amd.generative_sensing_module.model import VQModel
    p = testing.small_train_params(default_params("google_earth"))
    p["phase"] = phase
    return training.AutoencoderTrainer(VQModel(**p), phase=phase, lr=1e-4)


def test_validation_epoch_end_arithmetic():
    """epoch means of the step logs and the active share of a hand-filled histogram (host arithmetic only)"""
    tr = _small_trainer("codebook")
    tr.validation_epoch_start()
    assert tr.validation_epoch_end() == {}
    tr._record_validation({"val/rec_loss": 0.5, "val/rgb_l1": 1.0})
    tr._record_validation({"val/rec_loss": 0.25, "val/rgb_l1": 2.0})
    tr._record_validation({"val/rec_loss": 0.75, "val/rgb_l1": 3.0, "val/psnr": 20.0})       # a key seen once: its own count
    h = torch.zeros(64, dtype=torch.int32)
    h[[0, 5, 63]] = torch.tensor([3, 1, 7], dtype=torch.int32)
    tr._val_hist = h
    out = tr.validation_epoch_end()
    assert out == {"val/rec_loss": 0.5, "val/rgb_l1": 2.0, "val/psnr": 20.0, "val/codebook_active_percentage": 3 / 64}
    tr.validation_epoch_start()                                      # a new epoch starts from nothing
    assert int(tr._val_hist.sum()) == 0 and tr.validation_epoch_end() == {"val/codebook_active_percentage": 0.0}
    # the phase that trains the encoder alone has no codebook health number
    tr2 = _small_trainer("conditional_generation")
    tr2._record_validation({"val/rec_loss": 1.0})
    assert tr2.validation_epoch_end() == {"val/rec_loss": 1.0}


def test_fixture_is_internally_consistent(golden):
    g = golden("eval_step_small.npz")
    eps = float(np.finfo(np.float32).eps)
    for tag in ("d0", "d1"):
        v = {k[len(tag) + 1:]: float(g[k]) for k in g.files if k.startswith(tag + ".")}
        assert set(v) == {"val/aeloss", "val/total_loss", "val/quant_loss", "val/rec_loss", "val/p_loss", "val/d_weight", "val/disc_factor",
                          "val/g_loss", "val/disc_loss", "val/logits_real", "val/logits_fake", "val/rgb_l1", "val/disparity_l1"}
        assert v["val/d_weight"] == 0.0 and v["val/p_loss"] == 0.0
        assert abs(v["val/total_loss"] - (v["val/rec_loss"] + v["val/quant_loss"])) <= 4 * eps * v["val/total_loss"]
        assert v["val/aeloss"] == v["val/total_loss"]
        assert abs(v["val/rec_loss"] - (3 * v["val/rgb_l1"] + v["val/disparity_l1"]) / 4) <= 8 * eps * v["val/rec_loss"]
        assert v["val/g_loss"] == -v["val/logits_fake"]
    assert float(g["d0.val/disc_factor"]) == 1.0 and float(g["d1.val/disc_factor"]) == 0.0
    assert float(g["d0.val/disc_loss"]) > 0.0 and float(g["d1.val/disc_loss"]) == 0.0
    assert g["indices"].shape == (2, 32 * 32) and g["indices"].min() >= 0 and g["indices"].max() < 64
    bn = [k for k in g.files if k.startswith("bn.")]
    assert len(bn) == 6 and all(np.abs(g[k] - (0.0 if k.endswith("mean") else 1.0)).max() > 0.1 for k in bn)     # non-trivial statistics


def test_fp64_restatement_reproduces_the_reference_metrics(golden):
    """pins `psnr_ref` / `ssim_ref` (the oracle of the GPU tests) to numbers the reference's own PSNR / SSIM classes produced"""
    g = golden("eval_step_small.npz")
    assert [str(n) for n in g["metric_names"]] == ["psnr", "psnr_visible", "ssim", "ssim_visible"]
    for (a, b, vis), want in zip(fixture_images(g), g["metrics_per_image"]):
        got = list(psnr_ref(a, b, vis)) + list(ssim_ref(a, b, vis))
        for x, w in zip(got, want):
            assert abs(x - w) <= 1e-9 * abs(w), (got, want)
        assert abs(psnr_ref(a, b) - want[0]) <= 1e-9 * want[0] and abs(ssim_ref(a, b) - want[2]) <= 1e-9 * abs(want[2])


def test_metrics_have_no_cpu_fallback():
    from sgam_neurips22_amd import metrics
    from sgam.generative_sensing_module.modules.misc import metrics as alias
    assert alias.PSNR is metrics.PSNR and alias.SSIM is metrics.SSIM
    a = torch.zeros(16, 16, 3)
    with pytest.raises(_lib.SgamHipError):
        metrics.psnr(a, a)
    with pytest.raises(_lib.SgamHipError):
        metrics.SSIM()(a.numpy(), a.numpy())
