"""The reference's image metrics (sgam/generative_sensing_module/modules/misc/metrics.py: `PSNR`, `SSIM`, each with an
optional visibility mask) on the HIP kernels of csrc/eval.hip.  The reference computes them with cv2 / numpy on the host.

    psnr(img1, img2, visibility_mask=None)     ssim(img1, img2, visibility_mask=None)

Inputs are DEVICE tensors on the 0..255 scale, shaped (H,W), (H,W,C) or (B,H,W,C); any dtype (converted to fp32, the
kernels' input format; the sums are fp64).  The mask is per pixel: (H,W), (H,W,1) or the reference's channel-repeated
(H,W,C), with a leading B where the images have one.  Return conventions are the reference's: a float, or the pair
(all, visible) with a mask.  A multi-channel SSIM is the mean of the per-channel values; a batch gives the mean of the
per-image values (the reference takes one image at a time).  A mask that is zero everywhere makes the visible value a NaN
(0 / 0, what the reference's numpy division yields), never an exception; identical images make PSNR +inf.

There is no CPU fallback: an input that is not on the device raises `SgamHipError`."""
import math

import torch

from . import _lib
from .ops import SgamHipError, _p, _stream, check


def _device_f32(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise SgamHipError(f"{what} must be a tensor on the GPU: the metrics run on the HIP kernels, there is no CPU fallback")
    return t.to(torch.float32).contiguous()


def _bhwc(img, what):
    t = _device_f32(img, what)
    if t.dim() == 2:
        return t[None, :, :, None]
    if t.dim() == 3:
        return t[None]
    if t.dim() == 4:
        return t
    raise ValueError("Wrong input image dimensions.")


def _pixel_mask(mask, shape):
    """-> (B,H,W) fp32 dense, or None"""
    if mask is None:
        return None
    B, H, W, C = shape
    m = _device_f32(mask, "visibility_mask")
    if m.numel() == B * H * W * C and C > 1:
        m = m.reshape(B, H, W, C)
        if not torch.equal(m, m[..., :1].expand_as(m)):
            raise ValueError("visibility_mask differs between channels: a per-pixel mask is expected")
        m = m[..., 0]
    if m.numel() != B * H * W:
        raise ValueError(f"visibility_mask of shape {tuple(mask.shape)} does not match images of shape {(B, H, W, C)}")
    return m.reshape(B, H, W).contiguous()


def recon_stats(rec, target, mask=None, with_sq=False, map255=False, channels=None):
    """sgam_recon_stats_f32 on rec (B,H,W,ld) / target (B,H,W,C) dense NHWC fp32 (`channels` = C real channels of rec, default
    target's) -> (B, 6) float64 host array of per-image sums (include/sgam_hip.h)"""
    lib = _lib.load()
    B, H, W, ld = rec.shape
    C = int(channels if channels is not None else target.shape[3])
    assert target.shape == (B, H, W, C) and rec.is_contiguous() and target.is_contiguous()
    n = lib.sgam_recon_stats_partials(B, H * W)
    part = torch.empty((B, n // (6 * B), 6), device=rec.device, dtype=torch.float64)
    check(lib.sgam_recon_stats_f32(_p(rec), _p(target), _p(mask) if mask is not None else None, _p(part), B, H * W, C, ld,
                                   int(bool(with_sq)), int(bool(map255)), _stream()), "sgam_recon_stats_f32")
    return part.cpu().numpy().sum(axis=1)


def ssim_sums(img1, img2, mask=None, map255=False, channels=None):
    """sgam_ssim_f32 on two (B,H,W,ld) dense NHWC fp32 tensors -> (B, C, 3) float64 host array: sum ssim_map, sum ssim_map *
    mask, sum mask over the valid region of every image and channel"""
    lib = _lib.load()
    B, H, W, ld1 = img1.shape
    C = int(channels if channels is not None else ld1)
    assert img2.shape[:3] == (B, H, W) and img1.is_contiguous() and img2.is_contiguous()
    n = lib.sgam_ssim_partials(B, H, W, C)
    if n < 0:
        check(int(n), "sgam_ssim_partials")
    part = torch.empty((B, C, n // (3 * B * C), 3), device=img1.device, dtype=torch.float64)
    check(lib.sgam_ssim_f32(_p(img1), _p(img2), _p(mask) if mask is not None else None, _p(part), B, H, W, C, ld1, img2.shape[3],
                            int(bool(map255)), _stream()), "sgam_ssim_f32")
    return part.cpu().numpy().sum(axis=2)


def _psnr_of(mse):
    if mse != mse:
        return float("nan")
    return math.inf if mse <= 0.0 else 20.0 * math.log10(255.0 / math.sqrt(mse))


def psnr_from_stats(stats, pixels, channels, masked):
    """(B,6) sums of recon_stats(with_sq=True) -> mean over the images of the per-image PSNR [, the same over visible pixels]:
    mse = sum d^2 / (pixels * channels), visible mse = sum d^2 mask / (channels * sum mask) (metrics.py:18-20 with the
    reference's channel-repeated mask)"""
    allv = [_psnr_of(float(s[3]) / (pixels * channels)) for s in stats]
    out = sum(allv) / len(allv)
    if not masked:
        return out
    vis = [_psnr_of(float(s[4]) / (channels * float(s[5])) if s[5] > 0 else float("nan")) for s in stats]
    return out, sum(vis) / len(vis)


def ssim_from_sums(sums, valid_pixels, masked):
    """(B,C,3) sums of ssim_sums -> mean over images and channels of ssim_map.mean() [, of sum(ssim_map * mask) / sum(mask)]"""
    out = float(sums[..., 0].mean() / valid_pixels)
    if not masked:
        return out
    vis = [float(s[1] / s[2]) if s[2] > 0 else float("nan") for s in sums.reshape(-1, 3)]
    return out, sum(vis) / len(vis)


def psnr(img1, img2, visibility_mask=None):
    """Peak signal-to-noise ratio, images on the 0..255 scale (the reference's `PSNR.__call__`)"""
    a, b = _bhwc(img1, "img1"), _bhwc(img2, "img2")
    if a.shape != b.shape:
        raise ValueError("Input images must have the same dimensions.")
    B, H, W, C = a.shape
    m = _pixel_mask(visibility_mask, a.shape)
    # every channel enters the squared error; the kernel squares its first three columns, so wider images go in slices
    stats = None
    for c in range(0, C, 3):
        st = recon_stats(a[..., c:c + 3].contiguous(), b[..., c:c + 3].contiguous(), m, with_sq=True)
        if stats is None:
            stats = st
        else:
            stats[:, 3:5] += st[:, 3:5]
    return psnr_from_stats(stats, H * W, C, m is not None)


def ssim(img1, img2, visibility_mask=None):
    """Structural similarity, images on the 0..255 scale (the reference's `SSIM.__call__` / `_ssim`)"""
    a, b = _bhwc(img1, "img1"), _bhwc(img2, "img2")
    if a.shape != b.shape:
        raise ValueError("Input images must have the same dimensions.")
    B, H, W, C = a.shape
    m = _pixel_mask(visibility_mask, a.shape)
    return ssim_from_sums(ssim_sums(a, b, m), (H - 10) * (W - 10), m is not None)


class PSNR:
    """Peak Signal to Noise Ratio
    img1 and img2 have range [0, 255]"""

    def __init__(self):
        self.name = "PSNR"

    @staticmethod
    def __call__(img1, img2, visibility_mask=None):
        return psnr(img1, img2, visibility_mask)


class SSIM:
    """Structure Similarity
    img1, img2: [0, 255]"""

    def __init__(self):
        self.name = "SSIM"

    @staticmethod
    def __call__(img1, img2, visibility_mask=None):
        return ssim(img1, img2, visibility_mask)

    @staticmethod
    def _ssim(img1, img2, visibility_mask=None):
        return ssim(img1, img2, visibility_mask)
