"""Test-side oracle: a tap-for-tap numpy restatement of Pillow's uint8 LANCZOS resize (two separable fixed-point passes,
horizontal first with a uint8 intermediate image, then vertical).  Independent of sgam_neurips22_amd.imageio: the tests
compare both against PIL itself."""
import math

import numpy as np

PRECISION_BITS = 22


def _lanczos3(x):
    def sinc(v):
        return 1.0 if v == 0.0 else math.sin(v * math.pi) / (v * math.pi)
    return sinc(x) * sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


def axis_coefficients(n_in, n_out):
    """[(first input index, int32 coefficients)] per output index: weights in float64, normalised, rounded half away from
    zero to 22 fractional bits"""
    scale = n_in / n_out
    fscale = max(scale, 1.0)
    support = 3.0 * fscale
    out = []
    for i in range(n_out):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        w = [_lanczos3((x - center + 0.5) / fscale) for x in range(lo, hi)]
        total = 0.0
        for v in w:
            total += v
        w = [v / total if total != 0.0 else v for v in w]
        k = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
        out.append((lo, np.array(k, np.int64)))
    return out


def _pass(img, n_out, axis):
    """one pass along `axis` of a (H, W, C) uint8 image"""
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    res = np.empty((n_out,) + img.shape[1:], np.uint8)
    for i, (lo, k) in enumerate(axis_coefficients(img.shape[0], n_out)):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, img[lo:lo + len(k)], axes=(0, 0))
        assert np.abs(acc).max() < 2 ** 31          # the int32 accumulator of the C code and of the kernel does not overflow
        res[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(res, 0, axis)


def resize_lanczos_u8(img, size):
    """(H, W, C) uint8 -> (size[0], size[1], C) uint8, equal to np.array(Image.fromarray(img).resize((size[1], size[0]), LANCZOS))"""
    h, w = img.shape[:2]
    out = img
    if size[1] != w:
        out = _pass(out, size[1], 1)
    if size[0] != h:
        out = _pass(out, size[0], 0)
    return out
