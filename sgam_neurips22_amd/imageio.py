"""Device image ops of the training data path (csrc/imageio.hip): PIL's uint8 LANCZOS resize and
`F.interpolate(mode='nearest')` of depth maps, bit for bit, on device tensors.  The host's share is the coefficient tables of
`Image.resize`: float64, once per (input size, output size), cached on the device."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import SgamHipError, check
from ._opscore import _c, _need_cuda, _p, _stream
from .ops_aux import rgb_lut

PRECISION_BITS = 22          # Pillow, 8-bit channels: 32 - 8 - 2
LANCZOS_SUPPORT = 3.0
SENTINEL, SENTINEL_REPLACEMENT = 65504.0, -99999.0      # data/google_earth.py:174


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


def lanczos_tables(n_in, n_out):
    """(bounds int32 [n_out][2] = (first input index, taps), coef int32 [n_out][K]) of one axis, as `Image.resize` computes
    them: window centre (i + 0.5) * in / out, support 3 * max(in / out, 1), weights normalised in float64 and rounded half
    away from zero to 22 fractional bits."""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = LANCZOS_SUPPORT * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    coef = np.zeros((n_out, ksize), np.int32)
    ss = 1.0 / filterscale
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = np.array([_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)], np.float64)
        ww = 0.0
        for v in w:             # the reference's left-to-right sum
            ww += v
        if ww != 0.0:
            w = w / ww
        q = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS))
        coef[i, :xmax] = np.trunc(q).astype(np.int32)
        bounds[i] = (xmin, xmax)
    return bounds, coef


_TABLES = {}


def _device_tables(n_in, n_out, device):
    key = (n_in, n_out, str(device))
    if key not in _TABLES:
        b, k = lanczos_tables(n_in, n_out)
        _TABLES[key] = (np.ascontiguousarray(b), torch.from_numpy(b).to(device), torch.from_numpy(k).to(device), k.shape[1])
    return _TABLES[key]


def _dense_out(t, shape, dtype, device, what):
    if t is None:
        return None
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != device:
        raise SgamHipError(f"{what}: expected a contiguous {dtype} tensor of shape {tuple(shape)} on {device}, "
                           f"got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def resize_lanczos_u8(images_u8, size, out_u8=None, out_f32=None):
    """`PIL.Image.resize((size[1], size[0]), LANCZOS)` of (M, Hin, Win, 3) uint8 device images, all in one launch.  Writes the
    uint8 result into `out_u8` and / or `float32(u / 127.5 - 1.0)` into `out_f32` (dense (M, H, W, 3) tensors or views, e.g.
    a batch tensor reshaped); with neither given, a new uint8 tensor is returned.  Same size in and out: the conversion alone.
    Returns (out_u8, out_f32) as given, or the new tensor."""
    _need_cuda(images_u8, out_u8, out_f32)
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3:
        raise SgamHipError(f"resize_lanczos_u8: expected (M, H, W, 3) uint8, got {images_u8.dtype} {tuple(images_u8.shape)}")
    src = _c(images_u8)
    M, Hin, Win, _ = src.shape
    Hout, Wout = int(size[0]), int(size[1])
    dev = src.device
    made = out_u8 is None and out_f32 is None
    if made:
        out_u8 = torch.empty((M, Hout, Wout, 3), dtype=torch.uint8, device=dev)
    _dense_out(out_u8, (M, Hout, Wout, 3), torch.uint8, dev, "resize_lanczos_u8 out_u8")
    _dense_out(out_f32, (M, Hout, Wout, 3), torch.float32, dev, "resize_lanczos_u8 out_f32")
    if (Hin, Win) == (Hout, Wout):
        hb_h = hb = hk = vb_h = vb = vk = None
        KH = KV = 0
    else:
        hb_h, hb, hk, KH = _device_tables(Win, Wout, dev)
        vb_h, vb, vk, KV = _device_tables(Hin, Hout, dev)
    hp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    check(_lib.load().sgam_resize_lanczos_u8(_p(src), M, Hin, Win, Hout, Wout, hp(hb_h), _p(hb), _p(hk), KH, hp(vb_h), _p(vb), _p(vk),
                                             KV, _p(rgb_lut(dev)), _p(out_u8), _p(out_f32), _stream()), "sgam_resize_lanczos_u8")
    return out_u8 if made else (out_u8, out_f32)


def resize_nearest(depths, size, replace_sentinel=None, mask_out=None, out=None):
    """`F.interpolate(depths[:, None], size=size)` (nearest) of (M, Hin, Win) float32 device maps -> (M, H, W).
    `replace_sentinel=(sentinel, value)` rewrites outputs equal to `sentinel` (the sources' 65504 -> -99999);
    `mask_out` (M, H, W) float32 receives `resized != 65504` (the sentinel of `replace_sentinel` when given) as 0 / 1."""
    _need_cuda(depths, mask_out, out)
    if depths.dtype != torch.float32 or depths.dim() != 3:
        raise SgamHipError(f"resize_nearest: expected (M, H, W) float32, got {depths.dtype} {tuple(depths.shape)}")
    src = _c(depths)
    M, Hin, Win = src.shape
    Hout, Wout = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty((M, Hout, Wout), dtype=torch.float32, device=src.device)
    _dense_out(out, (M, Hout, Wout), torch.float32, src.device, "resize_nearest out")
    _dense_out(mask_out, (M, Hout, Wout), torch.float32, src.device, "resize_nearest mask_out")
    sentinel, value = replace_sentinel if replace_sentinel is not None else (SENTINEL, SENTINEL_REPLACEMENT)
    check(_lib.load().sgam_resize_nearest_f32(_p(src), M, Hin, Win, Hout, Wout, _p(out), int(replace_sentinel is not None),
                                              float(sentinel), float(value), _p(mask_out), _stream()), "sgam_resize_nearest_f32")
    return out
