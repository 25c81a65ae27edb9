"""Device image ops of the training data path (csrc/imageio.hip): PIL's uint8 LANCZOS and BICUBIC resize,
`F.interpolate(mode='nearest')` of depth maps and the single-frame dataset's depth arithmetic, bit for bit, on device tensors.
The host's share is the coefficient tables of `Image.resize`: float64, once per (filter, input size, output size), cached on
the device; and the few constants of the depth arithmetic, rounded to the precision numpy would use."""
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
BICUBIC_SUPPORT = 2.0
SENTINEL, SENTINEL_REPLACEMENT = 65504.0, -99999.0      # data/google_earth.py:174


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


def _bicubic(x):
    a = -0.5                    # Pillow's BICUBIC
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def lanczos_tables(n_in, n_out):
    """(bounds int32 [n_out][2] = (first input index, taps), coef int32 [n_out][K]) of one axis, as `Image.resize` computes
    them: window centre (i + 0.5) * in / out, support 3 * max(in / out, 1), weights normalised in float64 and rounded half
    away from zero to 22 fractional bits."""
    return _filter_tables(n_in, n_out, _lanczos, LANCZOS_SUPPORT)


def bicubic_tables(n_in, n_out):
    """the same tables for `Image.resize`'s default filter: BICUBIC (a = -0.5), support 2 * max(in / out, 1)"""
    return _filter_tables(n_in, n_out, _bicubic, BICUBIC_SUPPORT)


def _filter_tables(n_in, n_out, filt, filter_support):
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = filter_support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    coef = np.zeros((n_out, ksize), np.int32)
    ss = 1.0 / filterscale
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = np.array([filt((x + xmin - center + 0.5) * ss) for x in range(xmax)], np.float64)
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


def _device_tables(n_in, n_out, device, filt="lanczos"):
    key = (filt, n_in, n_out, str(device))
    if key not in _TABLES:
        b, k = {"lanczos": lanczos_tables, "bicubic": bicubic_tables}[filt](n_in, n_out)
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


def resize_bicubic_u8(images_u8, size, out_f32=None, channels=3):
    """`PIL.Image.resize((size[1], size[0]))` — Pillow's default filter, BICUBIC — of (M, Hin, Win, 3) uint8 device images in one
    launch, as `float32(u / 127.5 - 1.0)` into channels 0..2 of `out_f32`: a contiguous (M, H, W, channels) float32 tensor,
    channels 3 or 4.  With 4 (an RGB-D batch tensor) the fourth channel is left as it was.  Same size in and out: the
    conversion alone.  Returns `out_f32` (a new tensor when none is given; its fourth channel is zero)."""
    _need_cuda(images_u8, out_f32)
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3:
        raise SgamHipError(f"resize_bicubic_u8: expected (M, H, W, 3) uint8, got {images_u8.dtype} {tuple(images_u8.shape)}")
    if channels not in (3, 4):
        raise SgamHipError(f"resize_bicubic_u8: channels must be 3 or 4, not {channels!r}")
    src = _c(images_u8)
    M, Hin, Win, _ = src.shape
    Hout, Wout = int(size[0]), int(size[1])
    dev = src.device
    if out_f32 is None:
        out_f32 = torch.zeros((M, Hout, Wout, channels), dtype=torch.float32, device=dev)
    _dense_out(out_f32, (M, Hout, Wout, channels), torch.float32, dev, "resize_bicubic_u8 out_f32")
    if (Hin, Win) == (Hout, Wout):
        hb_h = hb = hk = vb_h = vb = vk = None
        KH = KV = 0
    else:
        hb_h, hb, hk, KH = _device_tables(Win, Wout, dev, "bicubic")
        vb_h, vb, vk, KV = _device_tables(Hin, Hout, dev, "bicubic")
    hp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    check(_lib.load().sgam_resize_bicubic_u8(_p(src), M, Hin, Win, Hout, Wout, hp(hb_h), _p(hb), _p(hk), KH, hp(vb_h), _p(vb), _p(vk),
                                             KV, _p(rgb_lut(dev)), _p(out_f32), channels, _stream()), "sgam_resize_bicubic_u8")
    return out_f32


CODEC_MODES = {"half": 0, "float32": 1, "float64": 2}


def codec_constants(dataset, arith, K=None):
    """the 7 doubles `sgam_frame_depth_codec_f32` reads — (add, sub, div, K00, K00 ** 2, K02, K12) — rounded the way numpy
    rounds the Python-float constants of data/base.py:85-88, 111-115 when it meets an array of the file's dtype"""
    if dataset == "google_earth":
        if arith not in ("half", "float32"):
            raise SgamHipError(f"frame_depth_codec: google_earth maps are computed in 'half' or 'float32', not {arith!r}")
        t = np.float16 if arith == "half" else np.float32
        return [10.0, float(t(1 / 14.765625)), float(t(1 / 10.099975586 - 1 / 14.765625)), 0.0, 0.0, 0.0, 0.0]
    if dataset == "clevr-infinite":
        if arith != "float64":
            raise SgamHipError(f"frame_depth_codec: clevr-infinite maps are computed in 'float64', not {arith!r}")
        K = None if K is None else np.asarray(K)
        if K is None or K.dtype != np.float64 or K.shape[0] < 2 or K.shape[1] < 3:
            raise SgamHipError("frame_depth_codec: clevr-infinite needs K, a float64 matrix of at least 2 x 3 (already scaled)")
        return [0.0, 1 / 16, 1 / 7 - 1 / 16, float(K[0][0]), float(K[0][0] ** 2), float(K[0][2]), float(K[1][2])]
    raise NotImplementedError(dataset)


def frame_depth_codec(depths, size, dataset, arith, K=None, out=None, channel=3):
    """The single-frame dataset's depth channel (data/base.py:76-88, 104-115) of (M, Hin, Win) float32 device maps (half files
    staged as float32): nearest resize to `size`, then `2 * ((1 / d' - lo) / (hi - lo)) - 1` with d' = d + 10 (google_earth) or
    the ray -> z conversion with `K` (clevr-infinite), every step rounded as numpy rounds it for a file of dtype `arith`:
    "half" | "float32" (google_earth), "float64" (clevr-infinite).  Written to `out[..., channel]`, a contiguous (M, H, W, C)
    float32 tensor with C <= 4; no other channel is touched.  Without `out`: a new (M, H, W, 1) tensor, channel 0."""
    _need_cuda(depths, out)
    if depths.dtype != torch.float32 or depths.dim() != 3:
        raise SgamHipError(f"frame_depth_codec: expected (M, H, W) float32, got {depths.dtype} {tuple(depths.shape)}")
    consts = codec_constants(dataset, arith, K)
    src = _c(depths)
    M, Hin, Win = src.shape
    Hout, Wout = int(size[0]), int(size[1])
    if out is None:
        out, channel = torch.empty((M, Hout, Wout, 1), dtype=torch.float32, device=src.device), 0
    if out.dim() != 4 or not 1 <= out.shape[3] <= 4 or not 0 <= int(channel) < out.shape[3]:
        raise SgamHipError(f"frame_depth_codec out: expected (M, H, W, C <= 4) with channel < C, got {tuple(out.shape)}, channel {channel}")
    _dense_out(out, (M, Hout, Wout, out.shape[3]), torch.float32, src.device, "frame_depth_codec out")
    check(_lib.load().sgam_frame_depth_codec_f32(_p(src), M, Hin, Win, Hout, Wout, CODEC_MODES[arith], (ctypes.c_double * 7)(*consts),
                                                 _p(out), int(out.shape[3]), int(channel), _stream()), "sgam_frame_depth_codec_f32")
    return out
