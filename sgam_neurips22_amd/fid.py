"""FID evaluation on the HIP backend: the reference's `modules/misc/pytorch_fid` (`inception.InceptionV3`,
`fid_score.get_fid_score` and the functions under it) without torchvision.

    InceptionV3(output_blocks=(3,), resize_input=True, normalize_input=True, requires_grad=False, use_fid_inception=True,
                weights=None)
    get_activations / calculate_activation_statistics / compute_statistics_of_path / calculate_frechet_distance /
    calculate_fid_given_paths / get_fid_score          — the reference's signatures and defaults
    ActivationStatistics(dims)                         — streaming mean / covariance on the device (no (N, dims) array)
    frechet_distance_from_features(f1, f2)             — the exact low-rank route for fewer images than dimensions

The network is the FID variant of Inception-v3 (94 conv + BatchNorm + ReLU layers; the `branch_pool` averages exclude the
padding from their divisor, `Mixed_7c` pools with a max).  It is an `nn.Module` only to carry torchvision's
`Inception3(num_classes=1008, aux_logits=False)` state-dict keys; its forward is a sequence of launches of libsgam_hip.so on
NHWC fp32 buffers: `sgam_inception_preprocess_f32`, `sgam_conv2d_relu_nhwc_f32` (fp32-in MFMA, BatchNorm folded into weight
and bias once per weight version in fp64, every branch writing its channel slice of the block's concatenated output),
`sgam_pool3x3_nhwc_f32`, `sgam_global_avgpool_nhwc_f32`.  There is no CPU path and no gradient.

Weights are never downloaded.  `weights` is a state dict or the path of the FID checkpoint; with None the file
`pt_inception-2015-12-05-6726825d.pth` is looked for in torch.hub's checkpoint directory."""
import ctypes
import os
import pathlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import ConvDesc, SgamHipError, check
from ._opscore import _p, _stream, _workspace

FID_WEIGHTS_FILE = "pt_inception-2015-12-05-6726825d.pth"
IMAGE_EXTENSIONS = {"bmp", "jpg", "jpeg", "pgm", "png", "ppm", "tif", "tiff", "webp"}
BN_EPS = 1e-3
POOL_MAX_S2, POOL_MAX_S1, POOL_AVG = 0, 1, 2
MAX_FORWARD_BATCH = 64          # images per launch sequence: keeps every activation inside the kernels' 32-bit byte offsets


class _ConvBN(nn.Module):
    """parameter holder of one conv (bias=False) + BatchNorm(eps=1e-3) + ReLU under torchvision's `conv` / `bn` names"""

    def __init__(self, cin, cout, k=1, stride=1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride, padding, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=BN_EPS)


class _Branches(nn.Module):
    def __init__(self, **convs):
        super().__init__()
        for name, args in convs.items():
            setattr(self, name, _ConvBN(*args))


def _block_a(cin, pf):
    return _Branches(branch1x1=(cin, 64), branch5x5_1=(cin, 48), branch5x5_2=(48, 64, 5, 1, 2), branch3x3dbl_1=(cin, 64),
                     branch3x3dbl_2=(64, 96, 3, 1, 1), branch3x3dbl_3=(96, 96, 3, 1, 1), branch_pool=(cin, pf))


def _block_b(cin):
    return _Branches(branch3x3=(cin, 384, 3, 2), branch3x3dbl_1=(cin, 64), branch3x3dbl_2=(64, 96, 3, 1, 1),
                     branch3x3dbl_3=(96, 96, 3, 2))


def _block_c(cin, c7):
    return _Branches(branch1x1=(cin, 192), branch7x7_1=(cin, c7), branch7x7_2=(c7, c7, (1, 7), 1, (0, 3)),
                     branch7x7_3=(c7, 192, (7, 1), 1, (3, 0)), branch7x7dbl_1=(cin, c7), branch7x7dbl_2=(c7, c7, (7, 1), 1, (3, 0)),
                     branch7x7dbl_3=(c7, c7, (1, 7), 1, (0, 3)), branch7x7dbl_4=(c7, c7, (7, 1), 1, (3, 0)),
                     branch7x7dbl_5=(c7, 192, (1, 7), 1, (0, 3)), branch_pool=(cin, 192))


def _block_d(cin):
    return _Branches(branch3x3_1=(cin, 192), branch3x3_2=(192, 320, 3, 2), branch7x7x3_1=(cin, 192),
                     branch7x7x3_2=(192, 192, (1, 7), 1, (0, 3)), branch7x7x3_3=(192, 192, (7, 1), 1, (3, 0)),
                     branch7x7x3_4=(192, 192, 3, 2))


def _block_e(cin):
    return _Branches(branch1x1=(cin, 320), branch3x3_1=(cin, 384), branch3x3_2a=(384, 384, (1, 3), 1, (0, 1)),
                     branch3x3_2b=(384, 384, (3, 1), 1, (1, 0)), branch3x3dbl_1=(cin, 448), branch3x3dbl_2=(448, 384, 3, 1, 1),
                     branch3x3dbl_3a=(384, 384, (1, 3), 1, (0, 1)), branch3x3dbl_3b=(384, 384, (3, 1), 1, (1, 0)),
                     branch_pool=(cin, 192))


# block name -> (kind, output channels); in execution order
_BLOCKS = [("Mixed_5b", "A", 256), ("Mixed_5c", "A", 288), ("Mixed_5d", "A", 288), ("Mixed_6a", "B", 768),
           ("Mixed_6b", "C", 768), ("Mixed_6c", "C", 768), ("Mixed_6d", "C", 768), ("Mixed_6e", "C", 768),
           ("Mixed_7a", "D", 1280), ("Mixed_7b", "E", 2048), ("Mixed_7c", "E", 2048)]


def _default_weights_path():
    return os.path.join(torch.hub.get_dir(), "checkpoints", FID_WEIGHTS_FILE)


class _Folded:
    """one conv ready to launch: packed weight (cout, taps * cin_pad), folded bias, geometry"""
    __slots__ = ("w", "bias", "cin", "cin_pad", "cout", "kh", "kw", "stride", "ph", "pw")


class InceptionV3(nn.Module):
    """The FID InceptionV3 returning feature maps (the reference's class of the same name)"""

    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}

    def __init__(self, output_blocks=(DEFAULT_BLOCK_INDEX,), resize_input=True, normalize_input=True, requires_grad=False,
                 use_fid_inception=True, weights=None):
        super().__init__()
        if not use_fid_inception:
            raise NotImplementedError("InceptionV3(use_fid_inception=False): only the FID variant of the network is built")
        if requires_grad:
            raise NotImplementedError("InceptionV3(requires_grad=True): the HIP forward has no backward pass")
        self.resize_input = resize_input
        self.normalize_input = normalize_input
        self.output_blocks = sorted(output_blocks)
        self.last_needed_block = max(output_blocks)
        assert self.last_needed_block <= 3, "Last possible output block index is 3"
        # torchvision's Inception3(num_classes=1008, aux_logits=False) attribute order = its state_dict order
        self.Conv2d_1a_3x3 = _ConvBN(3, 32, 3, 2)
        self.Conv2d_2a_3x3 = _ConvBN(32, 32, 3)
        self.Conv2d_2b_3x3 = _ConvBN(32, 64, 3, 1, 1)
        self.Conv2d_3b_1x1 = _ConvBN(64, 80, 1)
        self.Conv2d_4a_3x3 = _ConvBN(80, 192, 3)
        self.Mixed_5b = _block_a(192, 32)
        self.Mixed_5c = _block_a(256, 64)
        self.Mixed_5d = _block_a(288, 64)
        self.Mixed_6a = _block_b(288)
        self.Mixed_6b = _block_c(768, 128)
        self.Mixed_6c = _block_c(768, 160)
        self.Mixed_6d = _block_c(768, 160)
        self.Mixed_6e = _block_c(768, 192)
        self.Mixed_7a = _block_d(768)
        self.Mixed_7b = _block_e(1280)
        self.Mixed_7c = _block_e(2048)
        self.fc = nn.Linear(2048, 1008)         # part of the checkpoint; no output block reads it
        for p in self.parameters():
            p.requires_grad = False
        self._folded = None
        if weights is None:
            weights = _default_weights_path()
            if not os.path.exists(weights):
                raise FileNotFoundError(
                    f"InceptionV3: the FID checkpoint {FID_WEIGHTS_FILE} is not at {weights} and is never downloaded; pass "
                    "weights=<state dict or path of that file> or place it there")
        if isinstance(weights, (str, os.PathLike)):
            weights = torch.load(os.fspath(weights), map_location="cpu")
        self.load_state_dict(weights)
        self.eval()

    # ---- weights -------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, *args, **kwargs):
        self._folded = None
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self._folded = None                 # .to(device) / .float(): fold again from where the parameters now live
        return super()._apply(fn, *args, **kwargs)

    def _fold(self):
        """conv.weight * gamma / sqrt(var + eps), beta - mean * gamma / sqrt(var + eps), formed in fp64, rounded to fp32 once and
        packed for the MFMA conv; Cin is padded to a multiple of 4 (the stem's 3 -> 4: the preprocessing writes a zero channel)"""
        lib = _lib.load()
        folded = {}
        for name, m in self.named_modules():
            if not isinstance(m, _ConvBN):
                continue
            w = m.conv.weight.detach()
            if not w.is_cuda:
                raise SgamHipError("InceptionV3 runs on the HIP backend only: move it to 'cuda' (there is no CPU fallback)")
            g = m.bn.weight.detach().double() / torch.sqrt(m.bn.running_var.detach().double() + m.bn.eps)
            w32 = (w.double() * g[:, None, None, None]).float().contiguous()
            f = _Folded()
            f.bias = (m.bn.bias.detach().double() - m.bn.running_mean.detach().double() * g).float().contiguous()
            f.cout, f.cin, f.kh, f.kw = w.shape
            f.cin_pad = (f.cin + 3) // 4 * 4
            f.stride = m.conv.stride[0]
            f.ph, f.pw = m.conv.padding
            f.w = torch.empty((f.cout, f.kh * f.kw * f.cin_pad), device=w.device, dtype=torch.float32)
            check(lib.sgam_pack_conv_weight(_p(w32), _p(f.w), f.cout, f.cin, f.kh, f.kw, f.cout, f.cin_pad, _stream()),
                  "sgam_pack_conv_weight")
            folded[name] = f
        self._folded = folded

    # ---- launches ------------------------------------------------------------------------------------------------------------
    def _conv(self, name, x, out=None, off=0):
        """x (B,H,W,C) dense -> conv + bias + ReLU; into out[..., off:off + cout] when `out` (a block's concatenated map) is given"""
        f = self._folded[name]
        B, Hi, Wi, C = x.shape
        if C != f.cin_pad:
            raise SgamHipError(f"InceptionV3.{name}: input of {C} channels, the layer takes {f.cin}")
        Ho = (Hi + 2 * f.ph - f.kh) // f.stride + 1
        Wo = (Wi + 2 * f.pw - f.kw) // f.stride + 1
        if Ho < 1 or Wo < 1:
            raise ValueError(f"InceptionV3.{name}: a {Hi} x {Wi} map is too small for its {f.kh} x {f.kw} kernel (images of at "
                             "least 75 x 75 reach the last block without resize_input)")
        if out is None:
            out = torch.empty((B, Ho, Wo, f.cout), device=x.device, dtype=torch.float32)
        assert out.shape[:3] == (B, Ho, Wo) and off + f.cout <= out.shape[3]
        d = ConvDesc(B=B, Hi=Hi, Wi=Wi, Cin=f.cin_pad, Ho=Ho, Wo=Wo, N=f.cout, KH=f.kh, KW=f.kw, stride=f.stride, pad_t=f.ph,
                     pad_l=f.pw, upsample2x=0, lda=C, ldb=f.w.shape[1], ldc=out.shape[3], ldr=0, n_valid=f.cout, bias_per_row=0)
        lib = _lib.load()
        nb = lib.sgam_conv2d_workspace_bytes(ctypes.byref(d))
        ws = _workspace(nb, "sgam_conv2d_relu_nhwc_f32", x.device, d)
        check(lib.sgam_conv2d_relu_nhwc_f32(ctypes.byref(d), _p(x), _p(f.w), _p(f.bias), ctypes.c_void_p(out.data_ptr() + 4 * off),
                                            _p(ws), nb, _stream()), "sgam_conv2d_relu_nhwc_f32")
        return out

    def _chain(self, block, names, x, out=None, off=0):
        """the convs `names` of `block` (None: the stem, whose layers have no prefix) one after the other; the last one into `out`"""
        pre = f"{block}." if block else ""
        for n in names[:-1]:
            x = self._conv(pre + n, x)
        return self._conv(pre + names[-1], x, out, off)

    def _block(self, name, kind, cout, x):
        B, H, W, C = x.shape
        if kind in ("B", "D"):
            Ho, Wo = pool3x3_out_size(H, W, POOL_MAX_S2)
        else:
            Ho, Wo = H, W
        out = torch.empty((B, Ho, Wo, cout), device=x.device, dtype=torch.float32)
        run = lambda names, off, src=x: self._chain(name, names, src, out, off)         # noqa: E731
        if kind == "A":
            run(["branch1x1"], 0)
            run(["branch5x5_1", "branch5x5_2"], 64)
            run(["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], 128)
            run(["branch_pool"], 224, pool3x3(x, POOL_AVG))
        elif kind == "B":
            run(["branch3x3"], 0)
            run(["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], 384)
            pool3x3(x, POOL_MAX_S2, out, 480)
        elif kind == "C":
            run(["branch1x1"], 0)
            run(["branch7x7_1", "branch7x7_2", "branch7x7_3"], 192)
            run([f"branch7x7dbl_{i}" for i in range(1, 6)], 384)
            run(["branch_pool"], 576, pool3x3(x, POOL_AVG))
        elif kind == "D":
            run(["branch3x3_1", "branch3x3_2"], 0)
            run([f"branch7x7x3_{i}" for i in range(1, 5)], 320)
            pool3x3(x, POOL_MAX_S2, out, 512)
        else:
            run(["branch1x1"], 0)
            b3 = self._conv(f"{name}.branch3x3_1", x)
            run(["branch3x3_2a"], 320, b3)
            run(["branch3x3_2b"], 704, b3)
            bd = self._chain(name, ["branch3x3dbl_1", "branch3x3dbl_2"], x)
            run(["branch3x3dbl_3a"], 1088, bd)
            run(["branch3x3dbl_3b"], 1472, bd)
            run(["branch_pool"], 1856, pool3x3(x, POOL_MAX_S1 if name == "Mixed_7c" else POOL_AVG))
        return out

    def forward_nhwc(self, frames, last_block=None):
        """frames: (B,H,W,3) uint8, or (B,H,W,3) fp32 in [0,1], on the device -> {block index: NHWC fp32 output} for the
        blocks up to `last_block` (default: the last one asked for at construction); block 3 is the (B,1,1,2048) average"""
        if not (isinstance(frames, torch.Tensor) and frames.is_cuda):
            raise SgamHipError("InceptionV3 runs on the HIP backend only: the input must be a tensor on the GPU")
        if frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"InceptionV3: frames of shape (B,H,W,3), uint8 or fp32, not {tuple(frames.shape)} {frames.dtype}")
        if self._folded is None:
            self._fold()
        last = self.last_needed_block if last_block is None else last_block
        x = preprocess(frames, self.resize_input, self.normalize_input)
        outs = {}
        x = self._chain(None, ["Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"], x)
        x = outs[0] = pool3x3(x, POOL_MAX_S2)
        if last >= 1:
            x = self._chain(None, ["Conv2d_3b_1x1", "Conv2d_4a_3x3"], x)
            x = outs[1] = pool3x3(x, POOL_MAX_S2)
        for i, (name, kind, cout) in enumerate(_BLOCKS):
            if last < (2 if i < 8 else 3):
                break
            x = self._block(name, kind, cout, x)
            if i == 7:
                outs[2] = x
        if last >= 3:
            outs[3] = global_avgpool(x).reshape(x.shape[0], 1, 1, x.shape[3])
        return outs

    def forward(self, inp):
        """inp: Bx3xHxW in (0, 1) on the device (the reference's contract) -> list of the selected block outputs, ascending,
        as NCHW views of the NHWC buffers.  (B,H,W,3) uint8 frames are taken as they are."""
        if inp.dtype != torch.uint8:
            if inp.dim() != 4 or inp.shape[1] != 3:
                raise ValueError(f"InceptionV3: input of shape Bx3xHxW expected, not {tuple(inp.shape)}")
            from .ops_aux import nchw_to_nhwc
            if not inp.is_cuda:
                raise SgamHipError("InceptionV3 runs on the HIP backend only: the input must be a tensor on the GPU")
            inp = nchw_to_nhwc(inp)
        outs = self.forward_nhwc(inp)
        return [outs[i].permute(0, 3, 1, 2) for i in self.output_blocks]

    def features(self, frames, dims=2048):
        """(B,H,W,3) device frames -> (B, dims) fp32 on the device: the block of `dims` channels, averaged over its map"""
        block = self.BLOCK_INDEX_BY_DIM[dims]
        out = []
        for i in range(0, frames.shape[0], MAX_FORWARD_BATCH):
            y = self.forward_nhwc(frames[i:i + MAX_FORWARD_BATCH].contiguous(), block)[block]
            out.append(y.reshape(y.shape[0], dims) if block == 3 else global_avgpool(y))
        return out[0] if len(out) == 1 else torch.cat(out)


# ---- kernel wrappers ----------------------------------------------------------------------------------------------------------
def preprocess(frames, resize_input=True, normalize_input=True):
    """(B,H,W,3) uint8 or fp32 in [0,1] -> (B,299,299,4) fp32 (input size without resize_input), channel 3 zero"""
    B, H, W, _ = frames.shape
    frames = frames.contiguous()
    Ho, Wo = (299, 299) if resize_input else (H, W)
    out = torch.empty((B, Ho, Wo, 4), device=frames.device, dtype=torch.float32)
    check(_lib.load().sgam_inception_preprocess_f32(_p(frames), int(frames.dtype == torch.uint8), B, H, W, _p(out), Ho, Wo,
                                                    int(bool(normalize_input)), _stream()), "sgam_inception_preprocess_f32")
    return out


def pool3x3_out_size(H, W, mode):
    ho, wo = ctypes.c_int32(), ctypes.c_int32()
    rc = _lib.load().sgam_pool3x3_out_size(H, W, mode, ctypes.byref(ho), ctypes.byref(wo))
    if rc != 0:
        raise ValueError(f"3 x 3 pool (mode {mode}): a {H} x {W} map is too small")
    return ho.value, wo.value


def pool3x3(x, mode, out=None, off=0):
    """x (B,H,W,C) NHWC fp32 -> the pooled map; into out[..., off:off + C] when `out` is given"""
    B, H, W, C = x.shape
    Ho, Wo = pool3x3_out_size(H, W, mode)
    if out is None:
        out = torch.empty((B, Ho, Wo, C), device=x.device, dtype=torch.float32)
    assert out.shape[:3] == (B, Ho, Wo) and off + C <= out.shape[3]
    x = x.contiguous()
    check(_lib.load().sgam_pool3x3_nhwc_f32(_p(x), B, H, W, C, C, ctypes.c_void_p(out.data_ptr() + 4 * off),
                                            out.shape[3], mode, _stream()), "sgam_pool3x3_nhwc_f32")
    return out


def global_avgpool(x):
    """(B,H,W,C) dense NHWC fp32 -> (B,C): fp64 accumulation, one rounding"""
    B, H, W, C = x.shape
    out = torch.empty((B, C), device=x.device, dtype=torch.float32)
    check(_lib.load().sgam_global_avgpool_nhwc_f32(_p(x), B, H * W, C, C, _p(out), _stream()), "sgam_global_avgpool_nhwc_f32")
    return out


class ActivationStatistics:
    """Streaming mean and covariance (np.mean / np.cov with the N - 1 divisor) of feature batches, accumulated in fp64 on
    the device by sgam_activation_stats_update_f64: no (N, dims) array has to exist."""

    def __init__(self, dims, device="cuda"):
        n = _lib.load().sgam_activation_stats_state_doubles(dims)
        if n < 0:
            raise ValueError(f"ActivationStatistics: dims {dims} out of range")
        self.dims, self.count = int(dims), 0
        self.state = torch.empty((n,), device=device, dtype=torch.float64)

    def update(self, features):
        if not (isinstance(features, torch.Tensor) and features.is_cuda):
            raise SgamHipError("ActivationStatistics.update: features must be a tensor on the GPU (there is no CPU fallback)")
        if features.dim() != 2 or features.shape[1] != self.dims:
            raise ValueError(f"ActivationStatistics.update: (n, {self.dims}) features expected, not {tuple(features.shape)}")
        f = features.float().contiguous()
        if f.shape[0] == 0:
            return self
        check(_lib.load().sgam_activation_stats_update_f64(_p(f), f.shape[0], self.dims, self.dims, _p(self.state),
                                                           int(self.count == 0), _stream()), "sgam_activation_stats_update_f64")
        self.count += int(f.shape[0])
        return self

    def finalize(self):
        """-> (mu (dims,), sigma (dims, dims)) float64 numpy arrays"""
        if self.count < 1:
            raise ValueError("ActivationStatistics.finalize: no features were added")
        mu = torch.empty((self.dims,), device=self.state.device, dtype=torch.float64)
        sigma = torch.empty((self.dims, self.dims), device=self.state.device, dtype=torch.float64)
        check(_lib.load().sgam_activation_stats_finalize_f64(_p(self.state), self.dims, _p(mu), _p(sigma), _stream()),
              "sgam_activation_stats_finalize_f64")
        return mu.cpu().numpy(), sigma.cpu().numpy()

    def save(self, path):
        mu, sigma = self.finalize()
        np.savez(path, mu=mu, sigma=sigma)
        return path


# ---- the reference's fid_score surface ----------------------------------------------------------------------------------------
def _load_batch(files, workers, device):
    """decode with PIL on host threads into one pinned uint8 staging buffer, upload once"""
    from PIL import Image

    def decode(path):
        with Image.open(path) as im:
            return np.array(im.convert("RGB"))
    with ThreadPoolExecutor(max(1, int(workers or 1))) as pool:
        imgs = list(pool.map(decode, files))
    shape = imgs[0].shape
    for f, im in zip(files, imgs):
        if im.shape != shape:
            raise ValueError(f"images of one call must share a size: {files[0]} is {shape[1]} x {shape[0]}, {f} is "
                             f"{im.shape[1]} x {im.shape[0]}")
    stage = torch.empty((len(imgs),) + shape, dtype=torch.uint8, pin_memory=True)
    for i, im in enumerate(imgs):
        stage[i] = torch.from_numpy(im)
    return stage.to(device, non_blocking=True)


def _feature_batches(files, model, batch_size, dims, device, num_workers):
    """yield (n, dims) fp32 device features, batch by batch; `files` is a list of paths or a (N,H,W,3) tensor of frames"""
    model.eval()
    n = len(files)
    if n == 0:
        raise ValueError("get_activations: no images")
    if batch_size > n:
        print("Warning: batch size is bigger than the data size. Setting batch size to data size")
        batch_size = n
    for i in range(0, n, batch_size):
        if isinstance(files, torch.Tensor):
            frames = files[i:i + batch_size].to(device)
        else:
            frames = _load_batch([os.fspath(f) for f in files[i:i + batch_size]], num_workers, device)
        yield model.features(frames, dims)


def get_activations(files, model, batch_size=50, dims=2048, device="cuda", num_workers=1):
    """-> (N, dims) float64 array of pooled Inception features; `files`: image paths, or a (N,H,W,3) uint8 / fp32 tensor"""
    pred = np.empty((len(files), dims))
    start = 0
    for f in _feature_batches(files, model, batch_size, dims, device, num_workers):
        pred[start:start + f.shape[0]] = f.cpu().numpy()
        start += f.shape[0]
    return pred


def calculate_activation_statistics(files, model, batch_size=50, dims=2048, device="cuda", num_workers=1):
    """-> mu (dims,), sigma (dims, dims): mean and covariance of the features, accumulated on the device"""
    stats = ActivationStatistics(dims, device)
    for f in _feature_batches(files, model, batch_size, dims, device, num_workers):
        stats.update(f)
    return stats.finalize()


def _image_files(path):
    path = pathlib.Path(path)
    return sorted(f for ext in IMAGE_EXTENSIONS for f in path.glob(f"*.{ext}"))


def compute_statistics_of_path(path, model, batch_size, dims, device, num_workers=1):
    path = os.fspath(path)
    if path.endswith(".npz"):
        with np.load(path) as f:
            return f["mu"][:], f["sigma"][:]
    return calculate_activation_statistics(_image_files(path), model, batch_size, dims, device, num_workers)


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """d^2 = |mu1 - mu2|^2 + tr(sigma1 + sigma2 - 2 sqrt(sigma1 sigma2)) on the host with scipy's sqrtm, step for step as the
    reference: a non-finite root of the (singular) product is retried with eps added to both diagonals, and a complex root
    is accepted when its diagonal's imaginary part is within 1e-3 of zero."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    if mu1.shape != mu2.shape:
        raise AssertionError("Training and test mean vectors have different lengths")
    if sigma1.shape != sigma2.shape:
        raise AssertionError("Training and test covariances have different dimensions")
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        print(f"fid calculation produces singular product; adding {eps} to diagonal of cov estimates")
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)


def frechet_distance_from_features(f1, f2):
    """The same distance from the two feature sets (N1, d), (N2, d) themselves.  With A_i = (f_i - mean) / sqrt(N_i - 1),
    sigma_i = A_i^T A_i, and the non-zero eigenvalues of sigma1 sigma2 are the squared singular values of A2 A1^T, so
    tr sqrt(sigma1 sigma2) = sum of the singular values of that N2 x N1 matrix: exact for any rank, no d x d square root and
    no eps retry.  fp64 on the host (a small SVD, not a hot path)."""
    f1 = f1.detach().cpu().numpy() if isinstance(f1, torch.Tensor) else f1
    f2 = f2.detach().cpu().numpy() if isinstance(f2, torch.Tensor) else f2
    f1, f2 = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    if f1.ndim != 2 or f2.ndim != 2 or f1.shape[1] != f2.shape[1] or f1.shape[0] < 2 or f2.shape[0] < 2:
        raise ValueError(f"frechet_distance_from_features: (N1, d) and (N2, d) with N >= 2, not {f1.shape} and {f2.shape}")
    m1, m2 = f1.mean(axis=0), f2.mean(axis=0)
    a1 = (f1 - m1) / np.sqrt(f1.shape[0] - 1)
    a2 = (f2 - m2) / np.sqrt(f2.shape[0] - 1)
    diff = m1 - m2
    sv = np.linalg.svd(a2 @ a1.T, compute_uv=False)
    return float(diff @ diff + (a1 * a1).sum() + (a2 * a2).sum() - 2.0 * sv.sum())


def calculate_fid_given_paths(generated_path, gt_path, batch_size, device, dims, num_workers=1, model=None):
    """FID of two paths (image directories or .npz statistics); `model`: an InceptionV3 to use instead of the checkpoint's"""
    for p in (generated_path, gt_path):
        if not os.path.exists(p):
            raise RuntimeError(f"Invalid path: {p}")
    if model is None:
        model = InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[dims]]).to(device)
    m1, s1 = compute_statistics_of_path(generated_path, model, batch_size, dims, device, num_workers)
    m2, s2 = compute_statistics_of_path(gt_path, model, batch_size, dims, device, num_workers)
    return calculate_frechet_distance(m1, s1, m2, s2)


def get_fid_score(generated_path, gt_path, batch_size=64, num_workers=0, device="cuda:0", dims=2048, model=None):
    device = torch.device("cuda" if device is None else device)
    if num_workers is None:
        num_workers = min(len(os.sched_getaffinity(0)), 8)
    return calculate_fid_given_paths(generated_path, gt_path, batch_size, device, dims, num_workers, model=model)


# ---- scene level ---------------------------------------------------------------------------------------------------------------
LOWRANK_MAX_PRODUCT = 1 << 22       # "auto": the low-rank route while the N2 x N1 matrix stays small (2048 x 2048)


def _side(s):
    """one side of a comparison as given -> a (N,H,W,3) tensor of frames, a sorted list of image files, or the path (str) of a
    .npz of saved statistics"""
    if isinstance(s, torch.Tensor):
        return s
    s = os.fspath(s)
    return s if s.endswith(".npz") else _image_files(s)


def _side_features(s, model, batch_size, dims, device, num_workers):
    """frames or image files (a `_side` that is not saved statistics) -> (N, dims) fp32 features on the device"""
    return torch.cat(list(_feature_batches(s, model, batch_size, dims, device, num_workers)))


def fid_between(a, b, model, dims=2048, method="auto", batch_size=50, device="cuda", num_workers=1):
    """Fréchet distance between two sides, each a (N,H,W,3) tensor of frames, a directory of images or a .npz of statistics.
    method "lowrank" needs two feature sets; "sqrtm" is the reference's route; "auto" takes the low-rank route when both
    sides are feature sets with N1 * N2 <= LOWRANK_MAX_PRODUCT."""
    if method not in ("auto", "lowrank", "sqrtm"):
        raise ValueError(f"fid: method 'auto', 'lowrank' or 'sqrtm', not {method!r}")

    a, b = _side(a), _side(b)
    is_set = [not isinstance(s, str) for s in (a, b)]
    if method == "lowrank" and not all(is_set):
        raise ValueError("fid: method='lowrank' needs the features of both sides; a .npz holds only statistics")
    if all(is_set) and (method == "lowrank" or (method == "auto" and len(a) * len(b) <= LOWRANK_MAX_PRODUCT)):
        fa = _side_features(a, model, batch_size, dims, device, num_workers)
        fb = _side_features(b, model, batch_size, dims, device, num_workers)
        return frechet_distance_from_features(fa, fb)
    stats = []
    for s in (a, b):
        if isinstance(s, str):
            stats.append(compute_statistics_of_path(s, model, batch_size, dims, device, num_workers))
        else:
            stats.append(calculate_activation_statistics(s, model, batch_size, dims, device, num_workers))
    return float(calculate_frechet_distance(*stats[0], *stats[1]))
