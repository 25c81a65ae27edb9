"""Encoder / Decoder of the conditional VQGAN on the HIP backend.

Same constructor kwargs, attribute names and ``state_dict`` keys as the reference's
``sgam/generative_sensing_module/modules/diffusionmodules/model.py`` (Encoder :342-433, Decoder
:437-539, ResnetBlock :78-137, AttnBlock :140-192, Upsample :38-53, Downsample :56-75, Normalize
:34-35), so checkpoints and callers drop in unchanged — but no layer ever runs a torch op: the
``nn.Conv2d`` / ``nn.GroupNorm`` objects are parameter containers only, and every ``forward`` is a
sequence of calls into libsgam_hip.so (MFMA implicit-GEMM convolutions, GroupNorm+swish, softmax).

Activations stay NHWC between layers (``forward_nhwc``); the public ``forward`` of each module takes
and returns NCHW like the reference and pays one layout hop on each side.
"""
import numpy as np
import os

import torch
import torch.nn as nn

from .... import ops


class Conv2d(nn.Conv2d):
    """nn.Conv2d as a parameter container + HIP execution.  Packed weights ([Cout_pad][taps][Cin_pad],
    K contiguous — the B operand layout of the implicit GEMM) are cached per (storage, version)."""

    @staticmethod
    def pack_key(dtype):
        """the weight form `dtype` activations multiply with: on the split path fp32 weights pre-split into fp16 hi/lo planes"""
        return "f32x" if dtype == torch.float32 and ops.F32_MODE == "split" else dtype

    def _packed(self, dtype=torch.float32):
        w = self.weight
        key = (w.data_ptr(), w._version, str(w.device))
        if getattr(self, "_pack_key", None) != key:
            self._packs = {}
            self._pack_bias = None if self.bias is None else self.bias.detach().float().contiguous()
            self._pack_key = key
        dtype = self.pack_key(dtype)
        if dtype not in self._packs:
            self._packs[dtype] = ops.pack_conv_weight(w, dtype=dtype)
            if dtype in ops.H16 and self.kernel_size == (3, 3) and self.stride == (1, 1):
                # the 16-bit halo kernel reads a fragment-ordered copy (packed on first use, csrc/h16_halo.hip)
                self._packs[dtype]._sgam_frag_src = w
        return self._packs[dtype], self._pack_bias

    def forward_nhwc(self, x, residual=None, upsample2x=False, pad=None, gn=None, out_dtype=None, norm=None):
        """gn = (scale/shift table from GroupNorm.stats_nhwc, swish flag): GroupNorm(+swish) of the input fused
        into the operand staging of the implicit GEMM (fp32 path only).  The kernel family follows x.dtype:
        fp32 -> fp32-in MFMA parity path, bf16/fp16 -> 16-bit MFMA throughput path."""
        wp, b = self._packed(x.dtype)
        kh, kw = self.kernel_size
        if pad is None:
            pad = (self.padding[0], self.padding[1], self.padding[0], self.padding[1])  # t, l, b, r
        return ops.conv2d_nhwc(x, wp, b, cout=self.out_channels, kh=kh, kw=kw, stride=self.stride[0],
                               pad_t=pad[0], pad_l=pad[1], pad_b=pad[2], pad_r=pad[3], upsample2x=upsample2x,
                               residual=residual, cin=wp.shape[1] // (kh * kw), gn=gn, out_dtype=out_dtype, norm=norm)

    def forward(self, x):
        cin_pad = self._packed()[0].shape[1] // (self.kernel_size[0] * self.kernel_size[1])
        return ops.nhwc_to_nchw(self.forward_nhwc(ops.nchw_to_nhwc(x, c_pad=cin_pad)))


class GroupNorm(nn.GroupNorm):
    def stats_nhwc(self, x):
        """(B,C,2) scale/shift table for the fused conv prologue."""
        return ops.groupnorm_stats(x, self.weight.detach(), self.bias.detach(), groups=self.num_groups, eps=self.eps)

    def forward_nhwc(self, x, swish=False):
        return ops.groupnorm_nhwc(x, self.weight.detach(), self.bias.detach(), swish, groups=self.num_groups,
                                  eps=self.eps)

    def forward(self, x):
        return ops.nhwc_to_nchw(self.forward_nhwc(ops.nchw_to_nhwc(x)))


# Measured on MI355X (profiles/): with fp32-in MFMA the convolution is matrix-pipe bound and the
# per-tap re-normalisation of the fused prologue (9x the swish work, on the same wavefronts that feed the MFMAs)
# costs more (+19 us on the 128->128 @256^2 layer) than the stand-alone HBM-bound normalise pass it removes
# (~12 us).  The fused kernel stays available (and parity-tested) behind this switch.
FUSE_GROUPNORM_INTO_CONV = False
# AttnBlock on the split-fp32 path: normalise inside the q | k | v GEMM (measured)
FUSE_NORM_INTO_QKV = os.environ.get("SGAM_FUSE_NORM_QKV", "1") != "0"


def _norm_conv(norm, swish, conv, x, **kw):
    """GroupNorm(+swish) followed by a convolution."""
    if FUSE_GROUPNORM_INTO_CONV:
        return conv.forward_nhwc(x, gn=(norm.stats_nhwc(x), swish), **kw)
    if (x.dtype == torch.float32 and ops.F32_MODE == "split") or x.dtype in ops.H16:
        # ops decides per launch: normalise inside the halo-staged 3x3 kernel where that kernel runs, else a separate pass
        return conv.forward_nhwc(x, norm=(norm.weight.detach(), norm.bias.detach(), swish, norm.num_groups, norm.eps), **kw)
    return conv.forward_nhwc(norm.forward_nhwc(x, swish=swish), **kw)


def Normalize(in_channels):
    return GroupNorm(num_groups=32, num_channels=in_channels, eps=1e-6, affine=True)


def nonlinearity(x):
    """swish; standalone NCHW use only — inside the network swish is fused into the GroupNorm kernel."""
    raise ops.SgamHipError("nonlinearity() is fused into GroupNorm on the HIP backend (GroupNorm.forward_nhwc(swish=True))")


class _NHWCModule(nn.Module):
    def forward(self, x, *unused):
        return ops.nhwc_to_nchw(self.forward_nhwc(ops.nchw_to_nhwc(x)))


class Upsample(_NHWCModule):
    def __init__(self, in_channels, with_conv):
        super().__init__()
        self.with_conv = with_conv
        if not with_conv:
            raise NotImplementedError("Upsample(with_conv=False) is not on the SGAM hot path")
        self.conv = Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1)

    def forward_nhwc(self, x):
        # nearest 2x folded into the conv's gather (K6 + K1)
        return self.conv.forward_nhwc(x, upsample2x=True)


class Downsample(_NHWCModule):
    def __init__(self, in_channels, with_conv):
        super().__init__()
        self.with_conv = with_conv
        if not with_conv:
            raise NotImplementedError("Downsample(with_conv=False) is not on the SGAM hot path")
        self.conv = Conv2d(in_channels, in_channels, kernel_size=3, stride=2, padding=0)

    def forward_nhwc(self, x):
        # F.pad(x, (0,1,0,1)) + stride-2 conv: zero padding on the right/bottom only (K2)
        return self.conv.forward_nhwc(x, pad=(0, 0, 1, 1))


class ResnetBlock(_NHWCModule):
    def __init__(self, *, in_channels, out_channels=None, conv_shortcut=False, dropout=0.0, temb_channels=512):
        super().__init__()
        out_channels = in_channels if out_channels is None else out_channels
        self.in_channels, self.out_channels = in_channels, out_channels
        self.use_conv_shortcut = conv_shortcut
        self.norm1 = Normalize(in_channels)
        self.conv1 = Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
        if temb_channels > 0:
            self.temb_proj = nn.Linear(temb_channels, out_channels)  # never used: temb is None on this path
        self.norm2 = Normalize(out_channels)
        self.dropout = nn.Dropout(dropout)  # p = 0 in every SGAM config; identity at inference
        self.conv2 = Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1)
        if in_channels != out_channels:
            if conv_shortcut:
                self.conv_shortcut = Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
            else:
                self.nin_shortcut = Conv2d(in_channels, out_channels, kernel_size=1, stride=1, padding=0)

    def forward_nhwc(self, x):
        h = _norm_conv(self.norm1, True, self.conv1, x)
        if self.in_channels != self.out_channels:
            x = (self.conv_shortcut if self.use_conv_shortcut else self.nin_shortcut).forward_nhwc(x)
        return _norm_conv(self.norm2, True, self.conv2, h, residual=x)  # x + h in the conv epilogue

    def forward(self, x, temb=None):
        if temb is not None:
            raise NotImplementedError("timestep embeddings are not used by SGAM's VQGAN")
        return super().forward(x)


BLOCKDIAG_MAX_ROWS = 4096      # B * n up to which a batch of small attention blocks runs as one block-diagonal chain (64 MB of scores)


class AttnBlock(_NHWCModule):
    """Single-head spatial self-attention (reference :168-192) as MFMA GEMMs + a row softmax:
    [q|k|v] = GN(x) Wqkv^T (GroupNorm fused into the operand staging), S = q k^T, P = softmax(S c^-1/2),
    O = P v (v transposed once so that the key axis is contiguous), out = x + O Wp^T."""

    def __init__(self, in_channels):
        super().__init__()
        self.in_channels = in_channels
        self.norm = Normalize(in_channels)
        self.q = Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.k = Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.v = Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.proj_out = Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)

    def _packed_qkv(self):
        ws = (self.q.weight, self.k.weight, self.v.weight)
        key = tuple((w.data_ptr(), w._version) for w in ws) + (str(ws[0].device),)
        if getattr(self, "_qkv_key", None) != key:
            c = self.in_channels
            self._wqkv = {torch.float32: torch.cat([m.weight.detach().reshape(c, c) for m in (self.q, self.k, self.v)],
                                                   0).float().contiguous()}
            self._bqkv = torch.cat([m.bias.detach() for m in (self.q, self.k, self.v)]).float().contiguous()
            self._qkv_key = key
        return self._wqkv, self._bqkv

    ROUTES = ("block", "block_front", "flash_proj", "flash", "small", "blockdiag") + tuple(
        f"image_{a}{f}" for f in ("", ".norm", ".table") for a in ("flash_proj", "flash", "chain"))

    def route(self, dtype, B, H, W, has_stats):
        """The launch sequence (one of ROUTES; tabulated in DESIGN.md, "Which sequence a block takes") of a (B, H, W, C) input of
        `dtype`, from shapes and switches alone: host-side library queries, no GPU.  `has_stats`: the input carries its producer's
        chunk statistics (ops.gn_stats).  block / block_front: the fused front end + flash (+ the merge inside proj_out); flash_proj /
        flash / small / blockdiag: one q | k | v GEMM for the batch, then that attention; image_*: that attention one image at a
        time, the suffix naming the q | k | v front ("" GroupNorm inside one batched GEMM, ".norm" a normalise pass + a GEMM per
        image, ".table" the {scale, shift} prologue of the fp32-in MFMA GEMM)."""
        C, n = self.in_channels, H * W
        flash = ops.attention_fusable(n, C)
        one_chain = B > 1 and B * n <= BLOCKDIAG_MAX_ROWS and n % 4 == 0
        if dtype in ops.H16:
            if flash and has_stats and ops.ATTN_BLOCK_H16 and ops.attn_block_h16_fits(n, C, B):
                return "block" if ops.ATTN_BLOCK_H16_PROJ else "block_front"
            if ops.attention_small_fits(n, C, B):
                return "small"
            if B > 1 and (flash or one_chain):
                return "flash" if flash else "blockdiag"
            return "image_flash.norm" if flash else "image_chain.norm"
        split = ops.F32_MODE == "split"
        if split and not FUSE_GROUPNORM_INTO_CONV and FUSE_NORM_INTO_QKV and ops.gemm_gn_fits(B * n, 3 * C, C, n):
            if flash and ops.ATTN_BLOCK_F32X and ops.ATTN_PROJ:
                return "block"
            if B > 1 and flash:
                return "flash_proj" if ops.ATTN_PROJ else "flash"
            if ops.attention_small_fits(n, C, B):
                return "small"
            if one_chain:
                return "blockdiag"
            front = ""
        else:
            front = ".table" if FUSE_GROUPNORM_INTO_CONV else ".norm"
        if split and flash:
            return ("image_flash_proj" if ops.ATTN_PROJ else "image_flash") + front
        return "image_chain" + front

    def forward_nhwc(self, x):
        B, H, W, C = x.shape
        route, _, front = self.route(x.dtype, B, H, W, ops.gn_stats(x) is not None).partition(".")
        wqkvs, bqkv = self._packed_qkv()
        wp, bp = self.proj_out._packed(x.dtype)
        wkey = x.dtype if front == "table" else Conv2d.pack_key(x.dtype)      # (the table front multiplies on the fp32-in MFMA)
        if wkey not in wqkvs:
            w32 = wqkvs[torch.float32]
            wqkvs[wkey] = ops.split_rows(w32, ops._pow2_scale(float(w32.abs().max()))) if wkey == "f32x" else ops.cast(w32, x.dtype)
        wqkv, scale = wqkvs[wkey], int(C) ** (-0.5)
        if route in ("block", "block_front"):
            if x.dtype in ops.H16:
                return self._block_h16(x, bqkv, scale, route == "block")
            return self._block_f32x(x, wqkv, bqkv, wp, bp, scale)
        if route.startswith("image_"):
            return self._per_image(x, route[len("image_"):], front, wqkv, bqkv, wp, bp, scale)
        # a batch (lock-stepped scenes, warp candidates) is ONE launch sequence: the images are stacked along the rows of the
        # q | k | v projection and the attention keeps every query inside its image
        qkv = self._qkv(x, wqkv, bqkv)
        if route == "flash_proj":
            return ops.view_nhwc(ops.attention_proj(qkv, C, scale, wp, bp, x.reshape(B * H * W, C), B=B), B, H, W)
        # ... and proj_out runs as the 1x1 convolution it is (per-image GroupNorm statistics of the block output from its epilogue)
        return self.proj_out.forward_nhwc(self._attend(route, qkv, C, scale, B).view(B, H, W, C), residual=x)

    def _qkv(self, x, wqkv, bqkv):
        """q | k | v of the whole batch, (B n, 3C): GroupNorm applied while the GEMM stages its operand on the split-fp32 path
        (csrc/gemm_gn_f32x.hip: no normalise pass), a normalise pass and the generic GEMM in 16 bits"""
        B, H, W, C = x.shape
        if x.dtype in ops.H16:
            return ops.gemm_nt(self.norm.forward_nhwc(x, swish=False).reshape(B * H * W, C), wqkv, bias=bqkv)
        mr = ops.groupnorm_meanrstd(x, self.norm.eps)
        return ops.gemm_gn_f32x(x.reshape(B * H * W, C), mr, self.norm.weight.detach(), self.norm.bias.detach(), wqkv, bqkv, H * W)

    @staticmethod
    def _attend(kind, qkv, C, scale, B=1):
        """softmax(q k^T scale) v of B images stacked along the rows of qkv (B n, 3C) -> (B n, C).  'flash': one pass over the keys, no
        (n, n) scores; 'small': the 16 x 16 maps in one launch; 'chain' (B = 1) / 'blockdiag': v^T, score GEMM, row soft-max — over
        the columns of a row's own image only: 8 x the score FLOPs of B separate chains at B = 8, against 5 launches per IMAGE —
        and P v; scores and soft-max in fp32, q / k / v and P in the dtype of qkv"""
        if kind == "flash":
            return ops.attention(qkv, C, scale, B=B)
        if kind == "small":
            return ops.attention_small(qkv, C, scale, B=B)
        rows = qkv.shape[0]
        block = rows // B if kind == "blockdiag" else 0
        if qkv.dtype in ops.H16:
            vt = ops.transpose_h16(qkv[:, 2 * C:])                                        # (C, rows) = v^T
            s = ops.gemm_nt(qkv[:, :C], qkv[:, C:2 * C], out_dtype=torch.float32)
            return ops.gemm_nt(ops.softmax_rows_h16(s, scale, qkv.dtype, block=block), vt)
        vt = ops.nhwc_to_nchw(qkv[:, 2 * C:].unsqueeze(0).unsqueeze(0), c=C).view(C, rows)
        s = ops.gemm_nt(qkv[:, :C], qkv[:, C:2 * C])
        ops.softmax_rows_(s, scale, block=block)
        return ops.gemm_nt(s, vt, a_scale=1024.0)                                         # probabilities lifted before the split

    def _per_image(self, x, attend, front, wqkv, bqkv, wp, bp, scale):
        B, H, W, C = x.shape
        n = H * W
        if front == "":
            qkv_all = self._qkv(x, wqkv, bqkv)
        elif front == "table":
            table, h = self.norm.stats_nhwc(x), x                         # (B, C, 2), no swish for attention
        else:
            table, h = None, self.norm.forward_nhwc(x, swish=False)
        out = torch.empty_like(x)
        for b in range(B):
            xb, ob = x[b].reshape(n, C), out[b].reshape(n, C)
            qkv = qkv_all[b * n:(b + 1) * n] if front == "" else ops.gemm_nt(
                h[b].reshape(n, C), wqkv, bias=bqkv, gn=None if table is None else (table[b:b + 1], False))   # (n, 3C)
            if attend == "flash_proj":
                # one pass over the keys AND proj_out + residual: the merge of the key ranges is the projection's operand staging
                ob = ops.attention_proj(qkv, C, scale, wp, bp, xb, out=ob)
            else:
                ob = ops.gemm_nt(self._attend(attend, qkv, C, scale), wp, bias=bp, residual=xb, out=ob)
            if B == 1:
                # statistics of the block output for the next GroupNorm.  They describe ONE image's rows, and `out` is that image
                # only at B = 1: a per-image loop over a batch leaves none
                ops.carry_gn_stats(out, ob)
        return out

    def _block_f32x(self, x, wqkv, bqkv, wp, bp, scale):
        """three launches: GroupNorm + q | k | v with K / V^T written straight in the attention's fragment order (the GEMM + split
        launch's arithmetic, equal to fp32 round-off), one pass over the keys, merge + proj_out + residual (csrc/attention.hip)"""
        B, H, W, C = x.shape
        wqkvs = self._wqkv
        if "f32x_perm" not in wqkvs:
            wqkvs["f32x_perm"] = ops.split_rows(ops.permute_rows_for_transposed_product(wqkvs[torch.float32]), wqkv.scale)
        mr = ops.groupnorm_meanrstd(x, self.norm.eps)
        ob = ops.attn_block_f32x(x.reshape(B * H * W, C), mr, self.norm.weight.detach(), self.norm.bias.detach(), wqkvs["f32x_perm"], bqkv,
                                 C, scale, wp, bp, B=B)
        return ops.view_nhwc(ob, B, H, W)

    def _block_h16(self, x, bqkv, scale, fuse_proj):
        """GroupNorm (from the producer's chunk statistics) inside the q | k | v projection, K / V^T straight into the attention's
        fragment order (csrc/attention.hip: attn_qkv_gn_h16_kernel), flash, and the merge fused into proj_out + x (`fuse_proj`: 4
        launches) or on its own ahead of the proj_out convolution — instead of normalise (2) + GEMM + split + flash + merge"""
        B, H, W, C = x.shape
        wqkvs = self._wqkv
        wkey = ("frag", x.dtype)
        if wkey not in wqkvs:
            wqkvs[wkey] = ops.pack_qkv_weight_h16(wqkvs[torch.float32], x.dtype)
        proj = None
        if fuse_proj:
            pkey = ("proj_frag", x.dtype, self.proj_out.weight.data_ptr(), self.proj_out.weight._version)
            if pkey not in wqkvs:
                wqkvs[pkey] = (ops.pack_weight_tp_h16(self.proj_out.weight.detach().reshape(C, C).float().contiguous(), x.dtype),
                               self.proj_out.bias.detach().float().contiguous())
            proj = wqkvs[pkey]
        o = ops.attn_block_h16(x.reshape(B * H * W, C), ops.gn_stats(x), self.norm.weight.detach(), self.norm.bias.detach(),
                               self.norm.eps, wqkvs[wkey], bqkv, C, scale, B=B, proj=proj)
        if fuse_proj:
            return ops.view_nhwc(o, B, H, W)
        return self.proj_out.forward_nhwc(o.view(B, H, W, C), residual=x)


def _make_attn_list():
    return nn.ModuleList()


class Encoder(_NHWCModule):
    def __init__(self, *, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks, attn_resolutions, dropout=0.0,
                 resamp_with_conv=True, in_channels, resolution, z_channels, double_z=True, **ignore_kwargs):
        super().__init__()
        self.ch, self.temb_ch = ch, 0
        self.num_resolutions = len(ch_mult)
        self.num_res_blocks = num_res_blocks
        self.resolution = resolution
        self.in_channels = in_channels
        self.conv_in = Conv2d(in_channels, ch, kernel_size=3, stride=1, padding=1)
        # attention placement follows ddconfig.resolution bookkeeping, NOT the real input size
        res = resolution
        widths = [ch * m for m in (1,) + tuple(ch_mult)]
        self.down = nn.ModuleList()
        for lv in range(self.num_resolutions):
            stage = nn.Module()
            stage.block, stage.attn = nn.ModuleList(), _make_attn_list()
            cin, cout = widths[lv], widths[lv + 1]
            for _ in range(num_res_blocks):
                stage.block.append(ResnetBlock(in_channels=cin, out_channels=cout, temb_channels=0, dropout=dropout))
                cin = cout
                if res in attn_resolutions:
                    stage.attn.append(AttnBlock(cin))
            if lv != self.num_resolutions - 1:
                stage.downsample = Downsample(cin, resamp_with_conv)
                res //= 2
            self.down.append(stage)
        top = widths[-1]
        self.mid = nn.Module()
        self.mid.block_1 = ResnetBlock(in_channels=top, out_channels=top, temb_channels=0, dropout=dropout)
        self.mid.attn_1 = AttnBlock(top)
        self.mid.block_2 = ResnetBlock(in_channels=top, out_channels=top, temb_channels=0, dropout=dropout)
        self.norm_out = Normalize(top)
        self.conv_out = Conv2d(top, 2 * z_channels if double_z else z_channels, kernel_size=3, stride=1, padding=1)

    def forward_nhwc(self, x):
        """x: (B,H,W,32) NHWC with the in_channels real channels first, rest zero."""
        h = self.conv_in.forward_nhwc(x)
        for lv, stage in enumerate(self.down):
            for ib, blk in enumerate(stage.block):
                h = blk.forward_nhwc(h)
                if len(stage.attn) > 0:
                    h = stage.attn[ib].forward_nhwc(h)
            if lv != self.num_resolutions - 1:
                h = stage.downsample.forward_nhwc(h)
        h = self.mid.block_2.forward_nhwc(self.mid.attn_1.forward_nhwc(self.mid.block_1.forward_nhwc(h)))
        return _norm_conv(self.norm_out, True, self.conv_out, h)

    def forward(self, x):
        return ops.nhwc_to_nchw(self.forward_nhwc(ops.nchw_to_nhwc(x, c_pad=32)))


class Decoder(_NHWCModule):
    def __init__(self, *, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks, attn_resolutions, dropout=0.0,
                 resamp_with_conv=True, in_channels, resolution, z_channels, give_pre_end=False, **ignorekwargs):
        super().__init__()
        self.ch, self.temb_ch = ch, 0
        self.num_resolutions = len(ch_mult)
        self.num_res_blocks = num_res_blocks
        self.resolution = resolution
        self.in_channels = in_channels
        self.give_pre_end = give_pre_end
        self.out_ch = out_ch
        width = ch * ch_mult[-1]
        res = resolution // 2 ** (self.num_resolutions - 1)
        self.z_shape = (1, z_channels, res, res)
        print("Working with z of shape {} = {} dimensions.".format(self.z_shape, int(np.prod(self.z_shape))))
        self.conv_in = Conv2d(z_channels, width, kernel_size=3, stride=1, padding=1)
        self.mid = nn.Module()
        self.mid.block_1 = ResnetBlock(in_channels=width, out_channels=width, temb_channels=0, dropout=dropout)
        self.mid.attn_1 = AttnBlock(width)
        self.mid.block_2 = ResnetBlock(in_channels=width, out_channels=width, temb_channels=0, dropout=dropout)
        stages = []
        for lv in reversed(range(self.num_resolutions)):
            stage = nn.Module()
            stage.block, stage.attn = nn.ModuleList(), _make_attn_list()
            cout = ch * ch_mult[lv]
            for _ in range(num_res_blocks + 1):
                stage.block.append(ResnetBlock(in_channels=width, out_channels=cout, temb_channels=0, dropout=dropout))
                width = cout
                if res in attn_resolutions:
                    stage.attn.append(AttnBlock(width))
            if lv != 0:
                stage.upsample = Upsample(width, resamp_with_conv)
                res *= 2
            stages.append(stage)
        self.up = nn.ModuleList(reversed(stages))  # index = resolution level, like the reference
        self.norm_out = Normalize(width)
        self.conv_out = Conv2d(width, out_ch, kernel_size=3, stride=1, padding=1)

    def forward_nhwc(self, z):
        self.last_z_shape = (z.shape[0], z.shape[3], z.shape[1], z.shape[2])
        h = self.conv_in.forward_nhwc(z)
        h = self.mid.block_2.forward_nhwc(self.mid.attn_1.forward_nhwc(self.mid.block_1.forward_nhwc(h)))
        for lv in reversed(range(self.num_resolutions)):
            stage = self.up[lv]
            for ib, blk in enumerate(stage.block):
                h = blk.forward_nhwc(h)
                if len(stage.attn) > 0:
                    h = stage.attn[ib].forward_nhwc(h)
            if lv != 0:
                h = stage.upsample.forward_nhwc(h)
        if self.give_pre_end:
            return h
        return _norm_conv(self.norm_out, True, self.conv_out, h, out_dtype=torch.float32)  # RGB-D leaves in fp32
