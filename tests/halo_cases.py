"""The case table of the halo-staged 3x3 convolutions (csrc/conv_f32x.hip: conv3x3_f32x_halo2_kernel, csrc/h16_halo.hip:
conv3x3_h16_halo_kernel) and their split-K combines: one row per member of the two kernel families at the smallest shape that
still reaches it, with the plan that forces it, the kernel-name fragment the row exists for and the split it expects.

Plain data plus two helpers (`desc`, `forced_plan`).  tests/test_halo_cases_cpu.py proves the table against the planner entry
points without a GPU; tests/test_gpu_halo_conv.py runs every row against float64.

What a row says:
  family      "f32x" (split fp32, ops.set_f32_mode("split")), "bf16" or "fp16"
  B Cin Cout  batch and widths; H, W is the SOURCE map (the output is 2H x 2W on an `ups` row)
  gn          None | "table" (GroupNorm from a {mean, rstd} table) | "swish" (table + swish) | "folded" (a producer + consumer
              pair of the row's shape: the consumer folds the producer's chunk partials itself; with swish) | "folded_plain"
              (the same without swish)
  res         a residual is added
  cin_pitch   channel pitch of x (0: dense); res_pitch: channel pitch of the residual (0: dense)
  plan        the forced (bm, bn, ksplit)
  runs        the (bm, bn, ksplit) that plan runs as (a 256-row plan on an 8-row map falls back to 128 rows; a split of three
              slabs in two is 2 + 1 ...)
  slabs       32-channel slabs the first workgroup of the split walks
  kernel      fragment of the kernel_timeline name the row exists for; combine: the same for the split-K combine (None: whole K)
  stats       the GroupNorm chunk statistics of the output leave with it (ops.gn_stats)
  out32       16-bit families: the fp32-output form
  cout_pad    rows of the packed weight where it is not the packer's default
"""
import contextlib
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from sgam_neurips22_amd import ops
from sgam_neurips22_amd._lib import ConvDesc

TORCH_DTYPE = {"f32x": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
HT = {"bf16": 0, "fp16": 1}


@dataclass(frozen=True)
class HaloCase:
    tag: str
    family: str
    B: int
    Cin: int
    Cout: int
    H: int
    W: int
    plan: Tuple[int, int, int]
    kernel: str
    ups: bool = False
    gn: Optional[str] = None
    res: bool = False
    cin_pitch: int = 0
    res_pitch: int = 0
    runs: Optional[Tuple[int, int, int]] = None
    slabs: int = 0
    combine: Optional[str] = None
    stats: bool = False
    out32: bool = False
    cout_pad: Optional[int] = None

    @property
    def Ho(self):
        return 2 * self.H if self.ups else self.H

    @property
    def Wo(self):
        return 2 * self.W if self.ups else self.W

    @property
    def N(self):
        """rows of the packed weight (ops.pack_conv_weight)"""
        if self.cout_pad:
            return self.cout_pad
        if self.family == "f32x" and self.Cout <= 32:
            return 32
        return (self.Cout + 127) // 128 * 128

    @property
    def folded(self):
        return self.gn in ("folded", "folded_plain")

    @property
    def swish(self):
        return self.gn in ("swish", "folded")

    @property
    def ksplit(self):
        return (self.runs or self.plan)[2]

    @property
    def plan_dtype(self):
        """the dtype argument of ops.plan_key"""
        return "f32x" if self.family == "f32x" else TORCH_DTYPE[self.family]

    def __str__(self):
        return self.tag


def desc(case, with_plan=True):
    """the ConvDesc ops.conv2d_nhwc builds for this row (with_plan: with the forced plan filled in, as ops._apply_plan leaves it)"""
    d = ConvDesc(B=case.B, Hi=case.H, Wi=case.W, Cin=case.Cin, Ho=case.Ho, Wo=case.Wo, N=case.N, KH=3, KW=3, stride=1, pad_t=1, pad_l=1,
                 upsample2x=int(case.ups), lda=case.cin_pitch or case.Cin, ldb=9 * case.Cin, ldc=case.Cout,
                 ldr=(case.res_pitch or case.Cout) if case.res else 0, n_valid=case.Cout, bias_per_row=0)
    if with_plan:
        d.plan_bm, d.plan_bn, d.plan_ksplit = case.plan
    return d


@contextlib.contextmanager
def forced_plan(case):
    """ops.PLAN_CACHE[key of the row] = the row's plan for the duration of the block"""
    key = ops.plan_key(desc(case, with_plan=False), case.plan_dtype)
    old = ops.PLAN_CACHE.get(key)
    ops.PLAN_CACHE[key] = tuple(case.plan)
    try:
        yield key
    finally:
        if old is None:
            ops.PLAN_CACHE.pop(key, None)
        else:
            ops.PLAN_CACHE[key] = old


# ---------------------------------------------------------------------------------------------------------------------------------
# split fp32: conv3x3_f32x_halo2_kernel<BM, BN, GN, UPS, GNF, NB> (defaulted tail left off, as the launch sites spell it)
# ---------------------------------------------------------------------------------------------------------------------------------
_XK = "halo2_kernel<%s>"
_XGM = "splitk_reduce_gm_f32x_kernel<%d>"
_XRM = "splitk_reduce_f32x_kernel"


def _x(name, B, Cin, Cout, H, W, plan, kernel, **kw):
    return HaloCase("f32x-" + name, "f32x", B, Cin, Cout, H, W, plan, _XK % kernel, **kw)


F32X_CASES = [
    # one 8 x 8 tile: all four borders are padding inside one halo; one slab (the peeled "last slab" only), ring of 3
    _x("tile8x8_slab1_ring3", 1, 32, 128, 8, 8, (64, 128, 1), "64,128,false", slabs=1, stats=True, res=True),
    # three slabs split in two: 2 + 1 (the one-slab workgroup enters the peel at its end), batch of 3, group-major combine
    _x("uneven_2p1_b3", 3, 96, 128, 8, 24, (64, 128, 2), "64,128,false", slabs=2, combine=_XGM % 32, stats=True, res=True),
    # 128-row tile: one 8 x 16 tile per image; one tile column of three tile rows
    _x("tile128_single", 2, 64, 256, 8, 16, (128, 128, 1), "128,128,false", slabs=2, stats=True),
    _x("tile128_column", 2, 64, 256, 24, 16, (128, 128, 1), "128,128,false", slabs=2, stats=True, res=True),
    _x("tile128_gn", 2, 128, 128, 16, 32, (128, 128, 1), "128,128,true", gn="table", slabs=4, stats=True, res=True),
    # 64-row tile with the table GroupNorm: ring of 6 (even slabs, small grid) and ring of 3 (three slabs per workgroup; the input
    # has 12 channels per group)
    _x("tile64_gn_ring6", 1, 256, 128, 16, 16, (64, 128, 1), "64,128,true,false,false,6", gn="swish", slabs=8, stats=True),
    _x("tile64_gn_ring3_cin384", 1, 384, 128, 16, 16, (64, 128, 4), "64,128,true", gn="swish", slabs=3, combine=_XGM % 32,
       stats=True, res=True),
    # the folding form at B > 1 (partials indexed b * chunks_in * 32): ring of 6, and ring of 3 behind a grid of 640 workgroups
    _x("fold_ring6_b2", 2, 128, 128, 16, 16, (64, 128, 4), "64,128,true,false,true,6", gn="folded", slabs=1, combine=_XGM % 32,
       stats=True, res=True),
    _x("fold_ring3_b5", 5, 256, 256, 32, 32, (64, 128, 4), "64,128,true,false,true", gn="folded", slabs=2, combine=_XGM % 16,
       stats=True, res=True),
    # narrow outputs: ONE 32-channel tile, four wavefronts stacked along M
    _x("out4_plain", 2, 128, 4, 8, 16, (128, 32, 1), "128,32,false", slabs=4, res=True),
    _x("out4_gn", 2, 128, 4, 8, 16, (128, 32, 1), "128,32,true", gn="swish", slabs=4),
    _x("out32_plain", 2, 128, 32, 8, 16, (128, 32, 1), "128,32,false", slabs=4),
    _x("out32_gn", 2, 128, 32, 8, 16, (128, 32, 1), "128,32,true", gn="table", slabs=4, res=True),
    # the 64-channel tile (2 x 2 wavefronts)
    _x("tile64x64_out64", 2, 128, 64, 8, 8, (64, 64, 1), "64,64,false", slabs=4, cout_pad=64, res=True),
    _x("tile64x64_out64_gn", 2, 128, 64, 8, 8, (64, 64, 1), "64,64,true", gn="table", slabs=4, cout_pad=64),
    _x("tile64x64_out128", 2, 128, 128, 8, 8, (64, 64, 1), "64,64,false", slabs=4, stats=True),
    _x("tile64x64_out128_gn", 2, 128, 128, 8, 8, (64, 64, 1), "64,64,true", gn="swish", slabs=4, stats=True, res=True),
    # nearest-2x upsampled input at the smallest source patches
    _x("ups128_src4x8", 2, 64, 128, 4, 8, (128, 128, 1), "128,128,false,true", ups=True, slabs=2, stats=True, res=True),
    _x("ups64_src4x4", 2, 64, 128, 4, 4, (64, 128, 1), "64,128,false,true", ups=True, slabs=2, stats=True),
    _x("ups64_src12x4", 1, 96, 128, 12, 4, (64, 128, 1), "64,128,false,true", ups=True, slabs=3, stats=True, res=True),
    # lda > Cin and ldr > ldc: x and the residual are channel slices of wider tensors
    _x("pitch_tile64", 2, 64, 128, 8, 24, (64, 128, 1), "64,128,false", slabs=2, stats=True, res=True, cin_pitch=96, res_pitch=192),
    _x("pitch_tile128", 2, 64, 128, 8, 32, (128, 128, 1), "128,128,false", slabs=2, stats=True, res=True, cin_pitch=96, res_pitch=192),
    # 12 output channels per group: a wavefront's 32 columns do not hold whole groups, so the epilogue cannot deliver the
    # statistics (stats=False: the layer takes the statistics pass)
    _x("out384_tile64_b1", 1, 128, 384, 16, 16, (64, 128, 1), "64,128,false", slabs=4),
    _x("out384_tile64_b2", 2, 128, 384, 16, 16, (64, 128, 1), "64,128,false", slabs=4, res=True),
    _x("out384_tile128_b1", 1, 128, 384, 16, 16, (128, 128, 1), "128,128,false", slabs=4, res=True),
    _x("out384_tile128_b2", 2, 128, 384, 16, 16, (128, 128, 1), "128,128,false", slabs=4),
    # the four combines: row-major without statistics (N = 384) and with them, group-major at 32 (above), 16 and 8 channels per tile
    _x("out384_rowmajor_combine", 1, 128, 384, 16, 16, (64, 128, 2), "64,128,false", slabs=2, combine=_XRM, res=True),
    _x("combine_rowmajor_stats", 1, 64, 128, 64, 64, (64, 128, 2), "64,128,false", slabs=1, combine=_XRM, stats=True, res=True),
    _x("combine_gm16", 1, 64, 256, 32, 32, (64, 128, 2), "64,128,false", slabs=1, combine=_XGM % 16, stats=True, res=True),
    _x("combine_gm8", 1, 64, 128, 32, 64, (64, 128, 2), "64,128,false", slabs=1, combine=_XGM % 8, stats=True),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# 16-bit: conv3x3_h16_halo_kernel<BM, 128, HT, GN, UPS, SW, GNF, NB>; every row for bf16 (HT = 0) and fp16 (HT = 1)
# ---------------------------------------------------------------------------------------------------------------------------------
_HK = "halo_kernel<%s>"
_HGM = "h16_splitk_reduce_gm_kernel<{ht},%d>"
_HRM = "h16_splitk_reduce_kernel<{ht}>"
_R6 = ",true,false,6"          # tail of a ring-of-6 name: SW (spelled out), GNF = false, NB = 6


def _h(name, B, Cin, Cout, H, W, plan, kernel, **kw):
    return (name, B, Cin, Cout, H, W, plan, _HK % kernel, kw)


_H16_ROWS = [
    # the 256-row tile (16 x 16 pixels): plain / GroupNorm / GroupNorm + swish / upsampled, and split in two
    _h("t256_plain_b1", 1, 128, 128, 16, 16, (256, 128, 1), "256,128,{ht},false,false", slabs=4, stats=True, res=True),
    _h("t256_gn_b2_16x32", 2, 128, 128, 16, 32, (256, 128, 1), "256,128,{ht},true,false,false", gn="table", slabs=4, stats=True),
    _h("t256_gnswish_b2", 2, 128, 128, 16, 16, (256, 128, 1), "256,128,{ht},true,false", gn="swish", slabs=4, stats=True, res=True),
    _h("t256_ups_b2_src8x8", 2, 128, 128, 8, 8, (256, 128, 1), "256,128,{ht},false,true", ups=True, slabs=4, stats=True, res=True),
    _h("t256_split2_b1_16x32", 1, 128, 128, 16, 32, (256, 128, 2), "256,128,{ht},false,false", slabs=2, combine=_HGM % 32,
       stats=True, res=True),
    # 256 rows asked on an 8-row map: the 128-row kernel runs
    _h("t256_falls_back_8x16", 2, 128, 128, 8, 16, (256, 128, 1), "128,128,{ht},false,false", runs=(128, 128, 1), slabs=4, stats=True),
    # the 128-row tile: a single tile per image, and its GroupNorm / upsampled forms
    _h("t128_single", 2, 32, 128, 8, 16, (128, 128, 1), "128,128,{ht},false,false", slabs=1, stats=True, res=True),
    _h("t128_gn", 2, 128, 128, 8, 16, (128, 128, 1), "128,128,{ht},true,false,false", gn="table", slabs=4, stats=True, res=True),
    _h("t128_gnswish", 2, 128, 128, 8, 16, (128, 128, 1), "128,128,{ht},true,false", gn="swish", slabs=4, stats=True),
    _h("t128_ups_src4x8", 2, 64, 128, 4, 8, (128, 128, 1), "128,128,{ht},false,true", ups=True, slabs=2, stats=True),
    # the 64-row tile, ring of 3: an odd slab count walked whole
    _h("t64_ring3_odd", 1, 96, 128, 8, 8, (64, 128, 1), "64,128,{ht},false,false", slabs=3, stats=True, res=True),
    _h("t64_ring3_ups_src4x4", 1, 96, 128, 4, 4, (64, 128, 1), "64,128,{ht},false,true", ups=True, slabs=3, stats=True),
    _h("t64_ring3_gnswish_cin384", 1, 384, 128, 16, 16, (64, 128, 4), "64,128,{ht},true,false", gn="swish", slabs=3,
       combine=_HGM % 32, stats=True, res=True),
    _h("t64_ring3_gn_cin384", 1, 384, 128, 16, 16, (64, 128, 4), "64,128,{ht},true,false,false", gn="table", slabs=3,
       combine=_HGM % 32, stats=True),
    # ... ring of 6
    _h("t64_ring6", 1, 128, 128, 8, 8, (64, 128, 1), "64,128,{ht},false,false" + _R6, slabs=4, stats=True, res=True),
    _h("t64_ring6_gn", 1, 128, 128, 8, 8, (64, 128, 1), "64,128,{ht},true,false,false,false,6", gn="table", slabs=4, stats=True),
    _h("t64_ring6_gnswish", 1, 128, 128, 8, 8, (64, 128, 1), "64,128,{ht},true,false" + _R6, gn="swish", slabs=4, stats=True, res=True),
    _h("t64_ring6_ups_src4x4", 1, 128, 128, 4, 4, (64, 128, 1), "64,128,{ht},false,true" + _R6, ups=True, slabs=4, stats=True),
    # uneven split-K: 2 + 1 (a one-slab workgroup in the peel) and 3 + 2
    _h("uneven_2p1", 2, 96, 128, 16, 16, (64, 128, 2), "64,128,{ht},false,false", slabs=2, combine=_HGM % 32, stats=True, res=True),
    _h("uneven_3p2", 1, 160, 128, 16, 16, (64, 128, 2), "64,128,{ht},false,false", slabs=3, combine=_HGM % 32, stats=True),
    # narrow outputs through the tail store (nb + 16 > n_lim), 16-bit and fp32 output
    _h("out4_t128", 2, 128, 4, 8, 16, (128, 128, 1), "128,128,{ht},false,false", slabs=4, res=True),
    _h("out8_t64", 2, 128, 8, 8, 16, (64, 128, 1), "64,128,{ht},false,false" + _R6, slabs=4, res=True),
    _h("out12_t128", 2, 128, 12, 8, 16, (128, 128, 1), "128,128,{ht},false,false", slabs=4, res=True),
    _h("out20_t64", 2, 128, 20, 8, 16, (64, 128, 1), "64,128,{ht},false,false" + _R6, slabs=4, res=True),
    _h("out4_t128_f32out", 2, 128, 4, 8, 16, (128, 128, 1), "128,128,{ht},false,false", slabs=4, out32=True),
    _h("out8_t64_f32out", 2, 128, 8, 8, 16, (64, 128, 1), "64,128,{ht},false,false" + _R6, slabs=4, out32=True, res=True),
    _h("out12_t128_f32out", 2, 128, 12, 8, 16, (128, 128, 1), "128,128,{ht},false,false", slabs=4, out32=True, res=True),
    _h("out20_t64_f32out", 2, 128, 20, 8, 16, (64, 128, 1), "64,128,{ht},false,false" + _R6, slabs=4, out32=True),
    # 12 output channels per group, whole K (stats=False: see the split-fp32 rows)
    _h("out384_t64", 2, 128, 384, 16, 16, (64, 128, 1), "64,128,{ht},false,false" + _R6, slabs=4, res=True),
    _h("out384_t128", 2, 128, 384, 16, 16, (128, 128, 1), "128,128,{ht},false,false", slabs=4),
    # pitches
    _h("pitch_t64", 2, 64, 128, 8, 16, (64, 128, 1), "64,128,{ht},false,false" + _R6, slabs=2, stats=True, res=True,
       cin_pitch=96, res_pitch=192),
    _h("pitch_t128", 2, 64, 128, 8, 16, (128, 128, 1), "128,128,{ht},false,false", slabs=2, stats=True, res=True,
       cin_pitch=96, res_pitch=192),
    # the folding form at B = 2 and the four combines
    _h("fold_b2", 2, 256, 256, 16, 16, (64, 128, 8), "64,128,{ht},true,false,true,true,6", gn="folded", slabs=1, combine=_HGM % 32,
       stats=True, res=True),
    _h("fold_plain_b2", 2, 256, 256, 16, 16, (64, 128, 4), "64,128,{ht},true,false,false,true,6", gn="folded_plain", slabs=2,
       combine=_HGM % 32, stats=True),
    _h("out384_rowmajor_combine", 1, 128, 384, 16, 16, (64, 128, 2), "64,128,{ht},false,false" + _R6, slabs=2, combine=_HRM, res=True),
    _h("combine_rowmajor_stats", 1, 64, 128, 64, 64, (64, 128, 2), "64,128,{ht},false,false", slabs=1, combine=_HRM, stats=True, res=True),
    _h("combine_gm16", 1, 64, 256, 32, 32, (64, 128, 2), "64,128,{ht},false,false", slabs=1, combine=_HGM % 16, stats=True, res=True),
    _h("combine_gm8", 1, 64, 128, 32, 64, (64, 128, 2), "64,128,{ht},false,false", slabs=1, combine=_HGM % 8, stats=True),
]


def _expand_h16():
    out = []
    for fam in ("bf16", "fp16"):
        for name, B, Cin, Cout, H, W, plan, kernel, kw in _H16_ROWS:
            kw = dict(kw)
            if kw.get("combine"):
                kw["combine"] = kw["combine"].format(ht=HT[fam])
            out.append(HaloCase(f"{fam}-{name}", fam, B, Cin, Cout, H, W, plan, kernel.format(ht=HT[fam]), **kw))
    return out


H16_CASES = _expand_h16()
CASES = F32X_CASES + H16_CASES
