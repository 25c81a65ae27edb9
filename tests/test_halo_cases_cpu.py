"""CPU: the case table of tests/halo_cases.py is what it says.  The planner entry points of the library work without a device, so
every row's descriptor, tile, split, workspace, statistics and folding expectations are proven here before any GPU time is spent
(tests/test_gpu_halo_conv.py then proves the kernel each row names against float64)."""
import ctypes
import os
import sys

import pytest

from sgam_neurips22_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import halo_cases as HC  # noqa: E402

ref = ctypes.byref


def _plan(fn, d):
    bm, bn, ks = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    rc = fn(ref(d), ref(bm), ref(bn), ref(ks))
    return rc, (bm.value, bn.value, ks.value)


def test_the_table_is_complete_and_its_tags_are_unique():
    tags = [c.tag for c in HC.CASES]
    assert len(set(tags)) == len(tags)
    assert len(HC.H16_CASES) == 2 * len(HC._H16_ROWS) and {c.family for c in HC.CASES} == {"f32x", "bf16", "fp16"}
    # every member the launch sites of the two families spell, by name fragment (the 16-bit ones for both types)
    want_x = ["128,128,false", "128,128,true", "128,128,false,true", "64,128,false", "64,128,true", "64,128,false,true",
              "64,128,true,false,false,6", "64,128,true,false,true", "64,128,true,false,true,6", "128,32,false", "128,32,true",
              "64,64,false", "64,64,true"]
    have = {c.kernel for c in HC.F32X_CASES}
    assert [k for k in want_x if HC._XK % k not in have] == []
    for ht in (0, 1):
        want_h = [f"{bm},128,{ht},{v}" for bm in (256, 128, 64) for v in ("false,false", "true,false", "true,false,false", "false,true")]
        want_h += [f"64,128,{ht},{v}" for v in ("false,false,true,false,6", "true,false,true,false,6", "true,false,false,false,6",
                                                "false,true,true,false,6", "true,false,true,true,6", "true,false,false,true,6")]
        have = {c.kernel for c in HC.H16_CASES}
        assert [k for k in want_h if HC._HK % k not in have] == []
    combines = {c.combine for c in HC.CASES if c.combine}
    assert {HC._XRM, HC._XGM % 32, HC._XGM % 16, HC._XGM % 8} <= combines
    for ht in (0, 1):
        assert {s.format(ht=ht) for s in (HC._HRM, HC._HGM % 32, HC._HGM % 16, HC._HGM % 8)} <= combines


@pytest.mark.parametrize("case", HC.F32X_CASES, ids=str)
def test_split_fp32_row_is_what_it_says(case):
    lib = _lib.load()
    d = HC.desc(case)
    rc, got = _plan(lib.sgam_conv2d_f32x_plan, d)
    assert rc == 0, "the descriptor validates"
    assert lib.sgam_conv2d_f32x_uses_halo(ref(d)) == 1
    assert got == tuple(case.runs or case.plan)
    ks, M = case.ksplit, case.B * case.Ho * case.Wo
    assert lib.sgam_conv2d_f32x_workspace_bytes(ref(d)) == (ks * M * case.N * 4 if ks > 1 else 0)
    total = case.Cin // 32
    assert 1 <= case.slabs <= total and -(-total // case.slabs) == ks, "slabs per workgroup and the split agree"
    assert (case.combine is not None) == (ks > 1)
    chunks = lib.sgam_conv2d_f32x_stats_chunks(ref(d))
    assert (chunks > 0) == case.stats, chunks
    if case.gn:
        assert lib.sgam_conv2d_f32x_gn_fusable(ref(d)) == 1 and case.Cin % 128 == 0 and not case.ups
    if case.folded:
        # the producer of the pair has the row's own shape: its chunk count is what the consumer is asked to fold
        assert 1 <= chunks <= 16 and lib.sgam_conv2d_f32x_gn_foldable(ref(d), chunks) == 1
    elif case.gn:
        assert [c for c in range(1, 17) if lib.sgam_conv2d_f32x_gn_foldable(ref(d), c) == 1] == []


@pytest.mark.parametrize("case", HC.H16_CASES, ids=str)
def test_16bit_row_is_what_it_says(case):
    lib = _lib.load()
    d = HC.desc(case)
    rc, _ = _plan(lib.sgam_conv2d_h16_plan, d)          # (the generic kernel's plan: the call validates the descriptor)
    assert rc == 0, "the descriptor validates"
    assert lib.sgam_conv2d_h16_uses_halo(ref(d)) == 1
    bm, bn, ks = case.runs or case.plan
    M, hw = case.B * case.Ho * case.Wo, case.Ho * case.Wo
    # the halo planner of the 16-bit family has no plan query of its own: the split shows in the workspace, the tile height in the
    # chunk count of a whole-K launch (one chunk per (tile, row half)), and the kernel name proves both on the GPU
    assert bn == 128 and lib.sgam_conv2d_halo_h16_workspace_bytes(ref(d)) == (ks * M * case.N * 4 if ks > 1 else 0)
    total = case.Cin // 32
    assert 1 <= case.slabs <= total and -(-total // case.slabs) == ks, "slabs per workgroup and the split agree"
    assert (case.combine is not None) == (ks > 1)
    chunks = lib.sgam_conv2d_h16_stats_chunks(ref(d))
    assert (chunks > 0) == case.stats, chunks
    assert not (case.out32 and case.stats), "the fp32-output form leaves no statistics (ops._conv_h16)"
    if case.stats and ks == 1:
        assert chunks == (hw // bm) * 2
    if case.gn:
        assert case.Cin % 128 == 0 and not case.ups
    if case.folded:
        assert 1 <= chunks <= 16 and lib.sgam_conv2d_h16_gn_foldable(ref(d), chunks) == 1
    elif case.gn:
        assert [c for c in range(1, 17) if lib.sgam_conv2d_h16_gn_foldable(ref(d), c) == 1] == []


def _desc(N, hw, bm, **kw):
    base = dict(B=2, Hi=hw, Wi=hw, Cin=128, Ho=hw, Wo=hw, N=N, KH=3, KW=3, stride=1, pad_t=1, pad_l=1, upsample2x=0, lda=128,
                ldb=1152, ldc=N, ldr=0, n_valid=N, bias_per_row=0, plan_bm=bm, plan_bn=128, plan_ksplit=1)
    base.update(kw)
    return _lib.ConvDesc(**base)


def test_epilogue_statistics_need_whole_groups_per_wavefront():
    """Both epilogues fold the output statistics per wavefront, over the groups inside its 32 columns (`groups_here = columns / 4
    / (cpg / 4)`, `g = wn0 / cpg + lane`): right only when 32 % cpg == 0.  N = 384 (cpg 12) would put columns 32..43 into the
    group that covers 24..35 and never write group 31; N = 2048 (cpg 64) would write nothing.  No whole-K descriptor of such a
    width may be promised chunk statistics — the layer takes the statistics pass."""
    lib = _lib.load()
    for N in (384, 640, 768, 896, 1152, 2048):
        assert 32 % (N // 32) != 0
        for bm in (64, 128):
            for hw in (16, 64):
                d = _desc(N, hw, bm)
                assert _plan(lib.sgam_conv2d_f32x_plan, d) == (0, (bm, 128, 1))
                assert lib.sgam_conv2d_f32x_stats_chunks(ref(d)) == 0 and lib.sgam_conv2d_f32x_stats_mode(ref(d)) == 0, (N, bm, hw)
                assert lib.sgam_conv2d_h16_uses_halo(ref(d)) == 1 and lib.sgam_conv2d_halo_h16_workspace_bytes(ref(d)) == 0
                assert lib.sgam_conv2d_h16_stats_chunks(ref(d)) == 0, (N, bm, hw)
        assert lib.sgam_conv2d_h16_stats_chunks(ref(_desc(N, 16, 256))) == 0
        # the generic split-fp32 kernel shares the epilogue (a 1x1 convolution, heuristic plan aside)
        g = _desc(N, 64, 64, KH=1, KW=1, pad_t=0, pad_l=0, ldb=128)
        assert lib.sgam_conv2d_f32x_uses_halo(ref(g)) == 0 and lib.sgam_conv2d_f32x_stats_chunks(ref(g)) == 0
    # the widths the model ships keep their statistics
    for N in (128, 256, 512, 1024):
        for bm in (64, 128):
            d = _desc(N, 16, bm)
            assert lib.sgam_conv2d_f32x_stats_chunks(ref(d)) == (256 // bm) * 2
            assert lib.sgam_conv2d_h16_stats_chunks(ref(d)) == (256 // bm) * 2
