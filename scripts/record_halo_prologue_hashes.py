"""Record what the split-fp32 kernels write behind their prologues into tests/golden/halo_prologue_hashes.json.

The prologues of conv3x3_f32x_halo2_kernel, conv_gemm_f32x_kernel and the split-K combines (csrc/conv_f32x.hip) may fetch their
arguments in one batch and map workgroups to tiles without gridDim (the change this file was recorded for); requesting the
GroupNorm parameters ahead of the halo and the weight fragments, without a branch around a request, was measured with it and not
kept (profiles/HISTORY.md), its rows stay for the next attempt — no bit of an output, of a split-K partial or of the GroupNorm
chunk statistics may move, and no kernel name of the launch timeline.  Per case of `cases()` the file holds the kernel names of
ops.kernel_timeline, the sha256 of the output, the (chunks, sha256) of the chunk statistics that leave with it and, for a split-K
plan, the sha256 of the workspace (the ksplit partial tiles, before the combine).  A wrong tile map, a parameter of the wrong
channel or chunk, a table entry read before it was written: each is a wrong hash.  tests/test_gpu_halo_prologue.py replays the
cases against the file; tests/test_halo_prologue_cases_cpu.py proves the rows against the planner without a GPU.

The file is recorded from a build of the commit BEFORE the change and names that build (`recorded_from`, `lib_digest`); it is never
re-recorded from the code under test:

    SGAM_LIB_DIR=<dir> python -m sgam_neurips22_amd.build          # in a checkout of the earlier commit
    SGAM_HIP_LIB=<dir>/libsgam_hip.so python scripts/record_halo_prologue_hashes.py        (needs the GPU)

Rows (the smallest shapes that reach each changed line; plans forced with halo_cases.forced_plan; T = workgroups of the launch):
  folding form, ring of six <64,128,true,false,true,6>: the consumer alone, fed seeded chunk partials [B][chunks_in][32][2], so that
      chunks_in takes the values at the edges of the two predicates of the fold (lane sub < chunks_in, sub + 8 < chunks_in): 1, 2,
      8, 9 and 16.  The producers of the model leave 2 .. 16 (a power of two, or 6); 1 and 9 pass the host rule
      (sgam_conv2d_f32x_gn_foldable takes 1 .. 16) and only these rows reach them.  One slab per workgroup (128 inputs split in
      four) and two (256 in four); B = 1 and B = 2 (the partials of image 1 lie chunks_in * 32 pairs on); maps 8 x 8 (T = 4: fewer
      workgroups than XCDs), 8 x 24 (T = 12: T % 8 != 0, the bijective form of the tile map), 16 x 16, 32 x 32; with / without swish
  folding form, ring of three <64,128,true,false,true>: behind a grid of 640 workgroups, one and two slabs
  table form, for <64,64,true>, <64,128,true>, <64,128,true,false,false,6>, <128,128,true> and <128,32,true>: 128 inputs (the smallest
      width the fused GroupNorm takes: threads 128 .. 255 and three of the four rounds of the table build are masked) with and without
      swish, and 1024 inputs (XGN_MAXC: every thread, every round) on one 8 x 8 (8 x 16) tile per image; B = 2 (the table of image 1)
  entry code of the generic kernel: the encoder's stride-2 convolution on <64,64,false,false> with T = 4, and split in two with T = 12
      and T = 20
  the combines: row-major with and without statistics, group-major at 32 (the folding rows), 16 and 8 channels per tile
The launcher always sets xcd_swizzle: the tile map without it is not reachable from the library's entry points and has no row.
"""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import halo_cases as HC  # noqa: E402
from sgam_neurips22_amd import _lib, ops, testing  # noqa: E402
from sgam_neurips22_amd._lib import ConvDesc  # noqa: E402


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RA = _load("record_halo_readahead_hashes")      # _record (output, statistics, workspace, kernel names) and _mean_rstd are shared with it
EPI = RA.EPI
FIXTURE = os.path.join(ROOT, "tests", "golden", "halo_prologue_hashes.json")
_GM = HC._XGM
FOLD6, FOLD3 = "64,128,true,false,true,6", "64,128,true,false,true"

CHUNKS_IN = {}          # tag of a folding row -> chunk partials per image it is fed


def _fold(name, B, Cin, Cout, H, W, chunks_in, kernel, swish, slabs, combine):
    c = HC._x(name, B, Cin, Cout, H, W, (64, 128, 4), kernel, gn="folded" if swish else "folded_plain", slabs=slabs, combine=combine,
              stats=True, res=True)
    CHUNKS_IN[c.tag] = chunks_in
    return c


def _rows():
    x, out = HC._x, []
    out += [
        _fold("pro_fold1_c1_b1_8x8", 1, 128, 128, 8, 8, 1, FOLD6, True, 1, _GM % 32),
        _fold("pro_fold1_c2_b2_8x24", 2, 128, 128, 8, 24, 2, FOLD6, False, 1, _GM % 32),
        _fold("pro_fold1_c8_b2_16x16", 2, 128, 128, 16, 16, 8, FOLD6, True, 1, _GM % 32),
        _fold("pro_fold1_c9_b1_8x24", 1, 128, 128, 8, 24, 9, FOLD6, True, 1, _GM % 32),
        _fold("pro_fold1_c16_b2_32x32", 2, 128, 128, 32, 32, 16, FOLD6, False, 1, _GM % 16),
        _fold("pro_fold2_c1_b2_8x8", 2, 256, 128, 8, 8, 1, FOLD6, False, 2, _GM % 32),
        _fold("pro_fold2_c8_b1_8x24", 1, 256, 128, 8, 24, 8, FOLD6, True, 2, _GM % 32),
        _fold("pro_fold2_c9_b2_16x16", 2, 256, 128, 16, 16, 9, FOLD6, True, 2, _GM % 32),
        _fold("pro_fold2_c16_b1_32x32", 1, 256, 128, 32, 32, 16, FOLD6, True, 2, _GM % 16),
        _fold("pro_fold1_ring3_grid640", 5, 128, 256, 32, 32, 16, FOLD3, True, 1, _GM % 16),
        _fold("pro_fold2_ring3_grid640", 5, 256, 256, 32, 32, 9, FOLD3, False, 2, _GM % 16),
    ]
    # table form: (kernel fragment, plan at 128 inputs, Cout, H, W, plan at 1024 inputs, combine)
    for frag, plan, cout, H, W, big_plan, combine in (
            ("64,64,true", (64, 64, 1), 128, 8, 8, (64, 64, 1), None),
            ("64,128,true", (64, 128, 4), 128, 8, 8, (64, 128, 32), _GM % 32),              # one slab per workgroup: the ring of three
            ("64,128,true,false,false,6", (64, 128, 1), 128, 8, 8, (64, 128, 1), None),
            ("128,128,true", (128, 128, 1), 128, 8, 16, (128, 128, 1), None),
            ("128,32,true", (128, 32, 1), 4, 8, 16, (128, 32, 1), None)):
        n = "pro_tab" + frag.split(",true")[0].replace(",", "x") + ("_ring6" if frag.endswith("6") else "")
        st = cout >= 128
        out += [
            x(n + "_c128_table", 2, 128, cout, H, W, plan, frag, gn="table", slabs=128 // 32 // plan[2], combine=combine, stats=st, res=True),
            x(n + "_c128_swish", 2, 128, cout, H, W, plan, frag, gn="swish", slabs=128 // 32 // plan[2], combine=combine, stats=st),
            x(n + "_c1024_swish", 2, 1024, cout, H, W, big_plan, frag, gn="swish", slabs=1024 // 32 // big_plan[2], combine=combine, stats=st,
              res=True),
        ]
    out.append(x("pro_tab64x128_ring6_c1024_table", 2, 1024, 128, 8, 8, (64, 128, 1), "64,128,true,false,false,6", gn="table", slabs=32,
                 stats=True))
    # the combines the folding and table rows do not reach (shapes of tests/halo_cases.py)
    out += [
        x("pro_combine_rowmajor", 1, 128, 384, 16, 16, (64, 128, 2), "64,128,false", slabs=2, combine=HC._XRM, res=True),
        x("pro_combine_rowmajor_stats", 1, 64, 128, 64, 64, (64, 128, 2), "64,128,false", slabs=1, combine=HC._XRM, stats=True, res=True),
        x("pro_combine_gm8", 1, 64, 128, 32, 64, (64, 128, 2), "64,128,false", slabs=1, combine=_GM % 8, stats=True),
    ]
    return out


ROWS = _rows()
XG = "conv_gemm_f32x_kernel<64,64,false,false>"
# the generic kernel as the encoder's Downsample (3 x 3, stride 2, padding bottom / right): 16 x 16 x 128 -> 8 x 8 x 128; T = 2 B ksplit
GENERIC = [dict(id="generic-pro_s2_b2_T4", B=2, ksplit=1, T=4), dict(id="generic-pro_s2_b3_split2_T12", B=3, ksplit=2, T=12),
           dict(id="generic-pro_s2_b5_split2_T20", B=5, ksplit=2, T=20)]


def cases():
    out = [dict(id=c.tag, kind="halo", kernel=c.kernel, combine=c.combine) for c in ROWS]
    out += [dict(g, kind="generic", kernel=XG, combine="splitk_reduce" if g["ksplit"] > 1 else None) for g in GENERIC]
    return out


def _row(tag):
    return next(c for c in ROWS if c.tag == tag)


def grid_of(c):
    """workgroups of the row's main launch: M tiles x N tiles x split"""
    bm, bn, ks = c.runs or c.plan
    return (c.B * c.Ho * c.Wo // bm) * (c.N // bn) * ks


def _partials(c, dev):
    """seeded chunk partials [B][chunks_in][32][2] fp64 {sum, sum of squares} of a map of c.H x c.W x c.Cin: every chunk holds an equal
    share of the pixels, with a mean and a variance of its own per (image, chunk, group)"""
    n, t = CHUNKS_IN[c.tag], "pro." + c.tag
    per_chunk = c.H * c.W * (c.Cin // 32) / n
    mean = 0.2 + 0.3 * testing.seeded_tensor(t + ".pmean", (c.B, n, 32)).double()
    var = 0.5 + testing.seeded_tensor(t + ".pvar", (c.B, n, 32)).double().abs()
    return torch.stack([per_chunk * mean, per_chunk * (var + mean * mean)], dim=3).contiguous().reshape(-1).to(dev)


def _run_halo(case, dev):
    c = _row(case["id"])
    with HC.forced_plan(c):
        o = EPI._halo_operands(c, dev)
        gn = None
        if c.folded:
            gn = ((_partials(c, dev), CHUNKS_IN[c.tag]), o["g"], o["bt"], c.swish, 1e-6)
        elif c.gn:
            gn = (RA._mean_rstd(c, dev), o["g"], o["bt"], c.swish)
        return RA._record(c, lambda: EPI._conv(c, o, o["x"], o["wp"], o["bias"], o["res"], gn=gn))


class _Generic:
    """what RA._record reads off a row, for the generic kernel's cases"""
    def __init__(self, g):
        self.B, self.ksplit, self.Ho, self.Wo, self.N = g["B"], g["ksplit"], 8, 8, 128


def _run_generic(case, dev):
    B, C, H, t = case["B"], 128, 16, "pro." + case["id"]
    x = EPI._nhwc(testing.seeded_tensor(t + ".x", (B, C, H, H), 1.0, 0.2), dev)
    w = testing.seeded_tensor(t + ".w", (C, C, 3, 3), scale=(1.0 / (C * 9)) ** 0.5)
    wp = ops.pack_conv_weight(w.to(dev), dtype="f32x")
    bias = (0.05 + testing.seeded_tensor(t + ".bias", (C,), scale=0.1)).to(dev)
    res = EPI._nhwc(testing.seeded_tensor(t + ".r", (B, C, H // 2, H // 2)), dev)

    def call():
        out = torch.empty((B, H // 2, H // 2, C), device=dev, dtype=torch.float32)
        d = ConvDesc(B=B, Hi=H, Wi=H, Cin=C, Ho=H // 2, Wo=H // 2, N=wp.shape[0], KH=3, KW=3, stride=2, pad_t=0, pad_l=0, upsample2x=0,
                     lda=C, ldb=wp.stride(0), ldc=C, ldr=C, n_valid=C, bias_per_row=0)
        d.plan_bm, d.plan_bn, d.plan_ksplit = 64, 64, case["ksplit"]
        return ops._run_conv(d, x, wp, bias, res, out)
    return RA._record(_Generic(case), call)


def run_case(case, dev="cuda"):
    """-> dict(kernels, out, stats, ws) of one case on the GPU, in split mode"""
    old = ops.F32_MODE
    ops.set_f32_mode("split")
    try:
        with torch.no_grad():
            return (_run_halo if case["kind"] == "halo" else _run_generic)(case, dev)
    finally:
        ops.set_f32_mode(old)


reaches = EPI.reaches


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    lib = _lib.load()
    doc = {"recorded_from": lib.sgam_build_commit().decode(), "lib_digest": lib.sgam_build_digest().decode(), "cases": {}}
    for case in cases():
        first, rec = run_case(case), run_case(case)
        assert first == rec, f"{case['id']}: two runs differ: {first} {rec}"
        assert reaches(case, rec), f"{case['id']}: wanted {case['kernel']} / {case['combine']}, ran {rec['kernels']}"
        assert (rec["ws"] is not None) == (case["combine"] is not None), case["id"]
        doc["cases"][case["id"]] = rec
        print(case["id"], rec["kernels"], flush=True)
    with open(args.out, "w") as f:
        rows = ",\n".join(f"{json.dumps(cid)}: {json.dumps(rec)}" for cid, rec in doc["cases"].items())
        f.write('{"recorded_from": %s, "lib_digest": %s,\n"cases": {\n%s\n}}\n'
                % (json.dumps(doc["recorded_from"]), json.dumps(doc["lib_digest"]), rows))
    print("wrote", args.out, "from", doc["recorded_from"], doc["lib_digest"])


if __name__ == "__main__":
    main()
