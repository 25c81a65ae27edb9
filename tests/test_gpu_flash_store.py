"""GPU: how the split-fp32 frame's big writers store may change (width, cache policy), what they store may not.

tests/golden/flash_partial_hashes.json was recorded by scripts/record_flash_partial_hashes.py from a build of the commit in front of
the store-policy change (the file names that commit and the digest of the library that ran); it is not re-recorded from the code
under test.  Every row is replayed here: the sha256 of what ops.attention / ops.attention_proj return (both merges read the flash
kernel's partial O^T tiles back), the statistics that leave with the fused projection and the kernel names of the launch timeline
are the recorded ones.  (The variant of attn_flash_f32x_kernel that transposes its tile through LDS and stores sixteen-byte pieces
passed these rows and was not kept: profiles/HISTORY.md, "store policy".)

The second half replays captured chains through the sixteen-byte store site whose cache policy is a compile-time constant
(csrc/conv_f32x.hip: XST_AUX, write-through) — the FINAL output of each of the three halo tiles in a whole-K launch (no combine in the
chain, asserted by name), read by gn_finalize and a GroupNorm conv; split-K partial tiles read by the group-major combine whose output
a folding conv reads — at the smallest shapes that reach each tile: a launch that follows a
write-through store must see it exactly as it sees a write-back at the kernel boundary, twenty replays over, bit for bit what the
eager launches gave."""
import contextlib
import importlib.util
import json
import os

import pytest
import torch

from sgam_neurips22_amd import ops, testing
from sgam_neurips22_amd._lib import ConvDesc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_flash_partial_hashes", os.path.join(ROOT, "scripts", "record_flash_partial_hashes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
with open(REC.FIXTURE) as _f:
    DOC = json.load(_f)
FIX = DOC["cases"]
DEV = "cuda"

pytestmark = pytest.mark.gpu


def test_the_file_names_its_source_and_holds_every_case():
    assert DOC["recorded_from"] and len(DOC["lib_digest"]) == 12
    assert [c["id"] for c in REC.cases()] == list(FIX)
    assert all(REC.reaches(c, FIX[c["id"]]) for c in REC.cases())


@pytest.mark.parametrize("case", REC.cases(), ids=lambda c: c["id"])
def test_attention_result_and_kernels_are_the_recorded_ones(case):
    want, got = FIX[case["id"]], REC.run_case(case)
    assert got["kernels"] == want["kernels"]
    assert sum(REC.FLASH in k for k in got["kernels"]) == 1 and REC.reaches(case, got)
    assert got["out"] == want["out"]
    assert got["stats"] == want["stats"]


def _conv_operands(tag, C, H=16):
    x = testing.seeded_tensor(tag + ".x", (1, H, H, C), 1.0, 0.3).to(DEV)
    ws = [ops.pack_conv_weight(testing.seeded_tensor(f"{tag}.w{i}", (C, C, 3, 3), scale=(1.0 / (C * 9)) ** 0.5).to(DEV), dtype="f32x")
          for i in range(2)]
    bias = (0.05 + testing.seeded_tensor(tag + ".b", (C,), scale=0.1)).to(DEV)
    g, bt = (1 + 0.1 * testing.seeded_tensor(tag + ".g", (C,))).to(DEV), (0.1 * testing.seeded_tensor(tag + ".bt", (C,))).to(DEV)
    conv = lambda h, w, **kw: ops.conv2d_nhwc(h, w, bias, cout=C, kh=3, kw=3, pad_t=1, pad_l=1, **kw)  # noqa: E731
    return x, ws, g, bt, conv


@contextlib.contextmanager
def _plan(H, C, plan):
    """ops.PLAN_CACHE[key of the 3x3 C -> C conv on an H x H map] = plan for the duration of the block (None: the plan it has)"""
    d = ConvDesc(B=1, Hi=H, Wi=H, Cin=C, Ho=H, Wo=H, N=C, KH=3, KW=3, stride=1, pad_t=1, pad_l=1, upsample2x=0, lda=C, ldb=9 * C, ldc=C,
                 ldr=0, n_valid=C, bias_per_row=0)
    key, old = ops.plan_key(d, "f32x"), None
    if plan is not None:
        old = ops.PLAN_CACHE.get(key)
        ops.PLAN_CACHE[key] = tuple(plan)
    try:
        yield
    finally:
        if plan is not None:
            if old is None:
                ops.PLAN_CACHE.pop(key, None)
            else:
                ops.PLAN_CACHE[key] = old


def _final_output_chain(H, tile):
    """conv -> gn_finalize_stats -> GroupNorm conv on H x H x 128, whole K in one launch: the tile kernel `tile` stores its FINAL output
    (and the statistics from its epilogue), read by the two launches behind it; no partial tile, no combine"""
    x, ws, g, bt, conv = _conv_operands(f"fs.c128.{H}", 128, H)

    def run():
        h = conv(x, ws[0])
        return conv(h, ws[1], gn=(ops.groupnorm_meanrstd(h), g, bt, True))
    return run, lambda names: (sum("conv3x3_f32x_halo2_kernel<" + tile in k for k in names) == 2
                               and sum("gn_finalize_stats_kernel" in k for k in names) == 1 and len(names) == 3
                               and not any("splitk_reduce" in k for k in names))


def _splitk_chain():
    """split-K conv -> group-major combine -> conv that folds the combine's chunk statistics itself, at 16^2 x 512"""
    x, ws, g, bt, conv = _conv_operands("fs.c512", 512)

    def run():
        return conv(conv(x, ws[0]), ws[1], norm=(g, bt, True, 32, 1e-6))
    return run, lambda names: (sum("conv3x3_f32x_halo2_kernel" in k for k in names) == 2
                               and sum("splitk_reduce_gm_f32x_kernel" in k for k in names) == 2
                               and not any("gn_finalize" in k or "gn_small" in k or "gn_apply" in k for k in names))


# (id, map, channels, plan forced for the duration or None, chain): the whole-K rows are the three tiles that store final outputs —
# the 64 x 64 tile at the smallest map (its own plan there is split-K 4, so whole K is pinned), the 64 x 128 tile under its tuned
# plan at 128^2 (many tile waves) and the 128 x 128 tile at 256^2 (one tile wave, 33.5 MB stored in the launch's last microseconds)
CHAINS = [("final_output_16x16x128_tile64x64_whole_k", 16, 128, (64, 64, 1), lambda: _final_output_chain(16, "64,64,")),
          ("final_output_128x128x128_tile64x128", 128, 128, None, lambda: _final_output_chain(128, "64,128,")),
          ("final_output_256x256x128_tile128x128", 256, 128, None, lambda: _final_output_chain(256, "128,128,")),
          ("splitk_partials_16x16x512", 16, 512, None, _splitk_chain)]


@pytest.mark.parametrize("H,C,plan,chain", [c[1:] for c in CHAINS], ids=[c[0] for c in CHAINS])
def test_a_captured_chain_replays_the_eager_bits_twenty_times(H, C, plan, chain):
    old = ops.F32_MODE
    ops.set_f32_mode("split")
    try:
        with torch.no_grad(), _plan(H, C, plan):
            run, names_ok = chain()
            eager = run()
            recs, _ = ops.kernel_timeline(run)
            names = [r[0] for r in recs]
            assert names_ok(names), names
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = run()
            for i in range(20):
                g.replay()
                assert torch.equal(out, eager), f"replay {i} differs from the eager result"
            st, st_eager = ops.gn_stats(out), ops.gn_stats(eager)
            assert (st is None) == (st_eager is None) and (st is None or torch.equal(st[0], st_eager[0]))
    finally:
        ops.set_f32_mode(old)
