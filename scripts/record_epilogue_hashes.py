"""Record what the split-fp32 tile kernels' epilogues write into tests/golden/epilogue_f32x_hashes.json.

The epilogue shared by conv3x3_f32x_halo2_kernel / conv_gemm_f32x_kernel (csrc/conv_f32x.hip: xepilogue) and the one of
gemm_gn_f32x_kernel (csrc/gemm_gn_f32x.hip) may be rescheduled, never change a bit: per case of `cases()` the file holds the
kernel names of ops.kernel_timeline, the sha256 of the output and the (chunks, sha256) of the GroupNorm chunk statistics that
leave with it.  tests/test_gpu_epilogue_f32x.py replays the cases against the file.

The file is recorded from a build of the commit BEFORE a change to those epilogues and names that build (`recorded_from`,
`lib_digest`: sgam_build_commit / sgam_build_digest of the library that ran).  It is never re-recorded from the code under test:

    SGAM_LIB_DIR=<dir> python -m sgam_neurips22_amd.build          # in a checkout of the earlier commit
    SGAM_HIP_LIB=<dir>/libsgam_hip.so python scripts/record_epilogue_hashes.py        (needs the GPU)

Rows: every split-fp32 row of tests/halo_cases.py (residual on / off, pitches, n_valid 4 and 32 on the 128 x 32 tile, 12-channel
groups without statistics, the split-K workspace form with all four combines, B > 1), one of them in place (out is the residual
tensor); conv_gemm_f32x_kernel<64,64,false,false> as a 3x3 stride-2 convolution with asymmetric padding, whole K and split in
two, and as a GEMM of 72 rows (rows >= M masked) with a per-row bias + residual and with a per-column bias alone;
gemm_gn_f32x_kernel at (64, 128, 128) and (256, 512, 512) with / without residual and fused GroupNorm, with statistics, a
pitched residual, and out aliasing the residual.
"""
import argparse
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

FIXTURE = os.path.join(ROOT, "tests", "golden", "epilogue_f32x_hashes.json")
INPLACE_OF = "f32x-tile128_gn"          # the halo row that is also run with out = the residual tensor
GG = "gemm_gn_f32x_kernel<%s>"
XG = "conv_gemm_f32x_kernel<64,64,false,false>"


def _gg(name, M, N, K, gn, res, kernel, stats=True, res_pitch=0, alias=False):
    return dict(id=f"panel-{name}", kind="panel", combine=None, M=M, N=N, K=K, gn=gn, res=res, stats=stats, res_pitch=res_pitch, alias=alias,
                kernel=GG % kernel)


def cases():
    out = [dict(id=c.tag, kind="halo", kernel=c.kernel, combine=c.combine) for c in HC.F32X_CASES]
    out.append(dict(id=INPLACE_OF + "_inplace", kind="halo_inplace", kernel=_halo(INPLACE_OF).kernel, combine=None))
    out += [dict(id=f"generic-conv_s2_k{ks}", kind="conv_s2", ksplit=ks, kernel=XG, combine="splitk_reduce" if ks > 1 else None)
            for ks in (1, 2)]
    out += [dict(id="generic-gemm72_rowbias_res", kind="gemm72", bias_per_row=True, res=True, kernel=XG, combine=None),
            dict(id="generic-gemm72_colbias", kind="gemm72", bias_per_row=False, res=False, kernel=XG, combine=None)]
    for M, N, K, kc in ((64, 128, 128, 128), (256, 512, 512, 256)):
        for gn in (False, True):
            for res in (False, True):
                out.append(_gg(f"{M}x{N}x{K}_gn{int(gn)}_res{int(res)}", M, N, K, gn, res, f"{str(gn).lower()},{kc}"))
    out += [_gg("64x128x128_res_nostats", 64, 128, 128, False, True, "false,128", stats=False),
            _gg("64x128x128_res_pitch192", 64, 128, 128, False, True, "false,128", res_pitch=192),
            _gg("256x512x512_res_alias", 256, 512, 512, False, True, "false,256", alias=True),
            _gg("256x512x512_gn_res_alias", 256, 512, 512, True, True, "true,256", alias=True)]
    return out


def _halo(tag):
    return next(c for c in HC.F32X_CASES if c.tag == tag)


def _nhwc(x, dev):
    return x.permute(0, 2, 3, 1).contiguous().to(dev)


def _pitched(t, pitch, at, dev):
    """the device tensor — or, with a pitch, a channel slice of a wider one"""
    if not pitch:
        return t.to(dev)
    wide = torch.full(tuple(t.shape[:-1]) + (pitch,), -50.0, dtype=t.dtype)
    wide[..., at:at + t.shape[-1]] = t
    return wide.to(dev)[..., at:at + t.shape[-1]]


def _halo_operands(c, dev):
    t = "epi." + c.tag
    x = testing.seeded_tensor(t + ".x", (c.B, c.Cin, c.H, c.W), 1.0, 0.4)
    for b in range(c.B):
        x[b] = x[b] * (1.0 + 0.25 * b) + 0.3 * b
    w = testing.seeded_tensor(t + ".w", (c.Cout, c.Cin, 3, 3), scale=(1.0 / (c.Cin * 9)) ** 0.5)
    o = dict(x=_pitched(_nhwc(x, "cpu"), c.cin_pitch, 0, dev), wp=ops.pack_conv_weight(w.to(dev), cout_pad=c.cout_pad, dtype="f32x"),
             bias=(0.05 + testing.seeded_tensor(t + ".bias", (c.Cout,), scale=0.1)).to(dev),
             g=(1 + 0.1 * testing.seeded_tensor(t + ".g", (c.Cin,))).to(dev), bt=(0.1 * testing.seeded_tensor(t + ".bt", (c.Cin,))).to(dev),
             res=None)
    if c.res:
        o["res"] = _pitched(_nhwc(testing.seeded_tensor(t + ".r", (c.B, c.Cout, c.Ho, c.Wo)), "cpu"), c.res_pitch, 32, dev)
    return o


def _conv(c, o, x, wp, bias, res, **kw):
    return ops.conv2d_nhwc(x, wp, bias, cout=c.Cout, kh=3, kw=3, pad_t=1, pad_l=1, upsample2x=c.ups, residual=res, **kw)


def _run_halo(case, dev):
    c = _halo(case["id"])
    o = _halo_operands(c, dev)
    with HC.forced_plan(c):
        if c.folded:
            # producer (plain conv + residual through the split-K combine) and the consumer that folds its chunk partials
            w1 = testing.seeded_tensor("epi." + c.tag + ".w1", (c.Cin, c.Cin, 3, 3), scale=(1.0 / (c.Cin * 9)) ** 0.5)
            r1 = _nhwc(testing.seeded_tensor("epi." + c.tag + ".r1", (c.B, c.Cin, c.H, c.W)), dev)
            h = _conv(c, o, o["x"], ops.pack_conv_weight(w1.to(dev), dtype="f32x"), None, r1)
            return _record(lambda: _conv(c, o, h, o["wp"], o["bias"], o["res"], norm=(o["g"], o["bt"], c.swish, 32, 1e-6)), pre=h)
        gn = None if c.gn is None else (ops.groupnorm_meanrstd(o["x"]), o["g"], o["bt"], c.swish)
        return _record(lambda: _conv(c, o, o["x"], o["wp"], o["bias"], o["res"], gn=gn))


def _run_halo_inplace(case, dev):
    c = _halo(INPLACE_OF)
    o = _halo_operands(c, dev)
    gn = (ops.groupnorm_meanrstd(o["x"]), o["g"], o["bt"], c.swish)

    def call():
        buf = o["res"].clone()                  # the residual, overwritten by the result
        return ops._run_conv(HC.desc(c), o["x"], o["wp"], o["bias"], buf, buf, gn)
    return _record(call)


def _run_conv_s2(case, dev):
    """3x3, stride 2, padding on the bottom / right only (the encoder's Downsample): 16 x 16 x 128 -> 8 x 8 x 128, B = 2"""
    B, C, H = 2, 128, 16
    x = _nhwc(testing.seeded_tensor("epi.s2.x", (B, C, H, H), 1.0, 0.2), dev)
    w = testing.seeded_tensor("epi.s2.w", (C, C, 3, 3), scale=(1.0 / (C * 9)) ** 0.5)
    wp = ops.pack_conv_weight(w.to(dev), dtype="f32x")
    bias = (0.05 + testing.seeded_tensor("epi.s2.bias", (C,), scale=0.1)).to(dev)
    res = _nhwc(testing.seeded_tensor("epi.s2.r", (B, C, H // 2, H // 2)), dev)

    def call():
        out = torch.empty((B, H // 2, H // 2, C), device=dev, dtype=torch.float32)
        d = ConvDesc(B=B, Hi=H, Wi=H, Cin=C, Ho=H // 2, Wo=H // 2, N=wp.shape[0], KH=3, KW=3, stride=2, pad_t=0, pad_l=0, upsample2x=0,
                     lda=C, ldb=wp.stride(0), ldc=C, ldr=C, n_valid=C, bias_per_row=0)
        d.plan_bm, d.plan_bn, d.plan_ksplit = 64, 64, case["ksplit"]
        return ops._run_conv(d, x, wp, bias, res, out)
    return _record(call)


def _run_gemm72(case, dev):
    """out[72][128] = a[72][128] . w[128][128]^T on the 64 x 64 tile: the second row tile holds 8 rows"""
    M, N, K = 72, 128, 128
    a = testing.seeded_tensor("epi.g72.a", (M, K)).to(dev)
    w = ops.split_rows(testing.seeded_tensor("epi.g72.w", (N, K), scale=K ** -0.5).to(dev))
    bias = (0.05 + testing.seeded_tensor("epi.g72.bias", (M if case["bias_per_row"] else N,), scale=0.1)).to(dev)
    res = testing.seeded_tensor("epi.g72.r", (M, N)).to(dev) if case["res"] else None

    def call():
        out = torch.empty((M, N), device=dev, dtype=torch.float32)
        d = ConvDesc(B=1, Hi=1, Wi=M, Cin=K, Ho=1, Wo=M, N=N, KH=1, KW=1, stride=1, pad_t=0, pad_l=0, upsample2x=0, lda=K,
                     ldb=w.stride(0), ldc=N, ldr=N if case["res"] else 0, n_valid=N, bias_per_row=int(case["bias_per_row"]))
        d.plan_bm, d.plan_bn, d.plan_ksplit = 64, 64, 1
        return ops._run_conv(d, a, w, bias, res, out)
    return _record(call)


def _run_panel(case, dev):
    """the whole-K-panel kernel through its C entry point (ops reaches only some of these combinations); one image of M rows"""
    M, N, K, t = case["M"], case["N"], case["K"], "epi." + case["id"]
    lib, p = _lib.load(), ops._p
    x = testing.seeded_tensor(t + ".x", (M, K), 1.0, 0.3).to(dev)
    w = ops.split_rows(testing.seeded_tensor(t + ".w", (N, K), scale=K ** -0.5).to(dev))
    bias = (0.05 + testing.seeded_tensor(t + ".bias", (N,), scale=0.1)).to(dev)
    mr = g = bt = None
    if case["gn"]:
        mr = torch.stack([0.3 + 0.1 * testing.seeded_tensor(t + ".mean", (1, 32)),
                          1.0 + 0.1 * testing.seeded_tensor(t + ".rstd", (1, 32)).abs()], dim=2).contiguous().to(dev)
        g, bt = (1 + 0.1 * testing.seeded_tensor(t + ".g", (K,))).to(dev), (0.1 * testing.seeded_tensor(t + ".bt", (K,))).to(dev)
    res0 = _pitched(testing.seeded_tensor(t + ".r", (M, N)), case["res_pitch"], 32, dev) if case["res"] else None

    def call():
        res = res0.clone() if case["alias"] else res0
        out = res if case["alias"] else torch.empty((M, N), device=dev, dtype=torch.float32)
        chunks = M // 64 if case["stats"] else 0
        partial = torch.zeros((chunks * 32 * 2,), device=dev, dtype=torch.float64) if chunks else None
        ops.check(lib.sgam_gemm_panel_f32x(p(x), K, p(mr), p(g), p(bt), p(w.planes), float(w.scale), p(bias), p(res),
                                           res.stride(0) if res is not None else 0, p(out), N, p(partial), M, N, K, M, ops._stream()),
                  "sgam_gemm_panel_f32x")
        return ops._set_gn_stats(out, partial, chunks)
    return _record(call)


RUN = {"halo": _run_halo, "halo_inplace": _run_halo_inplace, "conv_s2": _run_conv_s2, "gemm72": _run_gemm72, "panel": _run_panel}


def run_case(case, dev="cuda"):
    """-> dict(kernels, out, stats[, pre]) of one case on the GPU, in split mode"""
    old = ops.F32_MODE
    ops.set_f32_mode("split")
    try:
        with torch.no_grad():
            return RUN[case["kind"]](case, dev)
    finally:
        ops.set_f32_mode(old)


def _record(fn, pre=None):
    box = []
    recs, _ = ops.kernel_timeline(lambda: box.append(fn()))
    out, st = box[0], ops.gn_stats(box[0])
    rec = dict(kernels=[r[0] for r in recs], out=testing.sha256(out).hex(),
               stats=None if st is None else [int(st[1]), testing.sha256(st[0]).hex()])
    if pre is not None:
        rec["pre"] = testing.sha256(pre).hex()
    return rec


def reaches(case, rec):
    """the launch the row exists for (and its split-K combine, or none) is among the row's kernels"""
    main = [k for k in rec["kernels"] if "splitk_reduce" not in k]
    comb = [k for k in rec["kernels"] if "splitk_reduce" in k]
    return (len(main) == 1 and case["kernel"] in main[0]
            and (len(comb) == 1 and case["combine"] in comb[0] if case["combine"] else comb == []))


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
        doc["cases"][case["id"]] = rec
        print(case["id"], rec["kernels"], flush=True)
    with open(args.out, "w") as f:
        rows = ",\n".join(f"{json.dumps(cid)}: {json.dumps(rec)}" for cid, rec in doc["cases"].items())
        f.write('{"recorded_from": %s, "lib_digest": %s,\n"cases": {\n%s\n}}\n'
                % (json.dumps(doc["recorded_from"]), json.dumps(doc["lib_digest"]), rows))
    print("wrote", args.out, "from", doc["recorded_from"], doc["lib_digest"])


if __name__ == "__main__":
    main()
