"""GPU: every member of the two halo-staged 3x3 convolution families (csrc/conv_f32x.hip: conv3x3_f32x_halo2_kernel, csrc/h16_halo.hip:
conv3x3_h16_halo_kernel) and of their split-K combines, one row of tests/halo_cases.py each, at the smallest shape that reaches it.

Per row: the result against the same operation in float64 on the CPU (16-bit rows: on the 16-bit-rounded operands, the staged
operand rounded once after GroupNorm — the definition of tests/test_gpu_h16.py), the kernel the row names in the launch timeline,
the GroupNorm statistics that leave with the output against the stored tensor, and a bit-identical second call.  Tolerances are
the project's own for these kernels (test_gpu_ops.py, test_gpu_h16.py); every figure is printed (`HALO_ERR row class error bound`)
before it is asserted.  tests/test_halo_cases_cpu.py proves the table itself without a GPU.

Measured on an MI355X when the file was written (largest error of all rows / the bound): split fp32 against float64 1.2e-6 / 2e-5,
fused against two-pass 2.4e-7 / 2e-6, folded against explicit 9.2e-8 / 3e-6; 16-bit output bf16 2.9e-3 / 5.9e-3, fp16 4.2e-4 /
7.3e-4; fp32-output form 4.8e-7 / 2e-5; 16-bit fused GroupNorm bf16 3.3e-3 / 1.6e-2, fp16 4.1e-4 / 2.0e-3; travelling statistics
mean 5.9e-8 / 2e-6 (16-bit 8.2e-8 / 1e-5), rstd 6.9e-8 / 2e-6 (16-bit 9.2e-8 / 1e-5).  The file takes 6.5 s (119 tests; 0.42 s for
the first row, which loads the library, 0.17 s for the B = 5 pair, under 0.1 s for every other)."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from sgam_neurips22_amd import _lib, ops, testing

sys.path.insert(0, os.path.dirname(__file__))
import halo_cases as HC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = {torch.bfloat16: 2 ** -8, torch.float16: 2 ** -11}
RES_AT = 32         # first channel of a pitched residual inside its wider tensor


@pytest.fixture(autouse=True)
def _split_mode():
    old = ops.F32_MODE
    ops.set_f32_mode("split")
    yield
    ops.set_f32_mode(old)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw64(y):
    return y.detach().float().permute(0, 3, 1, 2).cpu().double()


def _check(case, what, err, bound):
    print(f"HALO_ERR {case.tag} {what} {err:.3e} {bound:.3e}")
    assert err <= bound, f"{case.tag}: {what}: {err:.3e} > {bound:.3e}"


def _maxerr(a, b):
    return (a - b).abs().max().item()


class Operands:
    """seeded operands of a row: CPU masters (NCHW, in the row's type) and their device forms"""

    def __init__(self, case):
        self.case, self.dt = case, HC.TORCH_DTYPE[case.family]
        c, dt, t = case, self.dt, case.tag
        x = testing.seeded_tensor(t + ".x", (c.B, c.Cin, c.H, c.W), 1.0, 0.4)          # non-zero mean: zero padding is post-norm
        for b in range(c.B):                                                            # every image its own scale and shift
            x[b] = x[b] * (1.0 + 0.25 * b) + 0.3 * b
        self.x = x.to(dt)
        self.w = testing.seeded_tensor(t + ".w", (c.Cout, c.Cin, 3, 3), scale=(1.0 / (c.Cin * 9)) ** 0.5)
        self.bias = 0.05 + testing.seeded_tensor(t + ".bias", (c.Cout,), scale=0.1)
        self.g = 1 + 0.1 * testing.seeded_tensor(t + ".g", (c.Cin,))
        self.bt = 0.1 * testing.seeded_tensor(t + ".bt", (c.Cin,))
        self.res = testing.seeded_tensor(t + ".r", (c.B, c.Cout, c.Ho, c.Wo)).to(dt) if c.res else None
        self.xd = self._pitched(_nhwc(self.x), c.cin_pitch, 0, 100.0)
        self.rd = None if self.res is None else self._pitched(_nhwc(self.res), c.res_pitch, RES_AT, -50.0)
        self.wp = self.pack(self.w)
        self.bias_d, self.g_d, self.bt_d = self.bias.to(DEV), self.g.to(DEV), self.bt.to(DEV)

    @staticmethod
    def _pitched(t, pitch, at, filler):
        """the device tensor — or, with a pitch, a channel slice of a wider one whose other channels hold a value that no result survives"""
        if not pitch:
            return t.to(DEV)
        wide = torch.full(tuple(t.shape[:3]) + (pitch,), filler, dtype=t.dtype)
        wide[..., at:at + t.shape[3]] = t
        return wide.to(DEV)[..., at:at + t.shape[3]]

    def pack(self, w):
        c = self.case
        if c.family == "f32x":
            wp = ops.pack_conv_weight(w.to(DEV), cout_pad=c.cout_pad, dtype="f32x")
        else:
            wp = ops.pack_conv_weight(w.to(DEV), dtype=self.dt)
            wp._sgam_frag_src = w.to(DEV)
        assert wp.shape[0] == c.N and wp.stride(0) == 9 * c.Cin, "the row's descriptor is the one ops.conv2d_nhwc builds"
        return wp

    def conv(self, x, wp, bias, residual, **kw):
        c = self.case
        return ops.conv2d_nhwc(x, wp, bias, cout=c.Cout, kh=3, kw=3, pad_t=1, pad_l=1, upsample2x=c.ups, residual=residual,
                               out_dtype=torch.float32 if c.out32 else None, **kw)

    def reference(self, x, w, bias, res, gn):
        """float64: GroupNorm(+swish) of x, nearest-2x, conv, bias, residual.  x NCHW on the CPU in the row's type"""
        c, dt = self.case, self.dt
        swish = c.swish
        if c.family == "f32x":
            h = x.double()
            if gn:
                h = F.group_norm(h, 32, self.g.double(), self.bt.double(), eps=1e-6)
                h = h * torch.sigmoid(h) if swish else h
            wd = w.double()
        else:
            h = x.float()
            if gn:
                h = F.group_norm(h, 32, self.g, self.bt, eps=1e-6)
                h = (h * torch.sigmoid(h) if swish else h).to(dt).float()        # the staged operand is rounded once to 16 bits
            h, wd = h.double(), w.to(dt).double()
        if c.ups:
            h = F.interpolate(h, scale_factor=2.0, mode="nearest")
        ref = F.conv2d(h, wd, None if bias is None else bias.double(), padding=1)
        return ref if res is None else ref + res.double()


def _check_result(case, what, out, ref, fused_gn):
    """the project's tolerance for this family and form"""
    dt = HC.TORCH_DTYPE[case.family]
    scale = ref.abs().max().item()
    err = _maxerr(_nchw64(out), ref)
    if case.family == "f32x":
        _check(case, f"f32x_vs_fp64:{what}", err / max(1.0, scale), 2e-5)
    elif case.out32:
        _check(case, f"h16_f32out_vs_fp64:{what}", err / scale, 2e-5)
    elif fused_gn:
        _check(case, f"h16_fused_gn_vs_fp64:{what}", err / scale, 4 * EPS[dt])
    else:
        _check(case, f"h16_vs_fp64:{what}", err / scale, 1.5 * EPS[dt])


def _check_statistics(case, what, out, expect):
    """the chunk statistics that left with `out` (or, without them, the statistics pass) against the stored tensor in float64,
    and GroupNorm + swish of `out` against its copy without statistics and against torch"""
    c, dt = case, HC.TORCH_DTYPE[case.family]
    st = ops.gn_stats(out)
    # a row that expects statistics must carry them; one that does not (Cout = 384) ends in one of two states: no statistics and
    # a right statistics pass, or statistics that pass the very same checks
    assert st is not None or not expect, f"{c.tag}: the statistics did not leave with the output"
    src = "chunks" if st is not None else "pass"
    tol_m, tol_r = (2e-6, 2e-6) if c.family == "f32x" else (1e-5, 1e-5)
    o64 = _nchw64(out)
    og = o64.reshape(c.B, 32, -1)
    mr = ops.groupnorm_meanrstd(out).cpu().double()
    rstd = (og.var(-1, unbiased=False) + 1e-6).rsqrt()
    _check(c, f"stats_mean_{src}:{what}", _maxerr(mr[:, :, 0], og.mean(-1)), tol_m)
    _check(c, f"stats_rstd_{src}:{what}", ((mr[:, :, 1] - rstd).abs() / rstd).max().item(), tol_r)
    g = (1 + 0.1 * testing.seeded_tensor(c.tag + ".g2", (c.Cout,)))
    bt = 0.1 * testing.seeded_tensor(c.tag + ".bt2", (c.Cout,))
    y = ops.groupnorm_nhwc(out, g.to(DEV), bt.to(DEV), True)
    y2 = ops.groupnorm_nhwc(out.clone(), g.to(DEV), bt.to(DEV), True)             # the copy carries no statistics
    ref = F.group_norm(o64, 32, g.double(), bt.double(), eps=1e-6)
    ref = ref * torch.sigmoid(ref)
    scale = ref.abs().max().item()
    if c.family == "f32x":
        _check(c, f"gn_f32_vs_torch:{what}", _maxerr(_nchw64(y), ref) / max(1.0, scale), 2e-5)
        _check(c, f"gn_f32_vs_copy:{what}", _maxerr(y, y2) / scale, 2e-6)
    else:
        _check(c, f"gn_h16_vs_torch:{what}", _maxerr(_nchw64(y), ref) / scale, 1.5 * EPS[dt])
        _check(c, f"gn_h16_vs_copy:{what}", _maxerr(y.float(), y2.float()) / scale, 2 * EPS[dt])


def _check_variant(case, recs):
    names = [r[0] for r in recs]
    halo = [n for n in names if "halo" in n and "kernel<" in n]
    assert len(halo) == 1 and case.kernel in halo[0], f"{case.tag}: wanted {case.kernel}, ran {names}"
    combine = [n for n in names if "splitk_reduce" in n]
    if case.combine:
        assert len(combine) == 1 and case.combine in combine[0], f"{case.tag}: wanted {case.combine}, ran {names}"
    else:
        assert combine == [], names


def _same(a, b):
    sa, sb = ops.gn_stats(a), ops.gn_stats(b)
    return torch.equal(a, b) and (sa is None) == (sb is None) and (sa is None or (sa[1] == sb[1] and torch.equal(sa[0], sb[0])))


def _run_single(case):
    o = Operands(case)
    swish = case.swish
    with HC.forced_plan(case):
        gn = None if case.gn is None else (ops.groupnorm_meanrstd(o.xd), o.g_d, o.bt_d, swish)

        def call():
            return o.conv(o.xd, o.wp, o.bias_d, o.rd, gn=gn)
        out = call()
        recs, _ = ops.kernel_timeline(call)
        again = call()
        two_pass = o.conv(ops.groupnorm_nhwc(o.xd, o.g_d, o.bt_d, swish), o.wp, o.bias_d, o.rd) if case.gn and case.family == "f32x" else None
    assert out.dtype == (torch.float32 if case.out32 else o.dt) and tuple(out.shape) == (case.B, case.Ho, case.Wo, case.Cout)
    ref = o.reference(o.x, o.w, o.bias, o.res, case.gn)
    _check_result(case, "out", out, ref, fused_gn=case.gn is not None)
    if two_pass is not None:
        _check_result(case, "two_pass", two_pass, ref, fused_gn=False)
        _check(case, "f32x_fused_vs_two_pass", _maxerr(out, two_pass) / ref.abs().max().item(), 2e-6)
    _check_variant(case, recs)
    if case.Cout % 128 == 0 and not case.out32:
        _check_statistics(case, "out", out, case.stats)
    else:
        assert ops.gn_stats(out) is None and not case.stats
    assert _same(out, again), f"{case.tag}: a second call differs"


def _run_folded_pair(case):
    """producer (plain conv + residual through the split-K combine, which leaves <= 16 chunk partials per image) and consumer
    (GroupNorm + swish folded from those partials while it stages) of the row's shape"""
    o = Operands(case)
    dt = o.dt
    w1 = testing.seeded_tensor(case.tag + ".w1", (case.Cin, case.Cin, 3, 3), scale=(1.0 / (case.Cin * 9)) ** 0.5)
    r1 = testing.seeded_tensor(case.tag + ".r1", (case.B, case.Cin, case.H, case.W)).to(dt)
    wp1, r1d = o.pack(w1), _nhwc(r1).to(DEV)
    norm = (o.g_d, o.bt_d, case.swish, 32, 1e-6)
    with HC.forced_plan(case):
        h = o.conv(o.xd, wp1, None, r1d)
        assert ops.gn_stats(h) is not None and 1 <= ops.gn_stats(h)[1] <= 16

        def call():
            return o.conv(h, o.wp, o.bias_d, o.rd, norm=norm)
        out = call()
        recs, _ = ops.kernel_timeline(call)
        again = call()
        if case.family == "f32x":
            explicit = o.conv(ops.groupnorm_nhwc(h.clone(), o.g_d, o.bt_d, case.swish), o.wp, o.bias_d, o.rd)
        else:
            explicit = o.conv(h.clone(), o.wp, o.bias_d, o.rd, norm=norm)        # statistics pass + fold + table form
    _check_result(case, "producer", h, o.reference(o.x, w1, None, r1, None), fused_gn=False)
    _check_statistics(case, "producer", h, True)
    ref = o.reference(_nchw64(h).to(dt), o.w, o.bias, o.res, case.gn)
    _check_result(case, "out", out, ref, fused_gn=True)
    scale = explicit.float().abs().max().item()
    if case.family == "f32x":
        _check(case, "f32x_folded_vs_explicit", _maxerr(out, explicit) / scale, 3e-6)
    else:
        _check(case, "h16_folded_vs_explicit", _maxerr(out.float(), explicit.float()) / scale, 2 * EPS[dt])
    _check_variant(case, recs)
    _check_statistics(case, "out", out, case.stats)
    assert _same(out, again), f"{case.tag}: a second call differs"


@pytest.mark.parametrize("case", HC.CASES, ids=str)
def test_halo_conv_row(case):
    (_run_folded_pair if case.folded else _run_single)(case)


@pytest.mark.parametrize("family", ["f32x", "bf16", "fp16"])
@pytest.mark.parametrize("C,H,W", [(384, 16, 16), (384, 36, 36), (640, 8, 8)], ids=["384_small_map", "384_chunked", "640_small_map"])
def test_groupnorm_of_a_width_whose_groups_are_not_whole_vectors(family, C, H, W):
    """the statistics pass the Cout = 384 layers fall back to: GroupNorm(+swish) of 12 / 20 channels per group (a `ch_mult` with a
    3 or a 5) in the one-launch form of the small maps and in the chunked form, against torch in float64.  (A 16-bit group of 12
    channels is one and a half 16-byte vectors: the one-launch kernel used to normalise eight of them and leave four unwritten;
    the chunked form's apply pass keeps a lane on one column only while its stride is a multiple of the C / 8 (C / 4) vectors
    of a pixel, which the launch now sees to for 48, 80 or 96 of them.)"""
    dt = HC.TORCH_DTYPE[family]
    x = testing.seeded_tensor(f"gn{C}.x", (2, C, H, W), 1.5, 0.4)
    x[1] = x[1] * 0.5 - 0.7
    x = x.to(dt)
    g, bt = 1 + 0.1 * testing.seeded_tensor(f"gn{C}.g", (C,)), 0.1 * testing.seeded_tensor(f"gn{C}.bt", (C,))
    xd = _nhwc(x).to(DEV)
    for swish in (False, True):
        y = ops.groupnorm_nhwc(xd, g.to(DEV), bt.to(DEV), swish)
        ref = F.group_norm(x.double(), 32, g.double(), bt.double(), eps=1e-6)
        ref = ref * torch.sigmoid(ref) if swish else ref
        err, scale = _maxerr(_nchw64(y), ref), ref.abs().max().item()
        assert y.dtype == dt
        print(f"HALO_ERR {family}-gn{C}_{H}x{W}_swish{int(swish)} gn_vs_torch {err / max(1.0, scale):.3e}")
        assert err <= (2e-5 * max(1.0, scale) if family == "f32x" else 1.5 * EPS[dt] * scale)
    mr = ops.groupnorm_meanrstd(xd).cpu().double()
    og = x.double().reshape(2, 32, -1)
    tol = 2e-6 if family == "f32x" else 1e-5
    rstd = (og.var(-1, unbiased=False) + 1e-6).rsqrt()
    assert _maxerr(mr[:, :, 0], og.mean(-1)) <= tol and ((mr[:, :, 1] - rstd).abs() / rstd).max().item() <= tol


@pytest.mark.parametrize("tag", ["f32x-out384_tile64_b1", "f32x-out384_tile128_b2", "bf16-out384_t128", "fp16-out384_t128"])
def test_stats_entry_points_refuse_partials_where_groups_straddle_wavefronts(tag):
    """a whole-K descriptor with 12 channels per group is promised no chunk statistics (test_halo_cases_cpu.py); the entry points
    refuse a statistics buffer for it without launching, and run the same arguments without one"""
    case = next(c for c in HC.CASES if c.tag == tag)
    lib, o, d = _lib.load(), Operands(case), HC.desc(case)
    out = torch.empty((case.B, case.Ho, case.Wo, case.Cout), device=DEV, dtype=o.dt)
    partial = torch.zeros((case.B * 16 * 32 * 2,), device=DEV, dtype=torch.float64)
    p, s = ops._p, ops._stream()
    if case.family == "f32x":
        tail = (p(o.wp.planes), float(o.wp.scale), None, None, p(out))
        assert lib.sgam_conv2d_stats_nhwc_f32x(ctypes.byref(d), p(o.xd), 1.0, *tail, p(partial), None, 0, s) == -1
        assert lib.sgam_conv2d_nhwc_f32x(ctypes.byref(d), p(o.xd), 1.0, *tail, None, 0, s) == 0
    else:
        fw = ops._h16_frag(o.wp, d)
        head = (ctypes.byref(d), ops.H16[o.dt], p(o.xd), None, None, None, 0, p(fw.planes), None, None, p(out), 0)
        assert lib.sgam_conv2d_halo_nhwc_h16(*head, p(partial), None, 0, s) == -1
        assert lib.sgam_conv2d_halo_nhwc_h16(*head, None, None, 0, s) == 0
    torch.cuda.synchronize()
    ref = o.reference(o.x, o.w, None, None, None)
    _check_result(case, "raw_abi", out, ref, fused_gn=False)
