"""CPU: the rows of scripts/record_halo_prologue_hashes.py are what they say.  The planner entry points of the library work without
a device: every row's descriptor, tile, split, workspace, statistics, grid and folding expectations are proven here before any GPU
time is spent (tests/test_gpu_halo_prologue.py then replays the rows against the recorded hashes)."""
import ctypes
import importlib.util
import os
import sys

import pytest

from sgam_neurips22_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(__file__))
import halo_cases as HC  # noqa: E402

ref = ctypes.byref


def _recorder():
    spec = importlib.util.spec_from_file_location("record_halo_prologue_hashes",
                                                  os.path.join(ROOT, "scripts", "record_halo_prologue_hashes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


def test_tags_are_unique_and_every_changed_form_has_rows():
    tags = [c["id"] for c in REC.cases()]
    assert len(set(tags)) == len(tags)
    have = {c.kernel for c in REC.ROWS}
    want = ["64,128,true,false,true,6", "64,128,true,false,true", "64,64,true", "64,128,true", "64,128,true,false,false,6",
            "128,128,true", "128,32,true"]
    assert [k for k in want if HC._XK % k not in have] == []
    assert {HC._XRM, HC._XGM % 32, HC._XGM % 16, HC._XGM % 8} <= {c.combine for c in REC.ROWS if c.combine}
    # the fold's predicates (lane sub < chunks_in, sub + 8 < chunks_in) at their edges, for one and for two slabs, B = 1 and B = 2
    fold6 = [c for c in REC.ROWS if c.kernel == HC._XK % REC.FOLD6]
    for slabs in (1, 2):
        assert {REC.CHUNKS_IN[c.tag] for c in fold6 if c.slabs == slabs} >= {1, 8, 9, 16}
        assert {c.B for c in fold6 if c.slabs == slabs} == {1, 2}
    grids = [REC.grid_of(c) for c in fold6]
    assert min(grids) < 8 and any(g % 8 for g in grids if g > 8) and max(grids) <= 512
    assert all(REC.grid_of(c) > 512 for c in REC.ROWS if c.kernel == HC._XK % REC.FOLD3)
    # table form: the smallest and the largest width, with and without swish, for every member
    for k in want[2:]:
        rows = [c for c in REC.ROWS if c.kernel == HC._XK % k]
        assert {c.Cin for c in rows} == {128, 1024} and {c.gn for c in rows} == {"table", "swish"} and {c.B for c in rows} == {2}
    # generic kernel: fewer workgroups than XCDs, and counts that are no multiple of 8
    assert [g["T"] for g in REC.GENERIC] == [2 * g["B"] * g["ksplit"] for g in REC.GENERIC]
    assert min(g["T"] for g in REC.GENERIC) < 8 and sum(1 for g in REC.GENERIC if g["T"] > 8 and g["T"] % 8) >= 2


@pytest.mark.parametrize("case", REC.ROWS, ids=str)
def test_row_is_what_it_says(case):
    lib = _lib.load()
    d = HC.desc(case)
    bm, bn, ks = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert lib.sgam_conv2d_f32x_plan(ref(d), ref(bm), ref(bn), ref(ks)) == 0, "the descriptor validates"
    assert lib.sgam_conv2d_f32x_uses_halo(ref(d)) == 1
    assert (bm.value, bn.value, ks.value) == tuple(case.plan)
    M = case.B * case.Ho * case.Wo
    assert lib.sgam_conv2d_f32x_workspace_bytes(ref(d)) == (case.ksplit * M * case.N * 4 if case.ksplit > 1 else 0)
    total = case.Cin // 32
    assert 1 <= case.slabs <= total and -(-total // case.slabs) == case.ksplit, "slabs per workgroup and the split agree"
    assert (case.combine is not None) == (case.ksplit > 1)
    assert (lib.sgam_conv2d_f32x_stats_chunks(ref(d)) > 0) == case.stats
    if case.gn:
        assert lib.sgam_conv2d_f32x_gn_fusable(ref(d)) == 1 and case.Cin % 128 == 0
    if case.folded:
        assert lib.sgam_conv2d_f32x_gn_foldable(ref(d), REC.CHUNKS_IN[case.tag]) == 1
