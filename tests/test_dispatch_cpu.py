"""Which launch sequence an AttnBlock takes is decided by AttnBlock.route() from shapes, dtypes and switches alone: the route of every
case of tests/golden/dispatch_sequences.json (recorded on the GPU next to the launches, scripts/record_dispatch.py) is recomputed
here without one.  Also: the GroupNorm chunk statistics travel through ops.gn_stats / one setter only."""
import importlib.util
import json
import os

import pytest
import torch

from sgam_neurips22_amd import ops
from sgam_neurips22_amd.generative_sensing_module.modules.diffusionmodules import model as dm

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_dispatch", os.path.join(ROOT, "scripts", "record_dispatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
with open(REC.FIXTURE) as _f:
    FIX = json.load(_f)["cases"]
ATTN = [c for c in REC.cases() if c["kind"] == "AttnBlock"]


@pytest.mark.parametrize("case", ATTN, ids=lambda c: c["id"])
def test_route_on_the_cpu_is_the_recorded_route(case):
    want = FIX[case["id"]]
    before = {k: getattr(m, k) for k, m in REC.SWITCHES.items()}, ops.F32_MODE
    assert REC.attn_route(case, want["has_stats"]) == want["route"]
    assert want["route"] in dm.AttnBlock.ROUTES
    assert ({k: getattr(m, k) for k, m in REC.SWITCHES.items()}, ops.F32_MODE) == before


def test_every_documented_route_is_recorded_and_every_case_is_in_the_file():
    assert {c["id"] for c in REC.cases()} == set(FIX)
    assert set(dm.AttnBlock.ROUTES) == {FIX[c["id"]]["route"] for c in ATTN}


def test_flipping_a_switch_changes_the_route_exactly_as_recorded():
    flipped = set()
    for case in ATTN:
        if not case.get("switches"):
            continue
        base = dict(case, switches={})
        base_id = next(c["id"] for c in ATTN if not c.get("switches") and all(c.get(k) == base.get(k) for k in ("C", "H", "W", "B", "mode", "producer")))
        stats = FIX[case["id"]]["has_stats"]
        assert stats == FIX[base_id]["has_stats"]
        r0, r1 = REC.attn_route(base, stats), REC.attn_route(case, stats)
        assert (r0, r1) == (FIX[base_id]["route"], FIX[case["id"]]["route"])
        if r0 != r1:
            flipped |= set(case["switches"])
    assert flipped == {k for c in ATTN for k in c.get("switches", {})}      # every switch the cases flip moves at least one route


def test_route_reads_its_arguments_only():
    """no tensor, no device: the same answer from a block that was never moved to a GPU, and has_stats only matters in 16 bits"""
    blk = dm.AttnBlock(256)
    assert blk.route(torch.bfloat16, 1, 16, 16, True) in ("block", "block_front")
    assert blk.route(torch.bfloat16, 1, 16, 16, False) == "image_flash.norm"
    assert blk.route(torch.float32, 1, 16, 16, True) == blk.route(torch.float32, 1, 16, 16, False)


def test_statistics_follow_a_view_made_through_the_helper_and_the_setter_clears():
    t = torch.zeros(2 * 4 * 8, 32)
    part = torch.zeros(2 * 1 * 32 * 2, dtype=torch.float64)
    assert ops.gn_stats(t) is None
    ops._set_gn_stats(t, part, 1)
    assert ops.gn_stats(t)[0] is part and ops.gn_stats(t)[1] == 1
    assert ops.gn_stats(t.view(2, 4, 8, 32)) is None                     # a plain view drops them ...
    v = ops.view_nhwc(t, 2, 4, 8)
    assert v.shape == (2, 4, 8, 32) and v.data_ptr() == t.data_ptr() and ops.gn_stats(v)[0] is part and ops.gn_stats(v)[1] == 1
    assert ops._set_gn_stats(t, None) is t and ops.gn_stats(t) is None   # ... and a launch without statistics clears the tag
    assert ops.gn_stats(ops.view_nhwc(t, 2, 4, 8)) is None
    assert ops.gn_stats(ops.carry_gn_stats(torch.zeros(3), v))[0] is part


def test_the_statistics_attribute_is_touched_by_the_accessor_and_the_setter_only():
    hits = []
    for top in ("sgam_neurips22_amd", "tests", "scripts"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".sh", ".md")) and f != os.path.basename(__file__):
                    with open(os.path.join(d, f), errors="replace") as fh:
                        hits += [(os.path.relpath(os.path.join(d, f), ROOT), i) for i, line in enumerate(fh, 1) if "_gn_partials" in line]
    assert hits and {p for p, _ in hits} == {os.path.join("sgam_neurips22_amd", "_opscore.py")}, hits
    import inspect
    from sgam_neurips22_amd import _opscore
    lines = set()
    for fn in (_opscore.gn_stats, _opscore._set_gn_stats):
        src, first = inspect.getsourcelines(fn)
        lines |= set(range(first, first + len(src)))
    assert {i for _, i in hits} <= lines, hits
