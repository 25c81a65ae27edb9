"""GPU: the epilogues of the split-fp32 tile kernels write the bits they wrote before they were rescheduled.

tests/golden/epilogue_f32x_hashes.json was recorded by scripts/record_epilogue_hashes.py from a build of the commit in front of
the change that put all residual / bias loads of a wavefront in flight at once (the file names that commit and the digest of the
library that ran); it is not re-recorded from the code under test.  Every row is replayed here: the sha256 of the output, the
(chunks, sha256) of the GroupNorm chunk statistics that leave with it and the kernel names of the launch timeline are the recorded
ones.  The rows cover what tests/golden/dispatch_sequences.json does not: the <128,128,...> family, a per-row bias, a ragged M,
the pitched and the in-place residual (see the recorder's docstring)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_epilogue_hashes", os.path.join(ROOT, "scripts", "record_epilogue_hashes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
with open(REC.FIXTURE) as _f:
    DOC = json.load(_f)
FIX = DOC["cases"]

pytestmark = pytest.mark.gpu


def test_the_file_names_its_source_and_holds_every_case():
    assert DOC["recorded_from"] and len(DOC["lib_digest"]) == 12
    assert [c["id"] for c in REC.cases()] == list(FIX)
    assert all(REC.reaches(c, FIX[c["id"]]) for c in REC.cases())


@pytest.mark.parametrize("case", REC.cases(), ids=lambda c: c["id"])
def test_output_statistics_and_kernel_are_the_recorded_ones(case):
    want, got = FIX[case["id"]], REC.run_case(case)
    assert got["kernels"] == want["kernels"]
    assert REC.reaches(case, got)
    assert got.get("pre") == want.get("pre")
    assert got["out"] == want["out"]
    assert got["stats"] == want["stats"]
