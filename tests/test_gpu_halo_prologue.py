"""GPU: the split-fp32 kernels write the bits they wrote before their prologues were reordered.

tests/golden/halo_prologue_hashes.json was recorded by scripts/record_halo_prologue_hashes.py from a build of the commit in front of
the change (kernel arguments in one batch, the tile map without gridDim; the rows of the folding and the table form pin the
kernels whose GroupNorm parameter requests were moved ahead of the halo and the weight fragments, measured with it and not kept);
the file names that commit and the digest of the library that ran, and it is not re-recorded from the code under test.  Every row
is replayed here: the sha256 of the output, the (chunks, sha256) of the GroupNorm chunk statistics that leave with it, the sha256 of
the split-K partial tiles where the plan splits, and the kernel names of the launch timeline are the recorded ones.  The rows and
why they have their shapes: the recorder's docstring.

One kind of row the change was specified with does not exist: the tile map with the swizzle off (the launcher always sets it)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_halo_prologue_hashes",
                                                  os.path.join(ROOT, "scripts", "record_halo_prologue_hashes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
with open(REC.FIXTURE) as _f:
    DOC = json.load(_f)
FIX = DOC["cases"]

pytestmark = pytest.mark.gpu


def test_the_file_names_its_source_and_holds_every_case():
    assert DOC["recorded_from"] and "dirty" not in DOC["recorded_from"] and len(DOC["lib_digest"]) == 12
    assert [c["id"] for c in REC.cases()] == list(FIX)
    assert all(REC.reaches(c, FIX[c["id"]]) for c in REC.cases())
    assert all((FIX[c["id"]]["ws"] is not None) == (c["combine"] is not None) for c in REC.cases())


@pytest.mark.parametrize("case", REC.cases(), ids=lambda c: c["id"])
def test_output_statistics_partials_and_kernels_are_the_recorded_ones(case):
    want, got = FIX[case["id"]], REC.run_case(case)
    assert got["kernels"] == want["kernels"]
    assert REC.reaches(case, got)
    assert got["ws"] == want["ws"]
    assert got["out"] == want["out"]
    assert got["stats"] == want["stats"]
