"""GPU: the registration stack computes the bits it computed before its plumbing was folded.

tests/golden/registration_hashes.json was recorded by scripts/record_registration_hashes.py from a build of the commit in front of
the change that gave the registration code of geometry.py one cloud preparation, one Gauss-Newton step and one set of argument
checks, and the accumulate kernels of csrc/point_icp.hip one chunk skeleton (the file names that commit and the digest of the
library that ran); it is not re-recorded from the code under test.  Every case is replayed here and every hash — of each output
tensor's bytes, of each float's fp64 bits — and every count is the recorded one: no tolerance.  The tests against the numpy twins
(test_gpu_icp.py, test_gpu_colored_icp.py, test_gpu_global_registration.py) allow the chunk sums a reordering; this one does not."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_registration_hashes", os.path.join(ROOT, "scripts", "record_registration_hashes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
with open(REC.FIXTURE) as _f:
    DOC = json.load(_f)
FIX = DOC["cases"]

pytestmark = pytest.mark.gpu


def _leaves(v, path=""):
    if isinstance(v, dict):
        for k, x in v.items():
            yield from _leaves(x, f"{path}/{k}")
    elif isinstance(v, list):
        for i, x in enumerate(v):
            yield from _leaves(x, f"{path}/{i}")
    else:
        yield path, v


def test_the_file_names_its_source_and_holds_every_case():
    assert DOC["recorded_from"] and "dirty" not in DOC["recorded_from"] and len(DOC["lib_digest"]) == 12
    assert [c["id"] for c in REC.cases()] == list(FIX)
    assert all(len(list(_leaves(rec))) >= 2 for rec in FIX.values())


@pytest.mark.parametrize("case", REC.cases(), ids=lambda c: c["id"])
def test_every_output_is_the_recorded_one(case):
    want, got = dict(_leaves(FIX[case["id"]])), dict(_leaves(REC.run_case(case)))
    moved = sorted(k for k in set(want) | set(got) if want.get(k, "missing") != got.get(k, "missing"))
    assert not moved, f"{case['id']}: differ from the recording: {moved}"
