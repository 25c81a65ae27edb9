"""Record what the one-pass fp32 attention returns into tests/golden/flash_partial_hashes.json.

attn_flash_f32x_kernel (csrc/attention.hip) leaves its un-normalised partial O^T per key range in a workspace that the merge
(attn_combine_kernel, or attn_combine_proj_f32x_kernel with proj_out fused) reads back.  How those partials are stored may change,
never a bit of them: per case of `cases()` the file holds the kernel names of ops.kernel_timeline and the sha256 of the result
(and, for the fused projection, the (chunks, sha256) of the statistics that leave with it).  tests/test_gpu_flash_store.py
replays the cases against the file.

The file is recorded from a build of the commit BEFORE a change to that store and names that build (`recorded_from`,
`lib_digest`).  It is never re-recorded from the code under test:

    SGAM_LIB_DIR=<dir> python -m sgam_neurips22_amd.build          # in a checkout of the earlier commit
    SGAM_HIP_LIB=<dir>/libsgam_hip.so python scripts/record_flash_partial_hashes.py        (needs the GPU)

Rows (C = 256, scale 1/16): (B, n) = (1, 256) — one key block per range, the pipeline's shortest trip count; (1, 512); (1, 1024)
with the logits widened six-fold so that the running maximum moves and the accumulators are rescaled in place before they are
stored; (8, 256) — stacked images; and ops.attention_proj at (1, 256), whose merge reads the same partials.
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sgam_neurips22_amd import _lib, ops, testing  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "flash_partial_hashes.json")
C = 256
FLASH = "attn_flash_f32x_kernel"


def cases():
    return [dict(id="attn_B1_n256", kind="attention", B=1, n=256, widen=1.0),
            dict(id="attn_B1_n512", kind="attention", B=1, n=512, widen=1.0),
            dict(id="attn_B1_n1024_wide", kind="attention", B=1, n=1024, widen=6.0),
            dict(id="attn_B8_n256", kind="attention", B=8, n=256, widen=1.0),
            dict(id="proj_B1_n256", kind="proj", B=1, n=256, widen=1.0)]


def _qkv(case, dev):
    t = "flash." + case["id"]
    qkv = testing.seeded_tensor(t + ".qkv", (case["B"] * case["n"], 3 * C), 1.0, 0.1)
    qkv[:, :C] *= case["widen"]             # q alone: the logits scale with it
    return qkv.to(dev)


def run_case(case, dev="cuda"):
    """-> dict(kernels, out, stats) of one case on the GPU, in split mode"""
    old = ops.F32_MODE
    ops.set_f32_mode("split")
    try:
        with torch.no_grad():
            qkv, t = _qkv(case, dev), "flash." + case["id"]
            if case["kind"] == "attention":
                fn = lambda: ops.attention(qkv, C, 1.0 / 16, B=case["B"])  # noqa: E731
            else:
                wp = ops.split_rows(testing.seeded_tensor(t + ".wp", (C, C), scale=C ** -0.5).to(dev))
                bias = testing.seeded_tensor(t + ".bp", (C,), scale=0.1).to(dev)
                res = testing.seeded_tensor(t + ".res", (case["B"] * case["n"], C)).to(dev)
                fn = lambda: ops.attention_proj(qkv, C, 1.0 / 16, wp, bias, res, B=case["B"])  # noqa: E731
            box = []
            recs, _ = ops.kernel_timeline(lambda: box.append(fn()))
            out, st = box[0], ops.gn_stats(box[0])
            return dict(kernels=[r[0] for r in recs], out=testing.sha256(out).hex(),
                        stats=None if st is None else [int(st[1]), testing.sha256(st[0]).hex()])
    finally:
        ops.set_f32_mode(old)


def reaches(case, rec):
    """the flash kernel ran, once, followed by the merge the row names"""
    merge = "attn_combine_proj_f32x_kernel" if case["kind"] == "proj" else "attn_combine_kernel"
    return sum(FLASH in k for k in rec["kernels"]) == 1 and any(merge in k for k in rec["kernels"])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    lib = _lib.load()
    doc = {"recorded_from": lib.sgam_build_commit().decode(), "lib_digest": lib.sgam_build_digest().decode(), "cases": {}}
    for case in cases():
        first, rec = run_case(case), run_case(case)
        assert first == rec, f"{case['id']}: two runs differ: {first} {rec}"
        assert reaches(case, rec), f"{case['id']}: ran {rec['kernels']}"
        doc["cases"][case["id"]] = rec
        print(case["id"], rec["kernels"], flush=True)
    with open(args.out, "w") as f:
        rows = ",\n".join(f"{json.dumps(cid)}: {json.dumps(rec)}" for cid, rec in doc["cases"].items())
        f.write('{"recorded_from": %s, "lib_digest": %s,\n"cases": {\n%s\n}}\n'
                % (json.dumps(doc["recorded_from"]), json.dumps(doc["lib_digest"]), rows))
    print("wrote", args.out, "from", doc["recorded_from"], doc["lib_digest"])


if __name__ == "__main__":
    main()
