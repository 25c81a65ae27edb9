"""Fixture generator for the dataset tests — BUILD CONTAINER ONLY (needs /root/reference and networkx; never runs on the GPU box).

Imports the REFERENCE's data/google_earth.py, points its GoogleEarthValidation at the seeded synthetic dataset that
`sgam_neurips22_amd.testing.synth_dataset_dir` writes (the test rewrites the same files from the same seed), and records its
own samples.  (Scene names differ in more than their last four characters: the reference's graph cache keys on `name[:-4]`,
and would hand the second scene the first one's pickled graph otherwise; this backend has no such cache.)  The fixture is data (the reference's outputs); no reference source is copied.

Re-run:  python tests/golden/gen_golden_dataset.py     ->  dataset_ge_val.npz
"""
import importlib.util
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)

from sgam_neurips22_amd import testing  # noqa: E402

ARGS = dict(kind="google_earth", size=24, frames=12, splits=("val",), seed=21,
            scenes=("alpha_scene", "bravo_scene"))      # tests/test_dataset_cpu.py uses the same
RES, N_SRC, INDICES = [16, 16], 2, (0, 5, 13, 23)


def main():
    spec = importlib.util.spec_from_file_location("ref_google_earth", "/root/reference/data/google_earth.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    with tempfile.TemporaryDirectory() as tmp:
        root = testing.synth_dataset_dir(os.path.join(tmp, "ds"), **ARGS)
        ds = ref.GoogleEarthValidation(dataset_dir=root, dataset="google_earth", image_resolution=RES, n_src=N_SRC)
        out = {"length": np.array(len(ds))}
        for i in INDICES:
            for k, v in ds[i].items():
                out[f"{i}.{k}"] = v
    path = os.path.join(HERE, "dataset_ge_val.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
