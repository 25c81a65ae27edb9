"""Fixture generator for the single-frame (codebook phase) dataset tests — BUILD CONTAINER ONLY (needs /root/reference; never runs
on the GPU box).

Imports the REFERENCE's data/custom_codebook.py (and with it data/base.py), points its CustomValidation / CustomTrain at the seeded
synthetic datasets that `sgam_neurips22_amd.testing.synth_dataset_dir` + `synth_frame_lists` write (the test rewrites the same files
from the same seed), and records its own samples.  albumentations and skimage are not installed: they are stubbed.  The
albumentations stub's Compose returns its input after asserting that it already has the crop's shape — the reference's
SmallestMaxSize + CenterCrop is the identity behind a resize to a square resolution, made checkable.  `file_path_` values are
recorded relative to the dataset root.  The fixture is data (the reference's outputs); no reference source is copied.

Re-run:  python tests/golden/gen_golden_codebook_dataset.py     ->  dataset_codebook.npz
"""
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)

from sgam_neurips22_amd import testing  # noqa: E402

# tag -> (synth_dataset_dir arguments, dtype the depth maps are rewritten in); tests/test_codebook_dataset_cpu.py uses the same
CASES = {"ge_f16": (dict(kind="google_earth", size=24, frames=12, seed=31), np.float16),
         "ge_f32": (dict(kind="google_earth", size=24, frames=12, seed=32), None),
         "clevr": (dict(kind="clevr-infinite", size=24, frames=12, seed=33), None)}
RES, N_ORDER, N_SAMPLES = [16, 16], 8, 4


def stub_missing_packages():
    alb = types.ModuleType("albumentations")

    class _Op:
        def __init__(self, **kw):
            self.kw = kw

    class Compose:
        def __init__(self, ops):
            self.crop = ops[1].kw

        def __call__(self, image):
            assert image.shape[:2] == (self.crop["height"], self.crop["width"]), image.shape
            return {"image": image}

    alb.SmallestMaxSize = alb.CenterCrop = alb.RandomCrop = _Op
    alb.Compose = Compose
    sys.modules["albumentations"] = alb
    sk = types.ModuleType("skimage")
    sk.io = types.ModuleType("skimage.io")
    sys.modules["skimage"], sys.modules["skimage.io"] = sk, sk.io


def main():
    stub_missing_packages()
    for name in [m for m in sys.modules if m == "data" or m.startswith("data.")]:
        del sys.modules[name]
    sys.path.insert(0, "/root/reference")           # the REFERENCE's `data` package wins over the repository's alias package
    import data.custom_codebook as ref
    assert ref.__file__.startswith("/root/reference")
    tmp = tempfile.mkdtemp(prefix="cbk")
    while "im" in tmp:                               # (the reference finds a depth map by replacing every 'im' of the path)
        shutil.rmtree(tmp)
        tmp = tempfile.mkdtemp(prefix="cbk")
    out = {}
    try:
        for tag, (args, dtype) in CASES.items():
            root = testing.synth_dataset_dir(os.path.join(tmp, tag), **args)
            testing.synth_frame_lists(root, dtype)
            kind = args["kind"]
            kw = dict(image_resolution=RES, use_depth=True, convert_depth_flag=kind == "clevr-infinite", dataset_dir=root, dataset=kind,
                      depth_range=None)
            train = ref.CustomTrain(images_list_file=root + "/train.txt", **kw)
            val = ref.CustomValidation(images_list_file=root + "/val.txt", **kw)
            rel = lambda p: os.path.relpath(p, root)  # noqa: E731
            out[f"{tag}.train_length"], out[f"{tag}.length"] = np.array(len(train)), np.array(len(val))
            out[f"{tag}.order"] = np.array([rel(val[i]["file_path_"]) for i in range(N_ORDER)])
            indices = list(range(N_SAMPLES - 1))
            if kind == "google_earth":               # one sample whose depth map holds the 65504 sentinel
                indices.append(next(i for i in range(N_SAMPLES - 1, len(val))
                                    if (np.load(val.depth_data.labels["file_path_"][i]) == 65504).any()))
            else:
                indices.append(len(val) - 1)
            for i in indices:
                s = val[i]
                assert sorted(s) == ["file_path_", "image"] and s["image"].dtype == np.float32
                out[f"{tag}.{i}.image"], out[f"{tag}.{i}.file_path_"] = s["image"], np.array(rel(s["file_path_"]))
            s = train[5]
            out[f"{tag}.train5.image"], out[f"{tag}.train5.file_path_"] = s["image"], np.array(rel(s["file_path_"]))
    finally:
        shutil.rmtree(tmp)
    path = os.path.join(HERE, "dataset_codebook.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
