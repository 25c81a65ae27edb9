"""The reference's import path of `ImagePaths` (data/base.py), the per-file half of the single-frame datasets."""
from sgam_neurips22_amd.datasets import ImagePaths  # noqa: F401
