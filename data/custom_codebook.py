"""The reference's import path of the codebook phase's single-frame datasets (`data.custom_codebook.CustomTrain` in
DataModuleFromConfig)."""
from sgam_neurips22_amd.datasets import CustomBase, CustomTrain, CustomValidation, ImagePaths  # noqa: F401
