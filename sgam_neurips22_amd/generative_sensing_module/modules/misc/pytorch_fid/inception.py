"""The reference's import path of its FID network (modules/misc/pytorch_fid/inception.py): `InceptionV3` on the HIP kernels."""
from .....fid import FID_WEIGHTS_FILE, InceptionV3  # noqa: F401
