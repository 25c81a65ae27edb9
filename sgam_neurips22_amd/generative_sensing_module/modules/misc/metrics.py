"""The reference's import path of its image metrics (modules/misc/metrics.py): `PSNR`, `SSIM` on the HIP kernels."""
from ....metrics import PSNR, SSIM, psnr, ssim  # noqa: F401
