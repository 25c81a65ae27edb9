"""The reference's import path of its FID evaluation (modules/misc/pytorch_fid) on the HIP kernels: sgam_neurips22_amd/fid.py."""
