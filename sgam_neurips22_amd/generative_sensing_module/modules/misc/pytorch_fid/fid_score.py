"""The reference's import path of its FID score (modules/misc/pytorch_fid/fid_score.py) on the HIP kernels."""
from .....fid import (IMAGE_EXTENSIONS, ActivationStatistics, InceptionV3, calculate_activation_statistics,  # noqa: F401
                      calculate_fid_given_paths, calculate_frechet_distance, compute_statistics_of_path,
                      frechet_distance_from_features, get_activations, get_fid_score)
