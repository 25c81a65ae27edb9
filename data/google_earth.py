"""The reference's import path of the GoogleEarth datasets (`data.google_earth.GoogleEarthTrain` in DataModuleFromConfig)."""
from sgam_neurips22_amd.datasets import (GoogleEarthBase, GoogleEarthTest, GoogleEarthTrain,  # noqa: F401
                                         GoogleEarthValidation)
