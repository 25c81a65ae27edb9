"""Stand-in for the reference's ``data`` package: ``data.utils.utils`` (star-imported by main_scene_generation.py:6, and the data
module of the training configs) and the import paths of the training datasets (``data.google_earth``, ``data.clevr-infinite``,
``data.custom_codebook``, ``data.base``), which live in ``sgam_neurips22_amd.datasets``."""
