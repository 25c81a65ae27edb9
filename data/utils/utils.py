"""The names ``main_scene_generation.py`` star-imports from ``data.utils.utils`` (reference data/utils/utils.py:
OmegaConf :17, torch :20, np :18, instantiate_from_config :178-181), without the training-only dependencies
(wandb, pytorch_lightning, torchvision, omegaconf) that the inference path never touches — and the data module the
training configs name (`data.target: data.utils.utils.DataModuleFromConfig`, reference :196-311), Lightning-free."""
import numpy as np  # noqa: F401
import torch  # noqa: F401

from sgam_neurips22_amd.config import OmegaConf, instantiate_from_config  # noqa: F401

__all__ = ["OmegaConf", "torch", "np", "instantiate_from_config", "DataModuleFromConfig"]


class DataModuleFromConfig:
    """`DataModuleFromConfig(**config.data.params)`: the train / validation / test datasets of a training config and their
    loaders, as `sgam_neurips22_amd.datasets.BatchBuilder`s (train shuffled; validation and test in order, last short batch
    dropped; test = validation, like the reference).  `num_workers` and `use_depth` are accepted and unused, as in the
    reference's conditional-generation branch.  Beyond the reference: `backend` ("device" | "host"), `workers` (decode threads)
    and `seed` are handed to the loaders, and `single_frame_data`.  The `codebook` phase reads single RGB-D frames through
    `data.custom_codebook.CustomTrain` / `CustomValidation` (list files `dataset_dir + "/train.txt"` / `"/val.txt"`, `use_depth`
    as given, `convert_depth_flag` for clevr-infinite), under the same loader rules — with `single_frame_data=True`; without
    that key `setup()` refuses the phase, as it did before these datasets were built."""

    def __init__(self, batch_size, phase=None, wrap=False, num_workers=None, n_src=None, dataset=None, dataset_dir=None,
                 use_depth=None, image_resolution=None, depth_range=None, backend=None, workers=4, seed=None,
                 single_frame_data=False):
        self.batch_size, self.phase, self.wrap = batch_size, phase, wrap
        self.num_workers = num_workers if num_workers is not None else batch_size * 2
        self.backend, self.workers, self.seed = backend, workers, seed
        self.dataset_configs, self.datasets = {}, None
        if phase == "conditional_generation":
            stem = {"google_earth": "data.google_earth.GoogleEarth", "clevr-infinite": "data.clevr-infinite.Blender3d"}.get(dataset)
            if stem is None:
                raise NotImplementedError(dataset)
            params = {"dataset": dataset, "dataset_dir": dataset_dir, "n_src": n_src,
                      "image_resolution": list(image_resolution) if image_resolution is not None else None}
            self.dataset_configs["train"] = {"target": stem + "Train", "params": dict(params, seed=seed)}
            self.dataset_configs["validation"] = {"target": stem + "Validation", "params": dict(params)}
            self.dataset_configs["test"] = self.dataset_configs["validation"]
        elif phase == "codebook" and single_frame_data:
            params = {"dataset": dataset, "image_resolution": list(image_resolution), "dataset_dir": dataset_dir,
                      "use_depth": use_depth, "convert_depth_flag": "clevr-infinite" == dataset, "depth_range": depth_range}
            self.dataset_configs["train"] = {"target": "data.custom_codebook.CustomTrain",
                                             "params": dict(params, images_list_file=dataset_dir + "/train.txt")}
            self.dataset_configs["validation"] = {"target": "data.custom_codebook.CustomValidation",
                                                  "params": dict(params, images_list_file=dataset_dir + "/val.txt")}
            self.dataset_configs["test"] = self.dataset_configs["validation"]
        elif phase == "codebook":
            self.unbuilt = ("phase 'codebook' reads single frames through data.custom_codebook: pass single_frame_data=True "
                            "(`single_frame_data: true` in data.params) to build those datasets")
        else:
            raise NotImplementedError(phase)

    def prepare_data(self):
        pass

    def setup(self, stage=None):
        if getattr(self, "unbuilt", None):
            raise NotImplementedError(self.unbuilt)
        self.datasets = {k: instantiate_from_config(c) for k, c in self.dataset_configs.items()}

    def _loader(self, key, **kw):
        from sgam_neurips22_amd.datasets import BatchBuilder
        if self.datasets is None:
            self.setup()
        return BatchBuilder(self.datasets[key], self.batch_size, backend=self.backend, workers=self.workers, seed=self.seed, **kw)

    def train_dataloader(self):
        return self._loader("train", shuffle=True)

    def val_dataloader(self):
        return self._loader("validation", drop_last=True)

    def test_dataloader(self):
        return self._loader("test", drop_last=True)
