"""Time the training data path on a synthetic GoogleEarth-shaped dataset (512 x 512 PNGs -> 256 x 256, batch 4,
n_src 1, written to a temporary directory): milliseconds per batch of the host and the device backend (the device backend
split into the wait for the decode threads and the device part, by HIP events), and steps/s of `fit` on the full model with
each backend against steps/s on one resident batch.  `--mode codebook`: the same figures for the codebook phase's single
RGB-D frames (`CustomTrain` over list files; 512 x 512 PNG + float16 npy -> 256 x 256, batch 3, one frame per sample), with the
model in phase `codebook`.

    python scripts/loader_time.py [--mode pairs|codebook] [--batches 12] [--steps 12] [--workers 4] [--frames 24]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from sgam_neurips22_amd import datasets, testing  # noqa: E402
from sgam_neurips22_amd.config import default_params  # noqa: E402
from sgam_neurips22_amd.fit import fit  # noqa: E402
from sgam_neurips22_amd.generative_sensing_module.model import VQModel  # noqa: E402

LOSS = "sgam_neurips22_amd.generative_sensing_module.modules.losses.vqperceptual.VQLPIPSWithDiscriminator"


class Module:
    def __init__(self, root, backend, workers, batch_size=4, mode="pairs"):
        self.root, self.backend, self.workers, self.batch_size, self.mode = root, backend, workers, batch_size, mode

    def train_dataloader(self):
        if self.mode == "codebook":
            ds = datasets.CustomTrain(image_resolution=[256, 256], images_list_file=self.root + "/train.txt", use_depth=True,
                                      convert_depth_flag=False, dataset_dir=self.root, dataset="google_earth", depth_range=None)
        else:
            ds = datasets.GoogleEarthTrain(dataset_dir=self.root, dataset="google_earth", image_resolution=[256, 256], n_src=1, seed=0)
        return datasets.BatchBuilder(ds, self.batch_size, backend=self.backend, shuffle=True, seed=0, workers=self.workers)


def loader_ms(dm, batches):
    """(ms per batch, of which waiting for the decode threads, of which device work) with prefetch off and an idle consumer: the
    whole cost of a batch, nothing overlapped.  Host backend: the device part is the upload of the collated batch."""
    loader = dm.train_dataloader()
    loader.prefetch, loader.time_device = False, True
    it = iter(loader)
    next(it)                                          # staging, tables, first decode
    torch.cuda.synchronize()
    wall = wait = dev = 0.0
    done = 0
    while done < batches:
        t0 = time.perf_counter()
        try:
            batch = next(it)
        except StopIteration:
            it = iter(loader)
            continue
        events = loader.device_events
        if dm.backend == "host":
            events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            events[0].record()
            batch = {k: v.to("cuda") if hasattr(v, "to") else v for k, v in batch.items()}
            events[1].record()
        torch.cuda.synchronize()
        wall += (time.perf_counter() - t0) * 1e3
        wait += loader.decode_wait_ms
        dev += events[0].elapsed_time(events[1])
        done += 1
    loader.close()
    return wall / batches, wait / batches, dev / batches


def full_model(phase=None):
    p = default_params("google_earth")
    if phase is not None:
        p["phase"] = phase
    p["lossconfig"] = {"target": LOSS, "params": {"disc_start": 0, "perceptual_weight": 0.0, "disc_in_channels": 4, "disc_weight": 0.8,
                                                 "use_discriminative_loss": True}}
    torch.manual_seed(0)
    m = VQModel(**p)
    m.load_state_dict(testing.synthetic_state_dict(m.state_dict(), seed=0))
    m = m.to("cuda")
    m.init_loss()
    return m


def fit_rate(dm, steps):
    m = full_model("codebook" if dm.mode == "codebook" else None)
    fit(m, dm, 2)                                     # warm: packs, workspaces, staging
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit(m, dm, 2 + steps)
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def resident_rate(dm, steps):
    m = full_model("codebook" if dm.mode == "codebook" else None)
    loader = dm.train_dataloader()
    batch = next(iter(loader))
    loader.close()
    for i in range(2):
        m.training_step(dict(batch), i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        m.training_step(dict(batch), 2 + i)
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--mode", choices=("pairs", "codebook"), default="pairs")
    ap.add_argument("--repeats", type=int, default=1, help="host / device alternated this many times")
    a = ap.parse_args()
    res = {"mode": a.mode, "threads_available": len(os.sched_getaffinity(0)), "workers": a.workers}
    bs = 3 if a.mode == "codebook" else 4
    holder = tempfile.TemporaryDirectory(prefix="loader")
    while "im" in holder.name:                        # (the single-frame datasets replace every 'im' of a path to find its depth map)
        holder.cleanup()
        holder = tempfile.TemporaryDirectory(prefix="loader")
    with holder as tmp:
        root = testing.synth_dataset_dir(os.path.join(tmp, "ds"), "google_earth", size=512, scenes=("scene_a",), frames=a.frames,
                                         splits=("train",))
        if a.mode == "codebook":
            import numpy as np
            testing.synth_frame_lists(root, np.float16, splits=("train",))
        for rep in range(a.repeats):
            for backend in ("host", "device"):
                for workers in sorted({1, a.workers}):
                    ms, wait, dev = loader_ms(Module(root, backend, workers, bs, a.mode), a.batches)
                    res[f"{backend}_w{workers}" + (f"_run{rep + 1}" if a.repeats > 1 else "")] = {
                        "ms_per_batch": round(ms, 2), "decode_wait_ms": round(wait, 2), "device_ms": round(dev, 3)}
        if not a.no_fit:
            res["fit_steps_per_s"] = {b: round(fit_rate(Module(root, b, a.workers, bs, a.mode), a.steps), 2) for b in ("host", "device")}
            res["resident_steps_per_s"] = round(resident_rate(Module(root, "device", a.workers, bs, a.mode), a.steps), 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
