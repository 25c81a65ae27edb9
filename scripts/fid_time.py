"""Rates of the FID evaluation (sgam_neurips22_amd/fid.py) on synthetic weights — the numbers of DESIGN.md §4.7.1.

    python scripts/fid_time.py [--sizes 64,256] [--n 512] [--batch 50] [--json out.json]

Per image size: images/s of `get_activations` at batch 50 from uint8 frames already on the device, and from PNG files (PIL decode on
host threads, pinned staging, one upload per batch).  Once: the per-launch timeline of one batch's forward through sgam_prof_*
(time by kernel, the forward's share of the fp32-MFMA roof), the statistics update per batch of 2048-d features, and the two
distance routes at N = 64 and N = 2048 images per side."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sgam_neurips22_amd import fid  # noqa: E402
from sgam_neurips22_amd.ops_aux import kernel_timeline  # noqa: E402

import inception_oracle as IO  # noqa: E402

F32_MFMA_PEAK = 157.3e12        # v_mfma_f32_32x32x2_f32 on 256 CUs at 2.4 GHz (csrc/conv_gemm.hip)


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256")
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = "cuda"
    model = fid.InceptionV3(weights=IO.synthetic_state_dict(0)).to(dev)
    out = {"n": a.n, "batch": a.batch, "sizes": {}}
    g = torch.Generator().manual_seed(0)
    for size in [int(s) for s in a.sizes.split(",")]:
        frames = torch.randint(0, 256, (a.n, size, size, 3), generator=g, dtype=torch.uint8)
        on_dev = frames.to(dev)
        t_dev = timed(lambda: fid.get_activations(on_dev, model, a.batch, 2048, dev))
        with tempfile.TemporaryDirectory() as tmp:
            from PIL import Image
            files = []
            for i in range(a.n):
                files.append(os.path.join(tmp, f"im_{i:05d}.png"))
                Image.fromarray(frames[i].numpy()).save(files[-1])
            t_png = timed(lambda: fid.get_activations(files, model, a.batch, 2048, dev, num_workers=8), reps=1)
        out["sizes"][size] = {"device_frames_img_per_s": a.n / t_dev, "png_files_img_per_s": a.n / t_png}
        print(f"{size} x {size}: {a.n / t_dev:9.1f} images/s from device frames, {a.n / t_png:9.1f} images/s from PNG files")
    # per-launch timeline of one batch
    batch = torch.randint(0, 256, (a.batch, 256, 256, 3), generator=g, dtype=torch.uint8).to(dev)
    model.features(batch)
    recs, bracket = kernel_timeline(lambda: model.features(batch))
    by_kernel, flops, ms_total = {}, 0.0, 0.0
    for name, ms, fl, _, _ in recs:
        ms = max(ms - bracket, 0.0)
        head = name.split("<")[0].lstrip("(")
        by_kernel[head] = by_kernel.get(head, 0.0) + ms
        flops += fl
        ms_total += ms
    out["forward"] = {"launches": len(recs), "ms": ms_total, "gflop": flops / 1e9, "by_kernel_ms": by_kernel,
                      "fraction_of_f32_mfma_roof": flops / (ms_total * 1e-3) / F32_MFMA_PEAK}
    print(f"forward of {a.batch} images: {len(recs)} launches, {ms_total:.2f} ms on the device, {flops / 1e9:.1f} GFLOP in the convs: "
          f"{100 * out['forward']['fraction_of_f32_mfma_roof']:.1f} % of the fp32-MFMA roof")
    for k, v in sorted(by_kernel.items(), key=lambda kv: -kv[1]):
        print(f"    {k:40s} {v:8.3f} ms")
    # statistics update per batch
    feats = torch.randn((a.batch, 2048), device=dev)
    st = fid.ActivationStatistics(2048, dev).update(feats)
    out["stats_update_ms"] = 1e3 * timed(lambda: st.update(feats))
    out["stats_finalize_ms"] = 1e3 * timed(st.finalize)
    print(f"statistics: update of a ({a.batch}, 2048) batch {out['stats_update_ms']:.3f} ms, finalize + download {out['stats_finalize_ms']:.1f} ms")
    # distance routes
    out["distance_s"] = {}
    for n in (64, 2048):
        rng = np.random.default_rng(n)
        f1, f2 = rng.standard_normal((n, 2048)), rng.standard_normal((n, 2048)) + 0.1
        t = time.perf_counter()
        low = fid.frechet_distance_from_features(f1, f2)
        t_low = time.perf_counter() - t
        s1, s2 = IO.statistics(f1), IO.statistics(f2)
        t = time.perf_counter()
        sq = float(fid.calculate_frechet_distance(*s1, *s2))
        t_sq = time.perf_counter() - t
        out["distance_s"][n] = {"lowrank": t_low, "sqrtm": t_sq, "lowrank_value": low, "sqrtm_value": sq}
        print(f"distance at N = {n}: low-rank {t_low:.3f} s ({low:.6f}), sqrtm {t_sq:.3f} s ({sq:.6f})")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
