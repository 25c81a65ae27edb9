"""Times of the reprojection view consistency (csrc/view_consistency.hip) and of fuse_frames — the numbers of DESIGN.md §4.4.12.

    python scripts/view_consistency_time.py [--json profiles/view_consistency_time.json] [--frames 32]

On one MI355X.  A GoogleEarth scene object whose store is filled with 32 seeded smooth RGB-D frames at 256 x 256 at the poses of its
own trajectory (nothing is generated: the model only gives the scene its device).  geometry.view_consistency on the store's
tensors for pairs "all" (992) and "earlier" (496), with and without the per-pixel maps: device events around a synchronised window
of back-to-back calls (each call: one upload of the pairs and poses, the kernel, the fold).  Algorithmic bytes: 14 B per source
pixel and pair (the source depth and colour, 7 B; the share of the target's four depths and twelve colour bytes a pixel has when
its neighbours read the same ones, 7 B) plus the maps' 9 B where written, over the time, against the HBM figure of DESIGN §5.
scene.view_consistency (with its host read and summaries) and scene.fuse_frames of the same frames by a host clock around a
synchronised call.  No threshold was set in advance: recorded numbers, not gates."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from sgam_neurips22_amd import _lib, geometry, testing  # noqa: E402

HBM_PEAK = 8.0e12
DEV = "cuda"
TOLERANCE = 0.05


def device_ms(fn, window_s=0.3, most=200):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    reps = int(max(3, min(most, window_s * 1e3 / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, reps


def host_ms(fn):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t), out


def filled_scene(n_frames):
    from sgam_neurips22_amd.config import default_params
    from sgam_neurips22_amd.generative_sensing_module.model import VQModel
    from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
    m = VQModel(**default_params("google_earth"))
    m.load_state_dict(testing.synthetic_state_dict(m.state_dict(), seed=0))
    scene = InfiniteSceneGeneration(m.to(DEV).eval(), "google_earth", output_dim=(n_frames, 1),
                                    seed_frame=synthetic_seed_frame("google_earth", 0))
    for k in range(1, n_frames):
        rgb, depth = synthetic_seed_frame("google_earth", k)
        rgb_u8 = torch.from_numpy(rgb).to(DEV)
        scene.curr = k
        scene.save_to_store(scene._ordered_grid_coords[k], rgb_u8, rgb_u8.float() / 255.0, torch.from_numpy(depth).to(DEV))
    assert len(scene.frames) == n_frames
    return scene


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "view_consistency_time.json"))
    ap.add_argument("--frames", type=int, default=32)
    args = ap.parse_args()
    lib = _lib.load()
    scene = filled_scene(args.frames)
    coords = scene._stored_coords(None, "view_consistency_time")
    depths, rgbs = [scene.frames[c]["depth"] for c in coords], [scene.frames[c]["rgb_u8"] for c in coords]
    Ts = np.stack([np.asarray(scene.transform_grid[c[0]][c[1]]["T"], dtype=np.float64) for c in coords])
    z0, z1 = scene._Z_RANGE[scene.data]
    H, W = scene.image_resolution
    F = len(coords)
    out = {"script": "view_consistency_time", "device": torch.cuda.get_device_name(0), "build": lib.sgam_build_commit().decode(),
           "hbm_peak_tb_s": HBM_PEAK / 1e12, "frames": F, "H": H, "W": W, "depth_tolerance": TOLERANCE, "unit": "ms", "kernel": [], "scene": []}
    for name in ("all", "earlier"):
        pairs = [(s, t) for s in range(F) for t in range(F) if s != t and (name == "all" or t < s)]
        for maps in (False, True):
            call = lambda: geometry.view_consistency(depths, rgbs, scene.K, Ts, z0, z1, TOLERANCE, pairs=pairs, maps=maps)  # noqa: E731
            ms, reps = device_ms(call)
            nbytes = len(pairs) * H * W * (14 + (9 if maps else 0))
            total = geometry.consistency_summary(call()["sums"])
            rec = {"pairs": name, "P": len(pairs), "maps": maps, "ms": ms, "reps": reps, "pairs_per_s": len(pairs) / (ms * 1e-3),
                   "algorithmic_bytes": nbytes, "tb_per_s": nbytes / (ms * 1e-3) / 1e12, "fraction_of_hbm_peak": nbytes / (ms * 1e-3) / HBM_PEAK,
                   "in_view_share": (total["n_valid"] - total["out_of_view"]) / max(total["n_valid"] + total["invalid"], 1),
                   "covisibility": total["covisibility"]}
            out["kernel"].append(rec)
            print(rec, flush=True)
    for name in ("all", "earlier"):
        ms, res = host_ms(lambda: scene.view_consistency(TOLERANCE, pairs=name))
        rec = {"call": f"scene.view_consistency(pairs={name!r})", "P": len(res["pairs"]), "host_clock_ms": ms}
        out["scene"].append(rec)
        print(rec, flush=True)
    ms, vol = host_ms(lambda: scene.fuse_frames())
    rec = {"call": "scene.fuse_frames()", "frames": F, "host_clock_ms": ms, "ms_per_frame": ms / F, "bricks": vol.stats()[0],
           "max_bricks": vol.max_bricks}
    out["scene"].append(rec)
    print(rec, flush=True)
    os.makedirs(os.path.dirname(args.json), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.json)


if __name__ == "__main__":
    main()
