"""Times of the batched direct RGB-D odometry (csrc/rgbd_odometry.hip) — the numbers of DESIGN.md §4.4.13.

    python scripts/rgbd_odometry_time.py [--json profiles/rgbd_odometry_time.json] [--frames 32] [--icp consecutive|all|none]

On one MI355X.  The set-up of scripts/view_consistency_time.py: a GoogleEarth scene object whose store is filled with 32 seeded
smooth RGB-D frames at 256 x 256 at the poses of its own trajectory (nothing is generated).  geometry.rgbd_odometry on the store's
tensors for the consecutive pairs (P = 31) and every pair i < j (P = 496), iterations (20, 10, 5), from the stored relative poses:
device events around a synchronised window of back-to-back whole calls (pyramid, one upload, 35 iterations of two launches, the
information pass), the pyramid alone, and one iteration (accumulate + update) per level on running pairs.  Where the time goes: the
accumulate against the update per level, and the algorithmic bytes of an accumulate — 8 B per source pixel and pair (depth and
intensity), the same again for the share of the target's eight corner reads a pixel has when its neighbours read the same ones —
against the HBM figure of DESIGN §5.  Next to it, by a host clock around the second of two synchronised calls, scene.optimize_poses_rgbd
and scene.optimize_poses(estimation="colored") — multiway_registration's loop of one coloured ICP per pair — on the same frames, with
the optimize_pose_graph both end with timed on its own (on the odometry's graph), so that what is left is the building of the graph:
--icp consecutive times the latter with the loop closures switched off (31 registrations), --icp all with every candidate pair.
No threshold was set in advance: recorded numbers, not gates."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sgam_neurips22_amd import _lib, geometry  # noqa: E402
from view_consistency_time import DEV, HBM_PEAK, device_ms, filled_scene  # noqa: E402

MAX_DEPTH_DIFF = 0.05
ITERATIONS = (20, 10, 5)


def host_once_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "rgbd_odometry_time.json"))
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--icp", default="consecutive", choices=("consecutive", "all", "none"))
    args = ap.parse_args()
    lib = _lib.load()
    scene = filled_scene(args.frames)
    coords = scene._stored_coords(None, "rgbd_odometry_time")
    depths, rgbs = [scene.frames[c]["depth"] for c in coords], [scene.frames[c]["rgb_u8"] for c in coords]
    Ts = np.stack([np.asarray(scene.transform_grid[c[0]][c[1]]["T"], dtype=np.float64) for c in coords])
    z0, z1 = scene._Z_RANGE[scene.data]
    H, W = scene.image_resolution
    F = len(coords)
    out = {"script": "rgbd_odometry_time", "device": torch.cuda.get_device_name(0), "build": lib.sgam_build_commit().decode(),
           "hbm_peak_tb_s": HBM_PEAK / 1e12, "frames": F, "H": H, "W": W, "max_depth_diff": MAX_DEPTH_DIFF, "iterations": list(ITERATIONS),
           "unit": "ms", "odometry": [], "scene": []}
    ms, reps = device_ms(lambda: geometry.rgbd_pyramid(depths, rgbs, scene.K, len(ITERATIONS)))
    out["pyramid_ms"] = ms
    print("pyramid", ms, "ms", flush=True)
    pyr = geometry.rgbd_pyramid(depths, rgbs, scene.K, len(ITERATIONS))
    inv = [np.linalg.inv(T) for T in Ts]
    for name, pairs in (("consecutive", [(i, i + 1) for i in range(F - 1)]), ("all", [(i, j) for i in range(F) for j in range(i + 1, F)])):
        P = len(pairs)
        init = np.stack([Ts[j] @ inv[i] for i, j in pairs])
        call = lambda: geometry.rgbd_odometry(depths, rgbs, scene.K, pairs, z0, z1, MAX_DEPTH_DIFF, init=init, iterations=ITERATIONS)  # noqa: E731
        ms, reps = device_ms(call, most=20)
        res = call()
        status = res["status"].cpu().numpy()
        rec = {"pairs": name, "P": P, "whole_call_ms": ms, "reps": reps, "ms_per_iteration": ms / sum(ITERATIONS), "ms_per_pair": ms / P,
               "status_counts": [int((status == k).sum()) for k in range(3)], "mean_steps": float(res["iterations"].mean().item()),
               "mean_fitness": float(torch.nan_to_num(res["fitness"]).mean().item()), "levels": []}
        # one iteration per level with every pair running (criteria of zero never stop a pair; a fresh state each time)
        run = geometry._RgbdOdometry(pyr, pairs, init, z0, z1, MAX_DEPTH_DIFF, geometry.LAMBDA_GEOMETRIC, rows=1)
        run.workspace_for(P)
        start = run.state.clone()
        for level, (h, w) in enumerate(pyr["sizes"]):
            def both():
                run.accumulate(level, 0, P, True)
                run.update(level, 0, P, 0, True, 0.0, 0.0)
            run.state.copy_(start)
            acc, _ = device_ms(lambda: run.accumulate(level, 0, P, True))
            it, _ = device_ms(both)
            nbytes = P * h * w * 16
            rec["levels"].append({"level": level, "H": h, "W": w, "accumulate_ms": acc, "iteration_ms": it, "update_ms": it - acc,
                                  "algorithmic_bytes": nbytes, "tb_per_s": nbytes / (acc * 1e-3) / 1e12,
                                  "fraction_of_hbm_peak": nbytes / (acc * 1e-3) / HBM_PEAK})
        out["odometry"].append(rec)
        print(rec, flush=True)
    # the scene-level calls, each timed on its second run (the first pays one-time set-up), and the pose-graph optimisation both end with
    # on its own: what is left is what building the graph costs
    scene.optimize_poses_rgbd(MAX_DEPTH_DIFF, iterations=ITERATIONS)
    ms, fix = host_once_ms(lambda: scene.optimize_poses_rgbd(MAX_DEPTH_DIFF, iterations=ITERATIONS))
    graph = geometry.multiway_rgbd(depths, rgbs, scene.K, Ts, z0, z1, MAX_DEPTH_DIFF, iterations=ITERATIONS)["graph"]
    pg, _ = host_once_ms(lambda: geometry.optimize_pose_graph(graph, max_correspondence_distance=MAX_DEPTH_DIFF))
    rec = {"call": "scene.optimize_poses_rgbd()", "edges": len(fix["edges"]), "host_clock_ms": ms, "optimize_pose_graph_ms": pg,
           "graph_building_ms": ms - pg, "status": fix["status"]}
    out["scene"].append(rec)
    print(rec, flush=True)
    if args.icp != "none":
        kw = dict(loop_closure_stride=F) if args.icp == "consecutive" else {}
        scene.optimize_poses(MAX_DEPTH_DIFF, estimation="colored", **kw)
        ms, ref = host_once_ms(lambda: scene.optimize_poses(MAX_DEPTH_DIFF, estimation="colored", **kw))
        n = max(len(ref["edges"]) + len(ref["missing_odometry"]), 1)
        rec = {"call": f"scene.optimize_poses(estimation='colored'), pairs {args.icp}", "edges": len(ref["edges"]), "host_clock_ms": ms,
               "graph_building_ms": ms - pg, "graph_building_ms_per_registration": (ms - pg) / n,
               "missing_odometry": len(ref["missing_odometry"]), "status": ref["status"]}
        out["scene"].append(rec)
        print(rec, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.json)


if __name__ == "__main__":
    main()
