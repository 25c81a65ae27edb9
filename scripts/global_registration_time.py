"""What global registration costs, stage by stage, against nothing but itself: normals, FPFH (k-NN search + counts +
combine) of one cloud, the nearest feature, the RANSAC hypotheses, their scores with and without the gathering of the valid ones, the
winner's inliers plus the refit, and a whole geometry.register_ransac — for clouds of --sizes points (default 8192 and 32768, what
voxel sampling leaves of a scene) and --hypotheses hypotheses (default 100 000).  Also the nearest-feature kernel's achieved fp32
operation rate against the VALU roof for its arithmetic: three unfused, unpacked IEEE operations per pair and dimension
(-ffp-contract=off), one per lane and clock, 256 CUs x 64 lanes x 2.4 GHz = 39.3 T operations/s (a quarter of the 157.3 TFLOPS
spec, which counts packed fused multiply-adds).

    python scripts/global_registration_time.py [--sizes 8192 32768] [--hypotheses 100000] [--repeats 3] [--feature-k 32]

The clouds are samples of an analytic surface (z = 0.3 sin 1.7x + 0.2 cos 2.3y + 0.1xy over a square grown with the point count so
that the density stays that of a voxel-sampled scene at voxel_size 0.05); the target is another sample of it moved by 140 degrees.
Per `measuring-on-mi355x`: every shape warmed up, each repeat a window of >= 0.2 s of calls between device events, the stages
alternated within a repeat, median and spread.  One process, one JSON line."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from flythrough_time import _spread, _timed  # noqa: E402

VALU_OPS_PER_S = 256 * 64 * 2.4e9            # one unpacked fp32 operation per lane and clock
VOXEL = 0.05


def _surface(np, n, seed, side):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, side, n), rng.uniform(0, side, n)
    return np.stack([x, y, 0.3 * np.sin(1.7 * x) + 0.2 * np.cos(2.3 * y) + 0.1 * x * y / max(1.0, side / 4.0)], axis=1).astype(np.float32)


def _motion(np):
    w = np.radians(140.0) * np.array([1.0, -2.0, 1.5]) / np.linalg.norm([1.0, -2.0, 1.5])
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / (th * th) * K @ K
    T[:3, 3] = [0.6, -0.7, 0.9]
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 32768])
    ap.add_argument("--hypotheses", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--feature-k", type=int, default=32)
    args = ap.parse_args()
    import numpy as np
    import torch
    from sgam_neurips22_amd import _lib, geometry
    if not torch.cuda.is_available():
        raise SystemExit("global_registration_time.py measures on the GPU: no device found")
    dev = "cuda"
    T = _motion(np)
    distance, radius = 1.5 * VOXEL, 5.0 * VOXEL
    out = {"script": "global_registration_time", "hypotheses": args.hypotheses, "repeats": args.repeats, "feature_k": args.feature_k,
           "voxel_size": VOXEL, "max_correspondence_distance": distance, "feature_radius": radius,
           "build": _lib.load().sgam_build_commit().decode(), "unit": "ms"}
    rows = []
    for n in args.sizes:
        side = math.sqrt(n) * VOXEL                                        # one point per voxel footprint
        view = np.array([side / 2, side / 2, 50.0])
        src = torch.from_numpy(_surface(np, n, 1, side)).to(dev)
        tgt = geometry.transform_points(torch.from_numpy(_surface(np, n, 2, side)).to(dev), T)
        zeros = torch.zeros((n,), dtype=torch.int32, device=dev)
        views = (torch.from_numpy(view.astype(np.float32))[None].to(dev),
                 torch.from_numpy((T[:3, :3] @ view + T[:3, 3]).astype(np.float32))[None].to(dev))
        src_n, tgt_n = geometry.estimate_normals(src, 16, views[0], zeros), geometry.estimate_normals(tgt, 16, views[1], zeros)
        fs, ft = geometry.fpfh(src, src_n, args.feature_k, radius), geometry.fpfh(tgt, tgt_n, args.feature_k, radius)
        match = geometry.match_features(fs, ft)
        corr = geometry.correspondences_of(match)
        hyp = geometry.ransac_hypotheses(src, tgt, corr, distance, args.hypotheses)
        score = geometry.ransac_score(src, tgt, corr, hyp["poses"], hyp["valid"], distance)
        whole = geometry.register_ransac(src, tgt, corr, distance, max_iterations=args.hypotheses)
        truth = geometry.register_icp(src, tgt, distance, init=T, target_normals=tgt_n)
        fine = geometry.register_icp(src, tgt, distance, init=whole["transformation"], target_normals=tgt_n)
        dT = fine["transformation"].cpu().numpy() - truth["transformation"].cpu().numpy()
        row = {"n": n, "correspondences": int(corr.shape[0]), "valid_hypotheses": whole["valid_hypotheses"],
               "inliers": whole["inliers"]["count"], "ransac_fitness": whole["fitness"], "icp_fitness": fine["fitness"],
               "pose_difference_to_icp_from_the_truth": float(np.abs(dT).max())}

        def winner():
            win = geometry.ransac_inliers(src, tgt, corr, hyp["poses"], score["best"], distance)
            moved = geometry.transform_points(src, win["state"][:16].view(4, 4))
            hist = torch.zeros((4, geometry.ICP_ROW), dtype=torch.float64, device=dev)
            for it in range(4):
                geometry.icp_update(geometry.icp_accumulate(moved, tgt, None, win["index"], match["d2"]), it, 0.0, 0.0, win["state"], hist)

        variants = {
            "normals": lambda: geometry.estimate_normals(src, 16, views[0], zeros),
            "fpfh": lambda: geometry.fpfh(src, src_n, args.feature_k, radius),
            "match": lambda: geometry.match_features(fs, ft),
            "hypotheses": lambda: geometry.ransac_hypotheses(src, tgt, corr, distance, args.hypotheses),
            "score_compacted": lambda: geometry.ransac_score(src, tgt, corr, hyp["poses"], hyp["valid"], distance, compact=True),
            "score_every_lane": lambda: geometry.ransac_score(src, tgt, corr, hyp["poses"], hyp["valid"], distance, compact=False),
            "inliers_and_refit": winner,
            "register_ransac": lambda: geometry.register_ransac(src, tgt, corr, distance, max_iterations=args.hypotheses),
        }
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                ms[k].append(_timed(torch, fn))
        for k, v in ms.items():
            row[k + "_ms"] = _spread(v)
        ops = 3.0 * geometry.FPFH_DIM * n * n
        row["match_fp32_ops_per_s"] = ops / (row["match_ms"]["median"] * 1e-3)
        row["match_share_of_valu_roof"] = round(row["match_fp32_ops_per_s"] / VALU_OPS_PER_S, 4)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    out["sizes"] = rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
