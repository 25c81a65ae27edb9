"""What the cloud clean-up costs: k nearest neighbours at k = 8 / 16 / 32 on a real frame store's cloud — the uniform
grid against brute force against scipy's k-d tree (build + query(k), 16 threads: what a user does today) at Nr = Nq = 4 k ... 1 M —
voxel_sample at two voxel sizes, statistical_outliers, estimate_normals, and the whole
merged_point_cloud(voxel_size=..., nb_neighbors=20, normals=True) of the scene.

    python scripts/cloud_time.py [--frames 100] [--sizes 4096 16384 65536 262144 1048576] [--ks 8 16 32] [--repeats 5]
                                 [--brute-budget-ms 1000] [--kdtree-max 0] [--voxels 128 512] [--consumer-size 1048576]

The scene is geometry_time.py's: a GoogleEarth run on the splat branch (synthetic weights, 256 x 256, `--frames` frames).  The
reference set of a size is a strided sample of the store's valid points; the k-NN searches it with itself as the query set
(the point is its own first neighbour: the use of the outlier rule and of the normals).  Brute force is run while the size's
predicted time (pairs x the last measured time per pair at that k) stays under --brute-budget-ms.  --kdtree-max: largest size the
k-d tree is run at (0 = all).  --voxels: voxel edges as the longest box edge divided by these numbers.  --consumer-size: points
of the sample the outlier rule and the normals are timed on.  The crossover recorded per k is the smallest measured size from
which the grid (build + query) is faster than brute force.  Per `measuring-on-mi355x`: every shape warmed up, each repeat a
window of >= 0.2 s of calls between device events, the variants alternated within a repeat, median and spread; outputs of the two
kernels compared at every size both run.  One process, one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from flythrough_time import _spread, _timed  # noqa: E402
from pointview_time import _scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384, 65536, 262144, 1048576])
    ap.add_argument("--ks", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--brute-budget-ms", type=float, default=1000.0)
    ap.add_argument("--kdtree-max", type=int, default=0)
    ap.add_argument("--voxels", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--consumer-size", type=int, default=1048576)
    args = ap.parse_args()
    import numpy as np
    import torch
    from sgam_neurips22_amd import _lib, geometry
    if not torch.cuda.is_available():
        raise SystemExit("cloud_time.py measures on the GPU: no device found")
    scene = _scene(args.frames, rgbd=False)
    cloud = scene.merged_point_cloud()
    pts = cloud["points"]
    valid = pts[torch.isfinite(pts).all(dim=1)].contiguous()
    n_valid = int(valid.shape[0])
    out = {"script": "cloud_time", "frames": len(scene.frames), "points": int(pts.shape[0]), "valid_points": n_valid, "repeats": args.repeats,
           "build": _lib.load().sgam_build_commit().decode(), "unit": "ms", "auto_knn_grid_min_ref": geometry.AUTO_KNN_GRID_MIN_REF}

    def sample(size):
        n = n_valid if size == 0 or size > n_valid else size
        return valid[::max(1, n_valid // n)][:n].contiguous()

    # ---- k nearest neighbours
    rows, per_pair, crossover = [], {}, {}
    for size in args.sizes:
        ref = sample(size)
        n = int(ref.shape[0])
        grid = geometry.PointGrid(ref)
        row = {"n": n, "grid": {"cell_size": grid.cell_size, "dims": list(grid.dims)}}
        variants = {"grid_build": lambda: geometry.PointGrid(ref)}
        for k in args.ks:
            bufs = {"d2": torch.empty((n, k), dtype=torch.float32, device=ref.device), "index": torch.empty((n, k), dtype=torch.int32, device=ref.device)}
            variants[f"grid_query_k{k}"] = lambda k=k, bufs=bufs: grid.query_knn(ref, k, out=bufs)
            if k not in per_pair or per_pair[k] * n * n <= args.brute_budget_ms:
                variants[f"brute_k{k}"] = lambda k=k: geometry.knn(ref, ref, k, method="brute")
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        for k in args.ks:
            if f"brute_k{k}" in variants:
                a, b = geometry.knn(ref, ref, k, method="brute"), grid.query_knn(ref, k)
                row[f"outputs_equal_k{k}"] = bool(torch.equal(a["index"], b["index"]) and torch.equal(a["d2"].view(torch.int32), b["d2"].view(torch.int32)))
        ms = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name, fn in variants.items():
                ms[name].append(_timed(torch, fn))
        for name, v in ms.items():
            row[name + "_ms"] = _spread(v)
        for k in args.ks:
            total = row["grid_build_ms"]["median"] + row[f"grid_query_k{k}_ms"]["median"]
            row[f"grid_total_k{k}_ms"] = round(total, 4)
            if f"brute_k{k}" in variants:
                per_pair[k] = row[f"brute_k{k}_ms"]["median"] / (float(n) * n)
                faster = bool(total < row[f"brute_k{k}_ms"]["median"])
                row[f"grid_faster_k{k}"] = faster
                crossover[k] = (crossover.get(k) or n) if faster else None
        if args.kdtree_max == 0 or n <= args.kdtree_max:
            from scipy.spatial import cKDTree
            r64 = ref.cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            tree = cKDTree(r64)
            row["ckdtree_build_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            for k in args.ks:
                t0 = time.perf_counter()
                dist, _ = tree.query(r64, k=k, workers=16)
                row[f"ckdtree_query_k{k}_16_threads_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                got = grid.query_knn(ref, k)["d2"].cpu().numpy().astype(np.float64)
                row[f"max_rel_diff_to_ckdtree_d2_k{k}"] = float(np.max(np.abs(got - dist * dist) / np.maximum(dist * dist, 1e-30)))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del grid, ref, variants
    out["knn"] = rows
    out["measured_crossover_n_ref"] = {str(k): v for k, v in crossover.items()}

    # ---- voxel sampling of the whole store's valid points
    lo, hi = valid.amin(0), valid.amax(0)
    edge = float((hi - lo).max().item())
    out["voxel_sample"] = []
    for div in args.voxels:
        voxel = edge / div
        kept = int(geometry.voxel_sample(valid, voxel)["index"].numel())
        torch.cuda.synchronize()
        ms = [_timed(torch, lambda: geometry.voxel_sample(valid, voxel)) for _ in range(args.repeats)]
        out["voxel_sample"].append(dict(_spread(ms), points=n_valid, voxel_size=voxel, kept=kept))

    # ---- the consumers of the k-NN on one sample
    sub = sample(args.consumer_size)
    for name, fn in (("statistical_outliers_20", lambda: geometry.statistical_outliers(sub, 20, 2.0)),
                     ("estimate_normals_16", lambda: geometry.estimate_normals(sub, 16))):
        fn()
        torch.cuda.synchronize()
        out[name] = dict(_spread([_timed(torch, fn) for _ in range(args.repeats)]), points=int(sub.shape[0]))

    # ---- the scene-level call
    voxel = edge / args.voxels[-1]

    def whole():
        return scene.merged_point_cloud(voxel_size=voxel, nb_neighbors=20, normals=True)

    kept = int(whole()["index"].numel())
    torch.cuda.synchronize()
    out["merged_point_cloud_clean"] = dict(_spread([_timed(torch, whole) for _ in range(max(2, args.repeats // 2))]), voxel_size=voxel, kept=kept)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
