"""What the geometry metrics cost: exact nearest neighbours on a real frame store's cloud — brute force against the
uniform grid at Nr = Nq = 4 k ... 1 M and the whole store, the grid build on its own — unproject_frames against the host loop of
export_point_clouds, geometry_metrics end to end, and scipy's k-d tree (build + query, 16 threads: what a user does today) on the
same clouds.

    python scripts/geometry_time.py [--frames 100] [--sizes 4096 16384 65536 262144 1048576 0] [--repeats 5] [--brute-budget-ms 1000]
                                    [--kdtree-max 0] [--no-host-export]

The scene is a GoogleEarth run on the splat branch (synthetic weights, 256 x 256, `--frames` frames).  A size of 0 is the whole
store (6.5 M points at 100 frames).  The reference set of a size is a strided sample of the store's valid points, the query set the
sample between them moved by a few millimetres: the same surface, no point its own neighbour.  Brute force is run while the
size's predicted time (pairs x the last measured time per pair) stays under --brute-budget-ms.  --kdtree-max: largest size the
k-d tree is run at (0 = all).  The crossover recorded is the smallest measured size from which the grid (build + query) is faster.
Per `measuring-on-mi355x`: every shape warmed up, each repeat a window of >= 0.2 s of calls between device events, the variants
alternated within a repeat, median and spread; outputs of the two kernels compared at every size both run.  One process, one
JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from flythrough_time import _spread, _timed  # noqa: E402
from pointview_time import _scene  # noqa: E402

HBM_GBPS = 8000.0            # MI355X HBM3E peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384, 65536, 262144, 1048576, 0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--brute-budget-ms", type=float, default=1000.0)
    ap.add_argument("--kdtree-max", type=int, default=0)
    ap.add_argument("--no-host-export", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from sgam_neurips22_amd import _lib, geometry, pointcloud
    if not torch.cuda.is_available():
        raise SystemExit("geometry_time.py measures on the GPU: no device found")
    scene = _scene(args.frames, rgbd=False)
    coords = [c for c, _ in sorted(scene.frames.items(), key=lambda kv: (kv[1]["index"], kv[0]))]
    depths = [scene.frames[c]["depth"] for c in coords]
    rgbs = [scene.frames[c]["rgb_u8"] for c in coords]
    Ts = [scene.transform_grid[c[0]][c[1]]["T"] for c in coords]
    z0, z1 = scene._Z_RANGE[scene.data]
    F, (Hs, Ws) = len(coords), depths[0].shape
    out = {"script": "geometry_time", "frames": F, "H": Hs, "W": Ws, "repeats": args.repeats, "build": _lib.load().sgam_build_commit().decode(),
           "unit": "ms", "auto_grid_min_ref": geometry.AUTO_GRID_MIN_REF}

    # ---- unprojection: one launch against the host loop
    def unproject():
        return geometry.unproject_frames(depths, rgbs, scene.K, Ts, z0, z1)

    cloud = unproject()
    torch.cuda.synchronize()
    ms = [_timed(torch, unproject) for _ in range(args.repeats)]
    n_all = F * Hs * Ws
    moved = n_all * (4 + 3 + 12 + 3)                                   # depth + colour in, point + colour out
    out["unproject_frames"] = dict(_spread(ms), points=n_all, bytes=moved, gb_per_s=round(moved / (_spread(ms)["median"] * 1e-3) / 1e9, 1),
                                   share_of_hbm_peak=round(moved / (_spread(ms)["median"] * 1e-3) / 1e9 / HBM_GBPS, 4))
    if not args.no_host_export:
        host = []
        for _ in range(min(3, args.repeats)):
            t0 = time.perf_counter()
            for c in coords:                                           # export_point_clouds' loop without the file
                node = scene.transform_grid[c[0]][c[1]]
                Rt = np.eye(4)
                Rt[:3, :3], Rt[:3, 3] = node["R"], np.asarray(node["t"]).reshape(3)
                pointcloud.unproject_frame(scene.frames[c]["depth"].cpu().numpy(), scene.frames[c]["rgb_u8"].cpu().numpy(), scene.K, Rt)
            host.append((time.perf_counter() - t0) * 1e3)
        out["host_unproject_loop"] = _spread(host)

    pts = cloud["points"]
    valid = pts[torch.isfinite(pts).all(dim=1)].contiguous()
    shift = torch.tensor([0.003, -0.002, 0.001], dtype=torch.float32, device=pts.device)
    out["valid_points"] = int(valid.shape[0])

    # ---- nearest neighbours
    rows, per_pair, crossover = [], None, None
    for size in args.sizes:
        n = int(valid.shape[0]) if size == 0 or size > valid.shape[0] else size
        step = max(1, int(valid.shape[0]) // n)
        ref = valid[::step][:n].contiguous()
        qry = (valid[step // 2::step][:n] + shift).contiguous() if step > 1 else (valid + shift).contiguous()
        nq = int(qry.shape[0])
        row = {"n_ref": int(ref.shape[0]), "n_query": nq}
        grid = geometry.PointGrid(ref)
        row["grid"] = {"cell_size": grid.cell_size, "dims": list(grid.dims), "workspace_mb": round(grid.bytes / 2 ** 20, 1)}
        bufs = {"d2": torch.empty((nq,), dtype=torch.float32, device=pts.device), "index": torch.empty((nq,), dtype=torch.int32, device=pts.device)}
        variants = {"grid_build": lambda: geometry.PointGrid(ref), "grid_query": lambda: grid.query(qry, out=bufs)}
        run_brute = per_pair is None or per_pair * nq * ref.shape[0] <= args.brute_budget_ms
        if run_brute:
            variants["brute"] = lambda: geometry.nearest_neighbors(qry, ref, method="brute")
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        if run_brute:
            a, b = geometry.nearest_neighbors(qry, ref, method="brute"), grid.query(qry)
            row["outputs_equal"] = bool(torch.equal(a["index"], b["index"]) and torch.equal(a["d2"].view(torch.int32), b["d2"].view(torch.int32)))
        ms = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                ms[k].append(_timed(torch, fn))
        for k, v in ms.items():
            row[k + "_ms"] = _spread(v)
        g_total = row["grid_build_ms"]["median"] + row["grid_query_ms"]["median"]
        row["grid_total_ms"] = round(g_total, 4)
        if run_brute:
            per_pair = row["brute_ms"]["median"] / (nq * float(ref.shape[0]))
            row["brute_pairs_per_s"] = round(1e3 / per_pair, 0)
            row["grid_faster"] = bool(g_total < row["brute_ms"]["median"])
            if row["grid_faster"] and crossover is None:
                crossover = int(ref.shape[0])
            if not row["grid_faster"]:
                crossover = None
        if args.kdtree_max == 0 or n <= args.kdtree_max:
            from scipy.spatial import cKDTree
            r64, q64 = ref.cpu().numpy().astype(np.float64), qry.cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            tree = cKDTree(r64)
            t1 = time.perf_counter()
            dist, _ = tree.query(q64, k=1, workers=16)
            t2 = time.perf_counter()
            row["ckdtree_ms"] = {"build": round((t1 - t0) * 1e3, 1), "query_16_threads": round((t2 - t1) * 1e3, 1), "total": round((t2 - t0) * 1e3, 1)}
            got = grid.query(qry)["d2"].cpu().numpy().astype(np.float64)
            row["max_rel_diff_to_ckdtree_d2"] = float(np.max(np.abs(got - dist * dist) / np.maximum(dist * dist, 1e-30)))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del grid, ref, qry, bufs
    out["nearest_neighbours"] = rows
    out["measured_crossover_n_ref"] = crossover

    # ---- the scene-level call: unprojection of both sides, two searches, two reductions
    reference = (valid + shift).contiguous()

    def metrics():
        return scene.geometry_metrics(reference, 0.01)

    m = metrics()
    torch.cuda.synchronize()
    out["geometry_metrics"] = dict(_spread([_timed(torch, metrics) for _ in range(max(2, args.repeats // 2))]),
                                   result={k: (round(v, 8) if isinstance(v, float) else v) for k, v in m.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
