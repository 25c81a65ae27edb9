"""What rigid registration costs: one ICP iteration (transform, search, accumulate, update: four launches) and a whole
30-iteration geometry.register_icp, for the estimations of --estimation (default: the two geometric ones; "colored" adds coloured
ICP on the store's own colours, its gradients computed inside the timed call as a user's call does), with 65 536 source points against 65 536 / 262 144 / 1 048 576 target
points of a real frame store's cloud — beside scipy's k-d tree with a numpy Gauss-Newton loop (build + 30 x query on 16 threads:
what a user does today) — and scene.frame_drift of the whole scene.

    python scripts/icp_time.py [--frames 32] [--source 65536] [--targets 65536 262144 1048576] [--iterations 30] [--repeats 3]
                               [--distance 0.05] [--kdtree-max 0] [--estimation point_to_plane point_to_point colored]

The scene is geometry_time.py's: a GoogleEarth run on the splat branch (synthetic weights, 256 x 256, `--frames` frames).  The target
of a size is a strided sample of the store's valid points with normals from estimate_normals (k = 16, not timed here: cloud_time.py
does); the source is a strided sample of the target moved by 1 degree / 0.01 about the cloud's centre.  The stop criteria are set
to 0 so that every run does all its iterations.  Per `measuring-on-mi355x`: every shape warmed up, each repeat a window of >= 0.2 s
of calls between device events, the variants alternated within a repeat, median and spread.  One process, one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from flythrough_time import _spread, _timed  # noqa: E402
from pointview_time import _scene  # noqa: E402


def _rodrigues(np, w):
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / (th * th) * K @ K


def _host_icp(np, tree, src, tgt, nrm, distance, iterations):
    """the same Gauss-Newton loop with scipy's k-d tree (16 threads) and numpy in float64 -> (pose, seconds in the queries)"""
    T, in_query = np.eye(4), 0.0
    for _ in range(iterations):
        p = src @ T[:3, :3].T + T[:3, 3]
        t0 = time.perf_counter()
        dist, idx = tree.query(p, k=1, distance_upper_bound=distance, workers=16)
        in_query += time.perf_counter() - t0
        ok = np.isfinite(dist)
        p, q = p[ok], tgt[idx[ok]]
        if nrm is not None:
            n = nrm[idx[ok]]
            J = np.concatenate([np.cross(p, n), n], axis=1)
            r = ((p - q) * n).sum(1)
            A, g = J.T @ J, J.T @ r
        else:
            e = p - q
            S = (p[:, :, None] * p[:, None, :]).sum(0)
            A = np.zeros((6, 6))
            A[:3, :3] = np.trace(S) * np.eye(3) - S
            sp = p.sum(0)
            A[:3, 3:] = np.array([[0, -sp[2], sp[1]], [sp[2], 0, -sp[0]], [-sp[1], sp[0], 0]])
            A[3:, :3] = A[:3, 3:].T
            A[3:, 3:] = len(p) * np.eye(3)
            g = np.concatenate([np.cross(p, e).sum(0), e.sum(0)])
        xi = -np.linalg.solve(A, g)
        dT = np.eye(4)
        dT[:3, :3], dT[:3, 3] = _rodrigues(np, xi[:3]), xi[3:]
        T = dT @ T
    return T, in_query


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--source", type=int, default=65536)
    ap.add_argument("--targets", type=int, nargs="+", default=[65536, 262144, 1048576])
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--distance", type=float, default=0.05)
    ap.add_argument("--kdtree-max", type=int, default=0)
    ap.add_argument("--estimation", nargs="+", default=["point_to_plane", "point_to_point"],
                    choices=["point_to_plane", "point_to_point", "colored"])
    args = ap.parse_args()
    import numpy as np
    import torch
    from sgam_neurips22_amd import _lib, geometry
    if not torch.cuda.is_available():
        raise SystemExit("icp_time.py measures on the GPU: no device found")
    scene = _scene(args.frames, rgbd=False)
    cloud = scene.merged_point_cloud()
    pts = cloud["points"]
    is_point = torch.isfinite(pts).all(dim=1)
    valid, valid_colors = pts[is_point].contiguous(), cloud["colors"][is_point].contiguous()
    n_valid = int(valid.shape[0])
    out = {"script": "icp_time", "frames": len(scene.frames), "valid_points": n_valid, "repeats": args.repeats, "iterations": args.iterations,
           "max_correspondence_distance": args.distance, "build": _lib.load().sgam_build_commit().decode(), "unit": "ms"}
    centre = valid.double().mean(0).cpu().numpy()
    C = np.eye(4)
    C[:3, 3] = centre
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = _rodrigues(np, np.radians(1.0) * np.array([0.2, 1.0, -0.4]) / np.linalg.norm([0.2, 1.0, -0.4])), [0.006, -0.005, 0.006]
    M = C @ M @ np.linalg.inv(C)

    rows = []
    for size in args.targets:
        n = min(size, n_valid)
        tgt, tgt_colors = valid[::max(1, n_valid // n)][:n].contiguous(), valid_colors[::max(1, n_valid // n)][:n].contiguous()
        nrm = geometry.estimate_normals(tgt, 16)
        ns = min(args.source, n)
        src, src_colors = geometry.transform_points(tgt[::max(1, n // ns)][:ns].contiguous(), M), tgt_colors[::max(1, n // ns)][:ns].contiguous()
        row = {"n_target": n, "n_source": int(src.shape[0])}
        variants, truth = {}, np.linalg.inv(M)
        for name in args.estimation:
            normals = None if name == "point_to_point" else nrm
            colours = dict(source_colors=src_colors, target_colors=tgt_colors) if name == "colored" else {}
            # (one iteration: the gradients are there, as they are from the second iteration of a registration on)
            colored = (src_colors, tgt_colors, geometry.color_gradients(tgt, nrm, tgt_colors), geometry.LAMBDA_GEOMETRIC) if colours else None
            c = geometry._Correspondences(src, tgt, args.distance, "auto", None, "icp_time")
            state = geometry.icp_state(None, src.device, "icp_time")
            history = torch.zeros((1, geometry.ICP_ROW), dtype=torch.float64, device=src.device)

            def iteration(c=c, state=state, history=history, normals=normals, colored=colored):
                geometry.icp_update(c.step(state[:16].view(4, 4), normals, colored), 0, 0.0, 0.0, state, history)

            def whole(name=name, normals=normals, colours=colours):
                return geometry.register_icp(src, tgt, args.distance, estimation=name, target_normals=normals, max_iterations=args.iterations,
                                             relative_fitness=0.0, relative_rmse=0.0, check_every=None, **colours)

            variants[name + "_iteration"], variants[name + f"_register_{args.iterations}"] = iteration, whole
            reg = whole()
            T = reg["transformation"].cpu().numpy()
            row[name] = {"method": "grid" if isinstance(c.search, geometry.PointGrid) else "brute", "iterations": reg["iterations"], "status": reg["status"],
                         "fitness": reg["fitness"], "inlier_rmse": reg["inlier_rmse"], "rotation_error": float(np.linalg.norm(T[:3, :3] - truth[:3, :3])),
                         "translation_error": float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))}
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                ms[k].append(_timed(torch, fn))
        for k, v in ms.items():
            row[k + "_ms"] = _spread(v)
        if args.kdtree_max == 0 or n <= args.kdtree_max:
            from scipy.spatial import cKDTree
            s64, t64, n64 = src.cpu().numpy().astype(np.float64), tgt.cpu().numpy().astype(np.float64), nrm.cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            tree = cKDTree(t64)
            row["ckdtree_build_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            for name, normals in (("point_to_plane", n64), ("point_to_point", None)):
                if name not in args.estimation:
                    continue
                t0 = time.perf_counter()
                T, in_query = _host_icp(np, tree, s64, t64, normals, args.distance, args.iterations)
                row[f"ckdtree_numpy_{name}_{args.iterations}_16_threads_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                row[f"ckdtree_numpy_{name}_queries_ms"] = round(in_query * 1e3, 1)
                row[f"ckdtree_numpy_{name}_translation_error"] = float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del variants, tgt, nrm, src, tgt_colors, src_colors
    out["registrations"] = rows

    def drift():
        return scene.frame_drift(args.distance, max_iterations=args.iterations)

    d = drift()
    torch.cuda.synchronize()
    out["frame_drift"] = dict(_spread([_timed(torch, drift) for _ in range(args.repeats)]), entries=len(d),
                              converged=sum(1 for e in d if e["converged"]), degenerate=sum(1 for e in d if e["status"] == 2),
                              median_rotation_deg=float(np.nanmedian([e["rotation_deg"] for e in d])),
                              median_translation=float(np.nanmedian([e["translation"] for e in d])))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
