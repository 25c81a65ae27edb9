"""What segmenting a cloud costs: the fixed-radius count and the whole of DBSCAN (count, link, border, labels),
brute force against the grid, from 1 k to 1 M points (the crossover of method="auto"); the plane-score kernel at 64, 256 and 1000
hypotheses x 1 M points for each number R of hypotheses per lane (R0: the library's choice); segment_planes as a whole; and the CPU
context where the packages exist: sklearn's DBSCAN and a numpy plane score on the same clouds.

    python scripts/segmentation_time.py [--sizes 1024 4096 16384 65536 1048576] [--hypotheses 64 256 1000] [--repeats 5]
                                        [--brute-budget-ms 30000] [--sklearn-max 65536] [--out profiles/segmentation_time.json]

The cloud of a size is seeded: 60 % of the points on a floor (z noise 0.002), the rest in 24 boxes standing on it, scaled so that a
point has about 20 neighbours within eps = 0.05 on the floor.  Brute force is run while its predicted time (pairs x the last
measured time per pair) stays under --brute-budget-ms, at the largest size in one window of one call.  The per-launch split of a
DBSCAN call comes from the library's kernel timeline in a run of its own.  Per `measuring-on-mi355x`: every shape warmed up, each
repeat a window of >= 0.2 s of calls between device events, the variants alternated within a repeat, median and spread; the
outputs of the variants compared at every size both run.  One process, one JSON line, also written to --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from flythrough_time import _spread, _timed  # noqa: E402

EPS, MIN_POINTS, THRESHOLD = 0.05, 10, 0.01


def make_cloud(np, n, seed=0):
    rs = np.random.RandomState(seed)
    nf = (6 * n) // 10
    side = float(np.sqrt(nf * np.pi * EPS * EPS / 20.0))
    floor = np.c_[rs.rand(nf, 2) * side, rs.randn(nf) * 0.002]
    nb = n - nf
    centres = rs.rand(24, 2) * side * 0.9 + side * 0.05
    which = rs.randint(0, 24, nb)
    half = side / 40.0
    boxes = np.c_[centres[which] + (rs.rand(nb, 2) * 2 - 1) * half, 0.05 + rs.rand(nb) * 4 * half]
    return np.concatenate([floor, boxes]).astype(np.float32)[rs.permutation(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096, 16384, 65536, 1048576])
    ap.add_argument("--hypotheses", type=int, nargs="+", default=[64, 256, 1000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--brute-budget-ms", type=float, default=30000.0)
    ap.add_argument("--sklearn-max", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segmentation_time.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from sgam_neurips22_amd import _lib, geometry, ops_aux
    if not torch.cuda.is_available():
        raise SystemExit("segmentation_time.py measures on the GPU: no device found")
    out = {"script": "segmentation_time", "build": _lib.load().sgam_build_commit().decode(), "unit": "ms", "repeats": args.repeats,
           "eps": EPS, "min_points": MIN_POINTS, "threshold": THRESHOLD, "auto_radius_grid_min": geometry.AUTO_RADIUS_GRID_MIN,
           "auto_radius_count_grid_min": geometry.AUTO_RADIUS_COUNT_GRID_MIN}

    # ---- fixed radius and DBSCAN
    rows, per_pair, crossover = [], None, None
    for n in args.sizes:
        host = make_cloud(np, n)
        pts = torch.from_numpy(host).cuda()
        row = {"n": n}
        variants = {"grid_build": lambda: geometry.PointGrid(pts, EPS),
                    "count_grid": lambda: geometry.radius_count(pts, EPS, method="grid"),
                    "dbscan_grid": lambda: geometry.cluster_dbscan(pts, EPS, MIN_POINTS, method="grid")}
        brute = per_pair is None or per_pair * n * n <= args.brute_budget_ms
        if brute:
            variants["count_brute"] = lambda: geometry.radius_count(pts, EPS, method="brute")
            variants["dbscan_brute"] = lambda: geometry.cluster_dbscan(pts, EPS, MIN_POINTS, method="brute")
        long_brute = brute and per_pair is not None and per_pair * n * n > 200.0        # one call already fills the window
        g = geometry.cluster_dbscan(pts, EPS, MIN_POINTS, method="grid")
        row["n_clusters"], row["noise"], row["core"] = int(g["n_clusters"]), int((g["labels"] < 0).sum()), int(g["core"].sum())
        row["mean_neighbours"] = float(g["count"].float().mean())
        if brute:
            b = geometry.cluster_dbscan(pts, EPS, MIN_POINTS, method="brute")
            row["outputs_equal"] = bool(all(torch.equal(g[k], b[k]) for k in g))
        torch.cuda.synchronize()
        ms = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name, fn in variants.items():
                if long_brute and name.endswith("_brute") and ms[name]:
                    continue
                ms[name].append(_timed(torch, fn))
        for name, v in ms.items():
            row[name + "_ms"] = dict(_spread(v), windows=len(v))
        if brute:
            per_pair = row["count_brute_ms"]["median"] / (float(n) * n)
            row["grid_faster"] = bool(row["dbscan_grid_ms"]["median"] < row["dbscan_brute_ms"]["median"])      # (the grid's build included)
            crossover = (crossover or n) if row["grid_faster"] else None
        else:
            row["count_brute_ms"] = row["dbscan_brute_ms"] = "not measured"
        for method in ("grid", "brute") if brute and not long_brute else ("grid",):
            recs, bracket = ops_aux.kernel_timeline(lambda: geometry.cluster_dbscan(pts, EPS, MIN_POINTS, method=method))
            split = {}
            for name, t, *_ in recs:
                split[name] = round(split.get(name, 0.0) + max(t - bracket, 0.0), 4)
            row[f"dbscan_{method}_kernels_ms"] = split
        if n <= args.sklearn_max:
            try:
                from sklearn.cluster import DBSCAN
                t0 = time.perf_counter()
                ref = DBSCAN(eps=EPS, min_samples=MIN_POINTS, n_jobs=16).fit(host.astype(np.float64))
                row["sklearn_dbscan_16_jobs_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                row["sklearn_n_clusters"] = int(ref.labels_.max() + 1)
            except ImportError:
                row["sklearn_dbscan_16_jobs_ms"] = "package missing"
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del pts, g
    out["dbscan"] = rows
    out["measured_crossover_n"] = crossover

    # ---- the plane score at H x the largest size, per R; segment_planes as a whole
    n = max(args.sizes)
    host = make_cloud(np, n)
    pts = torch.from_numpy(host).cuda()
    out["plane_score"] = []
    for H in args.hypotheses:
        rs = np.random.RandomState(1)
        pick = host[rs.randint(0, n, (H, 3))].astype(np.float64)
        nrm = np.cross(pick[:, 1] - pick[:, 0], pick[:, 2] - pick[:, 0])
        nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
        planes_h = np.c_[nrm, -(nrm * pick[:, 0]).sum(1)].astype(np.float32)
        planes = torch.from_numpy(planes_h).cuda()
        score = {"n": n, "hypotheses": H, "pairs": float(n) * H}
        variants = {f"R{R}": (lambda R=R: geometry.plane_score(pts, planes, THRESHOLD, hypotheses_per_lane=R)) for R in (0, 1, 2, 4)}
        counts = {name: fn() for name, fn in variants.items()}
        score["outputs_equal"] = bool(all(torch.equal(counts["R1"], c) for c in counts.values()))
        torch.cuda.synchronize()
        ms = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name, fn in variants.items():
                ms[name].append(_timed(torch, fn))
        for name, v in ms.items():
            score[name + "_ms"] = _spread(v)
            score[name + "_pairs_per_ns"] = round(score["pairs"] / (score[name + "_ms"]["median"] * 1e6), 2)
        if H == max(args.hypotheses):
            t0 = time.perf_counter()
            want = np.zeros(H, dtype=np.int64)
            for h0 in range(0, H, 25):
                pl = planes_h[h0:h0 + 25]
                e = ((pl[:, 0:1] * host[None, :, 0] + pl[:, 1:2] * host[None, :, 1]) + pl[:, 2:3] * host[None, :, 2]) + pl[:, 3:4]
                want[h0:h0 + 25] = (np.abs(e) <= np.float32(THRESHOLD)).sum(axis=1)
            score["numpy_score_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            score["equal_to_numpy"] = bool(np.array_equal(want, counts["R1"].cpu().numpy()))
        out["plane_score"].append(score)
        print(json.dumps(score), file=sys.stderr, flush=True)
    H = max(args.hypotheses)
    seg = geometry.segment_planes(pts, THRESHOLD, 1, 3, H, 0)
    whole = lambda: geometry.segment_planes(pts, THRESHOLD, 1, 3, H, 0)  # noqa: E731
    out["segment_planes"] = dict(_spread([_timed(torch, whole) for _ in range(args.repeats)]), n=n, hypotheses=H, max_planes=1,
                                 count=int(seg["counts"][0]))
    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
