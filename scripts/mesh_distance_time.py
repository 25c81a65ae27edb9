"""What the queries against a mesh cost: meshops.point_mesh_distance by brute force against the triangle grid —
the grid's build (area pass, box, count, scan, scatter) timed on its own and included in the comparison — on a marching-cubes
sphere at several triangle counts with as many queries as triangles, and meshops.sample_points at the same counts.

    python scripts/mesh_distance_time.py [--lattices 6 8 10 12 20 28 40 56 80 160 320] [--repeats 5] [--brute-budget-ms 2000]

The mesh of a lattice size n is the zero surface of clip((|x - c| - 0.36 n) / 4, -1, 1) on an n^3 lattice of voxel 1 / n
(tests/mc_oracle.py, the host marching cubes the mesh tests use): about 4.8 n^2 triangles near the voxel scale.  The queries are
area-uniform samples of the surface moved by a Gaussian of two voxels: points near the surface, what surface_metrics asks.  Brute
force is run while the size's predicted time (pairs x the last measured time per pair) stays under --brute-budget-ms.  The
crossover recorded is the smallest measured triangle count from which the grid (build + query) is faster at every larger
measured count.  Per `measuring-on-mi355x`: every shape warmed up, each repeat a window of >= 0.2 s of calls between device
events, the variants alternated within a repeat, median and spread; the outputs of the two kernels compared at every size both
run.  One process, one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from flythrough_time import _spread, _timed  # noqa: E402


def sphere_mesh(n):
    import numpy as np
    import mc_oracle
    x = np.arange(n, dtype=np.float64)
    zz, yy, xx = np.meshgrid(x, x, x, indexing="ij")
    c = (n / 2 + 0.2, n / 2 - 0.3, n / 2 + 0.1)
    d = np.sqrt((xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2) - 0.36 * n
    return mc_oracle.marching_cubes(np.clip(d / 4.0, -1.0, 1.0).astype(np.float32), 1.0 / n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", type=int, nargs="+", default=[6, 8, 10, 12, 20, 28, 40, 56, 80, 160, 320])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--brute-budget-ms", type=float, default=2000.0)
    args = ap.parse_args()
    import torch
    from sgam_neurips22_amd import _lib, meshops
    if not torch.cuda.is_available():
        raise SystemExit("mesh_distance_time.py measures on the GPU: no device found")
    dev = "cuda"
    out = {"script": "mesh_distance_time", "repeats": args.repeats, "build": _lib.load().sgam_build_commit().decode(), "unit": "ms",
           "auto_grid_min_triangles": meshops.AUTO_GRID_MIN_TRIANGLES}
    rows, per_pair, crossover = [], None, None
    for n in args.lattices:
        m = sphere_mesh(n)
        mesh = meshops.make_mesh(torch.from_numpy(m["vertices"]).to(dev), torch.from_numpy(m["triangles"]).to(dev))
        nt = mesh.n_triangles
        qry = (meshops.sample_points(mesh, nt, seed=1)["points"] + torch.randn((nt, 3), device=dev, generator=torch.Generator(dev).manual_seed(n))
               * (2.0 / n)).contiguous()
        grid = meshops.TriangleGrid(mesh)
        row = {"lattice": n, "triangles": nt, "queries": nt,
               "grid": {"cell_size": grid.cell_size, "dims": list(grid.dims), "entries_per_triangle": round(grid.n_entries / max(grid.n_candidates, 1), 2),
                        "workspace_mb": round(grid.bytes / 2 ** 20, 2)}}
        variants = {"grid_build": lambda: meshops.TriangleGrid(mesh), "grid_query": lambda: grid.query(qry),
                    "sample_points": lambda: meshops.sample_points(mesh, nt, seed=2)}
        run_brute = per_pair is None or per_pair * nt * float(nt) <= args.brute_budget_ms
        if run_brute:
            variants["brute"] = lambda: meshops.point_mesh_distance(qry, mesh, method="brute")
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        if run_brute:
            a, b = meshops.point_mesh_distance(qry, mesh, method="brute", closest=True), grid.query(qry, closest=True)
            row["outputs_equal"] = bool(all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in ("d2", "triangle", "closest")))
        ms = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                ms[k].append(_timed(torch, fn))
        for k, v in ms.items():
            row[k + "_ms"] = _spread(v)
        g_total = row["grid_build_ms"]["median"] + row["grid_query_ms"]["median"]
        row["grid_total_ms"] = round(g_total, 4)
        if run_brute:
            per_pair = row["brute_ms"]["median"] / (nt * float(nt))
            row["brute_pairs_per_s"] = round(1e3 / per_pair, 0)
            row["grid_faster"] = bool(g_total < row["brute_ms"]["median"])
            if row["grid_faster"] and crossover is None:
                crossover = nt
            if not row["grid_faster"]:
                crossover = None
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del grid, mesh, qry
    out["sizes"] = rows
    out["measured_crossover_triangles"] = crossover
    print(json.dumps(out))


if __name__ == "__main__":
    main()
