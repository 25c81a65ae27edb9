"""What rays against a mesh cost: meshops.cast_rays and meshops.visible_points by brute force against the triangle
grid — the grid's build timed on its own and included in the comparison — on mesh_distance_time.py's marching-cubes spheres.

    python scripts/mesh_raycast_time.py [--lattices 6 8 10 12 20 28 40 56 80 160 320] [--poses 4] [--repeats 5] [--brute-budget-ms 2000]

Two workloads per triangle count, from --poses pinhole cameras on a circle of radius 1.6 around the sphere (radius 0.36), looking
at its centre, 256 x 256 pixels, focal length 256 (the sphere fills about half the image):
  primary     the P x 256 x 256 pixel rays (meshops.create_rays_pinhole, timed on its own) through cast_rays;
  visibility  as many area-uniform samples of the surface as it has triangles through visible_points (N x P any-hit rays
              formed inside the kernel).
Brute force is run while the size's predicted time (pairs x the last measured time per pair) stays under --brute-budget-ms.  The
crossovers recorded are the smallest measured triangle count from which the grid (build + query) is faster at every larger
measured count, per workload.  For context only, the coloured rasteriser (tsdf.render_mesh_rgbd, depth and normals) renders the
same poses.  Per `measuring-on-mi355x`: every shape warmed up, each repeat a window of >= 0.2 s of calls between device events,
the variants alternated within a repeat, median and spread; the outputs of the two kernels compared at every size both run.  One
process, one JSON line."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from flythrough_time import _spread, _timed  # noqa: E402
from mesh_distance_time import sphere_mesh  # noqa: E402

H = W = 256
FOCAL = 256.0


def look_at_poses(n, centre=(0.5, 0.5, 0.5), radius=1.6):
    """n world -> camera poses on a circle around `centre` in the plane y = centre.y, the camera's z axis towards the centre"""
    import numpy as np
    out = []
    for k in range(n):
        a = 2 * math.pi * (k + 0.25) / n
        eye = np.array(centre) + radius * np.array([math.cos(a), 0.15, math.sin(a)])
        z = np.array(centre) - eye
        z /= np.linalg.norm(z)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, -R @ eye
        out.append(T)
    return np.stack(out).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", type=int, nargs="+", default=[6, 8, 10, 12, 20, 28, 40, 56, 80, 160, 320])
    ap.add_argument("--poses", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--brute-budget-ms", type=float, default=2000.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    from sgam_neurips22_amd import _lib, meshops, tsdf
    if not torch.cuda.is_available():
        raise SystemExit("mesh_raycast_time.py measures on the GPU: no device found")
    dev = "cuda"
    K = np.array([[FOCAL, 0, (W - 1) / 2], [0, FOCAL, (H - 1) / 2], [0, 0, 1]])
    poses = look_at_poses(args.poses)
    rays = meshops.create_rays_pinhole(poses, K, H, W)
    n_rays = int(rays.numel() // 6)
    out = {"script": "mesh_raycast_time", "repeats": args.repeats, "build": _lib.load().sgam_build_commit().decode(), "unit": "ms",
           "poses": args.poses, "rays": n_rays, "auto_grid_min_triangles_rays": meshops.AUTO_GRID_MIN_TRIANGLES_RAYS,
           "create_rays_pinhole_ms": _spread([_timed(torch, lambda: meshops.create_rays_pinhole(poses, K, H, W)) for _ in range(args.repeats)])}
    rows, per_pair, crossover = [], {"primary": None, "visibility": None}, {"primary": None, "visibility": None}
    for n in args.lattices:
        m = sphere_mesh(n)
        mesh = meshops.make_mesh(torch.from_numpy(m["vertices"]).to(dev), torch.from_numpy(m["triangles"]).to(dev))
        nt = mesh.n_triangles
        pts = meshops.sample_points(mesh, nt, seed=1, colors=False)["points"]
        grid = meshops.TriangleGrid(mesh)
        row = {"lattice": n, "triangles": nt, "samples": nt,
               "grid": {"cell_size": grid.cell_size, "dims": list(grid.dims), "entries_per_triangle": round(grid.n_entries / max(grid.n_candidates, 1), 2)}}
        vis = dict(K=K, H=H, W=W, z_near=0.05, z_far=4.0)
        variants = {"grid_build": lambda: meshops.TriangleGrid(mesh), "primary_grid": lambda: grid.cast_rays(rays),
                    "visibility_grid": lambda: grid.visible_points(pts, poses, **vis),
                    "rasteriser": lambda: tsdf.render_mesh_rgbd(mesh, K, poses, H, W, 0.05, 4.0, normals=True, rgb=False)}
        brute = {"primary": lambda: meshops.cast_rays(rays, mesh, method="brute"),
                 "visibility": lambda: meshops.visible_points(pts, mesh, poses, method="brute", **vis)}
        pairs = {"primary": float(n_rays) * nt, "visibility": float(nt) * args.poses * nt}
        for k, fn in brute.items():
            if per_pair[k] is None or per_pair[k] * pairs[k] <= args.brute_budget_ms:
                variants[k + "_brute"] = fn
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        if "primary_brute" in variants:
            a, b = meshops.cast_rays(rays, mesh, method="brute", uv=True, normals=True), grid.cast_rays(rays, uv=True, normals=True)
            row["primary_outputs_equal"] = bool(all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a))
            row["primary_hits"] = int((b["triangle"] >= 0).sum().item())
        if "visibility_brute" in variants:
            a, b = brute["visibility"](), grid.visible_points(pts, poses, **vis)
            row["visibility_outputs_equal"] = bool(torch.equal(a["count"], b["count"]))
            row["visible_samples"] = int(b["visible"].sum().item())
        ms = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                ms[k].append(_timed(torch, fn))
        for k, v in ms.items():
            row[k + "_ms"] = _spread(v)
        for k in ("primary", "visibility"):
            total = row["grid_build_ms"]["median"] + row[k + "_grid_ms"]["median"]
            row[k + "_grid_total_ms"] = round(total, 4)
            if k + "_brute" in variants:
                per_pair[k] = row[k + "_brute_ms"]["median"] / pairs[k]
                faster = bool(total < row[k + "_brute_ms"]["median"])
                row[k + "_grid_faster"] = faster
                if faster and crossover[k] is None:
                    crossover[k] = nt
                if not faster:
                    crossover[k] = None
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del grid, mesh, pts
    out["sizes"] = rows
    out["measured_crossover_triangles"] = crossover
    print(json.dumps(out))


if __name__ == "__main__":
    main()
