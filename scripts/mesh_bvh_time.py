"""What the triangle BVH costs against the triangle grid: build and query of meshops.TriangleGrid and
meshops.TriangleBVH on two families of meshes — mesh_distance_time.py's marching-cubes spheres (uniform triangles: the grid's home
ground) and the same spheres inside a room of twelve large triangles (a box of edge --room around the unit box: the mixed-scale
case the BVH exists for).

    python scripts/mesh_bvh_time.py [--lattices 12 28 56 80 160] [--poses 4] [--repeats 5] [--room 10] [--window-ms 200]

Three workloads per mesh, as in mesh_distance_time.py and mesh_raycast_time.py:
  distance    as many queries as triangles, area-uniform samples of the sphere moved by N(0, 2 / lattice), through .query;
  primary     the P x 256 x 256 pixel rays of --poses cameras on a circle of radius 1.6 around the sphere through .cast_rays;
  visibility  as many samples of the sphere as it has triangles through .visible_points (N x P any-hit rays formed in the kernel).
Per `measuring-on-mi355x`: every shape warmed up, each repeat a window of >= --window-ms of calls between device events, grid and
BVH alternated within a repeat on the same device, median with the range; the outputs of the two compared at every size (equal
bits).  Memory per triangle and the tree's height are reported with the times.  One process, one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from flythrough_time import _spread, _timed  # noqa: E402
from mesh_distance_time import sphere_mesh  # noqa: E402
from mesh_raycast_time import FOCAL, H, W, look_at_poses  # noqa: E402


def with_room(m, edge):
    """the mesh and the twelve triangles of a box of the given edge around the unit box's centre"""
    import numpy as np
    v, t = m["vertices"], m["triangles"]
    corners = (np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], dtype=np.float64) * (edge / 2) + 0.5).astype(np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    box = np.array([tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))], dtype=np.int32) + len(v)
    return {"vertices": np.concatenate([v, corners]), "triangles": np.concatenate([t, box])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattices", type=int, nargs="+", default=[12, 28, 56, 80, 160])
    ap.add_argument("--poses", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--room", type=float, default=10.0)
    ap.add_argument("--window-ms", type=float, default=200.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    from sgam_neurips22_amd import _lib, meshops
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bvh_time.py measures on the GPU: no device found")
    dev = "cuda"
    K = np.array([[FOCAL, 0, (W - 1) / 2], [0, FOCAL, (H - 1) / 2], [0, 0, 1]])
    poses = look_at_poses(args.poses)
    rays = meshops.create_rays_pinhole(poses, K, H, W)
    vis = dict(K=K, H=H, W=W, z_near=0.05, z_far=4.0)
    out = {"script": "mesh_bvh_time", "repeats": args.repeats, "build": _lib.load().sgam_build_commit().decode(), "unit": "ms", "poses": args.poses,
           "rays": int(rays.numel() // 6), "room_edge": args.room}
    rows = []
    for n in args.lattices:
        sphere = sphere_mesh(n)
        for family, m in (("uniform", sphere), ("mixed", with_room(sphere, args.room))):
            mesh = meshops.make_mesh(torch.from_numpy(m["vertices"]).to(dev), torch.from_numpy(m["triangles"]).to(dev))
            ball = meshops.make_mesh(torch.from_numpy(sphere["vertices"]).to(dev), torch.from_numpy(sphere["triangles"]).to(dev))
            nt = mesh.n_triangles
            pts = meshops.sample_points(ball, ball.n_triangles, seed=1, colors=False)["points"]
            qry = (pts + torch.randn(pts.shape, device=dev, generator=torch.Generator(dev).manual_seed(n)) * (2.0 / n)).contiguous()
            grid, bvh = meshops.TriangleGrid(mesh), meshops.TriangleBVH(mesh)
            row = {"family": family, "lattice": n, "triangles": nt, "queries": int(qry.shape[0]),
                   "grid": {"cell_size": grid.cell_size, "dims": list(grid.dims), "entries_per_triangle": round(grid.n_entries / max(grid.n_candidates, 1), 2),
                            "bytes_per_triangle": round(grid.bytes / nt, 1)},
                   "bvh": {"height": bvh.height, "nodes": bvh.n_nodes, "bytes_per_triangle": round(bvh.bytes / nt, 1)}}
            variants = {}
            for name, acc, cls in (("grid", grid, meshops.TriangleGrid), ("bvh", bvh, meshops.TriangleBVH)):
                variants[name + "_build"] = lambda cls=cls: cls(mesh)
                variants[name + "_distance"] = lambda acc=acc: acc.query(qry)
                variants[name + "_primary"] = lambda acc=acc: acc.cast_rays(rays)
                variants[name + "_visibility"] = lambda acc=acc: acc.visible_points(pts, poses, **vis)
            for fn in variants.values():
                fn()
            torch.cuda.synchronize()
            a, b = grid.query(qry, closest=True), bvh.query(qry, closest=True)
            c, d = grid.cast_rays(rays, uv=True, normals=True), bvh.cast_rays(rays, uv=True, normals=True)
            row["outputs_equal"] = bool(all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a) and
                                        all(torch.equal(c[k].view(torch.int32), d[k].view(torch.int32)) for k in c) and
                                        torch.equal(grid.visible_points(pts, poses, **vis)["count"], bvh.visible_points(pts, poses, **vis)["count"]))
            row["primary_hits"] = int((d["triangle"] >= 0).sum().item())
            ms = {k: [] for k in variants}
            for _ in range(args.repeats):
                for k, fn in variants.items():
                    ms[k].append(_timed(torch, fn, args.window_ms))
            for k, v in ms.items():
                row[k + "_ms"] = _spread(v)
            for k in ("distance", "primary", "visibility"):
                row[k + "_bvh_over_grid"] = round(row["bvh_" + k + "_ms"]["median"] / row["grid_" + k + "_ms"]["median"], 3)
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del grid, bvh, mesh, ball, pts, qry
    out["sizes"] = rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
