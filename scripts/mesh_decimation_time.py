"""quadric-error decimation of a finished scene's mesh on the bench scene's final mesh — the rgbd_integration loop
of scripts/mesh_loop.py (bench.py's model and scene, STEPS frames after WARMUP), then colour_volume().extract_mesh_device() —:
meshops.simplify_quadric_decimation to 50 %, 10 % and 1 % of the triangles of the raw and of the `clean`-ed mesh, median [min -
max] ms of REPEATS runs after one warm-up, with the round count; the split of the rounds between the incidence rebuild, the edge
kernel and the rest; the distance from the original surface to the result (meshops.point_mesh_distance from SAMPLES area-uniform
samples) beside vertex clustering at the same triangle count; rounds and error at oversample 1, 2 and 4; and the numpy twin
(tests/decimation_oracle.py) once on a 129 x 129 bumped sheet beside the device, for scale.  SCENE=0 skips the scene."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from sgam_neurips22_amd import _lib, meshops
import decimation_oracle as DO
from test_decimation_cpu import grid

repeats, samples = max(5, int(os.environ.get("REPEATS", 5))), int(os.environ.get("SAMPLES", 65536))
dev = torch.device("cuda", 0)
lib = _lib.load()
print(f"build {lib.sgam_build_commit().decode()} digest {lib.sgam_build_digest().decode()}", flush=True)


def timed(name, fn, n=repeats):
    fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t))
    print(f"{name:52s} {np.median(ts):9.2f} ms [{min(ts):.2f} - {max(ts):.2f}] over {n}", flush=True)
    return out


def mean_distance(points, mesh):
    tree = meshops.TriangleBVH(mesh)
    return float(meshops.point_mesh_distance(points, mesh, accel=tree)["d2"].double().sqrt().mean())


def study(label, mesh, ratios, cluster_voxels=()):
    pts = meshops.sample_points(mesh, samples, seed=0, colors=False)["points"]
    nt = mesh.n_triangles
    for r in ratios:
        out = timed(f"{label}: decimate to {100 * r:g} %", lambda: meshops.simplify_quadric_decimation(mesh, target_ratio=r))
        print(f"  -> {out['mesh'].n_vertices} vertices, {out['mesh'].n_triangles} triangles, {out['rounds']} rounds, max_cost {out['max_cost']:.3e}, "
              f"{out['stopped']}; mean distance to the original surface {mean_distance(pts, out['mesh']):.4e}", flush=True)
    meshops.ROUND_SECONDS = {}
    meshops.simplify_quadric_decimation(mesh, target_ratio=ratios[1])
    total = sum(meshops.ROUND_SECONDS.values())
    print(f"  split of the rounds to {100 * ratios[1]:g} % (each phase synchronised): " +
          ", ".join(f"{k} {1e3 * v:.1f} ms ({100 * v / total:.0f} %)" for k, v in meshops.ROUND_SECONDS.items()), flush=True)
    meshops.ROUND_SECONDS = None
    for h in cluster_voxels:
        vc = timed(f"{label}: simplify_vertex_clustering({h:g})", lambda: meshops.simplify_vertex_clustering(mesh, h))["mesh"]
        qd = meshops.simplify_quadric_decimation(mesh, target_triangles=vc.n_triangles)
        print(f"  at {vc.n_triangles} / {qd['mesh'].n_triangles} triangles ({100 * vc.n_triangles / nt:.1f} %): mean distance clustering "
              f"{mean_distance(pts, vc):.4e}, decimation {mean_distance(pts, qd['mesh']):.4e} ({qd['rounds']} rounds)", flush=True)
    for o in (1.0, 2.0, 4.0):
        t = time.perf_counter()
        out = meshops.simplify_quadric_decimation(mesh, target_ratio=ratios[1], oversample=o)
        torch.cuda.synchronize()
        print(f"  oversample {o:g} to {100 * ratios[1]:g} %: {out['rounds']} rounds, {1e3 * (time.perf_counter() - t):.1f} ms, max_cost {out['max_cost']:.3e}, "
              f"mean distance {mean_distance(pts, out['mesh']):.4e}", flush=True)


v, t, c = grid(129, bump=True)
sheet = meshops.make_mesh(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(c).to(dev))
print(f"bumped sheet: {len(v)} vertices, {len(t)} triangles", flush=True)
study("sheet", sheet, (0.5, 0.1, 0.01), cluster_voxels=(1 / 16,))
if os.environ.get("HOST", "1") != "0":
    t0 = time.perf_counter()
    w = DO.decimate(v, t, c, target_ratio=0.1)
    print(f"twin, sheet to 10 %: {time.perf_counter() - t0:.1f} s (host, once), {w['rounds']} rounds", flush=True)
    g = meshops.simplify_quadric_decimation(sheet, target_ratio=0.1)
    same = np.array_equal(w["vertices"].view(np.uint32), g["mesh"].vertices.cpu().numpy().view(np.uint32)) and \
        np.array_equal(w["triangles"], g["mesh"].triangles.cpu().numpy()) and w["rounds"] == g["rounds"]
    print(f"the device equals the twin bit for bit: {same}", flush=True)

if os.environ.get("SCENE", "1") != "0":
    from bench import build_model, DATASET
    from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
    steps, warmup = int(os.environ.get("STEPS", 31)), int(os.environ.get("WARMUP", 3))
    model, sd, p = build_model(dev)
    model.enable_hip_graph(os.environ.get("NO_GRAPH", "0") != "1")
    sc = InfiniteSceneGeneration(model, DATASET, seed_index=0, output_dim=(steps + warmup + 4, 1), seed_frame=synthetic_seed_frame(DATASET, 0),
                                 use_rgbd_integration=True)
    for _ in range(steps + warmup):
        sc.one_step_prediction(sc.next_pose(sc.curr)); sc.curr += 1
    mesh = sc.colour_volume().extract_mesh_device()
    voxel = sc.volume.voxel_length
    print(f"bench scene after {steps + warmup} frames: {mesh.n_vertices} vertices, {mesh.n_triangles} triangles, voxel {voxel}", flush=True)
    study("scene", mesh, (0.5, 0.1, 0.01), cluster_voxels=(2 * voxel, 4 * voxel))
    kw = dict(min_triangles=100, smooth_iterations=5, voxel_size=2 * voxel)
    cleaned = meshops.clean(mesh, **kw)["mesh"]
    print(f"clean({kw}): {cleaned.n_vertices} vertices, {cleaned.n_triangles} triangles", flush=True)
    study("cleaned", cleaned, (0.5, 0.1, 0.01))
