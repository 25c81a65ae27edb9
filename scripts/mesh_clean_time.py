"""mesh clean-up of a finished scene on the bench scene's final mesh — the rgbd_integration loop of
scripts/mesh_loop.py (bench.py's model and scene, STEPS frames after WARMUP), then colour_volume().extract_mesh_device() —: every
operation of sgam_neurips22_amd/meshops.py and the whole `clean`, median [min - max] ms of REPEATS runs after one warm-up, beside
the numpy twin (tests/meshops_oracle.py) and the host tsdf.vertex_normals on the same arrays (once each, for comparison only)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from bench import build_model, DATASET
from sgam_neurips22_amd import meshops, tsdf
from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
import meshops_oracle as MO

steps, warmup, repeats = int(os.environ.get("STEPS", 31)), int(os.environ.get("WARMUP", 3)), max(5, int(os.environ.get("REPEATS", 5)))
host = os.environ.get("HOST", "1") != "0"
dev = torch.device("cuda", 0)
model, sd, p = build_model(dev)
model.enable_hip_graph(os.environ.get("NO_GRAPH", "0") != "1")
sc = InfiniteSceneGeneration(model, DATASET, seed_index=0, output_dim=(steps + warmup + 4, 1), seed_frame=synthetic_seed_frame(DATASET, 0),
                             use_rgbd_integration=True)
for _ in range(steps + warmup):
    sc.one_step_prediction(sc.next_pose(sc.curr)); sc.curr += 1
mesh = sc.colour_volume().extract_mesh_device()
voxel = sc.volume.voxel_length
print(f"bench scene after {steps + warmup} frames: {mesh.n_vertices} vertices, {mesh.n_triangles} triangles, voxel {voxel}", flush=True)


def timed(name, fn, n=repeats):
    fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t))
    print(f"{name:44s} {np.median(ts):9.2f} ms [{min(ts):.2f} - {max(ts):.2f}] over {n}", flush=True)
    return out


def once(name, fn):
    t = time.perf_counter()
    out = fn()
    print(f"{name:44s} {1e3 * (time.perf_counter() - t):9.2f} ms (host, once)", flush=True)
    return out


kw = dict(min_triangles=100, smooth_iterations=5, voxel_size=2 * voxel)
comp = timed("components", lambda: meshops.components(mesh))
n = comp["n_triangles"]
print(f"  {len(n)} components, the largest {int(n.max())} triangles, {int((n < 100).sum())} below 100 triangles")
timed("remove_small_components(min_triangles=100)", lambda: meshops.remove_small_components(mesh, min_triangles=100))
timed("incidence('triangles')", lambda: meshops.incidence(mesh, "triangles"))
csr = timed("incidence('vertices')", lambda: meshops.incidence(mesh, "vertices"))
print(f"  largest vertex degree {int(torch.diff(csr['offsets']).max())}")
timed("vertex_normals", lambda: meshops.vertex_normals(mesh))
timed("smooth_taubin(iterations=5)", lambda: meshops.smooth_taubin(mesh, 5))
s = timed(f"simplify_vertex_clustering({2 * voxel:g})", lambda: meshops.simplify_vertex_clustering(mesh, 2 * voxel))
print(f"  -> {s['mesh'].n_vertices} vertices, {s['mesh'].n_triangles} triangles")
c = timed(f"clean({kw})", lambda: meshops.clean(mesh, **kw))
print(f"  -> {c['mesh'].n_vertices} vertices, {c['mesh'].n_triangles} triangles")
if host:
    v, t = mesh.vertices[:mesh.n_vertices].cpu().numpy(), mesh.triangles[:mesh.n_triangles].cpu().numpy()
    col = mesh.vertex_colors[:mesh.n_vertices].cpu().numpy()
    once("host tsdf.vertex_normals", lambda: tsdf.vertex_normals(v, t))
    once("twin components", lambda: MO.components(t, len(v)))
    once("twin vertex_normals", lambda: MO.vertex_normals(v, t))
    once("twin smooth_taubin(iterations=5)", lambda: MO.smooth_taubin(v, t, 5))
    once("twin simplify_vertex_clustering", lambda: MO.simplify_vertex_clustering(v, t, 2 * voxel, col))
    w = once("twin clean", lambda: MO.clean(v, t, col, **kw))
    same = np.array_equal(w["vertices"].view(np.uint32), c["mesh"].vertices.cpu().numpy().view(np.uint32)) and \
        np.array_equal(w["triangles"], c["mesh"].triangles.cpu().numpy()) and \
        np.array_equal(w["vertex_normals"].view(np.uint32), c["vertex_normals"].cpu().numpy().view(np.uint32))
    print(f"clean on the device equals the twin bit for bit: {same}")
