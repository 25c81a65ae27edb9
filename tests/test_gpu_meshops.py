"""Mesh clean-up on the GPU (sgam_neurips22_amd/meshops.py, csrc/mesh_ops.hip) against its numpy twin (tests/meshops_oracle.py) bit
for bit: every rule on the marching-cubes meshes and hand meshes of tests/test_meshops_cpu.py in device buffers with poisoned
excess capacity, components on long descending / permuted strips, a 700-triangle fan, `clean` end to end and run to run, the
all-round sphere volume of tests/test_gpu_mesh.py, and a three-step rgbd scene through the scene-level parameters."""
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import meshops, pointcloud, testing
from sgam_neurips22_amd.tsdf import DeviceMesh, TsdfVolume, frustum_bounds, render_mesh_rgbd

sys.path.insert(0, os.path.dirname(__file__))
import mc_oracle  # noqa: E402
import meshops_oracle as MO  # noqa: E402
import test_meshops_cpu as C  # noqa: E402
from test_gpu_tsdf import sphere_depth  # noqa: E402
from test_tsdf_cpu import _K  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32


def upload(v, t, col=None, extra=(37, 53)):
    """a DeviceMesh whose buffers are larger than the mesh, the excess rows poisoned: NaN vertices / colours, 0x7fffffff indices"""
    nv, nt = len(v), len(t)
    vb = np.full((nv + extra[0], 3), np.nan, dtype=f32)
    tb = np.full((nt + extra[1], 3), 0x7fffffff, dtype=np.int32)
    vb[:nv], tb[:nt] = v, t
    cb = None
    if col is not None:
        cb = np.full_like(vb, np.nan)
        cb[:nv] = col
    counts = torch.tensor([nv, nt, 0, 0], dtype=torch.int32, device=DEV)
    return DeviceMesh(torch.from_numpy(vb).to(DEV), None if cb is None else torch.from_numpy(cb).to(DEV), torch.from_numpy(tb).to(DEV), counts, nv, nt)


def same(got, want):
    """array equality: the bits of floats, the values of integers; shapes and dtypes too"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        return np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return np.array_equal(got, want)


def same_mesh(mesh, want):
    assert mesh.n_vertices == mesh.vertices.shape[0] == len(want["vertices"]) and mesh.n_triangles == mesh.triangles.shape[0] == len(want["triangles"])
    assert mesh.counts.cpu().tolist() == [mesh.n_vertices, mesh.n_triangles, 0, 0]
    assert same(mesh.vertices, want["vertices"]) and same(mesh.triangles, want["triangles"])
    assert (mesh.vertex_colors is None) == (want["colors"] is None)
    if want["colors"] is not None:
        assert same(mesh.vertex_colors, want["colors"])
    return True


def check_all_rules(v, t, col, voxel_size, min_triangles):
    nv = len(v)
    mesh = upload(v, t, col)
    got, want = meshops.components(mesh), MO.components(t, nv)
    for k in ("vertex_label", "triangle_label", "labels", "n_triangles"):
        assert same(got[k], want[k]), k
    for kind in ("triangles", "vertices"):
        g, (off, items) = meshops.incidence(mesh, kind), MO.incidence(t, nv, kind)
        assert same(g["offsets"], off) and same(g["items"], items), kind
    keep = np.arange(len(t)) % 3 != 1
    g, w = meshops.select_triangles(mesh, torch.from_numpy(keep).to(DEV)), MO.select_triangles(v, t, keep, col)
    assert same_mesh(g["mesh"], w) and same(g["vertex_index"], w["vertex_index"])
    for kw in (dict(min_triangles=min_triangles), dict(keep_largest=1), dict(min_triangles=2, keep_largest=2)):
        g, w = meshops.remove_small_components(mesh, **kw), MO.remove_small_components(v, t, col, **kw)
        assert same_mesh(g["mesh"], w) and same(g["vertex_index"], w["vertex_index"]), kw
    assert same(meshops.vertex_normals(mesh), MO.vertex_normals(v, t))
    g = meshops.smooth_taubin(mesh, 3)
    assert same_mesh(g, dict(vertices=MO.smooth_taubin(v, t, 3), triangles=t, colors=col))
    assert same(meshops.smooth_taubin(mesh, 0).vertices, v)
    g, w = meshops.simplify_vertex_clustering(mesh, voxel_size), MO.simplify_vertex_clustering(v, t, voxel_size, col)
    assert same_mesh(g["mesh"], w) and same(g["vertex_index"], w["vertex_index"])
    return got


@pytest.mark.parametrize("name,voxel_size,min_triangles", [("three", 0.25, 200), ("noise", 2.5, 100), ("sphere", 0.25, 10)])
def test_every_rule_on_the_marching_cubes_meshes(name, voxel_size, min_triangles):
    m = C.mesh(name)
    comp = check_all_rules(m["vertices"], m["triangles"], m["colors"], voxel_size, min_triangles)
    assert len(comp["labels"]) == {"three": 3, "noise": 79, "sphere": 1}[name]


@pytest.mark.parametrize("name", sorted(C.HAND))
def test_every_rule_on_the_hand_meshes(name):
    v, t = C.HAND[name]
    check_all_rules(v, t, None, 0.75, 1)
    mesh = upload(v, t)
    none = meshops.select_triangles(mesh, torch.zeros(len(t), dtype=torch.bool, device=DEV))
    assert none["mesh"].n_vertices == none["mesh"].n_triangles == 0 and none["vertex_index"].numel() == 0
    every = meshops.select_triangles(mesh, torch.ones(len(t), dtype=torch.bool, device=DEV))
    w = MO.select_triangles(v, t, np.ones(len(t), bool))
    assert same_mesh(every["mesh"], w) and same(every["vertex_index"], w["vertex_index"])
    # an empty mesh in: an empty result, nothing launched
    empty = upload(np.zeros((0, 3), f32), np.zeros((0, 3), np.int32))
    assert meshops.components(empty)["labels"].numel() == 0 and meshops.vertex_normals(empty).shape == (0, 3)
    out = meshops.clean(empty, keep_largest=1, smooth_iterations=2, voxel_size=0.5)
    assert out["mesh"].n_vertices == out["mesh"].n_triangles == 0 and out["vertex_index"].numel() == 0


def test_clustering_hand_mesh_and_a_given_origin():
    v, t = C.cluster_hand()
    g = meshops.simplify_vertex_clustering(upload(v, t), 1.0, origin=(0, 0, 0))
    w = MO.simplify_vertex_clustering(v, t, 1.0, origin=(0, 0, 0))
    assert same_mesh(g["mesh"], w) and g["vertex_index"].cpu().tolist() == [0, 1, 2, 6]
    assert g["mesh"].triangles.cpu().tolist() == [[0, 1, 2], [2, 1, 0]]
    with pytest.raises(ValueError):
        meshops.simplify_vertex_clustering(upload(v, t), float("nan"))
    with pytest.raises(ValueError):
        meshops.incidence(upload(v, t), "edges")


@pytest.mark.parametrize("seed", [None, 7])
def test_components_on_long_strips(seed):
    """3 000 triangles whose vertex ids descend along the strip (or are permuted): long parent chains, twelve workgroups; the
    error flag stays 0 (components() raises otherwise)"""
    v, t = C.strip(3000, seed)
    got, want = meshops.components(upload(v, t)), MO.components(t, len(v))
    for k in ("vertex_label", "triangle_label", "labels", "n_triangles"):
        assert same(got[k], want[k]), k
    assert got["labels"].cpu().tolist() == [0] and got["n_triangles"].cpu().tolist() == [3000]
    assert int(got["vertex_label"].max()) == 0


def test_fan_incidence_normals_and_smoothing():
    v, t = C.fan(700)
    mesh = upload(v, t)
    for kind in ("triangles", "vertices"):
        g, (off, items) = meshops.incidence(mesh, kind), MO.incidence(t, len(v), kind)
        assert same(g["offsets"], off) and same(g["items"], items), kind
        assert int(off[4] - off[3]) == 700
    assert same(meshops.vertex_normals(mesh), MO.vertex_normals(v, t))
    assert same(meshops.smooth_taubin(mesh, 2).vertices, MO.smooth_taubin(v, t, 2))


def test_clean_end_to_end_and_run_to_run():
    m = C.mesh("three")
    v, t, col = m["vertices"], m["triangles"], m["colors"]
    kw = dict(min_triangles=200, keep_largest=2, smooth_iterations=4, voxel_size=0.2)
    want = MO.clean(v, t, col, **kw)
    runs = [meshops.clean(upload(v, t, col), **kw) for _ in range(2)]
    for got in runs:
        assert same_mesh(got["mesh"], want)
        assert same(got["vertex_normals"], want["vertex_normals"]) and same(got["vertex_index"], want["vertex_index"])
    assert len(want["triangles"]) > 500
    for k in ("vertices", "triangles", "vertex_colors"):
        assert torch.equal(getattr(runs[0]["mesh"], k).view(torch.int32), getattr(runs[1]["mesh"], k).view(torch.int32))
    plain = meshops.clean(upload(v, t, col), normals=False)                 # nothing asked: the same mesh, exactly sized
    assert plain["vertex_normals"] is None and same_mesh(plain["mesh"], dict(vertices=v, triangles=t, colors=col))


# ---------------------------------------------------------------- the all-round sphere volume of tests/test_gpu_mesh.py, rebuilt
def _look_at(eye, target):
    """world -> camera 4x4 looking from eye at target (camera +z forward, +y down)"""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, :3] = np.stack([x, y, z])
    T[:3, 3] = -T[:3, :3] @ eye
    return T


def _sphere_volume(voxel=0.05, trunc=0.5, radius=1.5, H=96, W=96, f=110.0):
    K = _K(f, (H - 1) / 2)
    centre = np.array([0.3, -0.2, 0.1])
    dirs = [np.array((a, b, c), dtype=np.float64) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    eyes = [centre + 5.0 * (d / np.linalg.norm(d) + np.array([0.013, 0.021, -0.017])) for d in dirs]
    poses = [_look_at(e, centre) for e in eyes]
    lo, hi = frustum_bounds(K, poses, H, W, 8.0, margin=trunc + 16 * voxel)
    vol = TsdfVolume(voxel, trunc, lo, hi, DEV, memory_budget_bytes=2 << 30)
    for T in poses:
        vol.integrate(torch.from_numpy(sphere_depth(K, T, H, W, centre, radius)).to(DEV), K, T)
    return vol, K, centre, radius, poses


def test_sphere_volume_loses_its_bubbles():
    vol, K, centre, radius, poses = _sphere_volume()
    mesh = vol.extract_mesh_device()
    comp = meshops.components(mesh)
    out = meshops.clean(mesh, keep_largest=1)
    m = out["mesh"]
    print(f"sphere volume: {len(comp['labels'])} components, {len(comp['labels']) - 1} removed; {mesh.n_triangles} -> {m.n_triangles} triangles")
    assert m.n_triangles < mesh.n_triangles and m.n_triangles > 0.9 * mesh.n_triangles
    tri = m.triangles.cpu().numpy()
    chi, (_, ucount), (_, dcount) = mc_oracle.euler_and_edges(tri)
    assert chi == 2 and (ucount == 2).all() and (dcount == 1).all()
    assert len(meshops.components(m)["labels"]) == 1
    n = out["vertex_normals"].cpu().numpy().astype(np.float64)
    radial = m.vertices.cpu().numpy().astype(np.float64) - centre
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    assert np.median((n * radial).sum(1)) > 0.95
    r = render_mesh_rgbd(m, K, poses[:2], 96, 96, 0.5, 8.0, normals=True)
    assert tuple(r["depth"].shape) == (2, 96, 96) and float((r["depth"] > 0).float().mean()) > 0.1


# ---------------------------------------------------------------- the scene level
def _scene_loop(mode, steps=3):
    from sgam_neurips22_amd.config import default_params
    from sgam_neurips22_amd.generative_sensing_module.model import VQModel
    from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
    p = default_params("google_earth")
    m = VQModel(**p)
    sd = testing.synthetic_state_dict(m.state_dict(), seed=0)
    sd["quantize.embedding.weight"] = testing.codebook_from_stats(0.0, 0.5, p["n_embed"], 256, 1)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    scene = InfiniteSceneGeneration(m, "google_earth", output_dim=(steps + 2, 1), seed_frame=synthetic_seed_frame("google_earth", 0, 256),
                                    use_rgbd_integration=True, rgbd_depth_render=mode)
    for _ in range(steps):
        scene.one_step_prediction(scene.next_pose(scene.curr))
        scene.curr += 1
    return scene


def test_scene_exports_renders_and_scores_the_cleaned_mesh(tmp_path):
    scene = _scene_loop("mesh")
    a, b = tmp_path / "a", tmp_path / "b"
    n = scene.export_triangle_mesh(str(a))
    assert isinstance(n, int) and scene.export_triangle_mesh(str(b), clean=None) == n
    name, cname = "rgbd_integrated_triangle_mesh.ply", "rgbd_integrated_triangle_mesh_clean.ply"
    raw = (a / name).read_bytes()
    assert (b / name).read_bytes() == raw and sorted(os.listdir(b)) == [name]
    kw = dict(min_triangles=50, smooth_iterations=2, voxel_size=0.03)
    counts = scene.export_triangle_mesh(str(b), clean=kw)
    assert (b / name).read_bytes() == raw and counts[name] == n
    src = scene.colour_volume().extract_triangle_mesh()
    want = MO.clean(src["vertices"], src["triangles"], src["vertex_colors"], **kw)
    back = pointcloud.read_triangle_mesh(str(b / cname))
    print(f"scene mesh: {n} -> {counts[cname]} triangles, {len(src['vertices'])} -> {len(back['vertices'])} vertices")
    assert 0 < counts[cname] == len(want["triangles"]) < n
    assert np.array_equal(back["vertices"], want["vertices"].astype(np.float64)) and np.array_equal(back["triangles"], want["triangles"])
    assert np.array_equal(back["normals"], want["vertex_normals"].astype(np.float64))
    assert np.array_equal(back["colors_u8"], np.round(np.clip(want["colors"].astype(np.float64), 0, 1) * 255).astype(np.uint8))
    with pytest.raises(ValueError, match="does not take"):
        scene.export_triangle_mesh(str(b), clean={"voxel": 1.0})
    poses = [scene.transform_grid[c[0]][c[1]]["T"] for c in scene._ordered_grid_coords[1:3]]
    views = scene.render_views(poses, source="mesh", mesh_clean=kw, H=64, W=64)
    assert tuple(views["rgb"].shape) == (2, 64, 64, 3) and tuple(views["depth"].shape) == (2, 64, 64) and views["rgb_u8"].dtype == torch.uint8
    assert all(bool((views["depth"][p] > 0).any()) for p in range(2))       # the cleaned mesh lies in front of the cameras that fused it
    with pytest.raises(ValueError, match="mesh_clean"):
        scene.render_views(poses, source="points", mesh_clean=kw)
    for extra in ({}, {"mesh_clean": kw}):
        s = scene.geometry_metrics(scene, 0.01, source="mesh", **extra)
        assert s["chamfer"] == 0.0 and s["fscore"] == 1.0 and s["n_pred"] == s["n_ref"] > 100
    assert s["n_pred"] == len(want["vertices"])
