"""The triangle BVH on the GPU (sgam_neurips22_amd/meshops.TriangleBVH, csrc/mesh_bvh.hip): the tables it builds against the numpy
twin (tests/bvh_oracle.py) bit for bit, and every query through it — distance, nearest hit, any hit, visibility — against the
brute-force truths of tests/meshquery_oracle.py and tests/raycast_oracle.py bit for bit, on the meshes and rays of
tests/test_bvh_cpu.py: hand meshes, exact copies (ties), one Morton code, a marching-cubes mesh in poisoned buffers, and the
mixed-scale mesh the structure exists for."""
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import _lib, geometry, meshops
from sgam_neurips22_amd.ops import SgamHipError

sys.path.insert(0, os.path.dirname(__file__))
import bvh_oracle as B  # noqa: E402
import meshquery_oracle as Q  # noqa: E402
import raycast_oracle as R  # noqa: E402
import test_bvh_cpu as BC  # noqa: E402
import test_meshops_cpu as C  # noqa: E402
import test_raycast_cpu as RC  # noqa: E402
from test_gpu_meshops import _scene_loop, same, upload  # noqa: E402
from test_gpu_meshquery import hand_queries, spanning_mesh  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
ONE_V, ONE_T = np.array([[0, 0, 0.5], [1, 0, 0.25], [0, 1, 0.75]], dtype=f32), np.array([[0, 1, 2]], dtype=np.int32)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def check_tables(v, t):
    """the device's tables equal the twin's: leaf order and records, children, boxes, heights -> (the tree, the twin)"""
    bvh, twin = meshops.TriangleBVH(upload(v, t)), B.Tree(v, t)
    n = twin.n
    assert (bvh.n_candidates, bvh.n_nodes, bvh.guard) == (n, 2 * n - 1, float(twin.guard))
    got = bvh.tables()
    assert same(got["records"], twin.device_records()), np.flatnonzero(got["records"][:, 3].cpu().view(torch.int32).numpy() != twin.ids)[:8]
    assert same(got["boxes"], twin.boxes) and same(got["children"], twin.children) and same(got["height"], twin.height)
    assert bvh.height == (int(twin.height[0]) if n > 1 else 0) and bvh.bytes == _lib.load().sgam_mesh_bvh_workspace_bytes(n)
    return bvh, twin


def check_rays(bvh, v, t, rays, windows=((0.0, np.inf),), want=None):
    """every window against the brute-force truth: t, triangle, uv, normal and the any-hit answer bit for bit -> the truths"""
    out = []
    for w, window in enumerate(windows):
        twin = want[w] if want is not None else R.cast_rays(v, t, rays, *window)
        out.append(twin)
        got = bvh.cast_rays(_t(rays), tnear=window[0], tfar=window[1], uv=True, normals=True)
        for k in ("t", "triangle", "uv", "normal"):
            assert same(got[k], twin[k]), (window, k, np.flatnonzero(got["triangle"].cpu().numpy() != twin["triangle"])[:8])
        bare = bvh.cast_rays(_t(rays), tnear=window[0], tfar=window[1])
        assert sorted(bare) == ["t", "triangle"] and same(bare["t"], twin["t"]) and same(bare["triangle"], twin["triangle"])
        hit = bvh.test_occlusions(_t(rays), tnear=window[0], tfar=window[1])
        assert hit.dtype == torch.bool and same(hit, twin["hit"]) and same(hit, np.isfinite(twin["t"])), window
    return out


def check_distance(bvh, v, t, q, max_distance=None):
    want = Q.mesh_distance(v, t, q, np.inf if max_distance is None else geometry.max_d2_of(max_distance))
    got = bvh.query(_t(q), max_distance=max_distance, closest=True)
    for k in ("d2", "triangle", "closest"):
        assert same(got[k], want[k]), (k, max_distance, np.flatnonzero(got["triangle"].cpu().numpy() != want["triangle"])[:8])
    bare = bvh.query(_t(q), max_distance=max_distance)
    assert sorted(bare) == ["d2", "triangle"] and same(bare["d2"], want["d2"]) and same(bare["triangle"], want["triangle"])
    return want


# ---------------------------------------------------------------- the build
def test_tables_of_one_and_two_triangles_and_one_code():
    bvh, _ = check_tables(ONE_V, ONE_T)
    assert bvh.n_nodes == 1 and bvh.height == 0
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], dtype=f32)
    bvh, twin = check_tables(v, np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32))
    assert twin.children.tolist() == [[1, 2]] and bvh.height == 1
    _, twin = check_tables(*BC.one_code_mesh())
    assert twin.ids.tolist() == list(range(37))


@pytest.mark.parametrize("nt", [255, 257, 603])
def test_tables_with_exact_copies_across_the_tile_edge(nt):
    v, t = spanning_mesh()
    t = np.concatenate([t, t, t])[:nt]
    _, twin = check_tables(v, t)
    assert twin.n == nt


def test_tables_of_a_marching_cubes_mesh_in_poisoned_buffers_and_run_to_run():
    m = C.mesh("sphere")
    v, t = m["vertices"], m["triangles"]
    bvh, twin = check_tables(v, t)
    assert 2 * np.log2(twin.n) + 8 >= bvh.height >= np.log2(twin.n)
    again = meshops.TriangleBVH(upload(v, t))
    for k, a in bvh.tables().items():
        assert torch.equal(a.view(torch.int32), again.tables()[k].view(torch.int32)), k      # identical bytes, run to run
    rays = _t(RC.mesh_rays(v, 600))
    first = bvh.cast_rays(rays, uv=True, normals=True)
    for k, a in again.cast_rays(rays, uv=True, normals=True).items():
        assert torch.equal(a.view(torch.int32), first[k].view(torch.int32)), k


# ---------------------------------------------------------------- rays
@pytest.mark.parametrize("n", [1, 63, 65, 257, 1000])
def test_one_triangle_and_every_ray_count(n):
    want = check_rays(meshops.TriangleBVH(upload(ONE_V, ONE_T)), ONE_V, ONE_T, RC.hand_rays(n, n))[0]
    assert want["triangle"][0] == 0 and (n < 5 or ((want["triangle"] == 0).sum() > 3 and (want["triangle"] == -1).sum() >= 3))


@pytest.mark.parametrize("order", [0, 1])
def test_adversarial_rays_on_the_lattice_in_both_triangle_orders(order):
    v, t = RC.lattice_mesh()
    t = t[::-1].copy() if order else t
    want = [RC.lattice_truth(w) for w in RC.WINDOWS] if not order else None
    bvh = meshops.TriangleBVH(upload(v, t))
    full = check_rays(bvh, v, t, RC.adversarial_rays(), windows=RC.WINDOWS, want=want)[0]
    assert (full["triangle"] >= 0).sum() > 100 and (full["triangle"] == -1).sum() > 40
    ties = np.array([[0.25, 0.25, 1.5, 0, 0, -1], [0.3125, 0.3125, 1.5, 0, 0, -1], [2, 0.25, 0.5, -1, 0, 0]], dtype=f32)
    tie = check_rays(bvh, v, t, ties)[0]                                    # exactly on a shared vertex / edge: the lower index of those hit
    assert tie["t"].tolist() == [0.75, 0.75, 1.5]


@pytest.mark.parametrize("name", ["lattice", "spanning", "mixed"])
def test_far_origins_face_grazing_and_random_rays(name):
    v, t = BC.MESHES[name]()
    bvh = meshops.TriangleBVH(upload(v, t))
    n = 0
    for rays, windows in ((BC.far_rays(v), ((0.0, np.inf),)), (BC.face_rays(BC.tree(name)), ((0.0, np.inf), (0.0, 1.0))),
                          (BC.random_rays(v, 700, 11), ((0.0, np.inf), (0.25, 1.0)))):
        for want in check_rays(bvh, v, t, rays, windows=windows):
            n += int((want["triangle"] >= 0).sum())
    assert n > 500


def test_copies_and_ties_across_the_tile_edge():
    v, t = spanning_mesh()
    t = np.concatenate([t, t, t])
    want = check_rays(meshops.TriangleBVH(upload(v, t)), v, t, RC.hand_rays(500, 7), windows=((0.0, np.inf), (0.2, 0.9)))[0]
    assert (want["triangle"] >= 0).sum() > 50 and want["triangle"].max() < 201          # of three copies the first wins


def test_marching_cubes_mesh_with_rows_that_are_not_rays():
    m = C.mesh("sphere")
    v, t = m["vertices"], m["triangles"]
    rays = RC.mesh_rays(v, 600)
    rays[17, 0], rays[555, 4] = np.nan, np.inf
    bvh = meshops.TriangleBVH(upload(v, t))
    want = check_rays(bvh, v, t, rays, windows=((0.0, np.inf), (0.5, 1.5)))[0]
    assert (want["triangle"] >= 0).sum() > 350 and (want["triangle"] == -1).sum() > 30 and want["triangle"][17] == want["triangle"][555] == -1
    shaped = bvh.cast_rays(_t(rays).reshape(6, 100, 6), uv=True, normals=True)
    assert tuple(shaped["t"].shape) == (6, 100) and tuple(shaped["uv"].shape) == (6, 100, 2) and tuple(shaped["normal"].shape) == (6, 100, 3)
    assert tuple(bvh.test_occlusions(_t(rays).reshape(6, 100, 6)).shape) == (6, 100)


# ---------------------------------------------------------------- distance
@pytest.mark.parametrize("nq", [1, 63, 65, 257])
def test_one_triangle_and_every_query_count(nq):
    want = check_distance(meshops.TriangleBVH(upload(ONE_V, ONE_T)), ONE_V, ONE_T, hand_queries(nq, [0, 0, 0], [1, 1, 1], nq))
    assert want["triangle"][0] == 0 and (nq < 5 or (want["triangle"] == -1).sum() == 3)


@pytest.mark.parametrize("name", ["lattice", "spanning", "mixed", "copies"])
def test_distance_with_ties_non_points_and_a_radius(name):
    v, t = BC.MESHES[name]() if name != "copies" else spanning_mesh()
    if name == "copies":
        t = np.concatenate([t, t, t])
    q = np.concatenate([BC.random_queries(v, 700, 4), BC.shared_edge_queries(v, t)])
    bvh = meshops.TriangleBVH(upload(v, t))
    want = check_distance(bvh, v, t, q)
    assert (want["triangle"] == -1).sum() == 3 and (name != "copies" or want["triangle"].max() < 201)
    near = check_distance(bvh, v, t, q, max_distance=0.05 * float((v.max(0) - v.min(0)).max()))
    assert 3 < (near["triangle"] == -1).sum() < len(q) - 50
    if name == "lattice":                                                   # queries on shared edges and vertices: several exact ties, the lower index
        a, b, c, _ = Q.corners(v, t)
        edge = BC.shared_edge_queries(v, t)
        tied = (lambda d2: d2 == d2.min(1, keepdims=True))(Q.point_triangle(a[None], b[None], c[None], edge[:, None])[0])
        assert (tied.sum(1) >= 2).sum() > 40 and (want["triangle"][-len(edge):] == tied.argmax(1)).all()


# ---------------------------------------------------------------- visibility
def test_visible_points_two_quads_and_the_sphere_from_four_poses():
    v, t = RC.two_quads()
    rs = np.random.RandomState(3)
    pts = np.concatenate([np.stack([rs.uniform(-1, 1, 300), rs.uniform(-1, 1, 300), np.full(300, 2.0)], 1),
                          np.stack([rs.uniform(-0.2, 0.2, 100), rs.uniform(-0.2, 0.2, 100), np.full(100, 1.0)], 1), rs.uniform(-3, 3, (100, 3))]).astype(f32)
    pts[7, 1] = np.nan
    cam = dict(fx=20.0, fy=20.0, cx=31.5, cy=31.5, H=64, W=64, z_near=0.1, z_far=4.0)
    K = np.array([[20.0, 0, 31.5], [0, 20.0, 31.5], [0, 0, 1]])
    one = np.eye(4, dtype=f32)[None]
    side = np.array([[[1, 0, 0, -0.8], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]], dtype=f32)
    mesh = upload(v, t)
    bvh = meshops.TriangleBVH(mesh)
    for poses in (one, np.concatenate([one, side])):
        for tol in (1e-3, 0.0):
            want = R.visibility(pts, v, t, poses, tolerance=tol, **cam)
            got = meshops.visible_points(_t(pts), mesh, poses, K, 64, 64, 0.1, 4.0, tolerance=tol, grid=bvh)
            assert same(got["count"], want) and same(got["visible"], want > 0), (len(poses), tol)
            assert same(bvh.visible_points(_t(pts), poses, K, 64, 64, 0.1, 4.0, tolerance=tol)["count"], want)
    assert want.max() == 2 and (want[:300] == 0).sum() > 20                 # (two poses, no tolerance: the last case of the loop)
    m = C.mesh("sphere")
    v, t = m["vertices"], m["triangles"]
    mid = (v.min(0).astype(np.float64) + v.max(0)) / 2
    poses = []
    for axis, sign in ((2, -1), (2, 1), (0, -1), (1, 1)):                   # four cameras around the sphere, looking at its middle
        z = np.zeros(3)
        z[axis] = -sign
        x = np.roll(z, 1)
        rot = np.stack([x, np.cross(z, x), z])
        centre = mid - z * 5.0
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = rot, -rot @ centre
        poses.append(M)
    poses = np.array(poses, dtype=f32)
    rs = np.random.RandomState(5)
    pts = np.concatenate([v[rs.randint(0, len(v), 250)], rs.uniform(v.min(0), v.max(0), (50, 3))]).astype(f32)
    far = {**cam, "z_far": 20.0}
    want = R.visibility(pts, v, t, poses, **far)
    mesh = upload(v, t)
    got = meshops.visible_points(_t(pts), mesh, poses, K, 64, 64, 0.1, 20.0, grid=meshops.TriangleBVH(mesh))
    assert same(got["count"], want) and want.max() >= 2 and (want == 0).sum() > 20
    with pytest.raises(ValueError, match="another mesh"):
        meshops.visible_points(_t(pts), mesh, poses, K, 64, 64, 0.1, 20.0, grid=bvh)


# ---------------------------------------------------------------- the public switches
def test_mixed_scale_mesh_through_accel_and_surface_metrics():
    v, t = BC.mixed_mesh()
    mesh = upload(v, t)
    bvh, grid = meshops.TriangleBVH(mesh), meshops.TriangleGrid(mesh)
    rays, q = _t(BC.random_rays(v, 500, 3)), _t(BC.random_queries(v, 500, 3))
    for method in ("auto", "brute", "grid"):
        for accel in (bvh, grid):
            cast = meshops.cast_rays(rays, mesh, method=method, uv=True, normals=True, accel=accel)
            dist = meshops.point_mesh_distance(q, mesh, method=method, closest=True, accel=accel)
            brute = meshops.cast_rays(rays, mesh, method="brute", uv=True, normals=True)
            for k in brute:
                assert torch.equal(cast[k].view(torch.int32), brute[k].view(torch.int32)), (method, type(accel).__name__, k)
            for k, a in meshops.point_mesh_distance(q, mesh, method="brute", closest=True).items():
                assert torch.equal(dist[k].view(torch.int32), a.view(torch.int32)), (method, type(accel).__name__, k)
            assert torch.equal(meshops.test_occlusions(rays, mesh, accel=accel), meshops.test_occlusions(rays, mesh, method="brute"))
    sphere = C.mesh("sphere")
    pred = upload(sphere["vertices"] + f32(0.01), sphere["triangles"])
    size = float(np.ptp(sphere["vertices"], axis=0).max())
    numbers = [meshops.surface_metrics(pred, mesh, 0.02 * size, n_samples=3000, seed=1, method=method, accelerator=accelerator)
               for method, accelerator in (("brute", "grid"), ("grid", "grid"), ("grid", "bvh"), ("auto", "bvh"), ("brute", "bvh"))]
    assert all(n == numbers[0] for n in numbers[1:]) and numbers[0]["recall"] < 0.01 and numbers[0]["precision"] > 0.5      # (the samples of the reference lie on its large box)
    with pytest.raises(ValueError):
        meshops.cast_rays(rays, upload(v, t), accel=bvh)                    # a tree of another mesh (equal, but not this one)
    with pytest.raises(ValueError):
        meshops.surface_metrics(pred, mesh, 0.1, n_samples=10, accelerator="tree")
    with pytest.raises(SgamHipError):
        bvh.cast_rays(rays.cpu())


def test_bad_indices_raise_and_empty_meshes_answer_without_a_launch():
    v, t = RC.lattice_mesh()
    bad = t.copy()
    bad[10, 1], bad[50, 2] = len(v), -1
    with pytest.raises(SgamHipError, match="outside the mesh"):
        meshops.TriangleBVH(upload(v, bad))
    rays, q = _t(RC.hand_rays(10)), _t(hand_queries(10, [0, 0, 0], [1, 1, 1]))
    for m in (upload(np.zeros((0, 3), f32), np.zeros((0, 3), np.int32)), upload(np.zeros((3, 3), f32), np.array([[0, 1, 2]], np.int32))):
        bvh = meshops.TriangleBVH(m)
        assert (bvh.n_candidates, bvh.n_nodes, bvh.height, bvh.bytes, bvh.tables()) == (0, 0, 0, 0, None)
        out = bvh.cast_rays(rays, uv=True, normals=True)
        assert out["triangle"].cpu().tolist() == [-1] * 10 and bool(torch.isinf(out["t"]).all()) and bool(torch.isnan(out["uv"]).all())
        assert not bool(bvh.test_occlusions(rays).any())
        d = bvh.query(q, closest=True)
        assert d["triangle"].cpu().tolist() == [-1] * 10 and bool(torch.isinf(d["d2"]).all()) and bool(torch.isnan(d["closest"]).all())
    bvh = meshops.TriangleBVH(upload(v, t))
    assert tuple(bvh.cast_rays(rays[:0], normals=True)["normal"].shape) == (0, 3) and tuple(bvh.query(q[:0])["d2"].shape) == (0,)
    for kw in (dict(tnear=-1.0), dict(tnear=2.0, tfar=1.0), dict(tnear=float("nan"))):
        with pytest.raises(ValueError):
            bvh.cast_rays(rays, **kw)
    with pytest.raises(ValueError):
        bvh.query(q, max_distance=-1.0)


def test_scene_metrics_and_visible_surface_through_the_bvh():
    scene = _scene_loop("mesh")
    voxel, n = float(scene.volume.voxel_length), 2048
    for kw in (dict(), dict(visible_from="frames")):
        grid = scene.geometry_metrics(scene, voxel, source="mesh", surface_samples=n, **kw)
        assert scene.geometry_metrics(scene, voxel, source="mesh", surface_samples=n, accelerator="bvh", **kw) == grid
    assert 0 < grid["n_ref"] < n and grid["n_ref"] + grid["n_ref_culled"] == n
    a, b = scene.visible_surface(n_samples=n), scene.visible_surface(n_samples=n, accelerator="bvh")
    assert all(torch.equal(a[k], b[k]) for k in ("points", "visible", "count")) and int(b["visible"].sum().item()) == grid["n_ref"]
    for call in (lambda: scene.geometry_metrics(scene, voxel, source="mesh", surface_samples=n, accelerator="tree"),
                 lambda: scene.visible_surface(n_samples=n, accelerator="auto")):
        with pytest.raises(ValueError, match="accelerator"):
            call()
