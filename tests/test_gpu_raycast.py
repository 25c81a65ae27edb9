"""Rays against a mesh on the GPU (sgam_neurips22_amd/meshops.py, csrc/mesh_ray.hip) against their numpy twin
(tests/raycast_oracle.py) bit for bit: the nearest hit and the any-hit by brute force and through the triangle grid (the same bits,
at every cell size) on hand meshes, on rays chosen to trouble the walk and on a marching-cubes mesh in device buffers with
poisoned excess capacity; pinhole rays; the visibility of points from cameras; and a three-step rgbd scene whose recall is
scored over the part of the reference its own cameras saw."""
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import meshops
from sgam_neurips22_amd.ops import SgamHipError

sys.path.insert(0, os.path.dirname(__file__))
import raycast_oracle as R  # noqa: E402
import test_meshops_cpu as C  # noqa: E402
import test_raycast_cpu as RC  # noqa: E402
from test_gpu_meshops import _scene_loop, same, upload  # noqa: E402
from test_gpu_meshquery import spanning_mesh  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
GRIDS = (("brute", {}), ("grid", {}), ("grid", {"cell_size": 0.125}), ("grid", {"cell_size": 0.3}))


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def check_rays(v, t, rays, methods=GRIDS, windows=((0.0, np.inf),), want=None):
    """every method and window against the twin: t, triangle, uv, normal and the any-hit answer bit for bit -> the twin's answers"""
    mesh, out = upload(v, t), []
    for w, window in enumerate(windows):
        twin = want[w] if want is not None else R.cast_rays(v, t, rays, *window)
        out.append(twin)
        for method, kw in methods:
            got = meshops.cast_rays(_t(rays), mesh, method=method, tnear=window[0], tfar=window[1], uv=True, normals=True, **kw)
            for k in ("t", "triangle", "uv", "normal"):
                assert same(got[k], twin[k]), (method, kw, window, k, np.flatnonzero(got["triangle"].cpu().numpy() != twin["triangle"])[:8])
            bare = meshops.cast_rays(_t(rays), mesh, method=method, tnear=window[0], tfar=window[1], **kw)
            assert sorted(bare) == ["t", "triangle"] and same(bare["t"], twin["t"]) and same(bare["triangle"], twin["triangle"])
            hit = meshops.test_occlusions(_t(rays), mesh, method=method, tnear=window[0], tfar=window[1], **kw)
            assert hit.dtype == torch.bool and same(hit, twin["hit"]) and same(hit, np.isfinite(twin["t"])), (method, kw, window)
    return out


@pytest.mark.parametrize("n", [1, 63, 65, 257, 1000])
def test_one_triangle_and_every_ray_count(n):
    v, t = np.array([[0, 0, 0.5], [1, 0, 0.25], [0, 1, 0.75]], dtype=f32), np.array([[0, 1, 2]], dtype=np.int32)
    rays = RC.hand_rays(n, n)
    want = check_rays(v, t, rays, methods=(("brute", {}), ("grid", {}), ("grid", {"cell_size": 0.1}), ("auto", {})))[0]
    assert want["triangle"][0] == 0 and (n < 5 or ((want["triangle"] == 0).sum() > 3 and (want["triangle"] == -1).sum() >= 3))


@pytest.mark.parametrize("nt", [255, 257, 603])
def test_triangle_counts_across_the_lds_tile_edge(nt):
    v, t = spanning_mesh()
    t = np.concatenate([t, t, t])[:nt]                                      # 201 triangles, then exact copies of them: ties go to the lower index
    rays = RC.hand_rays(500, 7)
    want = check_rays(v, t, rays, methods=(("brute", {}), ("grid", {}), ("grid", {"cell_size": 0.02})), windows=((0.0, np.inf), (0.2, 0.9)))[0]
    assert (want["triangle"] >= 0).sum() > 50
    if nt == 603:                                                           # a capped grid: the cell edge grew, the answers did not change
        mesh = upload(v, t)
        capped = meshops.TriangleGrid(mesh, cell_size=0.02, max_entries_per_triangle=3.0)
        assert capped.cell_size > 0.02
        got = capped.cast_rays(_t(rays), uv=True, normals=True)
        for k in ("t", "triangle", "uv", "normal"):
            assert same(got[k], want[k]), k
        assert same(capped.test_occlusions(_t(rays)), want["hit"])


def test_flat_grids_and_a_single_cell():
    v, t = RC.lattice_mesh()
    flat_v, flat_t = v[:81], t[:128]                                        # the sheet z = 1/4 alone: a grid one cell thick
    rays = RC.adversarial_rays()
    grid = meshops.TriangleGrid(upload(flat_v, flat_t), cell_size=0.125)
    assert grid.dims[2] == 1 and grid.dims[0] == 9
    check_rays(flat_v, flat_t, rays, methods=(("brute", {}), ("grid", {"cell_size": 0.125}), ("grid", {"cell_size": 5.0})), windows=RC.WINDOWS[:3])
    assert meshops.TriangleGrid(upload(v, t), cell_size=5.0).dims == (1, 1, 1)
    check_rays(v, t, rays, methods=(("grid", {"cell_size": 5.0}),))


@pytest.mark.parametrize("order", [0, 1])
def test_adversarial_rays_brute_equals_grid_equals_twin(order):
    v, t = RC.lattice_mesh()
    t = t[::-1].copy() if order else t
    rays = RC.adversarial_rays()
    want = [RC.lattice_truth(w) for w in RC.WINDOWS] if not order else None
    out = check_rays(v, t, rays, methods=GRIDS + (("grid", {"cell_size": 0.05}),), windows=RC.WINDOWS, want=want)
    full = out[0]
    assert (full["triangle"] >= 0).sum() > 100 and (full["triangle"] == -1).sum() > 40
    ties = np.array([[0.25, 0.25, 1.5, 0, 0, -1], [0.3125, 0.3125, 1.5, 0, 0, -1], [2, 0.25, 0.5, -1, 0, 0]], dtype=f32)
    tie = check_rays(v, t, ties)[0]                                         # exactly on a shared vertex / edge: the lower index of those hit
    assert tie["t"].tolist() == [0.75, 0.75, 1.5]
    a, b, c, _ = R.Q.corners(v, t)
    for i, ray in enumerate(ties):
        hit, tt, _, _ = R.ray_triangle(a, b, c, ray[:3], ray[3:], 0, np.inf, R.guard_of(v, t))
        assert (hit & (tt == tie["t"][i])).sum() >= 2 and tie["triangle"][i] == np.flatnonzero(hit & (tt == tie["t"][i])).min()


def test_marching_cubes_mesh_in_poisoned_buffers():
    m = C.mesh("sphere")
    v, t = m["vertices"], m["triangles"]
    rays = RC.mesh_rays(v, 600)
    rays[17, 0], rays[555, 4] = np.nan, np.inf
    default = meshops.TriangleGrid(upload(v, t))
    methods = (("brute", {}), ("grid", {}), ("grid", {"cell_size": default.cell_size / 3}), ("grid", {"cell_size": float((v.max(0) - v.min(0)).max()) * 2}), ("auto", {}))
    want = check_rays(v, t, rays, methods=methods, windows=((0.0, np.inf), (0.5, 1.5)))[0]
    assert (want["triangle"] >= 0).sum() > 350 and (want["triangle"] == -1).sum() > 30
    shaped = meshops.cast_rays(_t(rays).reshape(6, 100, 6), upload(v, t), uv=True, normals=True)
    assert tuple(shaped["t"].shape) == (6, 100) and tuple(shaped["uv"].shape) == (6, 100, 2) and tuple(shaped["normal"].shape) == (6, 100, 3)
    assert same(shaped["triangle"].reshape(-1), want["triangle"])
    assert tuple(meshops.test_occlusions(_t(rays).reshape(6, 100, 6), upload(v, t)).shape) == (6, 100)


def test_what_is_not_a_triangle_never_hits_and_bad_indices_raise():
    rs = np.random.RandomState(4)                                          # test_gpu_meshquery.test_what_is_not_a_triangle_never_wins' mesh
    v = rs.uniform(0, 2, (40, 3)).astype(f32)
    v[7] = np.nan
    v[11, 2] = np.inf
    t = rs.randint(0, 40, (90, 3)).astype(np.int32)
    t[::5, 1] = t[::5, 0]
    v[20], v[21], v[22] = [0.5, 0.5, 0.5], [1.0, 1.0, 1.0], [1.5, 1.5, 1.5]
    t[3] = [20, 21, 22]
    a2 = R.Q.area2(v, t)
    rays = RC.hand_rays(400, 5)
    rays[:, :3] *= 2
    rays[:, 3:] = rs.uniform(0, 2, (400, 3)).astype(f32) - rays[:, :3]
    want = check_rays(v, t, rays, methods=(("brute", {}), ("grid", {}), ("grid", {"cell_size": 0.2})))[0]
    assert (want["triangle"] >= 0).sum() > 100 and (a2[want["triangle"][want["triangle"] >= 0]] > 0).all()
    bad = t.copy()
    bad[10, 1], bad[50, 2] = len(v), -1
    mesh = upload(v, bad)
    for call in (lambda: meshops.cast_rays(_t(rays), mesh, method="brute"), lambda: meshops.cast_rays(_t(rays), mesh, method="grid"),
                 lambda: meshops.test_occlusions(_t(rays), mesh, method="brute"),
                 lambda: meshops.visible_points(_t(rays[:, :3]), mesh, np.eye(4)[None], np.eye(3), 8, 8, 0.1, 4.0, method="brute")):
        with pytest.raises(SgamHipError, match="outside the mesh"):
            call()


def test_no_launch_paths_and_argument_errors():
    v, t = RC.lattice_mesh()
    mesh = upload(v, t)
    empty = upload(np.zeros((0, 3), f32), np.zeros((0, 3), np.int32))
    no_area = upload(np.zeros((3, 3), f32), np.array([[0, 1, 2]], np.int32))
    rays = _t(RC.hand_rays(10))
    for method in ("brute", "grid", "auto"):
        for m in (empty, no_area):
            out = meshops.cast_rays(rays, m, method=method, uv=True, normals=True)
            assert out["triangle"].cpu().tolist() == [-1] * 10 and bool(torch.isinf(out["t"]).all()) and bool(torch.isnan(out["uv"]).all())
            assert not bool(meshops.test_occlusions(rays, m, method=method).any())
        out = meshops.cast_rays(rays[:0], mesh, method=method, normals=True)
        assert tuple(out["t"].shape) == (0,) and tuple(out["normal"].shape) == (0, 3)
    with pytest.raises(SgamHipError):
        meshops.cast_rays(rays.cpu(), mesh)
    for kw in (dict(method="tree"), dict(method="brute", cell_size=0.1), dict(tnear=-1.0), dict(tnear=2.0, tfar=1.0), dict(tnear=float("nan"))):
        with pytest.raises(ValueError):
            meshops.cast_rays(rays, mesh, **kw)
    with pytest.raises(ValueError):
        meshops.cast_rays(rays[:, :5], mesh)


def test_pinhole_rays_and_a_tessellated_plane():
    rs = np.random.RandomState(2)
    rot, _ = np.linalg.qr(rs.normal(0, 1, (3, 3)))
    poses = np.stack([np.eye(4), np.eye(4)]).astype(f32)
    poses[1, :3, :3], poses[1, :3, 3] = rot.astype(f32), [0.3, -0.2, 1.5]
    K = np.array([[70.0, 0, 23.5], [0, 65.0, 15.5], [0, 0, 1]])
    got = meshops.create_rays_pinhole(poses, K, 32, 48)
    assert same(got, R.rays_pinhole(poses, 70.0, 65.0, 23.5, 15.5, 32, 48)) and tuple(got.shape) == (2, 32, 48, 6)
    # the plane z = 2 in front of the identity pose: t is the view-space depth, 2, within the float64-measured bound
    n = 16
    k = np.linspace(-2, 2, n + 1)
    a, b = np.meshgrid(k, k, indexing="ij")
    v = np.stack([a, b, np.full_like(a, 2.0)], -1).reshape(-1, 3).astype(f32)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    q = (i * (n + 1) + j).reshape(-1)
    t = np.concatenate([np.stack([q, q + n + 1, q + 1], 1), np.stack([q + n + 1, q + n + 2, q + 1], 1)]).astype(np.int32)
    rays = got[0].reshape(-1, 6)
    want = check_rays(v, t, rays.cpu().numpy(), methods=(("brute", {}), ("grid", {})))[0]
    d = rays.cpu().numpy()[:, 3:].astype(np.float64)
    norm = np.linalg.norm(d, axis=1)
    hit = want["triangle"] >= 0
    assert hit.sum() >= hit.size - 64                                       # (Moeller-Trumbore is not watertight: a ray through an edge may miss)
    bound = RC.MEASURED_K * RC.FACTOR * RC.ULP * (2.0 * norm + 2.0) / (1.0 / norm)     # cos = 1 / |d| against the plane's normal
    assert (np.abs(want["t"][hit].astype(np.float64) - 2.0) * norm[hit] <= bound[hit]).all()


def test_visible_points_two_quads_and_the_twin():
    v, t = RC.two_quads()
    rs = np.random.RandomState(3)
    pts = np.concatenate([np.stack([rs.uniform(-1, 1, 300), rs.uniform(-1, 1, 300), np.full(300, 2.0)], 1),        # on the far quad
                          np.stack([rs.uniform(-0.2, 0.2, 100), rs.uniform(-0.2, 0.2, 100), np.full(100, 1.0)], 1),  # on the near quad
                          rs.uniform(-3, 3, (100, 3))]).astype(f32)
    pts[7, 1] = np.nan
    cam = dict(fx=20.0, fy=20.0, cx=31.5, cy=31.5, H=64, W=64, z_near=0.1, z_far=4.0)
    K = np.array([[20.0, 0, 31.5], [0, 20.0, 31.5], [0, 0, 1]])
    one = np.eye(4, dtype=f32)[None]
    side = np.array([[[1, 0, 0, -0.8], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]], dtype=f32)
    mesh = upload(v, t)
    for poses in (one, np.concatenate([one, side])):
        for tol in (1e-3, 0.0):
            want = R.visibility(pts, v, t, poses, tolerance=tol, **cam)
            for method, grid in (("brute", None), ("grid", None), ("auto", None), ("auto", meshops.TriangleGrid(mesh, cell_size=0.07))):
                got = meshops.visible_points(_t(pts), mesh, poses, K, 64, 64, 0.1, 4.0, tolerance=tol, method=method, grid=grid)
                assert same(got["count"], want) and same(got["visible"], want > 0), (len(poses), tol, method)
    want = R.visibility(pts, v, t, one, tolerance=1e-3, **cam)
    far, near = pts[:300], want[:300]
    shadow = (np.abs(far[:, 0]) < 0.39) & (np.abs(far[:, 1]) < 0.39)        # the near quad's shadow on the far one: |x|, |y| < 0.4
    lit = ((np.abs(far[:, 0]) > 0.41) | (np.abs(far[:, 1]) > 0.41)) & np.isfinite(far).all(1)
    assert shadow.sum() > 20 and (near[shadow] == 0).all() and (near[lit] == 1).all()
    assert (want[300:400] == 1).all()                                       # the tolerance keeps the near quad's own samples visible
    two = R.visibility(pts, v, t, np.concatenate([one, side]), tolerance=1e-3, **cam)
    assert two.max() == 2 and (two >= want).all() and (two[:300][shadow] == 1).sum() > 5
    nothing = meshops.visible_points(_t(pts), upload(np.zeros((0, 3), f32), np.zeros((0, 3), np.int32)), one, K, 64, 64, 0.1, 4.0)
    rays, inside = R.visibility_rays(pts, one, **cam)
    assert same(nothing["count"], (inside & R.is_ray(rays.reshape(-1, 6)).reshape(inside.shape)).sum(0).astype(np.int32))     # an empty mesh: the frustum alone
    assert tuple(meshops.visible_points(_t(pts[:0]), mesh, one, K, 64, 64, 0.1, 4.0)["count"].shape) == (0,)


def test_scene_recall_over_what_the_cameras_saw():
    scene = _scene_loop("mesh")
    voxel, n = float(scene.volume.voxel_length), 4096
    plain = scene.geometry_metrics(scene, voxel, source="mesh", surface_samples=n)
    seen = scene.geometry_metrics(scene, voxel, source="mesh", surface_samples=n, visible_from="frames")
    print(f"{seen['n_ref']} of {n} samples of the scene's own mesh are seen from its {len(scene.frames)} frames; recall {plain['recall']:.3f} -> {seen['recall']:.3f}")
    assert seen["n_ref"] + seen["n_ref_culled"] == n and 0 < seen["n_ref"] and "n_ref_culled" not in plain
    assert seen["recall"] >= plain["recall"] and seen["precision"] == plain["precision"] and seen["accuracy"] == plain["accuracy"]
    assert seen == scene.geometry_metrics(scene, voxel, source="mesh", surface_samples=n, visible_from="frames")     # equal run to run
    raw = scene.clean_triangle_mesh(normals=False)["mesh"]
    look = scene.visible_surface(n_samples=n)
    assert int(look["visible"].sum().item()) == seen["n_ref"] and tuple(look["points"].shape) == (n, 3)
    assert bool((look["visible"] == (look["count"] > 0)).all())
    poses = scene._visibility_poses("frames", "test")
    by_array = scene.geometry_metrics(raw, voxel, source="mesh", surface_samples=n, visible_from=poses)
    assert by_array == seen
    # align: the scene registered onto its own mesh moves by (nearly) nothing, and the cameras follow it into the reference's frame
    aligned = scene.geometry_metrics(raw, voxel, source="mesh", surface_samples=n, visible_from="frames", align={"max_correspondence_distance": 4 * voxel})
    assert aligned["n_ref"] + aligned["n_ref_culled"] == n and abs(aligned["n_ref"] - seen["n_ref"]) <= n // 100 and aligned["recall"] == 1.0
    assert float((aligned["transformation"].cpu() - torch.eye(4, dtype=torch.float64)).abs().max()) < 1e-3
    away = poses[:1].copy()
    away[0, :3, 3] += 1e4                                                   # a camera that sees nothing of the scene
    with pytest.raises(ValueError, match="cull kept none"):
        scene.geometry_metrics(raw, voxel, source="mesh", surface_samples=n, visible_from=away)
    with pytest.raises(ValueError, match="surface_samples"):
        scene.geometry_metrics(scene, voxel, source="mesh", visible_from="frames")
    with pytest.raises(ValueError, match="surface"):
        scene.geometry_metrics(raw.vertices[:raw.n_vertices].contiguous(), voxel, source="mesh", surface_samples=n, visible_from="frames")
    with pytest.raises(ValueError, match="visible_from"):
        scene.geometry_metrics(scene, voxel, source="mesh", surface_samples=n, visible_from="cameras")
    with pytest.raises(ValueError, match="visible_from"):
        scene.geometry_metrics(scene, voxel, source="mesh", surface_samples=n, visible_from=np.eye(4))
