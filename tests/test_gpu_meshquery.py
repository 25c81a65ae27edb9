"""Queries against a mesh on the GPU (sgam_neurips22_amd/meshops.py, csrc/mesh_query.hip) against their numpy twin
(tests/meshquery_oracle.py) bit for bit: point–mesh distance by brute force and by the triangle grid (the same bits, at every cell
size) on hand meshes and on the marching-cubes meshes of tests/test_meshops_cpu.py in device buffers with poisoned excess
capacity, the area-uniform sampler, surface_metrics, and a three-step rgbd scene scored as a surface."""
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import geometry, meshops
from sgam_neurips22_amd.ops import SgamHipError

sys.path.insert(0, os.path.dirname(__file__))
import meshquery_oracle as Q  # noqa: E402
import test_meshops_cpu as C  # noqa: E402
import test_meshquery_cpu as QC  # noqa: E402
from test_gpu_meshops import _scene_loop, same, upload  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
_TWIN = {}


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def check_distance(v, t, q, methods=(("brute", {}), ("grid", {})), max_distance=None, want=None):
    """every method against the twin: d2, triangle and closest bit for bit -> the twin's answer"""
    if want is None:
        want = Q.mesh_distance(v, t, q, np.inf if max_distance is None else geometry.max_d2_of(max_distance))
    mesh = upload(v, t)
    for method, kw in methods:
        got = meshops.point_mesh_distance(_t(q), mesh, method=method, max_distance=max_distance, closest=True, **kw)
        for k in ("d2", "triangle", "closest"):
            assert same(got[k], want[k]), (method, kw, k)
        bare = meshops.point_mesh_distance(_t(q), mesh, method=method, max_distance=max_distance, **kw)
        assert sorted(bare) == ["d2", "triangle"] and same(bare["d2"], want["d2"]) and same(bare["triangle"], want["triangle"])
    return want


def hand_queries(n, lo, hi, seed=0):
    """n queries around the box [lo, hi], NaN and inf rows among them (row 0 stays a point)"""
    rs = np.random.RandomState(seed)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    q = rs.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), (n, 3)).astype(f32)
    if n > 4:
        q[n // 3, 1] = np.nan
        q[n // 2, 0] = np.inf
        q[n - 2] = -np.inf
    return q


@pytest.mark.parametrize("nq", [1, 255, 257, 1000])
def test_single_triangle_every_region_and_query_count(nq):
    v, t = QC.HAND, np.array([[0, 1, 2]], dtype=np.int32)
    regions = np.array([p for p, _, _ in QC.REGION_QUERIES], dtype=f32)
    q = np.concatenate([regions, hand_queries(max(nq - len(regions), 0), [0, 0, -1], [4, 3, 1], nq)])[:nq] if nq > 1 else regions[6:7]
    want = check_distance(v, t, q)
    if nq > 1:
        assert want["region"][:10].tolist() == [r for _, r, _ in QC.REGION_QUERIES]
        assert (want["triangle"] == -1).sum() == (3 if nq > 14 else 0)


def test_shared_edge_tie_goes_to_the_lower_index():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=f32)
    t = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32)
    q = np.array([[0.5, 0.5, 1.0], [0.25, 0.75, 2.0], [1.0, 0.0, 0.5], [0.1, 0.1, 0.3], [0.9, 0.9, 0.3]], dtype=f32)
    for tri in (t, t[::-1].copy()):
        want = check_distance(v, tri, q)
        assert want["triangle"][:3].tolist() == [0, 0, 0] and want["d2"][:3].tolist() == [1.0, 4.0, 0.25]
    assert check_distance(v, t, q)["triangle"][3:].tolist() == [0, 1] and check_distance(v, t[::-1].copy(), q)["triangle"][3:].tolist() == [1, 0]


def test_what_is_not_a_triangle_never_wins():
    rs = np.random.RandomState(4)
    v = rs.uniform(0, 2, (40, 3)).astype(f32)
    v[7] = np.nan
    v[11, 2] = np.inf
    t = rs.randint(0, 40, (90, 3)).astype(np.int32)
    t[::5, 1] = t[::5, 0]                                                  # a repeated vertex
    v[20], v[21], v[22] = [0.5, 0.5, 0.5], [1.0, 1.0, 1.0], [1.5, 1.5, 1.5]
    t[3] = [20, 21, 22]                                                    # collinear: no area
    a2 = Q.area2(v, t)
    assert (a2 == 0).sum() >= 20 and (a2 > 0).sum() >= 40
    want = check_distance(v, t, hand_queries(257, [0, 0, 0], [2, 2, 2], 1))
    assert (a2[want["triangle"][want["triangle"] >= 0]] > 0).all()
    assert same(meshops.triangle_areas(upload(v, t)), (a2 * f32(0.5)).astype(f32))


def spanning_mesh():
    """about 200 small triangles in the unit box and one spanning the whole box"""
    rs = np.random.RandomState(8)
    centre = rs.uniform(0.05, 0.95, (200, 1, 3))
    small = (centre + rs.normal(0, 0.01, (200, 3, 3))).astype(f32)
    v = np.concatenate([small.reshape(-1, 3), np.array([[0, 0, 0], [1, 1, 0], [0.5, 0.5, 1]], dtype=f32)])
    t = np.arange(603, dtype=np.int32).reshape(201, 3)
    return v, np.concatenate([t[:77], t[200:], t[77:200]])                 # the large one in the middle of the list


def test_multi_cell_entries_and_the_growing_cell_edge():
    v, t = spanning_mesh()
    q = hand_queries(1000, [0, 0, 0], [1, 1, 1], 2)
    want = check_distance(v, t, q, methods=(("brute", {}), ("grid", {}), ("grid", {"cell_size": 0.02})))
    assert (want["triangle"] == 77).sum() > 50                             # the spanning triangle is the nearest for many queries
    mesh = upload(v, t)
    fine = meshops.TriangleGrid(mesh, cell_size=0.02, max_entries_per_triangle=1e9)
    capped = meshops.TriangleGrid(mesh, cell_size=0.02, max_entries_per_triangle=3.0)
    assert fine.cell_size == pytest.approx(0.02) and fine.n_entries > 50 * fine.n_candidates           # the spanning triangle alone fills a slab of cells
    assert capped.cell_size > fine.cell_size and capped.n_entries <= 3.0 * capped.n_candidates and capped.n_candidates == 201
    for grid in (fine, capped):
        got = grid.query(_t(q), closest=True)
        for k in ("d2", "triangle", "closest"):
            assert same(got[k], want[k]), k
    # more than 1024 scan tiles (1 048 576 cells): every lane of the tile scan takes more than one tile sum
    rs, h = np.random.RandomState(9), 1.0 / 64.0
    corner = rs.uniform(0.0, 1022.0 * h, (300, 1, 2))
    corner[0], corner[1] = 0.0, [1024.5 * h - 0.01, 1023.5 * h - 0.01]
    v = np.concatenate([corner + np.array([[0.0, 0.0], [0.01, 0.0], [0.0, 0.01]]), np.full((300, 3, 1), 0.25)], axis=2).reshape(-1, 3).astype(f32)
    v[4, 0], v[5, 1] = 1024.5 * h, 1023.5 * h
    t = np.arange(900, dtype=np.int32).reshape(300, 3)
    wide = meshops.TriangleGrid(upload(v, t), cell_size=h, max_entries_per_triangle=1e9)
    assert wide.cell_size == h and wide.n_candidates == 300 and -(-int(np.prod(wide.dims)) // 1024) > 1024, wide.dims
    q = hand_queries(300, [4, 4, 0], [12, 12, 0.5], 3)                     # over the mesh's extent: a shell walk of some 100 cells at most
    want, got = Q.mesh_distance(v, t, q), wide.query(_t(q), closest=True)
    for k in ("d2", "triangle", "closest"):
        assert same(got[k], want[k]), k


def mesh_queries(v):
    """1000 queries: inside the box, near the surface, outside the box (clamped cells, many shells), 1e3 box sizes away"""
    rs = np.random.RandomState(6)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    size = (hi - lo).max()
    away = rs.normal(0, 1, (100, 3))
    q = np.concatenate([rs.uniform(lo, hi, (300, 3)), v[rs.randint(0, len(v), 300)] + rs.normal(0, 0.01 * size, (300, 3)),
                        rs.uniform(lo - 3 * size, hi + 3 * size, (300, 3)), (lo + hi) / 2 + away / np.linalg.norm(away, axis=1, keepdims=True) * 1e3 * size])
    q = q.astype(f32)
    q[17, 0] = np.nan
    q[555] = np.inf
    return q


def twin(name):
    if name not in _TWIN:
        m = C.mesh(name)
        q = mesh_queries(m["vertices"])
        _TWIN[name] = (q, Q.mesh_distance(m["vertices"], m["triangles"], q))
    return _TWIN[name]


@pytest.mark.parametrize("name", ["sphere", "noise"])
def test_marching_cubes_meshes_brute_and_grid_give_the_twins_bits(name):
    m = C.mesh(name)
    v, t = m["vertices"], m["triangles"]
    q, want = twin(name)
    default = meshops.TriangleGrid(upload(v, t))
    assert default.n_entries <= 8 * default.n_candidates and max(default.dims) > 4
    one_cell = float((v.max(0) - v.min(0)).max()) * 2
    methods = (("brute", {}), ("grid", {}), ("grid", {"cell_size": one_cell}), ("grid", {"cell_size": default.cell_size / 4}), ("auto", {}))
    check_distance(v, t, q, methods=methods, want=want)
    assert meshops.TriangleGrid(upload(v, t), cell_size=one_cell).dims == (1, 1, 1)
    assert (want["triangle"] >= 0).sum() == 998


def test_max_distance_cuts_where_the_twin_cuts():
    m = C.mesh("sphere")
    v, t = m["vertices"], m["triangles"]
    q, full = twin("sphere")
    cut = float(np.sqrt(np.median(full["d2"][np.isfinite(full["d2"])])))
    want = check_distance(v, t, q, max_distance=cut)
    assert 300 < (want["triangle"] >= 0).sum() < 700 and np.isinf(want["d2"][want["triangle"] < 0]).all()
    on = np.concatenate([v[:64], q[:64]]).astype(f32)                     # vertices lie on the surface: the only hits at max_distance = 0
    want = check_distance(v, t, on, max_distance=0.0)
    assert (want["triangle"][:64] >= 0).all() and (want["d2"][:64] == 0).all() and (want["triangle"][64:] == -1).all()


def test_no_launch_paths_and_argument_errors():
    m = C.mesh("sphere")
    mesh = upload(m["vertices"], m["triangles"])
    empty = upload(np.zeros((0, 3), f32), np.zeros((0, 3), np.int32))
    q = _t(mesh_queries(m["vertices"])[:10])
    for method in ("brute", "grid", "auto"):
        out = meshops.point_mesh_distance(q, empty, method=method, closest=True)
        assert out["triangle"].cpu().tolist() == [-1] * 10 and bool(torch.isinf(out["d2"]).all()) and bool(torch.isnan(out["closest"]).all())
        out = meshops.point_mesh_distance(q[:0], mesh, method=method, closest=True)
        assert tuple(out["d2"].shape) == (0,) and tuple(out["triangle"].shape) == (0,) and tuple(out["closest"].shape) == (0, 3)
    no_area = upload(np.zeros((3, 3), f32), np.array([[0, 1, 2]], np.int32))
    assert meshops.point_mesh_distance(q, no_area, method="grid")["triangle"].cpu().tolist() == [-1] * 10
    assert meshops.sample_points(mesh, 0)["points"].shape == (0, 3)
    with pytest.raises(ValueError):
        meshops.sample_points(no_area, 4)
    with pytest.raises(SgamHipError):
        meshops.point_mesh_distance(q.cpu(), mesh)
    with pytest.raises(ValueError):
        meshops.point_mesh_distance(q, mesh, method="tree")
    with pytest.raises(ValueError):
        meshops.point_mesh_distance(q, mesh, method="brute", cell_size=0.1)
    with pytest.raises(ValueError):
        meshops.surface_metrics(mesh, q, 0.1)                              # a mesh needs n_samples


def test_vertex_index_out_of_range_raises():
    m = C.mesh("sphere")
    t = m["triangles"].copy()
    t[100, 1] = len(m["vertices"])                                         # one past the mesh: the poisoned capacity lies behind it
    t[2000, 2] = -1
    mesh = upload(m["vertices"], t)
    q = _t(mesh_queries(m["vertices"])[:300])
    for call in (lambda: meshops.point_mesh_distance(q, mesh, method="brute"), lambda: meshops.point_mesh_distance(q, mesh, method="grid"),
                 lambda: meshops.triangle_areas(mesh), lambda: meshops.sample_points(mesh, 16)):
        with pytest.raises(SgamHipError, match="outside the mesh"):
            call()


@pytest.mark.parametrize("n", [1, 255, 1025])
def test_sample_points_against_the_twin(n):
    m = C.mesh("noise")
    v, t, col = m["vertices"], m["triangles"], m["colors"]
    mesh = upload(v, t, col)
    for seed in (0, 0x1234567887654321):
        want = Q.sample(v, t, n, seed, colors=col, want_normals=True)
        got = meshops.sample_points(mesh, n, seed=seed, normals=True)
        for k in ("points", "triangle", "colors", "normals"):
            assert same(got[k], want[k]), (seed, k)
        again = meshops.sample_points(mesh, n, seed=seed, normals=True)
        assert all(torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)) for k in ("points", "triangle", "colors", "normals"))
        plain = meshops.sample_points(upload(v, t), n, seed=seed)
        assert plain["colors"] is None and "normals" not in plain and same(plain["points"], want["points"])
        assert meshops.sample_points(mesh, n, seed=seed, colors=False)["colors"] is None
        longer = meshops.sample_points(mesh, n + 300, seed=seed)
        assert same(longer["points"][:n], want["points"]) and same(longer["triangle"][:n], want["triangle"])
    assert not torch.equal(meshops.sample_points(mesh, n, seed=1)["points"], meshops.sample_points(mesh, n, seed=2)["points"])


def test_surface_metrics_against_the_twin():
    m, s = C.mesh("sphere"), C.mesh("three")
    a, b = (m["vertices"], m["triangles"]), (s["vertices"], s["triangles"])
    ma, mb = upload(*a), upload(*b)
    cloud = (a[0][::3] + f32(0.01)).astype(f32)
    cloud[5] = np.nan

    def nearest(p, c):
        return geometry.nearest_neighbors(_t(p), _t(c), "brute")["d2"].cpu().numpy()

    for pred, ref, dp, dr in ((a, b, ma, mb), (a, cloud, ma, _t(cloud)), (cloud, b, _t(cloud), mb)):
        want = Q.surface_metrics(pred, ref, 0.05, n_samples=777, seed=3, nearest=nearest)
        for method in ("brute", "grid"):
            got = meshops.surface_metrics(dp, dr, 0.05, n_samples=777, seed=3, method=method)
            assert sorted(got) == sorted(want)
            for k in want:
                assert got[k] == pytest.approx(want[k], rel=1e-12), (k, method)
    both = meshops.surface_metrics(_t(cloud), _t(a[0]), 0.05)
    assert both == geometry.cloud_metrics(_t(cloud), _t(a[0]), 0.05)


def test_scene_is_scored_as_a_surface():
    scene = _scene_loop("mesh")
    voxel = float(scene.volume.voxel_length)
    s = scene.geometry_metrics(scene, voxel, source="mesh", surface_samples=4096)
    assert s["precision"] == s["recall"] == s["fscore"] == 1.0 and s["n_pred"] == s["n_ref"] == 4096
    raw = scene.clean_triangle_mesh(normals=False)["mesh"]
    kw = dict(voxel_size=4 * voxel)
    # the reference: points ON the clustered mesh's own surface.  Scored by its vertices the scene is incomplete by about half an
    # edge of the simplification; scored as a surface it is complete up to rounding — the defect surface_samples removes
    clustered = scene.clean_triangle_mesh(normals=False, **kw)["mesh"]
    assert 0 < clustered.n_triangles < raw.n_triangles
    on_surface = meshops.sample_points(clustered, 4096, seed=7, colors=False)["points"]
    by_vertex = scene.geometry_metrics(on_surface, voxel, source="mesh", mesh_clean=kw)
    by_surface = scene.geometry_metrics(on_surface, voxel, source="mesh", mesh_clean=kw, surface_samples=4096)
    print(f"completeness of the mesh clustered at 4 voxels against points on its own surface: by vertices {by_vertex['completeness']:.3e}, "
          f"as a surface {by_surface['completeness']:.3e}; recall {by_vertex['recall']:.3f} / {by_surface['recall']:.3f} (voxel {voxel})")
    tol = QC.TOL_UNITS * QC.ULP * float(clustered.vertices[:clustered.n_vertices].abs().max())
    assert by_surface["completeness"] <= tol < by_vertex["completeness"]
    assert by_surface["recall"] == 1.0 >= by_vertex["recall"]
    as_mesh = scene.geometry_metrics(raw, voxel, source="mesh", surface_samples=4096)
    assert as_mesh["precision"] == as_mesh["recall"] == 1.0
    with pytest.raises(ValueError, match="surface_samples"):
        scene.geometry_metrics(raw, voxel, source="mesh")
    with pytest.raises(ValueError, match="voxel_size"):
        scene.geometry_metrics(scene, voxel, source="mesh", surface_samples=64, voxel_size=voxel)
    before = scene.geometry_metrics(scene, 0.01, source="mesh")
    assert before == scene.geometry_metrics(scene, 0.01, source="mesh", surface_samples=None)
    assert before["chamfer"] == 0.0 and before["fscore"] == 1.0 and before["n_pred"] == raw.n_vertices
