"""Quadric-error decimation on the GPU (meshops.simplify_quadric_decimation, csrc/mesh_simplify.hip) against its
numpy twin (tests/decimation_oracle.py) bit for bit: every case of tests/test_decimation_cpu.py — icospheres, flat and bumped
sheets, the fan and the degenerate shapes, with targets that stop inside the budget prefix, at "no_candidates", under max_error = 0
and after one round — in device buffers with poisoned excess capacity; the kernels one by one on one round's inputs; run to run;
the input left alone; the output through the rasteriser and the BVH; and a three-step rgbd scene through the scene-level
parameters."""
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import meshops, pointcloud
from sgam_neurips22_amd.tsdf import render_mesh_rgbd

sys.path.insert(0, os.path.dirname(__file__))
import decimation_oracle as DO  # noqa: E402
import test_decimation_cpu as C  # noqa: E402
from test_gpu_meshops import _scene_loop, same, same_mesh, upload  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32


def same_result(got, want):
    assert same_mesh(got["mesh"], want) and same(got["vertex_index"], want["vertex_index"])
    assert (got["rounds"], got["max_cost"], got["stopped"]) == (want["rounds"], want["max_cost"], want["stopped"])
    return True


@pytest.mark.parametrize("name,kw", C.CASES, ids=[f"{n}-{'-'.join(f'{k}={v}' for k, v in kw.items())}" for n, kw in C.CASES])
def test_bit_equality_with_the_twin(name, kw):
    v, t, c = C.mesh(name)
    got, want = meshops.simplify_quadric_decimation(upload(v, t, c), **kw), C.twin(name, **kw)
    print(f"{name} {kw}: {len(t)} -> {got['mesh'].n_triangles} triangles, {got['rounds']} rounds, max_cost {got['max_cost']:.3e}, {got['stopped']}")
    assert same_result(got, want)


@pytest.mark.parametrize("name", ["bump17", "fan", "zero_area", "ico2"])
def test_the_kernels_one_by_one(name):
    """the quadrics, one round's evaluation and its selection against the twin's, array by array (fp64 quadrics by their bits)"""
    v, t, c = C.mesh(name)
    mesh = upload(v, t, c)
    nv, nt = len(v), len(t)
    lib, flag = meshops._lib.load(), meshops._flag(DEV)
    p, st = meshops._p, meshops._stream
    by_tri, by_vert = meshops.incidence(mesh, "triangles"), meshops.incidence(mesh, "vertices")
    Q = torch.full((nv, 10), float("nan"), dtype=torch.float64, device=DEV)
    assert lib.sgam_mesh_quadric_init_f64(p(mesh.vertices), nv, p(mesh.triangles), nt, *meshops._csr_args(by_tri), 1.5, p(Q), p(flag), st()) == 0
    wantQ = DO.vertex_quadrics(v, t, 1.5)
    assert np.array_equal(Q.cpu().numpy().view(np.uint64), wantQ.view(np.uint64))
    edges, _, _, eoe = DO.edges_of(t, nv)
    ne = len(edges)
    ed, eo = torch.from_numpy(edges).to(DEV), torch.from_numpy(eoe).to(DEV)
    cost, removed = torch.empty((ne,), dtype=torch.float32, device=DEV), torch.empty((ne,), dtype=torch.int32, device=DEV)
    pos, col = torch.empty((ne, 3), dtype=torch.float32, device=DEV), torch.empty((ne, 3), dtype=torch.float32, device=DEV)
    assert lib.sgam_mesh_collapse_evaluate_f64(p(mesh.vertices), p(mesh.vertex_colors), nv, p(mesh.triangles), nt, p(Q), *meshops._csr_args(by_tri),
                                               *meshops._csr_args(by_vert), p(ed), ne, p(cost), p(removed), p(pos), p(col), p(flag), st()) == 0
    ev = DO.evaluate(v, c, t, wantQ, edges)
    assert same(cost, ev["cost"]) and same(removed, ev["removed"]) and same(pos, ev["position"]) and same(col, ev["color"])
    legal = np.sort(ev["cost"][np.isfinite(ev["cost"])])
    assert len(legal) > 0 and (len(legal) < ne) == (name != "ico2")      # (a closed sphere refuses no edge, a border some)
    for tau in (legal[0], legal[len(legal) // 2], legal[-1]):
        ws, nbytes = meshops.geometry.workspace("sgam_mesh_collapse_workspace_bytes", DEV, nv)
        key = torch.full((ne,), 7, dtype=torch.int64, device=DEV)
        assert lib.sgam_mesh_collapse_select_i32(nv, *meshops._csr_args(by_vert), p(eo), p(ed), p(cost), ne, float(tau), p(ws), nbytes, p(key), p(flag),
                                                 st()) == 0
        sel = DO.select(nv, by_vert["offsets"].cpu().numpy(), by_vert["items"].cpu().numpy(), edges, ev["cost"], tau)
        want = np.where(sel, (ev["cost"].view(np.uint32).astype(np.int64) << 32) | DO.edge_priority(np.arange(ne)).astype(np.int64), -1)
        assert sel.any() and same(key, want)
    assert int(flag.item()) == 0


def test_two_calls_give_equal_bits_and_leave_the_input_alone():
    v, t, c = C.mesh("bump17")
    mesh = upload(v, t, c)
    before = [x.clone() for x in (mesh.vertices, mesh.vertex_colors, mesh.triangles, mesh.counts)]
    a = meshops.simplify_quadric_decimation(mesh, target_triangles=128)
    b = meshops.simplify_quadric_decimation(mesh, target_triangles=128)
    for x, y in zip(before, (mesh.vertices, mesh.vertex_colors, mesh.triangles, mesh.counts)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))        # (bits: the poisoned rows are NaN)
    assert (a["rounds"], a["max_cost"], a["stopped"]) == (b["rounds"], b["max_cost"], b["stopped"])
    for k in ("vertices", "vertex_colors", "triangles"):
        assert torch.equal(getattr(a["mesh"], k).view(torch.int32), getattr(b["mesh"], k).view(torch.int32)), k
    assert torch.equal(a["vertex_index"], b["vertex_index"])
    # a target the mesh meets already: a copy, not the input's buffers
    same_size = meshops.simplify_quadric_decimation(mesh, target_ratio=1.0)
    assert same_size["rounds"] == 0 and same_size["stopped"] == "target" and same(same_size["mesh"].vertices, v) and same(same_size["mesh"].triangles, t)
    assert same_size["mesh"].vertices.data_ptr() != mesh.vertices.data_ptr()


def test_the_output_renders_and_builds_a_bvh():
    v, t, c = C.mesh("ico3")
    out = meshops.simplify_quadric_decimation(upload(v, t, (c * f32(255)).astype(f32)), target_triangles=320)["mesh"]
    K = np.asarray([[80.0, 0, 32], [0, 80.0, 32], [0, 0, 1]])
    T = np.eye(4)
    T[2, 3] = 3.0                                                           # the camera 3 in front of the unit sphere
    r = render_mesh_rgbd(out, K, T[None], 64, 64, 0.5, 8.0)
    depth = r["depth"][0]
    assert 0.1 < float((depth > 0).float().mean()) < 0.9 and abs(float(depth[32, 32]) - 2.0) < 0.05
    tree = meshops.TriangleBVH(out)
    assert tree.n_candidates == out.n_triangles == 320
    rays = torch.tensor([[0.0, 0.0, -3.0, 0.0, 0.0, 1.0], [0.0, 5.0, -3.0, 0.0, 0.0, 1.0]], device=DEV)
    hit = tree.cast_rays(rays)
    assert abs(float(hit["t"][0]) - 2.0) < 0.05 and int(hit["triangle"][1]) == -1
    d = meshops.point_mesh_distance(torch.from_numpy(v).to(DEV), out, accel=tree)["d2"]
    assert float(d.max()) < 0.05 ** 2                                       # the input's vertices lie near the decimated sphere


def test_scene_simplifies_and_exports(tmp_path):
    scene = _scene_loop("mesh")
    a, b = tmp_path / "a", tmp_path / "b"
    n = scene.export_triangle_mesh(str(a))
    name, sname = "rgbd_integrated_triangle_mesh.ply", "rgbd_integrated_triangle_mesh_simplified.ply"
    counts = scene.export_triangle_mesh(str(b), simplify={"target_ratio": 0.25})
    assert (b / name).read_bytes() == (a / name).read_bytes() and counts[name] == n and sorted(os.listdir(b)) == sorted([name, sname])
    out = scene.simplify_triangle_mesh(target_ratio=0.25)
    print(f"scene mesh: {n} -> {counts[sname]} triangles in {out['rounds']} rounds, max_cost {out['max_cost']:.3e}, {out['stopped']}")
    assert out["mesh"].n_triangles == counts[sname] and (counts[sname] <= n // 4 or out["stopped"] in ("no_candidates", "max_rounds"))
    assert counts[sname] < n
    back = pointcloud.read_triangle_mesh(str(b / sname))
    assert np.array_equal(back["vertices"], out["mesh"].vertices.cpu().numpy().astype(np.float64))
    assert np.array_equal(back["triangles"], out["mesh"].triangles.cpu().numpy())
    assert np.array_equal(back["normals"], out["vertex_normals"].cpu().numpy().astype(np.float64))
    raw = scene.colour_volume().extract_mesh_device()
    assert raw.n_triangles == n and int(out["vertex_index"].max()) < raw.n_vertices
    cleaned = scene.simplify_triangle_mesh(clean=dict(min_triangles=50), target_ratio=0.5)
    assert 0 < cleaned["mesh"].n_triangles < n and int(cleaned["vertex_index"].max()) < raw.n_vertices
    for call in (lambda: scene.export_triangle_mesh(str(b), simplify={"ratio": 0.5}), lambda: scene.simplify_triangle_mesh(target=3),
                 lambda: scene.render_views(np.eye(4)[None], source="points", mesh_simplify={"target_ratio": 0.5})):
        with pytest.raises(ValueError, match="simplify"):
            call()
    poses = [scene.transform_grid[c[0]][c[1]]["T"] for c in scene._ordered_grid_coords[1:3]]
    views = scene.render_views(poses, source="mesh", mesh_simplify={"target_ratio": 0.25}, H=64, W=64)
    assert tuple(views["depth"].shape) == (2, 64, 64) and all(bool((views["depth"][p] > 0).any()) for p in range(2))
    s = scene.geometry_metrics(scene, 0.01, source="mesh", mesh_simplify={"target_ratio": 0.25})
    assert s["chamfer"] == 0.0 and s["n_pred"] == s["n_ref"] == out["mesh"].n_vertices
