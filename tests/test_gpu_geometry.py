"""GPU: the geometry kernels (csrc/point_nn.hip through sgam_neurips22_amd/geometry.py) — brute-force and grid nearest neighbours
equal to the numpy twin (tests/geometry_oracle.py) and to each other bit for bit (d2 as uint32, index exactly) at edge sizes, grid
shapes, ties, queries outside the box, varied cell sizes, NaN points and a distance limit; the fp64 reductions; the frame store
unprojected in one launch; and the scene-level callers merged_point_cloud / geometry_metrics on both warp branches."""
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import geometry, testing

sys.path.insert(0, os.path.dirname(__file__))
import geometry_oracle as GO  # noqa: E402
from test_geometry_cpu import cloud, frames_case, twin_unproject  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nn(q, r, method, **kw):
    out = geometry.nearest_neighbors(_t(q), _t(r), method=method, **kw)
    assert out["d2"].is_cuda and out["d2"].dtype == torch.float32 and out["index"].dtype == torch.int32
    assert out["d2"].shape == out["index"].shape == q.shape[:-1]
    return out["d2"].cpu().numpy(), out["index"].cpu().numpy()


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(_bits(got[0]), _bits(want[0])), what


def _check(q, r, max_distance=None, cell_sizes=(None,), what=""):
    """brute and grid (at every cell size) against the twin; returns the twin's (d2, index)"""
    want = GO.nn_brute(q, r, GO.max_d2_of(max_distance))
    _same(_nn(q, r, "brute", max_distance=max_distance), want, ("brute", what))
    for cs in cell_sizes:
        _same(_nn(q, r, "grid", max_distance=max_distance, cell_size=cs), want, ("grid", cs, what))
    return want


SIZES = (1, 63, 64, 65, 257)


@pytest.mark.parametrize("nq", SIZES)
def test_edge_sizes_equal_the_twin(nq):
    for nr in SIZES:
        d2, idx = _check(cloud(nq, 10 + nq), cloud(nr, 20 + nr), what=(nq, nr))
        assert (idx >= 0).all() and np.isfinite(d2).all()


def test_more_than_one_tile_and_workgroup():
    _check(cloud(2500, 1), cloud(3001, 2), what="2500 x 3001")


def test_batched_clouds_are_independent():
    q, r = np.stack([cloud(257, s) for s in (1, 2, 3)]), np.stack([cloud(65, s) for s in (4, 5, 6)])
    r[1, ::2] = np.nan
    r[2] = np.nan                                                       # a batch item without a valid reference point
    want = [GO.nn_brute(q[b], r[b]) for b in range(3)]
    for method in ("brute", "grid"):
        d2, idx = _nn(q, r, method)
        for b in range(3):
            _same((d2[b], idx[b]), want[b], (method, b))
    assert (want[2][1] == -1).all() and (want[1][1] % 2 == 1).all()


def test_grid_shapes():
    rs = np.random.RandomState(7)
    q = cloud(300, 3, -2.0, 12.0)
    # clusters far apart: most cells are empty
    centres = rs.uniform(0, 10, (6, 3))
    sparse = (centres[rs.randint(0, 6, 2000)] + rs.normal(0, 0.01, (2000, 3))).astype(f32)
    assert np.prod(geometry.grid_for(sparse.min(0), sparse.max(0), 2000)[2]) > 500
    _check(q, sparse, what="sparse")
    _check(sparse[::7], sparse, what="sparse on itself")
    # all points in one cell
    _check(q, cloud(500, 4), cell_sizes=(100.0,), what="one cell")
    # degenerate boxes: coplanar, collinear, a single point
    plane = cloud(700, 5)
    plane[:, 1] = 3.25
    _check(q, plane, what="coplanar")
    line = cloud(400, 6)
    line[:, 0], line[:, 2] = 2.5, -1.0
    _check(q, line, what="collinear")
    _check(line[::3], line, what="collinear on itself")
    _check(q, cloud(1, 8), what="single point")
    _check(q, np.repeat(cloud(1, 8), 5, axis=0), what="one point five times")
    # more than 1024 scan tiles (1 048 576 cells): every lane of the tile scan takes more than one tile sum
    h = 1.0 / 64.0
    wide = np.concatenate([[[0.0, 0.0], [1024.5 * h, 1023.5 * h]], rs.uniform(0.0, 1023.5 * h, (1998, 2))])
    wide = np.concatenate([wide, np.full((2000, 1), 0.5)], axis=1).astype(f32)
    dims = geometry.PointGrid(_t(wide), cell_size=h).dims
    assert -(-int(np.prod(dims)) // 1024) > 1024, dims
    _check(rs.uniform([-1.0, -1.0, 0.0], [17.0, 17.0, 1.0], (300, 3)).astype(f32), wide, cell_sizes=(h,), what="1025 scan tiles")


def test_exact_ties_go_to_the_lower_index_and_calls_repeat():
    r = cloud(600, 11)
    r2 = np.concatenate([r, r])
    q = np.concatenate([cloud(300, 12), r[::5]])
    d2, idx = _check(q, r2, what="duplicated")
    assert (idx < 600).all() and (d2[300:] == 0).all()
    lattice = np.stack(np.meshgrid(*[np.arange(6.0)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    d2, idx = _check(lattice + f32(0.5), lattice, cell_sizes=(None, 1.0, 0.37), what="cell centres: eight equal neighbours")
    assert (d2 == 0.75).all()
    for method in ("brute", "grid"):
        a, b = _nn(q, r2, method), _nn(q, r2, method)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_queries_outside_the_box_and_on_its_faces():
    r = cloud(3000, 13)
    lo, hi = r.min(0), r.max(0)
    rs = np.random.RandomState(14)
    q = [cloud(50, 15)]
    for axes in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 2), (0, 1, 2)):
        for sign, far in ((1, 3.0), (-1, 3.0), (1, 5e3), (-1, 1e6)):
            p = rs.uniform(lo, hi, (8, 3)).astype(f32)
            for a in axes:
                p[:, a] = (hi[a] if sign > 0 else lo[a]) + sign * f32(far)
            q.append(p)
    faces = rs.uniform(lo, hi, (60, 3)).astype(f32)                     # exactly on the faces, edges and corners of the box
    for k in range(60):
        for a in range(3):
            if (k >> a) & 1 or k % 3 == a:
                faces[k, a] = lo[a] if (k >> (a + 3)) & 1 else hi[a]
    q.append(faces)
    q.append(np.stack([lo, hi, f32(0.5) * (lo + hi)]))
    q = np.concatenate(q)
    d2, idx = _check(q, r, cell_sizes=(None, 0.3, 2.5), what="outside")
    assert (idx >= 0).all()


def test_results_do_not_depend_on_the_cell_size():
    r, q = cloud(5000, 16), cloud(1500, 17, 0.0, 11.0)
    h = geometry.PointGrid(_t(r)).cell_size
    d2, idx = _check(q, r, cell_sizes=(0.25 * h, h, 4 * h), what="cell sizes")
    md = float(np.sqrt(np.median(d2)))
    d2m, idxm = _check(q, r, max_distance=md, cell_sizes=(0.25 * h, h, 4 * h), what="cell sizes with a limit")
    assert 0.3 < (idxm >= 0).mean() < 0.7


def test_nan_points_are_not_points():
    rs = np.random.RandomState(18)
    r, q = cloud(2000, 19), cloud(900, 20)
    r[rs.choice(2000, 600, replace=False), rs.randint(0, 3, 600)] = np.nan
    r[rs.choice(2000, 20, replace=False), 1] = np.inf
    q[rs.choice(900, 200, replace=False), rs.randint(0, 3, 200)] = np.nan
    q[5, 2] = -np.inf
    d2, idx = _check(q, r, cell_sizes=(None, 0.4), what="NaN share")
    bad_q = ~np.isfinite(q).all(1)
    assert (idx[bad_q] == -1).all() and np.isinf(d2[bad_q]).all() and (idx[~bad_q] >= 0).all()
    assert np.isfinite(r[idx[~bad_q]]).all()
    d2, idx = _check(q, np.full((300, 3), np.nan, dtype=f32), what="all-NaN reference")
    assert (idx == -1).all() and (d2 == np.inf).all()


def test_max_distance_just_inside_and_just_outside():
    far = cloud(500, 21, 5.0, 9.0)
    r = np.concatenate([np.zeros((1, 3), f32), far])
    up = np.nextafter(f32(0.5), f32(1))
    q = np.array([[0.5, 0, 0], [up, 0, 0], [0, -0.5, 0], [0, 0, -up], [0.25, 0.25, 0.25], [7, 7, 7]], dtype=f32)
    d2, idx = _check(q, r, max_distance=0.5, cell_sizes=(None, 0.2, 3.0), what="limit 0.5")
    assert idx[:5].tolist() == [0, -1, 0, -1, 0] and d2[:5].tolist() == [0.25, np.inf, 0.25, np.inf, 0.1875]
    d2, idx = _check(cloud(400, 22), far, max_distance=0.0, what="limit 0")
    assert (idx == -1).all()
    d2, idx = _check(far[::3], far, max_distance=0.0, cell_sizes=(None, 0.1), what="limit 0 on itself")
    assert (d2 == 0).all()


@pytest.mark.parametrize("n", [1, 255, 4095, 4096, 4097, 20000])
def test_reductions_equal_the_twin(n):
    rs = np.random.RandomState(n)
    d2 = (rs.uniform(0, 3, n) ** 2).astype(f32)
    d2[rs.choice(n, n // 7, replace=False)] = np.inf
    d2[rs.choice(n, n // 9, replace=False)] = 0
    tau = 1.5
    d2[:: max(1, n // 5)] = f32(tau) * f32(tau)                        # on the threshold counts as within
    got, want = geometry.reduce_d2(_t(d2), tau), GO.reduce(d2, tau)
    assert got[2:] == want[2:]                                          # counts: exact
    for g, w in zip(got[:2], want[:2]):                                 # sums: the fold order is the only difference
        assert abs(g - w) <= 1e-12 * abs(w)
    if n == 20000:
        assert want[2] < n and 0 < want[3] < want[2]


@pytest.mark.parametrize("shape", [("google_earth", 48, 40, 3), ("clevr-infinite", 8, 8, 70)])
def test_unproject_frames_equal_the_twin(shape):
    data, Hs, Ws, F = shape
    case = frames_case(data, Hs, Ws, F=F, seed=F)
    out = geometry.unproject_frames([_t(d) for d in case["depths"]], [_t(c) for c in case["rgbs"]], case["K"], case["Ts"], case["z_near"],
                                    case["z_far"])
    assert set(out) == {"points", "colors"} and all(t.is_cuda for t in out.values())
    assert out["points"].shape == (F * Hs * Ws, 3) and out["colors"].shape == (F * Hs * Ws, 3) and out["colors"].dtype == torch.uint8
    pts = out["points"].cpu().numpy()
    assert np.array_equal(_bits(pts), _bits(twin_unproject(case)))
    assert np.array_equal(out["colors"].cpu().numpy(), np.concatenate([c.reshape(-1, 3) for c in case["rgbs"]]))
    nan = np.isnan(pts).all(1)
    assert nan.sum() == 10 * F and (np.isnan(pts).any(1) == nan).all()   # the seeded depths, all three coordinates, nothing else
    with np.errstate(invalid="ignore"):
        d = np.concatenate([x.ravel() for x in case["depths"]])
        assert np.array_equal(nan, ~(np.isfinite(d) & (d >= f32(case["z_near"])) & (d <= f32(case["z_far"]))))
    geo = geometry.unproject_frames([_t(d) for d in case["depths"]], None, case["K"], case["Ts"], case["z_near"], case["z_far"])
    assert set(geo) == {"points"} and np.array_equal(_bits(geo["points"].cpu().numpy()), _bits(pts))


def test_cloud_metrics_on_a_shifted_sparse_cloud():
    """a unit lattice against itself shifted by a quarter along x: the shifted copy of a point is its nearest (0.25 against 0.75
    and more), every number is exact"""
    lattice = np.stack(np.meshgrid(np.arange(7.0), np.arange(5.0), np.arange(3.0), indexing="ij"), -1).reshape(-1, 3).astype(f32)
    shifted = lattice + np.array([0.25, 0, 0], dtype=f32)
    for method in ("brute", "grid"):
        m = geometry.cloud_metrics(_t(lattice), _t(shifted), 0.25, method=method)
        assert m == {"chamfer": 0.125, "accuracy": 0.25, "completeness": 0.25, "precision": 1.0, "recall": 1.0, "fscore": 1.0,
                     "n_pred": 105, "n_ref": 105}
        assert geometry.cloud_metrics(_t(lattice), _t(shifted), 0.2, method=method)["fscore"] == 0.0
        assert geometry.chamfer_distance(_t(lattice), _t(shifted), method=method) == 0.125
    x, y = cloud(700, 30), cloud(900, 31)
    x[::9] = np.nan
    want = GO.cloud_metrics(x, y, 0.4, max_distance=0.8)
    got = geometry.cloud_metrics(_t(x), _t(y), 0.4, max_distance=0.8)
    assert set(got) == set(want) and got["n_pred"] == want["n_pred"] == 700 - 78 and got["n_ref"] == 900
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-12), k
    xb, yb = np.stack([cloud(100, 32), cloud(100, 33)]), np.stack([cloud(80, 34), cloud(80, 35)])
    assert geometry.chamfer_distance(_t(xb), _t(yb)) == pytest.approx(0.5 * (GO.chamfer(xb[0], yb[0]) + GO.chamfer(xb[1], yb[1])), rel=1e-12)


# ---------------------------------------------------------------- scenes
@pytest.fixture(scope="module")
def model(golden):
    """the synthetic-weights model of test_gpu_pointview"""
    from sgam_neurips22_amd.config import default_params
    from sgam_neurips22_amd.generative_sensing_module.model import VQModel
    g = golden("vqgan_full_ge256.npz")
    m = VQModel(**default_params("google_earth"))
    sd = testing.synthetic_state_dict(m.state_dict(), seed=0)
    sd["quantize.embedding.weight"] = testing.codebook_from_stats(float(g["zmean"]), float(g["zstd"]), 4096, 256, int(g["cb_seed"]))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _scene(model, **kw):
    from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
    scene = InfiniteSceneGeneration(model, "google_earth", output_dim=(4, 1), seed_frame=synthetic_seed_frame("google_earth", 0), **kw)
    scene.scene_expansion()
    assert len(scene.frames) == 4
    return scene


def _twin_of_scene(scene, coords):
    z0, z1 = scene._Z_RANGE[scene.data]
    case = dict(depths=[scene.frames[c]["depth"].cpu().numpy() for c in coords], K=scene.K,
                Ts=[scene.transform_grid[c[0]][c[1]]["T"] for c in coords], z_near=z0, z_far=z1)
    return twin_unproject(case)


@pytest.mark.parametrize("branch", ["splat", "rgbd"])
def test_scene_cloud_and_metrics(model, branch):
    scene = _scene(model, **(dict(use_rgbd_integration=True, tsdf_memory_budget_bytes=1 << 30) if branch == "rgbd" else {}))
    assert scene.use_rgbd_integration == (branch == "rgbd")
    coords = [c for c, _ in sorted(scene.frames.items(), key=lambda kv: (kv[1]["index"], kv[0]))]
    cloud4 = scene.merged_point_cloud()
    assert set(cloud4) == {"points", "colors"} and cloud4["points"].shape == (4 * 256 * 256, 3) and cloud4["points"].is_cuda
    pts = cloud4["points"].cpu().numpy()
    assert np.array_equal(_bits(pts), _bits(_twin_of_scene(scene, coords)))
    assert np.array_equal(cloud4["colors"].cpu().numpy(), np.concatenate([scene.frames[c]["rgb_u8"].cpu().numpy().reshape(-1, 3) for c in coords]))
    valid = np.isfinite(pts).all(1)
    assert valid.mean() > 0.5
    two = scene.merged_point_cloud(frames=[coords[2], coords[0]])       # the store's order, whatever order is asked for
    assert np.array_equal(_bits(two["points"].cpu().numpy()), _bits(_twin_of_scene(scene, [coords[0], coords[2]])))
    with pytest.raises(ValueError, match="no stored frame"):
        scene.merged_point_cloud(frames=[(9, 9)])
    with pytest.raises(ValueError, match="no stored frame"):
        scene.geometry_metrics(cloud4["points"], 0.01, frames=[coords[0], (9, 9)])
    # against itself: as a tensor, as a scene, as ground-truth frames
    gt = {"depths": [scene.frames[c]["depth"] for c in coords], "Ts_w2c": np.stack([scene.transform_grid[c[0]][c[1]]["T"] for c in coords]),
          "K": scene.K}
    for reference in (cloud4["points"], scene, gt):
        m = scene.geometry_metrics(reference, 0.01)
        assert m["chamfer"] == 0.0 and m["accuracy"] == 0.0 and m["completeness"] == 0.0
        assert m["precision"] == m["recall"] == m["fscore"] == 1.0 and m["n_pred"] == m["n_ref"] == int(valid.sum())
    # against its own points shifted by s: no distance exceeds |s| (plus the fp32 rounding of p + s and of d2: 2^-22 of the
    # largest coordinate covers three half-ulp shifts and the 2^-20 relative error of d2 at these sizes)
    s = np.array([0.003, -0.002, 0.001], dtype=f32)
    norm = float(np.linalg.norm(s.astype(np.float64)))
    shifted = cloud4["points"] + _t(s)
    slack = 2.0 ** -22 * float(np.abs(pts[valid]).max()) + 2.0 ** -19 * norm
    fwd = geometry.nearest_neighbors(cloud4["points"], shifted)["d2"].cpu().numpy()
    assert np.isfinite(fwd[valid]).all() and np.isinf(fwd[~valid]).all()
    assert float(np.sqrt(fwd[valid].astype(np.float64)).max()) <= norm + slack
    m = scene.geometry_metrics(shifted, 2 * norm)
    assert 0 < m["accuracy"] <= norm + slack and 0 < m["completeness"] <= norm + slack and m["chamfer"] <= 2 * (norm + slack) ** 2
    assert m["precision"] == m["recall"] == 1.0
    part = scene.geometry_metrics(cloud4["points"], 0.01, frames=coords[:1])
    assert part["n_pred"] == int(valid[:256 * 256].sum()) and part["accuracy"] == 0.0 and part["precision"] == 1.0 and part["n_ref"] == int(valid.sum())
