"""GPU: the pose-graph kernels (csrc/pose_graph.hip through sgam_neurips22_amd/geometry.py) against the numpy twin
(tests/posegraph_oracle.py): the linearisation, the assembly and the cost fold bit for bit; the dense SPD solve within the
backward-error bound of Cholesky; the Levenberg-Marquardt loop against the twin's first attempt and, on the scenarios of
tests/test_posegraph_cpu.py, against the truth and scipy within the bounds asserted there of the twin; multiway_registration on
overlapping windows of the ICP tests' surface; and the scene-level callers on both warp branches."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import geometry, testing

sys.path.insert(0, os.path.dirname(__file__))
import icp_oracle as IO  # noqa: E402
import posegraph_oracle as PO  # noqa: E402
from test_icp_cpu import EXACT_R, EXACT_T  # noqa: E402
from test_posegraph_cpu import (MU, N_RING, SCIPY_COST_REL, SCIPY_POSE_BOUND, TRUTH_BOUND, consistent, false_closure, noisy,  # noqa: E402
                                scipy_optimum)

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -53


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64).view(np.uint64)


def _graph(n_nodes, arrays):
    src, dst, T, info, unc = arrays
    return geometry.PoseGraph.from_tensors(n_nodes, _t(np.asarray(src, dtype=np.int64)), _t(np.asarray(dst, dtype=np.int64)), _t(T), _t(info),
                                           _t(np.asarray(unc, dtype=bool)))


# ---------------------------------------------------------------- linearisation and assembly
def _random_graph(n_nodes, n_edges, seed):
    """random poses, edges between random different nodes (duplicates as they fall), random measurements (not consistent: every
    residual is large), random SPD information, a third of the edges uncertain"""
    rng = np.random.default_rng(seed)
    poses = np.array([PO.random_pose(rng, rng.uniform(0.0, 2.5), rng.uniform(0.0, 3.0)) for _ in range(n_nodes)])
    src = rng.integers(0, n_nodes, n_edges)
    dst = (src + rng.integers(1, n_nodes, n_edges)) % n_nodes
    if n_edges >= 4:
        src[1], dst[1] = dst[0], src[0]                               # the first pair again, the other way round
        src[3], dst[3] = src[2], dst[2]                               # and a plain duplicate
    T = np.array([PO.random_pose(rng, rng.uniform(0.0, 2.5), rng.uniform(0.0, 3.0)) for _ in range(n_edges)])
    G = rng.normal(size=(n_edges, 6, 9))
    info = G @ G.transpose(0, 2, 1) * rng.uniform(0.5, 200.0, (n_edges, 1, 1))
    info = (info + info.transpose(0, 2, 1)) * 0.5
    unc = rng.uniform(size=n_edges) < 1 / 3
    if n_edges >= 4:
        unc[0], unc[2] = True, False
    return poses, (src, dst, T, info, unc)


@pytest.mark.parametrize("n_nodes,n_edges,fixed", [(2, 1, 0), (2, 63, 1), (3, 65, 2), (3, 257, 1), (11, 1, 4), (11, 63, 0), (11, 257, 10),
                                                   (22, 65, 5), (22, 257, 0), (43, 63, 3), (43, 257, 42)])
def test_linearisation_and_assembly_equal_the_twin(n_nodes, n_edges, fixed):
    poses, arrays = _random_graph(n_nodes, n_edges, 1000 * n_nodes + n_edges)
    src, dst, T, info, unc = arrays
    want = PO.linearize(poses, src, dst, T, info, unc, MU)
    H, b = PO.assemble(want["K"], want["g"], src, dst, n_nodes, fixed)
    free = np.arange(6 * n_nodes) // 6 != fixed
    want.update(H=H, b=b, F=np.array([PO.fold(want["cost"])]), **{"lambda": np.array([PO.TAU * max(0.0, np.diag(H)[free].max())])})
    if n_edges == 257 and n_nodes == 3:
        assert np.bincount(np.concatenate([src, dst])).min() >= 65      # every node has at least 65 incident edges
    got = geometry.pose_graph_linearize(_graph(n_nodes, arrays), _t(poses), MU, fixed=fixed)
    assert set(got) == set(want)
    for key in ("r", "J", "q", "l", "cost", "K", "g", "b", "H", "F", "lambda"):
        g = got[key].cpu().numpy()
        assert g.shape == want[key].shape, key
        diff = np.abs(g - want[key]).max()
        assert np.array_equal(_bits(g), _bits(want[key])), (key, diff)
    if n_edges > 1:
        assert unc.any() and (want["l"][unc] < 1.0).all() and (want["l"][~unc] == 1.0).all()
    F6 = slice(6 * fixed, 6 * fixed + 6)
    Hg = got["H"].cpu().numpy()
    assert np.array_equal(Hg[F6, F6], np.eye(6)) and (np.delete(Hg[F6], np.arange(6 * fixed, 6 * fixed + 6), axis=1) == 0).all()
    again = geometry.pose_graph_linearize(_graph(n_nodes, arrays), _t(poses), MU, fixed=fixed)
    assert all(np.array_equal(_bits(again[k]), _bits(got[k])) for k in got)


# ---------------------------------------------------------------- the solve
def _spd(n, seed, cond=1e4):
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.normal(size=(n, n)))[0]
    A = (Q * np.logspace(0.0, np.log10(cond), n)) @ Q.T if n > 1 else np.array([[3.7]])
    return (A + A.T) * 0.5, rng.normal(size=n)


def _solve_bound(n, A):
    """Higham's backward-error bound for a Cholesky solve with || |L| |L^T| || <= n ||A||, whatever the summation order, relative to
    ||A||_2 ||x||_2"""
    return (3 * n + 1) * n * U


def _check_solution(A, lam, b, x, what):
    n = len(b)
    Ad = A + lam * np.eye(n)
    norm = np.linalg.norm(Ad, 2)
    res = np.linalg.norm((Ad.astype(np.longdouble) @ x.astype(np.longdouble) - b.astype(np.longdouble)).astype(np.float64))
    bound = _solve_bound(n, Ad)
    ref = np.linalg.solve(Ad, b)
    cond = np.linalg.cond(Ad)
    fwd = np.linalg.norm(x - ref)
    print(what, "n", n, "residual / bound", res / (bound * norm * np.linalg.norm(x)), "forward / bound", fwd / (cond * bound * np.linalg.norm(x)),
          "cond", cond)
    assert res <= bound * norm * np.linalg.norm(x)
    assert fwd <= cond * bound * np.linalg.norm(x)


@pytest.mark.parametrize("n", [1, 6, 63, 64, 65, 127, 129, 258])
def test_spd_solve_meets_the_cholesky_bound(n):
    A, b = _spd(n, 40 + n)
    for lam in (None, 0.37):
        x, status = geometry.spd_solve(_t(A), _t(b), damping=lam)
        assert x.shape == (n,) and x.dtype == torch.float64 and float(status.item()) == 0.0
        _check_solution(A, lam or 0.0, b, x.cpu().numpy(), "random SPD")
    x2, _ = geometry.spd_solve(_t(A), _t(b), damping=torch.full((1,), 0.37, dtype=torch.float64, device=DEV))
    assert np.array_equal(_bits(x2), _bits(x))                            # a device damping, and equal run to run
    # only the lower triangle is read
    upper = A + np.triu(np.full((n, n), 7.0), 1)
    x3, _ = geometry.spd_solve(_t(upper), _t(b), damping=0.37)
    assert np.array_equal(_bits(x3), _bits(x))


def test_spd_solve_on_a_graph_matrix_and_with_a_leading_dimension():
    poses, arrays = _random_graph(43, 257, 77)
    lin = geometry.pose_graph_linearize(_graph(43, arrays), _t(poses), MU, fixed=3)
    H, b, lam = lin["H"], lin["b"], lin["lambda"]
    x, status = geometry.spd_solve(H, b, damping=lam)
    assert float(status.item()) == 0.0
    Hn = np.tril(H.cpu().numpy())
    Hn = Hn + np.tril(Hn, -1).T
    _check_solution(Hn, float(lam.item()), b.cpu().numpy(), x.cpu().numpy(), "graph H + lambda I")
    assert (x.cpu().numpy()[18:24] == 0).all()                            # the fixed node's step
    # ld > n: the matrix inside a wider buffer, whose other entries are never read (NaN) nor written
    n = 65
    A, rhs = _spd(n, 5)
    buf = torch.full((70, 80), float("nan"), dtype=torch.float64, device=DEV)
    buf[:n, :n] = _t(A)
    view = buf[:n, :n]
    assert view.stride(0) == 80
    x, status = geometry.spd_solve(view, _t(rhs))
    assert float(status.item()) == 0.0
    _check_solution(A, 0.0, rhs, x.cpu().numpy(), "ld 80")
    assert torch.isnan(buf[:, n:]).all() and torch.isnan(buf[n:]).all() and torch.equal(buf[:n, :n], _t(A))


def test_spd_solve_raises_the_flag_and_stops():
    good, rhs = _spd(64, 9)
    cases = {}
    v = np.random.default_rng(1).normal(size=65)
    cases["rank one"] = np.outer(v, v)
    late = np.zeros((66, 66))
    late[:64, :64], late[64:, 64:] = good, 1.0                           # the second panel's 2 x 2 block is singular
    cases["singular in the second panel"] = late
    nan = _spd(129, 3)[0]
    nan[70, 70] = np.nan
    cases["NaN"] = nan
    neg = _spd(6, 2)[0]
    neg[2, 2] = -1.0
    cases["negative pivot"] = neg
    for name, A in cases.items():
        n = len(A)
        x, status = geometry.spd_solve(_t(A), _t(np.ones(n)))
        assert float(status.item()) == 2.0, name
        assert (x == 0).all(), name                                      # nothing was written past the flag
    # a status that is already set: nothing runs
    status = torch.full((1,), 1.0, dtype=torch.float64, device=DEV)
    x, status = geometry.spd_solve(_t(good), _t(rhs), status=status)
    assert float(status.item()) == 1.0 and (x == 0).all()


# ---------------------------------------------------------------- the loop
def _optimize(n_nodes, arrays, **kw):
    kw.setdefault("line_process_weight", MU)
    return geometry.optimize_pose_graph(_graph(n_nodes, arrays), **kw)


def test_first_attempt_follows_the_twin():
    truth, arrays, init = false_closure()
    src, dst, T, info, unc = arrays
    twin = PO.run(init, src, dst, T, info, unc, MU, max_iterations=1)
    got = _optimize(N_RING, arrays, poses=init, max_iterations=1, reoptimize=False)
    # the step solves (H + lambda I) delta = b, H and b equal in bits: the two steps differ by at most cond * the solve bound *
    # |delta|, and a pose entry moves by at most |d omega| (|R| <= 1) + |d v| + |d omega| |t|
    lin = PO.linearize(init, src, dst, T, info, unc, MU)
    H, b = PO.assemble(lin["K"], lin["g"], src, dst, N_RING, 0)
    lam = PO.TAU * np.diag(H)[6:].max()
    Hd = H + lam * np.eye(len(b))
    delta = np.linalg.solve(Hd, b)
    tol = 2.0 * np.linalg.cond(Hd) * _solve_bound(len(b), Hd) * np.linalg.norm(delta) * (2.0 + np.abs(init[:, :3, 3]).max())
    diff = np.abs(got["poses"].cpu().numpy() - twin["poses"]).max()
    print("first attempt: largest pose entry off the twin", diff, "bound", tol, "|delta|", np.linalg.norm(delta))
    assert twin["history"][0, 4] == 1.0 and np.abs(twin["poses"] - init).max() > 0.05
    assert diff <= tol and tol <= 1e-4                                   # (three orders below the step itself)
    h = got["history"]
    assert h.shape == (1, 8) and h[0, 4] == 1.0 and h[0, 6] == 0.0 and got["status"] == 0 and got["iterations"] == 1 and not got["converged"]
    assert np.allclose(h[0, [0, 1, 2, 5]], twin["history"][0, [0, 1, 2, 5]], rtol=1e-6, atol=0) and h[0, 3] == twin["history"][0, 3]
    assert np.array_equal(got["poses"].cpu().numpy()[0], np.eye(4))
    lw = got["line_weights"].cpu().numpy()
    assert np.allclose(lw, twin["l"], rtol=1e-6, atol=1e-12) and (lw[~unc] == 1.0).all()


def test_consistent_ring_reaches_the_truth_and_freezes():
    truth, arrays, init = consistent()
    outs = [_optimize(N_RING, arrays, poses=p, max_iterations=30) for p in (init, _t(init))]
    out = outs[0]
    err = float(np.abs(out["poses"].cpu().numpy() - truth).max())
    h = out["history"]
    stop = int(np.flatnonzero(h[:, 6] == 1)[0])
    print("consistent ring: iterations", out["iterations"], "stopped at attempt", stop, "cost", out["cost"], "largest pose entry off", err)
    assert out["status"] == 1 and out["converged"] and err <= TRUTH_BOUND and out["history_second"] is None
    assert bool(out["kept"].all()) and bool((out["line_weights"] > 0.9).all())
    assert stop < 20 and h.shape == (30, 8) and (h[:stop, 6] == 0).all()
    assert np.array_equal(_bits(h[stop + 1:]), _bits(np.tile(h[stop + 1], (30 - stop - 1, 1)))) and h[-1, 6] == 1
    assert np.array_equal(h[stop + 1], [out["cost"], h[stop, 1], 0, 0, 0, 0, 1, h[stop, 7]])
    assert np.array_equal(out["poses"].cpu().numpy()[0], np.eye(4))
    # the whole optimisation twice: equal in every bit
    for key in ("poses", "line_weights", "history"):
        assert np.array_equal(_bits(outs[1][key]), _bits(out[key])), key
    assert (outs[1]["status"], outs[1]["iterations"], outs[1]["cost"]) == (out["status"], out["iterations"], out["cost"])


def test_noisy_ring_agrees_with_scipy():
    truth, arrays = noisy()
    out = _optimize(N_RING, arrays)
    want, want_cost = scipy_optimum()
    err = float(np.abs(out["poses"].cpu().numpy() - want).max())
    print("noisy ring: iterations", out["iterations"], "cost", out["cost"], "scipy", want_cost, "largest pose entry off", err)
    assert out["status"] == 1 and err <= SCIPY_POSE_BOUND and abs(out["cost"] - want_cost) <= SCIPY_COST_REL * want_cost


def test_false_loop_closure_is_pruned():
    truth, arrays, init = false_closure()
    unc = arrays[4]
    out = _optimize(N_RING, arrays, poses=init)
    l = out["line_weights"].cpu().numpy()
    err = float(np.abs(out["poses"].cpu().numpy() - truth).max())
    print("false closure: l of the false edge", l[-1], "least l of the true closures", l[:-1][unc[:-1]].min(), "largest pose entry off", err,
          "iterations", out["iterations"])
    assert out["status"] == 1 and l[-1] < 0.25 and (l[:-1] > 0.9).all()
    assert np.array_equal(out["kept"].cpu().numpy(), np.arange(len(l)) < len(l) - 1)
    assert err <= TRUTH_BOUND and out["history_second"] is not None and out["history_second"][-1, 6] == 1
    # the default mu from the graph: preference * distance^2 * mean Lambda[5][5] over the uncertain edges = 0.1 * 0.05 * 1000 = MU
    # (to the rounding of the square root)
    again = geometry.optimize_pose_graph(_graph(N_RING, arrays), max_correspondence_distance=0.05 ** 0.5, preference_loop_closure=0.1, poses=init)
    assert np.array_equal(_bits(again["poses"]), _bits(out["poses"])) or np.abs((again["poses"] - out["poses"]).cpu().numpy()).max() <= 1e-9
    with pytest.raises(ValueError, match="line_process_weight"):
        geometry.optimize_pose_graph(_graph(N_RING, arrays))


def test_edge_cases_on_the_device():
    g = geometry.PoseGraph(3, DEV)
    out = geometry.optimize_pose_graph(g)
    assert out["status"] == 1 and out["converged"] and out["iterations"] == 0 and torch.equal(out["poses"], torch.eye(4, dtype=torch.float64, device=DEV).repeat(3, 1, 1))
    # add_edge, a node without edges (it stays put) and a fixed node other than 0
    truth, (src, dst, T, info, unc), init = consistent()
    extra = PO.random_pose(np.random.default_rng(3), 0.4, 1.0)
    g = geometry.PoseGraph(N_RING + 1, DEV)
    for e in range(len(src)):
        g.add_edge(int(src[e]), int(dst[e]), T[e] if e % 2 else _t(T[e]), info[e] if e % 3 else _t(info[e]), uncertain=bool(unc[e]))
    assert len(g) == len(src)
    rel = np.linalg.inv(truth[5])
    start = np.concatenate([rel @ init, extra[None]])
    start[5] = np.eye(4)
    out = geometry.optimize_pose_graph(g, line_process_weight=MU, poses=start, fixed=5)
    P = out["poses"].cpu().numpy()
    assert out["status"] == 1 and np.array_equal(P[-1], extra) and np.array_equal(P[5], np.eye(4))
    assert np.abs(P[:-1] - rel @ truth).max() <= TRUTH_BOUND


# ---------------------------------------------------------------- multiway registration
WINDOW_DISTANCE = 0.15


@functools.lru_cache(maxsize=None)
def _windows():
    return PO.windows()


def test_multiway_registration_undoes_known_motions():
    clouds, normals, motions = _windows()
    assert all(1900 <= len(c) <= 2100 for c in clouds) and len(clouds) == 5
    # the registration of the pair (0, 3), which shares one strip (fitness 0.25: no candidate), replaced by a wrong pose
    C = np.eye(4)
    C[:3, 3] = [2.0, 2.0, 0.5]
    wrong = C @ IO.rigid(20.0, [0.3, -1.0, 0.5], [0.5, 0.0, 0.0]) @ np.linalg.inv(C) @ motions[3] @ np.linalg.inv(motions[0])
    out = geometry.multiway_registration([_t(c) for c in clouds], WINDOW_DISTANCE, normals=[_t(n) for n in normals],
                                         registrations={(0, 3): wrong})
    assert out["edges"] == [(0, 1, False), (0, 2, True), (0, 3, True), (1, 2, False), (1, 3, True), (2, 3, False), (2, 4, True), (3, 4, False)]
    assert out["missing_odometry"] == [] and out["registrations"][2] is None and out["registrations"][0]["converged"]
    l, kept = out["line_weights"].cpu().numpy(), out["kept"].cpu().numpy()
    print("multiway: status", out["status"], "iterations", out["iterations"], "cost", out["cost"], "line weights", l)
    assert out["status"] == 1 and l[2] < 0.25 and (np.delete(l, 2) > 0.9).all() and np.array_equal(kept, np.arange(8) != 2)
    P = out["poses"].cpu().numpy()
    assert np.array_equal(P[0], np.eye(4))
    for i in range(1, 5):
        # window i hangs on window 0 by a chain of at most i registrations, each within the exact-copy bounds
        eR, et, _ = IO.pose_error(P[i], np.linalg.inv(motions[i]))
        print("window", i, "R error", eR, "t error", et)
        assert eR <= i * EXACT_R and et <= i * EXACT_T
    # Lambda of an edge: the point-to-point sums at the registered pose, slot (5,5) the number of correspondences
    src, dst, T, info, unc = out["graph"].tensors()
    want = PO.information(clouds[0], clouds[1], WINDOW_DISTANCE, T[0].cpu().numpy())
    got = info[0].cpu().numpy()
    assert got[5, 5] == want[5, 5] and np.array_equal(got, got.T) and np.allclose(got, want, rtol=1e-12, atol=1e-9)
    assert np.array_equal(got, geometry.registration_information(_t(clouds[0]), _t(clouds[1]), WINDOW_DISTANCE, T[0]).cpu().numpy())
    # without the wrong pair nothing is pruned; point_to_point needs no normals
    plain = geometry.multiway_registration([_t(c) for c in clouds[:3]], WINDOW_DISTANCE, estimation="point_to_point", max_icp_iterations=60)
    assert plain["edges"] == [(0, 1, False), (0, 2, True), (1, 2, False)] and bool(plain["kept"].all()) and plain["history_second"] is None
    for i in range(1, 3):
        eR, et, _ = IO.pose_error(plain["poses"].cpu().numpy()[i], np.linalg.inv(motions[i]))
        assert eR <= i * EXACT_R and et <= i * EXACT_T


# ---------------------------------------------------------------- scenes
@pytest.fixture(scope="module")
def model(golden):
    """the synthetic-weights model of test_gpu_cloud"""
    from sgam_neurips22_amd.config import default_params
    from sgam_neurips22_amd.generative_sensing_module.model import VQModel
    g = golden("vqgan_full_ge256.npz")
    m = VQModel(**default_params("google_earth"))
    sd = testing.synthetic_state_dict(m.state_dict(), seed=0)
    sd["quantize.embedding.weight"] = testing.codebook_from_stats(float(g["zmean"]), float(g["zstd"]), 4096, 256, int(g["cb_seed"]))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


SCENE_DISTANCE = 0.1


@pytest.mark.parametrize("branch", ["splat", "rgbd"])
def test_scene_pose_optimisation(model, branch):
    from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
    kw = dict(use_rgbd_integration=True, tsdf_memory_budget_bytes=1 << 30) if branch == "rgbd" else {}
    scene = InfiniteSceneGeneration(model, "google_earth", output_dim=(3, 1), seed_frame=synthetic_seed_frame("google_earth", 0), **kw)
    scene.scene_expansion()
    assert len(scene.frames) == 3
    coords = [c for c, _ in sorted(scene.frames.items(), key=lambda kv: (kv[1]["index"], kv[0]))]
    grid_before = copy.deepcopy(scene.transform_grid)
    # pose_corrections=None: today's cloud and today's metrics, in every bit
    z0, z1 = scene._Z_RANGE[scene.data]
    today = geometry.unproject_frames([scene.frames[c]["depth"] for c in coords], [scene.frames[c]["rgb_u8"] for c in coords], scene.K,
                                      [scene.transform_grid[c[0]][c[1]]["T"] for c in coords], z0, z1)
    for cloud in (scene.merged_point_cloud(), scene.merged_point_cloud(pose_corrections=None)):
        assert torch.equal(cloud["points"].view(torch.int32), today["points"].view(torch.int32)) and torch.equal(cloud["colors"], today["colors"])
    pts = today["points"].cpu().numpy()
    valid = np.isfinite(pts).all(1)
    centre = pts[valid].astype(np.float64).mean(0)
    C = np.eye(4)
    C[:3, 3] = centre
    ref = geometry.transform_points(today["points"], C @ IO.rigid(2.0, [0.2, 1.0, -0.4], [0.012, -0.01, 0.012]) @ np.linalg.inv(C))
    plain = geometry.cloud_metrics(today["points"], ref, 0.01)
    assert scene.geometry_metrics(ref, 0.01) == plain and scene.geometry_metrics(ref, 0.01, pose_corrections=None) == plain
    # the hand-moved last frame of test_scene_alignment_and_frame_drift, the other way round: the copy's last frame gets the
    # geometry of frame 1 — depth, colour and pose — and its camera a 1 degree / 0.02 motion D of the world, T_last = T_first D:
    # its cloud is D^-1 times frame 1's cloud, an exact copy, and the correction that puts it back is D
    first, last = coords[1], coords[2]
    D = C @ IO.rigid(1.0, [1.0, 0.3, 0.2], [0.01, 0.015, -0.008]) @ np.linalg.inv(C)
    moved_scene = copy.copy(scene)
    moved_scene.frames = dict(scene.frames)
    moved_scene.frames[last] = dict(scene.frames[last], depth=scene.frames[first]["depth"], rgb_u8=scene.frames[first]["rgb_u8"])
    moved_scene.transform_grid = copy.deepcopy(scene.transform_grid)
    T_first = np.asarray(scene.transform_grid[first[0]][first[1]]["T"], dtype=np.float64)
    moved_scene.transform_grid[last[0]][last[1]]["T"] = T_first @ D
    out = moved_scene.optimize_poses(SCENE_DISTANCE, frames=[first, last])
    assert set(out) == {"coords", "corrections", "Ts_w2c", "edges", "line_weights", "kept", "missing_odometry", "converged", "status",
                        "iterations", "cost"}
    assert out["coords"] == [first, last] and out["edges"] == [(0, 1, False)] and out["missing_odometry"] == [] and out["status"] == 1
    corr = out["corrections"]
    assert corr.is_cuda and corr.dtype == torch.float64 and corr.shape == (2, 4, 4)
    corr = corr.cpu().numpy()
    eR, et, _ = IO.pose_error(corr[1], D)
    print(branch, "correction of the moved frame: R error", eR, "t error", et, "iterations", out["iterations"], "cost", out["cost"])
    assert np.array_equal(corr[0], np.eye(4)) and eR <= EXACT_R and et <= EXACT_T
    assert np.allclose(out["Ts_w2c"][1], T_first @ D @ np.linalg.inv(corr[1]), rtol=0, atol=1e-12) and np.array_equal(out["Ts_w2c"][0], T_first)
    # the corrected frame lies on frame 1's points.  A rotation off by eR (Frobenius) about the world's origin moves a point at
    # radius r by at most eR r, the translation adds et; both clouds are fp32 unprojections, each coordinate a sum of four fp32
    # terms of size up to the scene's scale: 16 roundings of 2^-24 of it cover the two
    want = scene.merged_point_cloud(frames=[first])["points"].cpu().numpy()
    scale = float(max(np.abs(want[np.isfinite(want).all(1)]).max(), np.abs(np.linalg.inv(T_first)[:3, 3]).max()))
    bound = EXACT_R * scale * np.sqrt(3.0) + EXACT_T + 16 * 2.0 ** -24 * scale
    for fix in (out, {last: corr[1]}, {last: torch.from_numpy(corr[1]).to(DEV)}):
        got = moved_scene.merged_point_cloud(frames=[last], pose_corrections=fix)["points"].cpu().numpy()
        ok = np.isfinite(want).all(1)
        assert np.array_equal(np.isfinite(got).all(1), ok)
        print(branch, "corrected frame against frame 1: largest coordinate off", np.abs(got[ok] - want[ok]).max(), "bound", bound)
        assert np.abs(got[ok] - want[ok]).max() <= bound
    raw = moved_scene.merged_point_cloud(frames=[last])["points"].cpu().numpy()
    assert np.abs(raw[ok] - want[ok]).max() > 10 * bound                  # (uncorrected, the frame is visibly off)
    # the metrics of the moved scene against its own first two frames: with the corrections the copy lies on frame 1
    target = scene.merged_point_cloud(frames=[coords[0], first])["points"]
    off = moved_scene.geometry_metrics(target, 0.01, frames=[last])
    on = moved_scene.geometry_metrics(target, 0.01, frames=[last], pose_corrections=out)
    print(branch, "accuracy of the moved frame", off["accuracy"], "corrected", on["accuracy"])
    assert on["accuracy"] <= np.sqrt(3.0) * bound and on["accuracy"] < off["accuracy"] and on["precision"] == 1.0
    with pytest.raises(ValueError, match="pose_corrections"):
        moved_scene.merged_point_cloud(pose_corrections=[corr[1]])
    with pytest.raises(ValueError, match="pose_corrections"):
        moved_scene.geometry_metrics(target, 0.01, source="mesh", pose_corrections=out)
    # all three frames: a graph with a loop closure candidate, whatever the generated frames' fit; the original store is untouched
    whole = scene.optimize_poses(SCENE_DISTANCE, max_icp_iterations=10, max_iterations=20)
    assert whole["coords"] == coords and whole["corrections"].shape == (3, 4, 4) and whole["status"] in (0, 1, 2)
    assert torch.equal(whole["corrections"][0], torch.eye(4, dtype=torch.float64, device=DEV))
    assert all(np.array_equal(np.asarray(scene.transform_grid[c[0]][c[1]]["T"]), np.asarray(grid_before[c[0]][c[1]]["T"])) for c in coords)
    again = scene.merged_point_cloud()
    assert torch.equal(again["points"].view(torch.int32), today["points"].view(torch.int32))
