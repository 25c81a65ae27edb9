"""CPU: the numpy twin of the pose-graph optimiser (tests/posegraph_oracle.py) against outside references — a central finite
difference of the model, scipy.optimize.least_squares on the same cost, the truth of synthetic rings — before the same conditions
are asked of the kernels (tests/test_gpu_posegraph.py); the argument checks of the C entry points and of the Python front."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

from sgam_neurips22_amd import _lib, geometry

sys.path.insert(0, os.path.dirname(__file__))
import posegraph_oracle as PO  # noqa: E402

MU = 5.0
N_RING = 12
# The truth bound of the consistent scenarios.  The optimiser stops at max |b| < 1e-6 (or a cost that no longer moves); the pose
# error left is about H^-1 b.  The ring's information is >= 500 per edge and the softest mode of a 12-node ring of such springs
# has the stiffness 500 (2 sin(pi / 24))^2 = 34, so an error of 1e-6 * sqrt(66) / 34 = 2.4e-7 in the twist, and no more in a pose
# entry (rotations: entries move by at most the angle; translations: by the twist's v plus omega x t with |t| <= 3): 1e-6.
TRUTH_BOUND = 1e-6
# the noisy ring against scipy: 10x what the twin reached (8.4e-10 in the largest pose entry, the costs 3.160235882097455 and
# 3.160235882097444; the prototype of the rules reached 1.5e-9)
SCIPY_POSE_BOUND = 8.4e-9
SCIPY_COST_REL = 1e-12


def consistent():
    """(truth, graph arrays, initial guess 0.15 rad / 0.3 off)"""
    truth, src, dst, T, info, unc = PO.ring(N_RING, 0, stride=3)
    return truth, (src, dst, T, info, unc), PO.perturbed(truth, 1, 0.15, 0.3)


def false_closure():
    """the consistent ring plus one false uncertain edge (2 -> 8): the true measurement times a random pose 0.3 - 1.0 rad off"""
    truth, (src, dst, T, info, unc), init = consistent()
    rng = np.random.default_rng(5)
    wrong = PO.random_pose(rng, rng.uniform(0.3, 1.0), rng.uniform(0.3, 1.0)) @ np.linalg.inv(truth[8]) @ truth[2]
    return truth, (np.append(src, 2), np.append(dst, 8), np.concatenate([T, wrong[None]]),
                   np.concatenate([info, PO.INFORMATION[None]]), np.append(unc, True)), init


def noisy():
    """the ring with every measurement perturbed (0.01 rad / 0.01), all edges certain: a least-squares problem scipy can solve"""
    truth, src, dst, T, info, unc = PO.ring(N_RING, 0, stride=3, noise=0.01, certain_closures=True)
    return truth, (src, dst, T, info, unc)


@functools.lru_cache(maxsize=None)
def scipy_optimum():
    """(poses (N,4,4), cost F) of the noisy ring by scipy.optimize.least_squares: P_i = exp(x_i) truth_i, node 0 fixed, the
    residuals L_e^T r_e with Lambda_e = L_e L_e^T and numpy's own inverses"""
    from scipy.optimize import least_squares
    truth, (src, dst, T, info, _) = noisy()
    chol = [np.linalg.cholesky(L) for L in info]

    def poses_of(x):
        P = truth.copy()
        for i in range(1, N_RING):
            P[i] = PO.se3_exp(x[6 * (i - 1):6 * i]) @ truth[i]
        return P

    def fun(x):
        P = poses_of(x)
        return np.concatenate([chol[e].T @ PO.residual_numeric(P, src[e], dst[e], T[e]) for e in range(len(src))])

    sol = least_squares(fun, np.zeros(6 * (N_RING - 1)), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=1.0)
    return poses_of(sol.x), 2.0 * sol.cost


def optimize(arrays, **kw):
    src, dst, T, info, unc = arrays
    return PO.optimize(kw.pop("n_nodes", N_RING), src, dst, T, info, unc, kw.pop("mu", MU), **kw)


# ---------------------------------------------------------------- the model
def test_jacobian_matches_a_central_finite_difference():
    truth, (src, dst, T, info, unc), init = false_closure()
    lin = PO.linearize(init, src, dst, T, info, unc, MU)
    h, worst = 1e-6, 0.0
    for e in range(len(src)):
        s, t = src[e], dst[e]
        assert np.abs(lin["r"][e] - PO.residual_numeric(init, s, t, T[e])).max() <= 1e-14
        for node, sign in ((s, 1.0), (t, -1.0)):
            for k in range(6):
                x = np.zeros(6)
                x[k] = h
                Pp, Pm = init.copy(), init.copy()
                Pp[node], Pm[node] = PO.se3_exp(x) @ init[node], PO.se3_exp(-x) @ init[node]
                fd = (PO.residual_numeric(Pp, s, t, T[e]) - PO.residual_numeric(Pm, s, t, T[e])) / (2 * h)
                worst = max(worst, float(np.abs(fd - sign * lin["J"][e][:, k]).max()))
    print("largest |J - finite difference|", worst)
    assert worst <= 1e-6
    # q, l, the cost and the normal equations against plain matrix products
    J, r = lin["J"], lin["r"]
    q = np.einsum("ea,eab,eb->e", r, info, r)
    l = np.where(unc, (MU / (MU + q)) ** 2, 1.0)
    assert np.allclose(lin["q"], q, rtol=1e-13, atol=0) and np.allclose(lin["l"], l, rtol=1e-13, atol=0) and (lin["l"][~unc] == 1.0).all()
    assert np.allclose(lin["cost"], l * q + np.where(unc, MU * (np.sqrt(l) - 1) ** 2, 0.0), rtol=1e-12, atol=0)
    assert np.allclose(lin["K"], np.einsum("eaj,e,eab,ebk->ejk", J, l, info, J), rtol=1e-12, atol=1e-9)
    assert np.allclose(lin["g"], np.einsum("eaj,e,eab,eb->ej", J, l, info, r), rtol=1e-12, atol=1e-9)
    H, b = PO.assemble(lin["K"], lin["g"], src, dst, N_RING, 0)
    Jbig = np.zeros((len(src), 6, 6 * N_RING))
    for e in range(len(src)):
        Jbig[e][:, 6 * src[e]:6 * src[e] + 6], Jbig[e][:, 6 * dst[e]:6 * dst[e] + 6] = J[e], -J[e]
    Hd = np.einsum("eai,e,eab,ebj->ij", Jbig, l, info, Jbig)
    bd = -np.einsum("eai,e,eab,eb->i", Jbig, l, info, r)
    Hd[:6], Hd[:, :6], bd[:6] = 0.0, 0.0, 0.0
    Hd[:6, :6] = np.eye(6)
    assert np.allclose(H, Hd, rtol=1e-12, atol=1e-8) and np.allclose(b, bd, rtol=1e-12, atol=1e-8)
    assert np.array_equal(np.tril(H, -1), np.triu(H, 1).T) or np.abs(H - H.T).max() <= 1e-9       # off-diagonal blocks mirror exactly
    assert PO.fold(lin["cost"]) == pytest.approx(lin["cost"].sum(), rel=1e-14)


def test_noisy_ring_agrees_with_scipy_least_squares():
    truth, arrays = noisy()
    out = optimize(arrays)
    want, want_cost = scipy_optimum()
    err = float(np.abs(out["poses"] - want).max())
    print("noisy ring: status", out["status"], "iterations", out["iterations"], "cost", out["cost"], "scipy", want_cost, "largest pose entry off", err)
    assert out["status"] == 1 and out["converged"] and out["kept"].all() and out["history_second"] is None
    assert err <= SCIPY_POSE_BOUND and abs(out["cost"] - want_cost) <= SCIPY_COST_REL * want_cost and out["cost"] > 0.1


def test_a_trial_at_the_rounding_level_ends_the_run():
    """At the optimum the trial's cost differs from F by rounding only, and rounding decides the sign of rho.  With the gradient test
    out of reach (tolerance 0) and a solve that is exact to 1e-13 only, as a device solve is, the run must end converged whichever
    way the sign falls: accepted, F - F' <= relative_cost F, or rejected with |F - F'| <= relative_cost F — never by rejecting
    until lambda overflows."""
    truth, (src, dst, T, info, unc) = noisy()
    want, want_cost = scipy_optimum()
    ends = set()
    for seed in range(4):
        rng = np.random.default_rng(seed)

        def solve(H, lam, b):
            x = PO.cholesky_solve(H, lam, b)
            return None if x is None else x * (1.0 + 1e-13 * rng.normal(size=len(x)))

        out = PO.run(np.tile(np.eye(4), (N_RING, 1, 1)), src, dst, T, info, unc, MU, gradient_tolerance=0.0, solve=solve)
        h = out["history"]
        stop = int(np.flatnonzero(h[:, 6] != 0)[0])
        ends.add(h[stop, 4])
        assert out["state"][PO.S_STATUS] == 1 and stop < 20 and abs(h[stop, 0] - h[stop, 5]) <= 1e-12 * h[stop, 0]
        assert np.abs(out["poses"] - want).max() <= SCIPY_POSE_BOUND and abs(out["state"][PO.S_COST] - want_cost) <= SCIPY_COST_REL * want_cost
    assert ends == {0.0, 1.0}                                             # both ways occurred


def test_consistent_ring_reaches_the_truth():
    truth, arrays, init = consistent()
    out = optimize(arrays, poses=init)
    err = float(np.abs(out["poses"] - truth).max())
    print("consistent ring: iterations", out["iterations"], "cost", out["cost"], "largest pose entry off", err)
    assert np.abs(init - truth).max() > 0.05
    assert out["status"] == 1 and err <= TRUTH_BOUND and out["kept"].all() and (out["line_weights"] > 0.9).all()
    h = out["history"]
    stop = int(np.flatnonzero(h[:, 6] == 1)[0])
    assert stop < 20 and (h[stop + 1:] == h[stop + 1]).all() and h[-1, 6] == 1                     # the frozen rows repeat
    assert np.array_equal(out["poses"][0], np.eye(4))                                            # the fixed node never moves


def test_false_loop_closure_is_switched_off_and_pruned():
    truth, arrays, init = false_closure()
    unc = arrays[4]
    for reoptimize in (True, False):
        out = optimize(arrays, poses=init, reoptimize=reoptimize)
        l = out["line_weights"]
        err = float(np.abs(out["poses"] - truth).max())
        print("false closure: reoptimize", reoptimize, "l of the false edge", l[-1], "least l of the true closures", l[:-1][unc[:-1]].min(),
              "largest pose entry off", err)
        assert out["status"] == 1 and l[-1] < 0.25 and (l[:-1] > 0.9).all() and np.array_equal(out["kept"], np.arange(len(l)) < len(l) - 1)
        if reoptimize:
            assert err <= TRUTH_BOUND and out["history_second"] is not None
        else:
            assert out["history_second"] is None and err <= 1e-2        # (the bias of order l r the second pass removes)


def test_fixed_node_other_than_zero():
    truth, arrays, init = consistent()
    rel = np.linalg.inv(truth[5])
    truth5, init5 = rel @ truth, rel @ init                              # the same graph with node 5's correction the identity
    init5[5] = np.eye(4)
    out = optimize(arrays, poses=init5, fixed=5)
    assert out["status"] == 1 and np.abs(out["poses"] - truth5).max() <= TRUTH_BOUND and np.array_equal(out["poses"][5], np.eye(4))


# ---------------------------------------------------------------- edge cases
def test_empty_and_edgeless_graphs():
    out = PO.optimize(3, [], [], np.zeros((0, 4, 4)), np.zeros((0, 6, 6)), [], MU)
    assert out["status"] == 1 and out["converged"] and out["iterations"] == 0 and np.array_equal(out["poses"], np.tile(np.eye(4), (3, 1, 1)))
    out = PO.optimize(1, [], [], np.zeros((0, 4, 4)), np.zeros((0, 6, 6)), [], MU)
    assert out["status"] == 1 and out["poses"].shape == (1, 4, 4)


def test_node_without_edges_stays_put():
    truth, (src, dst, T, info, unc), init = consistent()
    extra = PO.random_pose(np.random.default_rng(3), 0.4, 1.0)
    out = PO.optimize(N_RING + 1, src, dst, T, info, unc, MU, poses=np.concatenate([init, extra[None]]))
    assert out["status"] == 1 and np.array_equal(out["poses"][-1], extra) and np.abs(out["poses"][:-1] - truth).max() <= TRUTH_BOUND


def test_disconnected_graph():
    """two rings without an edge between them: the one with the fixed node reaches the truth, the other is consistent in itself
    (its six free directions cost nothing and the damping keeps the solve regular)"""
    truth, (src, dst, T, info, unc), init = consistent()
    n = N_RING
    arrays = (np.concatenate([src, src + n]), np.concatenate([dst, dst + n]), np.concatenate([T, T]), np.concatenate([info, info]),
              np.concatenate([unc, unc]))
    out = PO.optimize(2 * n, *arrays, MU, poses=np.concatenate([init, init]))
    P = out["poses"]
    print("disconnected: status", out["status"], "iterations", out["iterations"], "cost", out["cost"])
    assert out["status"] == 1 and np.abs(P[:n] - truth).max() <= TRUTH_BOUND
    rel = np.array([np.linalg.inv(P[n]) @ P[n + i] for i in range(n)])
    assert np.abs(rel - truth).max() <= 10 * TRUTH_BOUND and out["cost"] <= 1e-10


def test_duplicate_edges_are_summed():
    """an edge given twice weighs twice: the same optimum as one edge of twice the information"""
    truth, (src, dst, T, info, unc) = noisy()
    twice = optimize((np.append(src, src[3]), np.append(dst, dst[3]), np.concatenate([T, T[3:4]]), np.concatenate([info, info[3:4]]),
                      np.append(unc, unc[3])))
    info2 = info.copy()
    info2[3] *= 2.0
    once = optimize((src, dst, T, info2, unc))
    assert twice["status"] == once["status"] == 1 and np.abs(twice["poses"] - once["poses"]).max() <= 1e-9
    assert abs(twice["cost"] - once["cost"]) <= 1e-12 * once["cost"]
    lin = PO.linearize(truth, [0, 0], [1, 1], T[:1].repeat(2, 0), info[:1].repeat(2, 0), [False, False], MU)
    H, b = PO.assemble(lin["K"], lin["g"], [0, 0], [1, 1], 2, 0)
    assert np.array_equal(H[6:, 6:], lin["K"][0] + lin["K"][1]) and np.array_equal(b[6:], lin["g"][0] + lin["g"][1])


# ---------------------------------------------------------------- the argument checks
def _check(src, dst, n_nodes, fixed=0):
    s, t = np.ascontiguousarray(src, dtype=np.int32), np.ascontiguousarray(dst, dtype=np.int32)
    return _lib.load().sgam_pose_graph_check(ctypes.c_void_p(s.ctypes.data), ctypes.c_void_p(t.ctypes.data), len(s), n_nodes, fixed)


def test_c_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    assert lib.sgam_abi_version() == _lib.ABI_VERSION == 10
    assert _check([0, 1], [1, 2], 3) == 0 and _check([], [], 1) == 0
    assert _check([0, 1], [1, 1], 3) == -1                               # s == t
    assert _check([0, 3], [1, 2], 3) == -1 and _check([0, -1], [1, 2], 3) == -1
    assert _check([0], [1], 2, fixed=2) == -1 and _check([0], [1], 0) == -1
    assert _check([0], [1], PO.MAX_NODES) == 0 and _check([0], [1], PO.MAX_NODES + 1) == -1
    many = np.zeros(PO.MAX_EDGES + 1, dtype=np.int32)
    assert _check(many[:-1], many[:-1] + 1, 2) == 0 and _check(many, many + 1, 2) == -1
    # NULL pointers and sizes beyond the caps: SGAM_EINVAL before any launch (no device is touched)
    one = ctypes.c_void_p(8)                                             # never dereferenced: every call below is refused
    assert lib.sgam_pose_graph_linearize(None, 2, one, one, one, one, one, 1, one, one, one, one, one, one, one, one, None) == -1
    assert lib.sgam_pose_graph_linearize(one, PO.MAX_NODES + 1, one, one, one, one, one, 1, one, one, one, one, one, one, one, one, None) == -1
    assert lib.sgam_pose_graph_linearize(one, 2, one, one, one, one, one, PO.MAX_EDGES + 1, one, one, one, one, one, one, one, one, None) == -1
    assert lib.sgam_pose_graph_linearize(one, 2, one, one, one, one, one, 0, one, one, one, one, one, one, one, one, None) == -1
    assert lib.sgam_pose_graph_assemble(one, one, 2, 2, one, one, one, one, 3, one, 0, one, one, None) == -1          # fixed outside the graph
    assert lib.sgam_pose_graph_assemble(one, one, 2, 0, one, one, one, one, 1, one, 0, one, one, None) == -1          # fewer blocks than nodes
    assert lib.sgam_pose_graph_assemble(one, one, 2, 0, one, one, one, one, 3, one, 0, None, one, None) == -1
    assert lib.sgam_pose_graph_fold(None, 1, None, None, 0, one, None) == -1 and lib.sgam_pose_graph_fold(one, 1, one, None, 6, one, None) == -1
    assert lib.sgam_pose_graph_gate(one, 6, -1, 1e-6, one, one, None) == -1 and lib.sgam_pose_graph_gate(one, 6, 0, float("nan"), one, one, None) == -1
    assert lib.sgam_pose_graph_trial(one, None, 1, one, one, None) == -1
    assert lib.sgam_pose_graph_decide(2, 0, one, 1, 0, 0.0, one, one, one, one, 1, one, one, None) == -1
    assert lib.sgam_pose_graph_decide(1, 0, one, 1, 0, -1.0, one, one, one, one, 1, one, one, None) == -1
    assert lib.sgam_spd_solve_workspace_doubles(0) == -1 and lib.sgam_spd_solve_workspace_doubles(6145) == -1
    assert lib.sgam_spd_solve_workspace_doubles(1) == 64 * 64 + 3 * 64 and lib.sgam_spd_solve_workspace_doubles(65) == 128 * 128 + 3 * 128
    assert lib.sgam_spd_solve_workspace_doubles(6144) == 6144 * 6144 + 3 * 6144
    assert lib.sgam_spd_solve_f64(one, 6145, 6145, None, one, one, 1 << 40, one, one, None) == -1
    assert lib.sgam_spd_solve_f64(one, 6, 5, None, one, one, 1 << 40, one, one, None) == -1                           # ld < n
    assert lib.sgam_spd_solve_f64(one, 6, 6, None, one, one, 64 * 64, one, one, None) == -1                           # workspace too small
    assert lib.sgam_spd_solve_f64(one, 6, 6, None, one, one, 1 << 40, one, None, None) == -1


def test_python_front_refuses_bad_arguments():
    with pytest.raises(ValueError, match="n_nodes"):
        geometry.PoseGraph(0)
    with pytest.raises(ValueError, match="n_nodes"):
        geometry.PoseGraph(PO.MAX_NODES + 1)
    g = geometry.PoseGraph(3)
    with pytest.raises(ValueError, match="two different nodes"):
        g.add_edge(1, 1, np.eye(4), np.eye(6))
    with pytest.raises(ValueError, match="an integer in 0..2"):
        g.add_edge(0, 3, np.eye(4), np.eye(6))
    assert len(g) == 0
    with pytest.raises(ValueError, match="PoseGraph"):
        geometry.optimize_pose_graph([(0, 1)])
    with pytest.raises(ValueError, match="fixed"):
        geometry.optimize_pose_graph(g, fixed=3)
    with pytest.raises(ValueError, match="max_iterations"):
        geometry.optimize_pose_graph(g, max_iterations=0)
    with pytest.raises(ValueError, match="edge_prune_threshold"):
        geometry.optimize_pose_graph(g, edge_prune_threshold=1.5)
    with pytest.raises(ValueError, match="gradient_tolerance"):
        geometry.optimize_pose_graph(g, gradient_tolerance=-1.0)
    with pytest.raises(ValueError, match="estimation"):
        geometry.multiway_registration([], 0.1, estimation="plane")
    with pytest.raises(ValueError, match="clouds"):
        geometry.multiway_registration([], 0.1)
    import torch
    cloud = torch.zeros((4, 3))
    with pytest.raises(ValueError, match="loop_closure_stride"):
        geometry.multiway_registration([cloud, cloud], 0.1, loop_closure_stride=0)
    with pytest.raises(ValueError, match="min_fitness"):
        geometry.multiway_registration([cloud, cloud], 0.1, min_fitness=2.0)
    with pytest.raises(ValueError, match="max_correspondence_distance"):
        geometry.multiway_registration([cloud, cloud], 0.0)
    with pytest.raises(ValueError, match="spd_solve"):
        geometry.spd_solve(torch.zeros((3, 3)), torch.zeros(3, dtype=torch.float64))
