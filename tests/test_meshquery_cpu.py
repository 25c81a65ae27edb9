"""CPU: the mesh-query kernels' numpy twin (tests/meshquery_oracle.py) against outside truth — a float64 point–triangle distance by
another route, region by region on a hand triangle, the reported closest points on the marching-cubes meshes of
tests/test_meshops_cpu.py, the statistics and the geometry of the area-uniform sampler, surface_metrics of a mesh against itself —
and the argument checks of the new entry points through ctypes.  tests/test_gpu_meshquery.py runs the kernels against the twin bit
for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest

from sgam_neurips22_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import meshquery_oracle as Q  # noqa: E402
import test_meshops_cpu as C  # noqa: E402

f32 = np.float32
ULP = 2.0 ** -23
# the largest |twin - truth| / (coordinate scale * 2^-23) of sqrt(d2) over every case of test_distance_against_float64_truth,
# measured on the CPU, and the factor allowed on top of it (the bound scales with the few dozen roundings of the rule)
MEASURED_UNITS, FACTOR = 2.32, 4.0
TOL_UNITS = MEASURED_UNITS * FACTOR


# ---------------------------------------------------------------- float64 truth, by another route than the rule's
def truth_distance(a, b, c, q):
    """distance from q to triangle (a, b, c), all (...,3) float64: the foot of q on the plane where it lies inside the three edge
    half-planes, otherwise the least distance to the three segments"""
    a, b, c, q = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (a, b, c, q)))

    def dot(u, v):
        return (u * v).sum(-1)

    def segment(p0, p1):
        e = p1 - p0
        t = np.clip(dot(q - p0, e) / dot(e, e), 0.0, 1.0)
        return np.linalg.norm(q - (p0 + e * t[..., None]), axis=-1)

    n = np.cross(b - a, c - a)
    foot = q - n * (dot(q - a, n) / dot(n, n))[..., None]
    inside = np.ones(foot.shape[:-1], dtype=bool)
    for p0, p1 in ((a, b), (b, c), (c, a)):
        inside &= dot(np.cross(p1 - p0, foot - p0), n) >= 0
    edges = np.minimum(np.minimum(segment(a, b), segment(b, c)), segment(c, a))
    return np.where(inside, np.abs(dot(q - a, n)) / np.sqrt(dot(n, n)), edges)


def units(twin_d2, truth, *coords):
    """|sqrt(twin d2) - truth| in units of (the largest |coordinate| among coords) * 2^-23"""
    scale = np.max([np.abs(np.asarray(x, dtype=np.float64)).max(-1) for x in coords], axis=0)
    return np.abs(np.sqrt(twin_d2.astype(np.float64)) - truth) / (scale * ULP)


HAND = np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], dtype=f32)
# queries constructed to fall into each region of HAND (a, b, c = the rows), with the region and the distance expected
REGION_QUERIES = [
    ((-1, -1, 0.5), 0, np.sqrt(2.25)), ((5, -0.5, 0), 1, np.sqrt(1.25)), ((-0.5, 4, 1), 2, np.sqrt(2.25)),
    ((2, -1, 0), 3, 1.0), ((4, 3, 0), 4, 2.4), ((-2, 1.5, 0), 5, 2.0), ((1, 1, 2), 6, 2.0),
    ((4, 0, 0), 1, 0.0),                       # on a vertex
    ((1, 0.5, 0), 6, 0.0),                     # in the plane, inside
    ((1e4 * 5, 1e4 * 5, 1e4 * 5), 1, None),    # 1e4 times the triangle's size away: b is the corner nearest that direction
]


def distance_cases():
    """[(name, a, b, c, q)] float32 (n,3) arrays, one query per triangle: every case the tolerance is measured over"""
    rs = np.random.RandomState(11)
    out = []
    t = rs.uniform(-1, 1, (4000, 3, 3)).astype(f32)
    out.append(("random", t[:, 0], t[:, 1], t[:, 2], rs.uniform(-2, 2, (4000, 3)).astype(f32)))
    out.append(("near", t[:, 0], t[:, 1], t[:, 2], (t.mean(1) + rs.normal(0, 0.05, (4000, 3))).astype(f32)))
    s = t.copy()
    s[:, 2] = (s[:, 0] + (s[:, 1] - s[:, 0]) * rs.uniform(0, 1, (4000, 1)) + rs.normal(0, 1e-3, (4000, 3))).astype(f32)
    out.append(("slivers", s[:, 0], s[:, 1], s[:, 2], rs.uniform(-2, 2, (4000, 3)).astype(f32)))
    small = (t * f32(0.01) + f32(5.0)).astype(f32)
    out.append(("offset", small[:, 0], small[:, 1], small[:, 2], (5.0 + rs.uniform(-0.05, 0.05, (4000, 3))).astype(f32)))
    d = rs.normal(0, 1, (4000, 3))
    far = (d / np.linalg.norm(d, axis=1, keepdims=True) * 1e4 * np.sqrt(3)).astype(f32)
    out.append(("far", t[:, 0], t[:, 1], t[:, 2], far))
    hq = np.array([q for q, _, _ in REGION_QUERIES], dtype=f32)
    out.append(("hand", *(np.broadcast_to(HAND[k], hq.shape) for k in range(3)), hq))
    return out


def mesh_cases():
    """[(name, vertices, triangles, queries)]: the marching-cubes meshes with queries inside, near and outside"""
    out = []
    for name in ("sphere", "noise"):
        m = C.mesh(name)
        v = m["vertices"]
        rs = np.random.RandomState(3)
        lo, hi = v.min(0), v.max(0)
        q = np.concatenate([rs.uniform(lo, hi, (120, 3)), v[rs.randint(0, len(v), 120)] + rs.normal(0, 0.01 * (hi - lo).max(), (120, 3)),
                            rs.uniform(lo - (hi - lo), hi + (hi - lo), (60, 3))]).astype(f32)
        out.append((name, v, m["triangles"], q))
    return out


def test_distance_against_float64_truth():
    """sqrt(d2) of the twin against the float64 restatement; the triangle index is not compared (exact ties on shared edges).
    Measured on the CPU: the largest error over all the cases below is 2.32 units of (coordinate scale * 2^-23) (queries near
    the triangle; random 1.52, slivers 1.18, offset 0.65, far 1.01, hand 0.14, sphere 0.57, noise 0.61); four times that, 9.28
    units, is allowed (MEASURED_UNITS, FACTOR above)."""
    worst = {}
    for name, a, b, c, q in distance_cases():
        d2, _, _ = Q.point_triangle(a, b, c, q)
        assert d2.dtype == f32 and np.isfinite(d2).all()
        worst[name] = units(d2, truth_distance(a, b, c, q), a, b, c, q).max()
    for name, v, t, q in mesh_cases():
        got = Q.mesh_distance(v, t, q)
        v64 = v.astype(np.float64)
        t = t[(np.cross(v64[t[:, 1]] - v64[t[:, 0]], v64[t[:, 2]] - v64[t[:, 0]]) ** 2).sum(1) > 0]      # (marching cubes leaves a few without area)
        truth = truth_distance(v64[t[:, 0]][None], v64[t[:, 1]][None], v64[t[:, 2]][None], q[:, None].astype(np.float64)).min(1)
        assert (got["triangle"] >= 0).all()
        worst[name] = units(got["d2"], truth, q, np.broadcast_to(np.abs(v).max(0), q.shape)).max()
    print("point-triangle distance, worst error in units of scale * 2^-23: " + ", ".join(f"{k} {x:.2f}" for k, x in worst.items()))
    assert all(np.isfinite(x) and x <= TOL_UNITS for x in worst.values()), worst


def test_region_coverage_on_a_hand_triangle():
    q = np.array([p for p, _, _ in REGION_QUERIES], dtype=f32)
    d2, x, region = Q.point_triangle(HAND[0], HAND[1], HAND[2], q)
    assert region.tolist() == [r for _, r, _ in REGION_QUERIES]
    assert sorted(set(region.tolist())) == [0, 1, 2, 3, 4, 5, 6]
    for k, (_, _, want) in enumerate(REGION_QUERIES):
        if want is not None:
            assert abs(np.sqrt(float(d2[k])) - want) <= TOL_UNITS * ULP * np.abs(q[k]).max(), (k, d2[k], want)
    assert d2[7] == 0 and d2[8] == 0 and np.array_equal(x[7], HAND[1])
    truth = truth_distance(HAND[0], HAND[1], HAND[2], q[9])
    assert abs(np.sqrt(float(d2[9])) - truth) <= TOL_UNITS * ULP * np.abs(q[9]).max()
    # every rotation of the corners names the same point (up to rounding) and the rotated region
    names = {0: 2, 1: 0, 2: 1, 3: 5, 4: 3, 5: 4, 6: 6}
    d2r, _, rr = Q.point_triangle(HAND[1], HAND[2], HAND[0], q[:9])
    assert rr.tolist() == [names[r] for r in region[:9].tolist()]
    assert np.abs(np.sqrt(d2r.astype(np.float64)) - np.sqrt(d2[:9].astype(np.float64))).max() <= TOL_UNITS * ULP * 5


def test_winner_rule_and_what_is_not_a_triangle():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [np.nan, 0, 0], [2, 2, 2]], dtype=f32)
    t = np.array([[0, 1, 2], [1, 3, 2], [0, 0, 1], [0, 1, 4], [5, 5, 5], [0, 1, 2]], dtype=np.int32)
    q = np.array([[0.5, 0.5, 1.0], [0.2, 0.2, 0.5], [0.9, 0.9, 0.25], [np.nan, 0, 0], [np.inf, 0, 0]], dtype=f32)
    got = Q.mesh_distance(v, t, q)
    assert got["triangle"].tolist() == [0, 0, 1, -1, -1]                   # the shared edge ties: the lower index; never 2..4; 5 repeats 0
    assert got["d2"][:3].tolist() == [1.0, 0.25, 0.0625] and np.isinf(got["d2"][3:]).all() and np.isnan(got["closest"][3:]).all()
    swapped = Q.mesh_distance(v, t[[1, 0]], q[:1])
    assert swapped["triangle"].tolist() == [0] and swapped["d2"][0] == got["d2"][0]
    cut = Q.mesh_distance(v, t, q, max_d2=f32(0.3) * f32(0.3))
    assert cut["triangle"].tolist() == [-1, -1, 1, -1, -1] and np.isinf(cut["d2"][[0, 1]]).all()
    assert Q.area2(v, t).tolist() == [1.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    assert Q.mesh_distance(v, np.array([[0, 1, 6]], np.int32), q)["bad_index"]


@pytest.mark.parametrize("name", ["sphere", "noise"])
def test_points_reported_lie_on_the_reported_triangle(name):
    _, v, t, q = [m for m in mesh_cases() if m[0] == name][0]
    got = Q.mesh_distance(v, t, q)
    x, tri = got["closest"], got["triangle"]
    assert np.array_equal(Q.dist2(x, q).astype(f32).view(np.uint32), got["d2"].view(np.uint32))
    a, b, c = (v[t[tri, k]] for k in range(3))
    again, _, _ = Q.point_triangle(a, b, c, x)                             # the distance of the reported point to its own triangle
    off = units(again, np.zeros(len(q)), x, np.broadcast_to(np.abs(v).max(0), q.shape))
    print(f"{name}: reported points off their triangle by at most {off.max():.2f} units")
    assert off.max() <= TOL_UNITS


# ---------------------------------------------------------------- sampling
def two_triangles():
    """areas 3 : 1 (a 3 x 2 right triangle and a 1 x 2 one, apart)"""
    v = np.array([[0, 0, 0], [3, 0, 0], [0, 2, 0], [5, 0, 1], [6, 0, 1], [5, 2, 1]], dtype=f32)
    return v, np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)


def test_sampling_is_binomial_in_the_areas():
    v, t = two_triangles()
    w, cdf = Q.weights(Q.area2(v, t))
    assert w.tolist() == [2 ** 32, (2 ** 32) // 3] and cdf[-1] == w.sum()
    s = Q.sample(v, t, 4096, seed=1)
    big = int((s["triangle"] == 0).sum())
    sigma = np.sqrt(4096 * 0.75 * 0.25)
    print(f"sampling: {big} of 4096 on the large triangle (3072 +- {sigma:.1f})")
    assert abs(big - 3072) <= 5 * sigma


def test_samples_lie_on_their_triangles():
    for v, t in (two_triangles(), (C.mesh("noise")["vertices"], C.mesh("noise")["triangles"])):
        s = Q.sample(v, t, 2048, seed=5, want_normals=True)
        assert (s["weights"] >= 0).all() and np.abs(s["weights"].astype(np.float64).sum(1) - 1).max() <= 4 * ULP
        tri = t[s["triangle"]]
        d2, _, _ = Q.point_triangle(v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]], s["points"])
        off = units(d2, np.zeros(len(d2)), s["points"], np.broadcast_to(np.abs(v).max(0), s["points"].shape))
        assert off.max() <= TOL_UNITS
        assert np.abs(np.linalg.norm(s["normals"].astype(np.float64), axis=1) - 1).max() <= 4 * ULP


def test_sampling_skips_what_is_not_a_triangle_keeps_prefixes_and_depends_on_the_seed():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 2], [np.nan, 1, 1], [3, 0, 0], [3, 1, 0], [4, 0, 0]], dtype=f32)
    t = np.array([[0, 0, 1], [0, 1, 2], [3, 3, 3], [0, 1, 4], [5, 6, 7], [0, 1, 1]], dtype=np.int32)
    col = np.arange(24, dtype=f32).reshape(8, 3)
    s = Q.sample(v, t, 3000, seed=9, colors=col)
    assert set(s["triangle"].tolist()) == {1, 4} and np.isfinite(s["points"]).all() and np.isfinite(s["colors"]).all()
    short = Q.sample(v, t, 700, seed=9, colors=col)
    for k in ("points", "triangle", "colors"):
        assert np.array_equal(short[k], s[k][:700])
    other = Q.sample(v, t, 700, seed=10)
    assert not np.array_equal(other["points"], short["points"])
    with pytest.raises(ValueError):
        Q.sample(v, t[[0, 2, 3]], 4)


def test_samples_of_the_sphere_lie_near_the_sphere():
    """| |x - c| - r | of every sample is within the bound of a marching-cubes VERTEX plus the sagitta e^2 / (8 r) of the longest
    edge e.  The vertex bound (tests/test_meshops_cpu.py asserts none for this mesh) is derived here: along a lattice edge of
    length h the field |x - c| - r is convex with second derivative at most 1 / (r - h), so the zero of its linear interpolant is
    off the sphere by at most h^2 / (8 (r - h)) — plus the fp32 rounding of the field and of the vertex, 2^-20 of the scale."""
    m = C.mesh("sphere")
    v, t = m["vertices"], m["triangles"]
    h, r = 0.1, C.SPHERE[0][1] * 0.1
    c = (np.array(C.SPHERE[0][0]) + 0.5) * h
    vertex_bound = h * h / (8 * (r - h)) + 4.0 * 2.0 ** -20
    assert np.abs(np.linalg.norm(v.astype(np.float64) - c, axis=1) - r).max() <= vertex_bound
    e = max(np.linalg.norm(v[t[:, i]].astype(np.float64) - v[t[:, j]].astype(np.float64), axis=1).max() for i, j in ((0, 1), (1, 2), (2, 0)))
    s = Q.sample(v, t, 4096, seed=2)
    off = np.abs(np.linalg.norm(s["points"].astype(np.float64) - c, axis=1) - r)
    print(f"sphere samples: off the sphere by at most {off.max():.2e} (vertex bound {vertex_bound:.2e} + sagitta {e * e / (8 * r):.2e})")
    assert off.max() <= vertex_bound + e * e / (8 * r)
    # by area: the share of the samples on each octant of the sphere is an eighth, within 5 sigma
    octant = ((s["points"].astype(np.float64) - c) > 0) @ np.array([1, 2, 4])
    assert np.abs(np.bincount(octant, minlength=8) - 512).max() <= 5 * np.sqrt(4096 * 0.125 * 0.875) + 0.02 * 512


def test_surface_metrics_of_a_mesh_against_itself():
    m = C.mesh("sphere")
    v, t = m["vertices"], m["triangles"]
    out = Q.surface_metrics((v, t), (v, t), 0.1, n_samples=512, seed=4)
    tol = TOL_UNITS * ULP * float(np.abs(v).max())
    assert out["accuracy"] <= tol and out["completeness"] <= tol and out["chamfer"] <= 2 * tol * tol
    assert out["precision"] == out["recall"] == out["fscore"] == 1.0 and out["n_pred"] == out["n_ref"] == 512
    assert sorted(out) == sorted(["chamfer", "accuracy", "completeness", "precision", "recall", "fscore", "n_pred", "n_ref"])


# ---------------------------------------------------------------- the entry points without a GPU
def test_mesh_query_argument_validation_without_gpu():
    lib = _lib.load()
    r16 = lambda n: (n + 15) & ~15                                          # noqa: E731
    assert lib.sgam_mesh_grid_workspace_bytes(1000, 4, 5, 6) == 48 * 1000 + r16(4 * 121) + r16(4 * 120) + r16(4 * 1)
    assert lib.sgam_mesh_grid_workspace_bytes(7, 64, 64, 64) == 48 * 7 + r16(4 * (2 ** 18 + 1)) + r16(4 * 2 ** 18) + r16(4 * 256)
    for bad in ((0, 4, 4, 4), (2 ** 31, 4, 4, 4), (10, 0, 4, 4), (10, 4, -1, 4), (10, 4096, 4096, 2), (10, 1 << 13, 1 << 13, 1)):
        assert lib.sgam_mesh_grid_workspace_bytes(*bad) == -1, bad
    one = ctypes.c_void_p(16)                                               # a non-NULL address that is never read: every call below returns first
    assert lib.sgam_mesh_distance_brute_f32(None, 3, one, 1, one, 1, 1.0, one, one, None, one, None) == -1
    assert lib.sgam_mesh_distance_brute_f32(one, 3, one, 1, one, 1, 1.0, one, one, None, None, None) == -1       # no flag
    assert lib.sgam_mesh_distance_brute_f32(one, 3, one, 0, one, 1, 1.0, one, one, None, one, None) == -1
    assert lib.sgam_mesh_distance_brute_f32(one, 3, one, 1, one, 1, -1.0, one, one, None, one, None) == -1
    assert lib.sgam_mesh_distance_brute_f32(one, 3, one, 1, one, 1, float("nan"), one, one, None, one, None) == -1
    assert lib.sgam_mesh_grid_count(one, 3, one, 1, 0.0, 0.0, 0.0, 1.0, 2, 2, 2, None, one, None) == -1
    assert lib.sgam_mesh_grid_count(one, 3, one, 1, 0.0, 0.0, 0.0, 0.0, 2, 2, 2, one, one, None) == -1          # cell size 0
    assert lib.sgam_mesh_grid_build(one, 3, one, 1, 0.0, 0.0, 0.0, 1.0, 2, 2, 2, 4, None, 1 << 20, one, None) == -1
    assert lib.sgam_mesh_grid_build(one, 3, one, 1, 0.0, 0.0, 0.0, 1.0, 2, 2, 2, 4, one, 8, one, None) == -1       # short workspace
    assert lib.sgam_mesh_grid_build(one, 3, one, 1, 0.0, 0.0, 0.0, 1.0, 2, 2, 2, 4, ctypes.c_void_p(24), 1 << 20, one, None) == -1   # unaligned
    assert lib.sgam_mesh_distance_grid_f32(None, 1, 4, 0.0, 0.0, 0.0, 1.0, 2, 2, 2, one, 1 << 20, 1.0, one, one, None, None) == -1
    assert lib.sgam_mesh_distance_grid_f32(one, 1, 4, 0.0, 0.0, 0.0, 1.0, 2, 2, 2, one, 8, 1.0, one, one, None, None) == -1
    assert lib.sgam_mesh_triangle_area2_f32(one, 3, one, 1, None, one, None) == -1
    assert lib.sgam_mesh_triangle_area2_f32(one, 0, one, 1, one, one, None) == -1
    assert lib.sgam_mesh_sample_f32(one, None, 3, one, 1, None, 0, 4, one, one, None, None, one, None) == -1
    assert lib.sgam_mesh_sample_f32(one, None, 3, one, 1, one, 0, 0, one, one, None, None, one, None) == -1
    assert lib.sgam_mesh_sample_f32(one, None, 3, one, 1, one, 0, 4, one, one, one, None, one, None) == -1       # colours out without colours in
