"""CPU: the numpy twin of quadric-error decimation (tests/decimation_oracle.py) earns its credentials — what a
quadric measures, the independence of a round's selected edges, a closed sphere that stays a closed manifold, a flat sheet that
collapses at no cost, a better surface than vertex clustering at the same triangle count, the degenerate shapes — and the argument
checks of meshops.simplify_quadric_decimation and of the C entry points, which need no GPU.  tests/test_gpu_decimation.py compares
the kernels with this twin bit for bit on the meshes built here."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

from sgam_neurips22_amd import _lib, tsdf

sys.path.insert(0, os.path.dirname(__file__))
import decimation_oracle as DO  # noqa: E402
import meshops_oracle as MO  # noqa: E402
import meshquery_oracle as MQ  # noqa: E402

f32 = np.float32
# the smallest target the flat 17 x 17 sheet reaches with max_cost == 0 (measured with the twin: below it the next collapse has to
# move a corner of the square or the straight border, which costs)
FLAT_17_TARGET = 2


# ---------------------------------------------------------------- meshes
def icosphere(subdivisions):
    """the unit icosphere: 12 / 42 / 162 / 642 vertices, 20 / 80 / 320 / 1280 triangles, outward orientation, colours = |xyz|"""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / math.sqrt(1.0 + g * g) for p in v]
    for _ in range(subdivisions):
        mid, new = {}, []

        def between(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in t:
            ab, bc, ca = between(a, b), between(b, c), between(c, a)
            new += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = new
    v = np.asarray(v).astype(f32)
    return v, np.asarray(t, dtype=np.int32), np.abs(v).astype(f32)


def grid(n, bump=False):
    """an n x n sheet over the unit square, 2 (n - 1)^2 triangles, z = 0 or a Gaussian bump of height 0.25; colours = (x, y, z)"""
    j, i = np.meshgrid(np.arange(n), np.arange(n))
    x, y = j.reshape(-1) / (n - 1), i.reshape(-1) / (n - 1)
    z = 0.25 * np.exp(-((x - 0.5) ** 2 + (y - 0.5) ** 2) / (2 * 0.15 ** 2)) if bump else np.zeros_like(x)
    v = np.stack([x, y, z], 1).astype(f32)
    a = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    t = np.concatenate([np.stack([a, a + 1, a + n + 1], 1), np.stack([a, a + n + 1, a + n], 1)]).astype(np.int32)
    return v, t, v.copy()


def fan(n):
    """n triangles around vertex 0 on a cone: one long CSR segment"""
    ang = np.arange(n + 1) * (2 * np.pi * 0.9 / n)
    v = np.concatenate([[[0.0, 0.0, 0.3]], np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1)]).astype(f32)
    t = np.stack([np.zeros(n, int), np.arange(1, n + 1), np.arange(2, n + 2)], 1).astype(np.int32)
    return v, t, (v * f32(0.5) + f32(0.5)).astype(f32)


_TETRA_V = np.asarray([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=f32)
_SQUARE_V = np.asarray([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], dtype=f32)
_g9 = grid(9)
HAND = {
    "tetrahedron": (_TETRA_V, np.asarray([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32), None),
    "one": (_SQUARE_V[:3].copy(), np.asarray([[0, 1, 2]], dtype=np.int32), _SQUARE_V[:3].copy()),
    "two": (_SQUARE_V, np.asarray([[0, 1, 2], [0, 2, 3]], dtype=np.int32), None),
    # the 9 x 9 sheet with one more triangle that has no area (it names vertex 40 twice); the same sheet with a vertex nobody names
    "zero_area": (_g9[0], np.concatenate([_g9[1], [[30, 40, 40]]]).astype(np.int32), _g9[2]),
    "unreferenced": (np.concatenate([_g9[0], [[5.0, 5.0, 5.0]]]).astype(f32), _g9[1], np.concatenate([_g9[2], [[0.1, 0.2, 0.3]]]).astype(f32)),
    "empty": (np.zeros((0, 3), f32), np.zeros((0, 3), np.int32), None),
    "fan": fan(64),
}

_MESHES = {}


def mesh(name):
    """the shared inputs, built once and never written: ico2 / ico3, flat9 / flat17, bump9 / bump17 / bump33 and HAND's"""
    if name not in _MESHES:
        if name in HAND:
            m = HAND[name]
        elif name.startswith("ico"):
            m = icosphere(int(name[3:]))
        else:
            m = grid(int(name[4:]), bump=name.startswith("bump"))
        for a in m:
            if a is not None:
                a.setflags(write=False)
        _MESHES[name] = m
    return _MESHES[name]


# the cases the GPU test replays bit for bit: (mesh, arguments)
CASES = [
    ("ico2", dict(target_triangles=80)), ("ico2", dict(target_ratio=0.5, max_rounds=1)), ("ico2", dict(target_triangles=0)),
    ("ico3", dict(target_triangles=320)), ("ico3", dict(target_triangles=1241, oversample=4.0)),
    ("flat9", dict(target_triangles=0, max_error=0.0)), ("flat9", dict(target_triangles=61)),
    ("flat17", dict(target_triangles=FLAT_17_TARGET)), ("flat17", dict(target_triangles=0, max_error=0.0)),
    ("bump9", dict(target_ratio=0.25)), ("bump9", dict(target_triangles=0)),
    ("bump17", dict(target_triangles=128)), ("bump17", dict(target_triangles=455, oversample=1.0)), ("bump17", dict(target_ratio=0.5, boundary_weight=0.0)),
    ("fan", dict(target_triangles=16)), ("fan", dict(target_triangles=0)), ("fan", dict(target_triangles=63, max_rounds=1)),
    ("tetrahedron", dict(target_triangles=2)), ("one", dict(target_triangles=0)), ("two", dict(target_triangles=1)),
    ("zero_area", dict(target_triangles=40)), ("unreferenced", dict(target_triangles=40)), ("empty", dict(target_triangles=0)),
]
_RESULTS = {}


def twin(name, **kw):
    """the twin's result for a case, computed once"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _RESULTS:
        v, t, c = mesh(name)
        _RESULTS[key] = DO.decimate(v, t, c, **kw)
    return _RESULTS[key]


def topology(t):
    """(euler characteristic over the vertices in use, the multiset of triangles per edge)"""
    t = np.asarray(t, dtype=np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    _, per_edge = np.unique(e, axis=0, return_counts=True)
    return len(np.unique(t)) - len(per_edge) + len(t), per_edge


def signed_volume(v, t):
    p = np.asarray(v, dtype=np.float64)[np.asarray(t, dtype=np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def area(v, t):
    p = np.asarray(v, dtype=np.float64)[np.asarray(t, dtype=np.int64)]
    return float(np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).sum() / 2.0)


# ---------------------------------------------------------------- rule 1
def test_a_vertex_quadric_vanishes_on_the_planes_of_its_triangles():
    v, t, _ = mesh("ico2")
    Q = DO.vertex_quadrics(v, t, boundary_weight=1.0)                       # closed: no boundary term
    one = DO.vertex_quadrics(v[t[0]], np.asarray([[0, 1, 2]]), boundary_weight=0.0)
    p = v.astype(np.float64)[t[0]]
    rng = np.random.default_rng(0)
    w = rng.dirichlet(np.ones(3), 64) * 3.0 - 2.0 / 3.0                         # affine combinations: points of the plane, outside the triangle too
    pts = w @ p
    scale = np.abs(one).max() * max(1.0, np.abs(pts).max()) ** 2
    for k in range(3):
        assert np.abs(DO.quadric_value(np.repeat(one[k:k + 1], 64, 0), pts)).max() <= 1e-12 * scale
    # the full quadric of a vertex is the sum over its triangles: at the vertex itself every plane passes through
    assert np.abs(DO.quadric_value(Q, v.astype(np.float64))).max() <= 1e-12 * np.abs(Q).max()
    off = DO.quadric_value(Q, 1.1 * v.astype(np.float64))
    assert (off > 1e-6 * np.abs(Q).max()).all()


def test_the_boundary_quadric_of_an_open_fan_is_positive_off_the_boundary_line():
    v, t, _ = mesh("two")                                                   # the unit square, diagonal 0 - 2
    with_b, without = DO.vertex_quadrics(v, t, 1.0), DO.vertex_quadrics(v, t, 0.0)
    B = with_b - without
    assert np.abs(without[:, [0, 1, 2, 3, 4, 5, 6]]).max() == 0 and (without[:, 7] > 0).all()      # the plane z = 0 only
    # vertex 1 = (1, 0, 0) lies on the border lines y = 0 and x = 1: its boundary quadric is 0 on both lines' crossing, > 0 elsewhere
    q1 = B[1:2]
    assert DO.quadric_value(q1, np.asarray([[1.0, 0.0, 0.0]]))[0] == 0.0
    assert DO.quadric_value(q1, np.asarray([[1.0, 0.0, 7.0]]))[0] == 0.0    # the planes are perpendicular to the triangle
    for p in ([0.5, 0.5, 0.0], [1.0, 0.5, 0.0], [0.5, 0.0, 0.0], [2.0, -1.0, 0.0]):
        assert DO.quadric_value(q1, np.asarray([p]))[0] > 0.0, p
    # the diagonal is used by two triangles: vertex 0's boundary planes are x = 0 and y = 0 only, so the diagonal direction costs
    assert DO.quadric_value(B[0:1], np.asarray([[0.0, 0.0, 3.0]]))[0] == 0.0
    assert DO.quadric_value(B[0:1], np.asarray([[0.5, 0.5, 0.0]]))[0] > 0.0
    # doubling the weight doubles the term
    assert np.array_equal(DO.vertex_quadrics(v, t, 2.0) - without, 2.0 * B)


def test_edge_priority_is_a_bijection_on_a_sample():
    p = DO.edge_priority(np.arange(1 << 16))
    assert p.dtype == np.uint32 and len(np.unique(p)) == 1 << 16
    for e in (0, 1, 12345, 0xffffffff):
        x = e
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xffffffff
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xffffffff
        assert int(DO.edge_priority(np.asarray([e]))[0]) == x ^ (x >> 16)


# ---------------------------------------------------------------- rule 6
@pytest.mark.parametrize("name,target", [("ico3", 320), ("flat17", FLAT_17_TARGET), ("bump17", 64)])
def test_no_two_selected_edges_have_adjacent_vertices(name, target):
    v, t, c = mesh(name)
    trace = []
    out = DO.decimate(v, t, c, target_triangles=target, trace=trace)
    assert out["rounds"] == len(trace) >= 2
    for r in trace:
        sel = r["edges"][r["selected"]].astype(np.int64)
        assert len(sel) >= 1 and set(r["chosen"]) <= set(r["selected"])
        nv = len(r["offsets"]) - 1
        owner_edge = np.full(nv, -1)
        ends = sel.reshape(-1)
        assert len(np.unique(ends)) == len(ends)                            # no vertex in two selected edges
        owner_edge[ends] = np.repeat(np.arange(len(sel)), 2)
        owner = np.repeat(np.arange(nv), np.diff(r["offsets"].astype(np.int64)))
        a, b = owner_edge[owner], owner_edge[r["items"]]
        assert not ((a >= 0) & (b >= 0) & (a != b)).any()                   # no neighbours in two different selected edges


# ---------------------------------------------------------------- the sphere
def test_icosphere_to_a_quarter_stays_a_closed_manifold():
    v, t, _ = mesh("ico3")
    assert v.shape == (642, 3) and t.shape == (1280, 3)
    out = twin("ico3", target_triangles=320)
    assert out["stopped"] == "target" and len(out["triangles"]) <= 320
    chi, per_edge = topology(out["triangles"])
    assert chi == 2 and (per_edge == 2).all()
    assert len(np.unique(out["triangles"])) == len(out["vertices"])
    vol, vol0 = signed_volume(out["vertices"], out["triangles"]), signed_volume(v, t)
    assert vol > 0
    radial = np.abs(np.linalg.norm(out["vertices"].astype(np.float64), axis=1) - 1.0)
    print(f"icosphere 1280 -> {len(out['triangles'])}: rounds {out['rounds']}, max radial error {radial.max():.3e}, mean {radial.mean():.3e}, "
          f"volume ratio {vol / vol0:.4f}, max_cost {out['max_cost']:.3e}")
    assert radial.max() < 0.05 and 0.9 < vol / vol0 < 1.1                  # (a 320-triangle icosphere itself has volume ratio 0.96)
    # vertex_index: every output vertex descends from a distinct input slot, in ascending order; colours are carried
    assert (np.diff(out["vertex_index"]) > 0).all() and out["colors"].shape == out["vertices"].shape


# ---------------------------------------------------------------- the flat sheet
def test_flat_grid_collapses_at_no_cost():
    v, t, _ = mesh("flat17")
    assert t.shape == (512, 3)
    out = twin("flat17", target_triangles=FLAT_17_TARGET)
    assert out["stopped"] == "target" and out["max_cost"] == 0.0 and len(out["triangles"]) <= FLAT_17_TARGET
    assert (out["vertices"][:, 2] == 0).all()
    assert abs(area(out["vertices"], out["triangles"]) - area(v, t)) <= 1e-6 * area(v, t)
    # the four corners survive in place: a vertex sits exactly there (in whichever slot: the survivor of an edge is its lower end, and
    # it takes the corner's position when that is the end without cost)
    for c in (0, 16, 16 * 17, 17 * 17 - 1):
        assert (out["vertices"] == v[c]).all(axis=1).sum() == 1, c
    assert len(out["vertices"]) == 4
    # and it is the smallest such target: with the cost capped at 0 nothing goes below it
    floor = twin("flat17", target_triangles=0, max_error=0.0)
    assert floor["stopped"] == "no_candidates" and floor["max_cost"] == 0.0 and len(floor["triangles"]) == FLAT_17_TARGET


# ---------------------------------------------------------------- against vertex clustering
def test_decimation_is_closer_to_the_surface_than_vertex_clustering():
    v, t, c = mesh("bump33")
    vc = MO.simplify_vertex_clustering(v, t, 0.125, c)
    n = len(vc["triangles"])
    qd = DO.decimate(v, t, c, target_triangles=n)
    assert 0 < len(qd["triangles"]) <= n < len(t)
    pts = MQ.sample(v, t, 4096, seed=0)["points"]
    d_vc = float(np.sqrt(MQ.mesh_distance(vc["vertices"], vc["triangles"], pts)["d2"].astype(np.float64)).mean())
    d_qd = float(np.sqrt(MQ.mesh_distance(qd["vertices"], qd["triangles"], pts)["d2"].astype(np.float64)).mean())
    print(f"bump33 2048 -> {n} (clustering) / {len(qd['triangles'])} (decimation, {qd['rounds']} rounds): mean distance {d_vc:.4e} / {d_qd:.4e}, "
          f"ratio {d_vc / d_qd:.2f}")
    assert d_qd < d_vc


# ---------------------------------------------------------------- degenerate shapes
def test_degenerate_shapes():
    v, t, _ = mesh("tetrahedron")
    out = twin("tetrahedron", target_triangles=2)
    assert out["stopped"] == "no_candidates" and out["rounds"] == 0 and np.array_equal(out["triangles"], t) and np.array_equal(out["vertices"], v)
    out = twin("one", target_triangles=0)                                   # the one triangle names both ends: it goes, nothing is left to flip
    assert out["stopped"] == "target" and out["rounds"] == 1 and len(out["triangles"]) == 0 and len(out["vertices"]) == 2
    out = twin("two", target_triangles=1)
    assert out["stopped"] == "target" and len(out["triangles"]) == 1 and len(out["vertices"]) == 3
    v, t, _ = mesh("zero_area")
    out = twin("zero_area", target_triangles=40)
    assert len(out["triangles"]) <= len(t) and out["triangles"].max() < len(out["vertices"])
    v, t, c = mesh("unreferenced")
    out = twin("unreferenced", target_triangles=40)
    assert out["stopped"] == "target" and len(out["triangles"]) <= 40
    assert out["vertex_index"][-1] == len(v) - 1 and np.array_equal(out["vertices"][-1], v[-1]) and np.array_equal(out["colors"][-1], c[-1])
    out = twin("empty", target_triangles=0)
    assert out["stopped"] == "target" and out["rounds"] == 0 and out["vertices"].shape == (0, 3) and out["triangles"].shape == (0, 3)
    v, t, _ = mesh("fan")
    out = twin("fan", target_triangles=16)
    assert out["stopped"] == "target" and len(out["triangles"]) <= 16
    assert 0 in out["vertex_index"] or len(out["triangles"]) == 0
    one = twin("fan", target_triangles=63, max_rounds=1)
    assert one["rounds"] == 1 and len(one["triangles"]) == 63 and one["stopped"] == "target"   # the budget prefix: one collapse of several selected


def test_the_budget_prefix_applies_fewer_edges_than_were_selected():
    for name, kw, left in (("ico3", dict(target_triangles=1241, oversample=4.0), 1240), ("fan", dict(target_triangles=63, max_rounds=1), 63)):
        v, t, c = mesh(name)
        trace = []
        out = DO.decimate(v, t, c, trace=trace, **kw)
        assert len(trace) == 1 and 1 <= len(trace[0]["chosen"]) < len(trace[0]["selected"]), name
        assert out["stopped"] == "target" and len(out["triangles"]) == left


def test_every_case_is_consistent():
    """what holds for every case the GPU test replays: sizes, indices in range, the stop reason's meaning"""
    reasons = set()
    for name, kw in CASES:
        v, t, c = mesh(name)
        out = twin(name, **kw)
        target = kw["target_triangles"] if "target_triangles" in kw else int(math.floor(kw["target_ratio"] * len(t)))
        assert out["stopped"] in ("target", "no_candidates", "max_rounds"), (name, kw)
        assert (len(out["triangles"]) <= target) == (out["stopped"] == "target"), (name, kw)
        assert out["rounds"] <= kw.get("max_rounds", 256) and out["max_cost"] <= kw.get("max_error", math.inf)
        assert len(out["vertex_index"]) == len(out["vertices"]) and (out["colors"] is None) == (c is None)
        if len(out["triangles"]):
            assert 0 <= out["triangles"].min() and out["triangles"].max() < len(out["vertices"])
        reasons.add(out["stopped"])
    assert reasons == {"target", "no_candidates", "max_rounds"}
    assert twin("ico2", target_ratio=0.5, max_rounds=1)["stopped"] == "max_rounds"
    assert twin("ico2", target_triangles=0)["stopped"] == "no_candidates"          # a closed surface ends at a tetrahedron


# ---------------------------------------------------------------- the Python entry's argument checks
def test_argument_checks_come_before_any_launch():
    import torch

    from sgam_neurips22_amd import meshops
    v, t, _ = mesh("one")
    host = tsdf.DeviceMesh(torch.from_numpy(v.copy()), None, torch.from_numpy(t.copy()), torch.tensor([3, 1, 0, 0], dtype=torch.int32), 3, 1)
    f = meshops.simplify_quadric_decimation
    for kw in (dict(), dict(target_triangles=1, target_ratio=0.5), dict(target_triangles=-1), dict(target_triangles=1.5), dict(target_triangles=True),
               dict(target_ratio=0.0), dict(target_ratio=1.5), dict(target_ratio=float("nan")), dict(target_ratio="half"),
               dict(target_triangles=1, max_error=-1.0), dict(target_triangles=1, max_error=float("nan")),
               dict(target_triangles=1, boundary_weight=-0.5), dict(target_triangles=1, boundary_weight=float("inf")),
               dict(target_triangles=1, oversample=0.0), dict(target_triangles=1, oversample=float("inf")), dict(target_triangles=1, oversample=None),
               dict(target_triangles=1, max_rounds=0), dict(target_triangles=1, max_rounds=2.5)):
        with pytest.raises(ValueError):
            f(host, **kw)
    for kw in (dict(target_triangles=0), dict(target_ratio=1.0), dict(target_triangles=5, max_error=float("inf"))):
        with pytest.raises(_lib.SgamHipError, match="no CPU fallback"):
            f(host, **kw)
    assert set(meshops.SIMPLIFY_KEYS) == {"target_triangles", "target_ratio", "max_error", "boundary_weight", "oversample", "max_rounds"}
    assert set(meshops.CLEAN_KEYS) == {"min_triangles", "keep_largest", "smooth_iterations", "voxel_size", "normals"}


# ---------------------------------------------------------------- the C entry points
def test_decimation_entry_points_refuse_bad_arguments_without_gpu():
    lib = _lib.load()
    assert lib.sgam_abi_version() == 10                                 # additive: the ABI version stays
    for name in ("sgam_mesh_quadric_init_f64", "sgam_mesh_collapse_evaluate_f64", "sgam_mesh_collapse_workspace_bytes",
                 "sgam_mesh_collapse_select_i32", "sgam_mesh_collapse_apply_f64"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    p, odd = ctypes.c_void_p(256), ctypes.c_void_p(264)                 # never dereferenced: every check comes before a launch

    def init(v=p, nv=8, tri=p, nt=10, off=p, items=p, n=30, bw=1.0, out=p, flag=p):
        return lib.sgam_mesh_quadric_init_f64(v, nv, tri, nt, off, items, n, bw, out, flag, None)

    for kw in (dict(v=None), dict(tri=None), dict(off=None), dict(items=None), dict(out=None), dict(flag=None), dict(nv=0), dict(nt=0),
               dict(nt=(1 << 28) + 1), dict(n=0), dict(n=31), dict(bw=-1.0), dict(bw=float("nan")), dict(bw=float("inf"))):
        assert init(**kw) == -1, kw

    def evaluate(v=p, col=p, nv=8, tri=p, nt=10, q=p, toff=p, titems=p, ntri=30, voff=p, vitems=p, nvert=40, edges=p, ne=20, cost=p, rem=p, pos=p,
                 cout=p, flag=p):
        return lib.sgam_mesh_collapse_evaluate_f64(v, col, nv, tri, nt, q, toff, titems, ntri, voff, vitems, nvert, edges, ne, cost, rem, pos, cout, flag,
                                                   None)

    for kw in (dict(v=None), dict(tri=None), dict(q=None), dict(toff=None), dict(titems=None), dict(voff=None), dict(vitems=None), dict(edges=None),
               dict(cost=None), dict(rem=None), dict(pos=None), dict(flag=None), dict(col=None), dict(cout=None), dict(nv=0), dict(nt=0), dict(ne=0),
               dict(ne=21), dict(ntri=0), dict(ntri=31), dict(nvert=0), dict(nvert=61)):
        assert evaluate(**kw) == -1, kw

    size = lib.sgam_mesh_collapse_workspace_bytes
    assert size(1) == 32 and size(4) == 32 and size(5) == 64 and size(0) == size(-2) == -1

    def select(nv=8, voff=p, vitems=p, nvert=40, eoe=p, edges=p, cost=p, ne=20, tau=0.5, w=p, wb=size(8), key=p, flag=p):
        return lib.sgam_mesh_collapse_select_i32(nv, voff, vitems, nvert, eoe, edges, cost, ne, tau, w, wb, key, flag, None)

    for kw in (dict(voff=None), dict(vitems=None), dict(eoe=None), dict(edges=None), dict(cost=None), dict(key=None), dict(flag=None), dict(nv=0),
               dict(nvert=0), dict(ne=0), dict(ne=21), dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf")), dict(w=None),
               dict(wb=size(8) - 1), dict(w=odd)):
        assert select(**kw) == -1, kw

    def apply(v=p, col=p, q=p, nv=8, tri=p, nt=10, toff=p, titems=p, ntri=30, edges=p, pos=p, color=p, ne=20, chosen=p, m=3, merge=p, vk=p, tk=p,
              flag=p):
        return lib.sgam_mesh_collapse_apply_f64(v, col, q, nv, tri, nt, toff, titems, ntri, edges, pos, color, ne, chosen, m, merge, vk, tk, flag, None)

    for kw in (dict(v=None), dict(q=None), dict(tri=None), dict(toff=None), dict(titems=None), dict(edges=None), dict(pos=None), dict(chosen=None),
               dict(merge=None), dict(vk=None), dict(tk=None), dict(flag=None), dict(col=None), dict(color=None), dict(nv=0), dict(nt=0), dict(ne=0),
               dict(m=0), dict(m=21), dict(ntri=0), dict(ntri=31)):
        assert apply(**kw) == -1, kw
